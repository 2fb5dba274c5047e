"""Leaf-ordered records for small LDS-resident surfaces (plan_residency, SurfaceRec::lds_root bit 31).

A resident surface keeps its triangle records in LDS either one per triangle behind the leaf references (ref-indexed) or one per leaf
reference in leaf order with no references (leaf-ordered). The layout changes where a record lies, never which records a leaf tests or
in which order, so everything a kernel computes must be bit-identical between PTX_LDS_LEAF_ORDER=0 and =1.

  1. Host, no GPU: the plan itself on the Cornell box (ARR_RES_* / ARR_LDS_ROOT / ARR_RES_PLAN): every leaf of a leaf-ordered surface
     holds byte copies of tri_isect[kd_refs[...]], ref-indexed surfaces are what they were, the sphere stays ref-indexed, res_bytes is
     the sum of the regions, the extras stay within the cap, and a budget too small for an expansion leaves residency alone.
  2. GPU: ptx_leaf_intersect_batch layout 2 (leaf order staged into LDS) against layouts 0 and 1 on one-leaf trees of 1, 2, 8 and 64
     triangles that include determinants outside the short reciprocal's range (tests/golden/tri_scaled_vectors.npz), so the IEEE
     re-test loop runs in the new layout; Cornell frames, a ray batch and a hybrid plaza frame under both settings.
Everything is bitwise.
"""
import os

import numpy as np
import pytest

from _common import _proc
from _routes import ctx  # noqa: F401  (a fixture)
from conftest import CORNELL, GOLD, product_from_dict

F = np.float32
NOT_RESIDENT = 0xFFFFFFFF
LO_BIT = 0x80000000
CAP = 4096                      # kLdsLeafOrderCap (flat_scene.hpp)
LDS_BUDGET = 160 * 1024         # kLdsBudget (ptx_api.cpp)
SHADE_BYTES = 176               # sizeof(ShadeRec)
VARS = ("PTX_LDS_LEAF_ORDER", "PTX_LDS_BUDGET", "PTX_WAVEFRONT", "PTX_FORCE_GLOBAL", "PTX_SURFACE_UNITS", "PTX_NO_HYBRID", "PTX_NO_HOT_HITREC")


@pytest.fixture
def env(monkeypatch):
    for v in VARS:
        monkeypatch.delenv(v, raising=False)
    return monkeypatch


def _pad16(b):
    return (b + 15) & ~15


def _extra(rg):
    """Leaf-ordered minus ref-indexed bytes of a surface: refs * 48 - tris * 48 - refs * 4."""
    return (int(rg[7]) - int(rg[3])) * 48 - int(rg[7]) * 4


def _ref_bytes(rg):
    return int(rg[5]) * 8 + int(rg[7]) * 4 + int(rg[3]) * 48


def _plan(ptx, s):
    p = s.array(ptx.ARR_RES_PLAN)
    return dict(rg=s.array(ptx.ARR_SURF_RANGE), root=s.array(ptx.ARR_LDS_ROOT), nodes=s.array(ptx.ARR_RES_NODES), refs=s.array(ptx.ARR_RES_REFS),
                tris=s.array(ptx.ARR_RES_TRIS), res_bytes=int(p[0]), n_resident=int(p[1]), lds_bytes=int(p[2]), n_hot=int(p[3]),
                kd_nodes=s.array(ptx.ARR_KD_NODES), kd_refs=s.array(ptx.ARR_KD_REFS), tri_isect=s.array(ptx.ARR_TRI_ISECT),
                mode=s.info()["lds_resident"])


def _marked(p):
    return [u for u, r in enumerate(p["root"]) if r != NOT_RESIDENT and r & LO_BIT]


def _greedy(rg, resident, left):
    """The rule: resident surfaces by ascending extra (ties: surface index); stop at the first positive extra that takes the running
    sum of positive extras past min(cap, what residency left of the budget)."""
    cap, spent, out = min(CAP, left), 0, []
    for u in sorted(resident, key=lambda u: (_extra(rg[u]), u)):
        e = _extra(rg[u])
        if e > 0:
            if spent + e > cap:
                break
            spent += e
        out.append(u)
    return sorted(out), spent


def _check_plan(p, n_surf):
    """Every resident leaf names the records the full arrays name, in its surface's layout; the arrays are the sum of the regions."""
    rg, n_tris, n_refs, n_nodes = p["rg"], 0, 0, 0
    for u in range(n_surf):
        r = int(p["root"][u])
        if r == NOT_RESIDENT:
            continue
        lo = bool(r & LO_BIT)
        t0, nt, node0, nn, ref0, nr = (int(v) for v in rg[u][2:8])
        nb = r & ~LO_BIT                                    # a surface's root is its first node (surf_range: kd_root)
        n_nodes += nn; n_tris += nr if lo else nt; n_refs += 0 if lo else nr
        for k in range(nn):
            f0, f1 = (int(v) for v in p["kd_nodes"][node0 + k])
            w0, w1 = (int(v) for v in p["nodes"][nb + k])
            if f1 & 3 != 3:
                assert (w0, w1 & 15, (w1 >> 4) - nb) == (f0, f1 & 15, (f1 >> 4) - node0), (u, k)
                continue
            c = f1 >> 2
            assert w1 == f1 and ref0 <= f0 and f0 + c <= ref0 + nr, (u, k)
            want = p["tri_isect"][p["kd_refs"][f0:f0 + c]]
            got = p["tris"][w0:w0 + c] if lo else p["tris"][p["refs"][w0:w0 + c]]
            assert got.tobytes() == want.tobytes(), (u, k, lo)
    assert (n_tris, n_refs, n_nodes) == (len(p["tris"]), len(p["refs"]), len(p["nodes"]))
    assert p["res_bytes"] == len(p["tris"]) * 48 + n_surf * SHADE_BYTES + _pad16(len(p["nodes"]) * 8) + _pad16(len(p["refs"]) * 4)


# ---------------------------------------------------------------------------- 1. the plan (no GPU)
def test_cornell_plan_leaf_orders_the_small_surfaces(ptx, env):
    env.setenv("PTX_LDS_LEAF_ORDER", "0")
    old = _plan(ptx, ptx.Scene.load_gltf(None, CORNELL))
    env.delenv("PTX_LDS_LEAF_ORDER")
    new = _plan(ptx, ptx.Scene.load_gltf(None, CORNELL))          # the default is the new layout
    env.setenv("PTX_LDS_LEAF_ORDER", "1")
    new1 = _plan(ptx, ptx.Scene.load_gltf(None, CORNELL))
    assert all(np.array_equal(new[k], new1[k]) for k in ("root", "nodes", "refs", "tris")) and new["res_bytes"] == new1["res_bytes"]
    rg, n = new["rg"], len(new["rg"])
    assert n == 7 and old["mode"] == new["mode"] == 1 and old["n_resident"] == new["n_resident"] == 7
    assert np.array_equal(old["tri_isect"], new["tri_isect"]) and np.array_equal(old["kd_refs"], new["kd_refs"])
    _check_plan(old, n)
    _check_plan(new, n)
    assert _marked(old) == []
    sphere = int(np.argmax(rg[:, 3]))
    assert int(rg[sphere, 3]) == 960 and _extra(rg[sphere]) > 300_000
    assert _marked(new) == [u for u in range(n) if u != sphere]                 # the boxes, the three wall surfaces, the light
    # the rule, from the surface sizes alone
    used = n * SHADE_BYTES + 48 + sum(_ref_bytes(rg[u]) for u in range(n))
    want, spent = _greedy(rg, range(n), LDS_BUDGET - used)
    assert _marked(new) == want and 0 < spent <= CAP
    assert new["res_bytes"] - old["res_bytes"] == sum(_extra(rg[u]) for u in want) - (_pad16(len(old["refs"]) * 4) - len(old["refs"]) * 4) \
        + (_pad16(len(new["refs"]) * 4) - len(new["refs"]) * 4)
    assert new["res_bytes"] <= LDS_BUDGET
    # the sphere is unchanged: its nodes, references and records are the old plan's, at their new offsets
    t0, nt, node0, nn, ref0, nr = (int(v) for v in rg[sphere][2:8])
    ro, rn = int(old["root"][sphere]), int(new["root"][sphere])
    assert not rn & LO_BIT
    lo, ln = old["nodes"][ro:ro + nn], new["nodes"][rn:rn + nn]
    leaf = (lo[:, 1] & 3) == 3
    assert np.array_equal(lo[:, 1] & 15, ln[:, 1] & 15) and np.array_equal(lo[leaf, 1], ln[leaf, 1]) and np.array_equal(lo[~leaf, 0], ln[~leaf, 0])
    fo, fn = int(lo[leaf, 0].min()), int(ln[leaf, 0].min())
    assert np.array_equal(lo[leaf, 0] - fo, ln[leaf, 0] - fn)
    so, sn = old["refs"][fo:fo + nr], new["refs"][fn:fn + nr]
    assert np.array_equal(so - so.min(), sn - sn.min())
    assert old["tris"][so.min():so.min() + nt].tobytes() == new["tris"][sn.min():sn.min() + nt].tobytes()


@pytest.mark.parametrize("slack, want", [(0, [0, 1, 3, 4]), (319, [0, 1, 3, 4]), (320, [0, 1, 2, 3, 4]), (1151, [0, 1, 2, 3, 4]), (1152, [0, 1, 2, 3, 4, 5])])
def test_budget_too_small_for_an_expansion_leaves_the_surface_ref_indexed(ptx, env, slack, want):
    """With `slack` bytes left beside the resident geometry: the white walls cost 320 B more in leaf order, the light 832 B more (320 +
    832 = 1152); the surfaces that get smaller are leaf-ordered whatever is left. Everything stays resident, as with the layout off."""
    env.setenv("PTX_LDS_LEAF_ORDER", "0")
    rg = ptx.Scene.load_gltf(None, CORNELL).array(ptx.ARR_SURF_RANGE)
    used = len(rg) * SHADE_BYTES + 48 + sum(_ref_bytes(r) for r in rg)
    env.setenv("PTX_LDS_BUDGET", str(used + slack))
    old = _plan(ptx, ptx.Scene.load_gltf(None, CORNELL))
    env.setenv("PTX_LDS_LEAF_ORDER", "1")
    new = _plan(ptx, ptx.Scene.load_gltf(None, CORNELL))
    assert [_extra(rg[2]), _extra(rg[5])] == [320, 832]
    assert old["mode"] == new["mode"] == 1 and old["n_resident"] == new["n_resident"] == 7 and _marked(old) == []
    assert _marked(new) == want == _greedy(rg, range(7), slack)[0]
    _check_plan(new, 7)
    assert new["res_bytes"] <= used + slack
    # one byte less and the sphere no longer fits: residency is decided before the layout and without it
    env.setenv("PTX_LDS_BUDGET", str(used - 1))
    for v in ("0", "1"):
        env.setenv("PTX_LDS_LEAF_ORDER", v)
        p = _plan(ptx, ptx.Scene.load_gltf(None, CORNELL))
        assert p["mode"] == 2 and p["n_resident"] == 6 and p["root"][6] == NOT_RESIDENT, v
        _check_plan(p, 7)


def test_plaza_level_3_plan_is_hybrid_under_both_settings(ptx, env):
    d = _proc().plaza_scene(level=3, sun=True, alpha=False)
    plans = {}
    for v in ("0", "1"):
        env.setenv("PTX_LDS_LEAF_ORDER", v)
        plans[v] = _plan(ptx, product_from_dict(ptx, None, d))
        _check_plan(plans[v], len(plans[v]["rg"]))
    old, new = plans["0"], plans["1"]
    big = int(np.argmax(new["rg"][:, 3]))
    assert int(new["rg"][big, 3]) == 1280 and old["mode"] == new["mode"] == 2
    assert [r == NOT_RESIDENT for r in old["root"]] == [r == NOT_RESIDENT for r in new["root"]] == [u == big for u in range(len(new["rg"]))]
    resident = [u for u in range(len(new["rg"])) if u != big]
    used = len(new["rg"]) * SHADE_BYTES + 48 + sum(_ref_bytes(new["rg"][u]) for u in resident)
    assert _marked(old) == [] and _marked(new) == _greedy(new["rg"], resident, LDS_BUDGET - used)[0] and len(_marked(new)) >= 1


# ---------------------------------------------------------------------------- 2. the kernels
RCP_LO, RCP_HI = F(2.0 ** -125), F(2.0 ** 126)        # rcp_core's range (device_core.hpp)
LEAF_SCALES = (-65, -64, -63, -40, 0, 40, 62, 63)
N_LEAVES = {1: 160, 2: 80, 8: 20, 64: 6}


def _det32(a, b, c, d):
    """The determinant of triangle.cpp:136-157 in binary32, in the reference's order."""
    with np.errstate(all="ignore"):
        mx, my, mz = (a - b).astype(F), (a - c).astype(F), d.astype(F)
        c1 = my[..., 1] * mz[..., 2] - mz[..., 1] * my[..., 2]
        c2 = mx[..., 1] * mz[..., 2] - mz[..., 1] * mx[..., 2]
        c3 = mx[..., 1] * my[..., 2] - my[..., 1] * mx[..., 2]
        return ((mx[..., 0] * c1 - my[..., 0] * c2) + mz[..., 0] * c3).astype(F)


def _nanbits(a):
    a = np.ascontiguousarray(a, np.float32)
    return np.where(np.isnan(a), np.uint32(0x7FC00000), a.view(np.uint32))


@pytest.mark.gpu
@pytest.mark.parametrize("n_tri", [1, 2, 8, 64])
def test_leaf_intersect_lds_leaf_order_equals_both_other_layouts(ctx, n_tri):
    g = dict(np.load(os.path.join(GOLD, "tri_scaled_vectors.npz")))
    scales = g["tri_k"].tolist()
    rng = np.random.default_rng(900 + n_tri)
    pool = [(i, k) for k in LEAF_SCALES for i in range(256)]
    n_retest = n_own_retest_hit = n_hit = 0
    for li in range(N_LEAVES[n_tri]):
        pick = [pool[p] for p in rng.choice(len(pool), n_tri, replace=False)]
        own = np.stack([g["tri_in"][i] * np.concatenate([np.full(12, np.ldexp(1.0, k)), np.ones(3)]).astype(F) for i, k in pick]).astype(F)
        ref_t = np.array([g["tri_out"][scales.index(k)][i, 0] for i, k in pick], F)
        refs = rng.permutation(n_tri).astype(np.uint32)
        with np.errstate(invalid="ignore"):
            finite = np.where(ref_t >= 0, ref_t, F(1)).astype(F)           # `<=` keeps a hit exactly at max_dist
        rays = np.concatenate([np.concatenate([own[:, 9:15], np.full((n_tri, 1), np.inf, F)], 1), np.concatenate([own[:, 9:15], finite[:, None]], 1)]).astype(F)
        got = [ctx.leaf_intersect(own[:, :9], rays, refs=refs, leaf_ordered=lo) for lo in (0, 1, 2)]
        for f in ("t", "beta", "gamma", "triangle"):
            for other in (0, 1):
                a, b = got[2][f], got[other][f]
                if f != "triangle":
                    a, b = _nanbits(a), _nanbits(b)
                np.testing.assert_array_equal(a, b, err_msg=f"leaf {li}: {f}, layout 2 against layout {other}")
        # which rays went through the IEEE re-test: some triangle of the leaf has a determinant outside rcp_core's range (or zero)
        det = _det32(own[None, :, 0:3], own[None, :, 3:6], own[None, :, 6:9], rays[:, None, 3:6])
        with np.errstate(invalid="ignore"):
            out = ~((np.abs(det) >= RCP_LO) & (np.abs(det) < RCP_HI))
        n_retest += int(out.any(1).sum())
        n_hit += int((got[2]["triangle"] >= 0).sum())
        # rays that the reference says hit their own triangle through such a determinant: only the re-test can report a hit for them
        with np.errstate(invalid="ignore"):
            own_out_hit = (ref_t >= 0) & out[np.arange(n_tri), np.arange(n_tri)]
        assert (got[2]["triangle"][:n_tri][own_out_hit] >= 0).all(), li
        n_own_retest_hit += int(own_out_hit.sum())
    total = 2 * n_tri * N_LEAVES[n_tri]
    assert n_retest >= total // 4 and n_own_retest_hit >= 10 and n_hit >= total // 8, (n_retest, n_own_retest_hit, n_hit, total)


def _cornell(ptx, ctx, env, v):
    env.setenv("PTX_LDS_LEAF_ORDER", v)
    s = ptx.Scene.load_gltf(ctx, CORNELL)
    env.delenv("PTX_LDS_LEAF_ORDER")
    return s


@pytest.mark.gpu
@pytest.mark.parametrize("bounces, tile", [(8, None), (0, None), (8, (17, 9, 50, 31))], ids=["8 bounces", "0 bounces", "tile"])
def test_cornell_frame_is_the_same_under_both_layouts(ptx, ctx, env, bounces, tile):
    frames = {}
    for v in ("0", "1"):
        s = _cornell(ptx, ctx, env, v)
        p = _plan(ptx, s)
        assert p["mode"] == 1 and len(_marked(p)) == (6 if v == "1" else 0), v       # the layout that was asked for is in effect
        assert p["lds_bytes"] <= LDS_BUDGET and p["lds_bytes"] == p["res_bytes"] + 144 * p["n_hot"]
        frame, st = s.render(96, 54, 4, bounces, tile=tile)
        frames[v] = (frame.copy(), st["rays"], st["samples"])
        s.close()
    assert frames["0"][0].shape == ((tile[3], tile[2], 4) if tile else (54, 96, 4))
    assert frames["0"][0].tobytes() == frames["1"][0].tobytes() and frames["0"][1:] == frames["1"][1:]
    assert frames["1"][1] > 0 or bounces == 0
    assert np.isfinite(frames["1"][0]).all() and frames["1"][0][..., 3].min() == 4


@pytest.mark.gpu
def test_cornell_ray_batch_is_the_same_under_both_layouts(ptx, ctx, env):
    """4 096 seeded rays that start inside the room (the world box of the model with the three wall surfaces, shrunk by a tenth)."""
    hits = {}
    for v in ("0", "1"):
        s = _cornell(ptx, ctx, env, v)
        if v == "0":
            ms, box, xf = s.array(ptx.ARR_MODEL_SURF), s.array(ptx.ARR_MODEL_AABB), s.array(ptx.ARR_MODEL_XFORM)
            room = int(np.argmax(ms[:, 1]))
            assert ms[room, 1] == 3
            x = xf[room].astype(np.float64)
            corners = np.array([[box[room][3 * ((c >> a) & 1) + a] for a in range(3)] for c in range(8)], np.float64)
            world = corners @ x[3:].reshape(3, 3) + x[:3]                     # basis columns are the rows of the reshaped block
            lo, hi = world.min(0), world.max(0)
            mid, half = (lo + hi) / 2, (hi - lo) / 2 * 0.9
            rng = np.random.default_rng(4096)
            o = (mid + half * rng.uniform(-1, 1, (4096, 3))).astype(F)
            d = rng.standard_normal((4096, 3))
            d = (d / np.linalg.norm(d, axis=1, keepdims=True)).astype(F)
        hits[v] = s.intersect(o, d)
        s.close()
    assert hits["0"].keys() == hits["1"].keys()
    for k in hits["0"]:
        assert np.asarray(hits["0"][k]).tobytes() == np.asarray(hits["1"][k]).tobytes(), k
    assert (hits["1"]["surface"] >= 0).mean() > 0.95 and len(np.unique(hits["1"]["surface"])) >= 6


@pytest.mark.gpu
def test_hybrid_plaza_frame_is_the_same_under_both_layouts(ptx, ctx, env):
    d = _proc().plaza_scene(level=3, sun=True, alpha=False)
    frames = {}
    env.setenv("PTX_WAVEFRONT", "0")
    for v in ("0", "1"):
        env.setenv("PTX_LDS_LEAF_ORDER", v)
        s = product_from_dict(ptx, ctx, d)
        env.delenv("PTX_LDS_LEAF_ORDER")
        p = _plan(ptx, s)
        big = int(np.argmax(p["rg"][:, 3]))
        assert p["mode"] == 2 and int(p["rg"][big, 3]) == 1280               # the ground and the small sphere in LDS, the large sphere in global memory
        assert [r == NOT_RESIDENT for r in p["root"]] == [u == big for u in range(len(p["rg"]))]
        assert (len(_marked(p)) >= 1) == (v == "1"), v
        frame, st = s.render(96, 54, 4, 8)
        assert ctx.timing()["pipeline"] == 0                                  # the fused kernel, not the queue pipeline
        frames[v] = (frame.copy(), st["rays"])
        s.close()
    assert frames["0"][0].tobytes() == frames["1"][0].tobytes() and frames["0"][1] == frames["1"][1]
    assert np.isfinite(frames["1"][0]).all() and frames["1"][1] > 96 * 54 * 4
