"""The triangle solve and the leaf loop's IEEE re-test far from unit scale, against the reference.

The fused kernels divide by the determinant with v_rcp_f32 and one Newton step (device_core.hpp: rcp_core), which is IEEE's quotient
only for 2^-125 <= |det| < 2^126. mesh_traverse's leaf loop keeps the largest rcp_key of a leaf's determinants and tests the whole
leaf again with the IEEE division when one lies outside. At unit scale only det == 0 gets there, and the re-test never finds a hit.
The determinant of a triangle scaled by 2^k scales with 4^k, so here geometry is scaled by 2^k, k around -63 and +63: the reference
still reports valid hits, through determinants on both sides of the range's ends.

  1. tests/golden/tri_scaled_vectors.npz (oracle/make_golden.py --only-tri-scaled): geometry::triangle::intersect of the compiled
     reference on 256 triangle / ray rows at 21 scales. The oracle is pinned to it bit for bit, and the rows are shown to cover both
     sides of the range (fixed bars below).
  2. ptx_leaf_intersect_batch runs mesh_traverse itself on one leaf of chosen triangles, in both record layouts: single triangles
     against the fixture, and mixed leaves (in-range and out-of-range determinants side by side, duplicates, shuffled references,
     finite max_dist) against the oracle's per-triangle results combined by the rule of mesh.cpp:381-389.
  3. procedural.plaza_scene scaled by 2^-65 ... 2^-60 on the fused kernel with LDS-resident (level 1) or hybrid (level 3) geometry, on
     the fused kernel with global geometry and on the queue pipeline, each route asserted as in tests/test_unit_limits.py: hit records against the oracle bit for
     bit, small renders bitwise equal across the routes.
Everything is bitwise; a NaN equals any NaN.
"""
import os

import numpy as np
import pytest

from _checks import _check_records, _same_hits
from _common import _proc
from _routes import clean_env, ctx, forced_routes, under_force_global  # noqa: F401  (clean_env and ctx are fixtures)
from conftest import GOLD, kd_stream_packed, kd_stream_preorder, oracle_from_dict, product_from_dict

F = np.float32
RCP_LO, RCP_HI = F(2.0 ** -125), F(2.0 ** 126)        # rcp_core's range: 2^-125 <= |det| < 2^126 (device_core.hpp)
SCALES = list(range(-66, -57)) + [-40, 0, 40] + list(range(58, 67))


def _nan_bits(a):
    """Bit patterns with every NaN mapped to one pattern."""
    a = np.ascontiguousarray(a, np.float32)
    return np.where(np.isnan(a), np.uint32(0x7FC00000), a.view(np.uint32))


def _pow2(k):
    return F(np.ldexp(1.0, int(k)))


def _det32(a, b, c, d):
    """The determinant of triangle.cpp:136-157 in binary32, the reference's operations in the reference's order."""
    with np.errstate(all="ignore"):
        mx, my, mz = (a - b).astype(F), (a - c).astype(F), d.astype(F)
        c1 = my[..., 1] * mz[..., 2] - mz[..., 1] * my[..., 2]
        c2 = mx[..., 1] * mz[..., 2] - mz[..., 1] * mx[..., 2]
        c3 = mx[..., 1] * my[..., 2] - my[..., 1] * mx[..., 2]
        return ((mx[..., 0] * c1 - my[..., 0] * c2) + mz[..., 0] * c3).astype(F)


def _in_range(det):
    with np.errstate(invalid="ignore"):
        ad = np.abs(det)
        return (ad >= RCP_LO) & (ad < RCP_HI)


def _out_nonzero(det):
    """A non-zero determinant outside rcp_core's range (an infinite one included; NaN is not counted)."""
    return ~_in_range(det) & (det != 0) & ~np.isnan(det)


@pytest.fixture(scope="module")
def tri_gold():
    g = dict(np.load(os.path.join(GOLD, "tri_scaled_vectors.npz")))
    assert g["tri_in"].shape == (256, 15) and g["tri_k"].tolist() == SCALES and g["tri_out"].shape == (len(SCALES), 256, 4)
    return g


def _rows_at(g, j):
    """The fixture's rows at scale SCALES[j]: corners and origin times 2^k (exact), the unit direction kept. -> [256, 15]"""
    r = g["tri_in"].copy()
    r[:, :12] *= _pow2(SCALES[j])
    return r


def _row_dets(g, j):
    r = _rows_at(g, j)
    return _det32(r[:, 0:3], r[:, 3:6], r[:, 6:9], r[:, 12:15])


# ---------------------------------------------------------------------------- 1. reference vectors at scale (no GPU)
def test_oracle_tri_intersect_matches_reference_at_every_scale(ora, tri_gold):
    for j, k in enumerate(SCALES):
        got = ora.tri_intersect(_rows_at(tri_gold, j))
        np.testing.assert_array_equal(_nan_bits(got), _nan_bits(tri_gold["tri_out"][j]), err_msg=f"k = {k}")


def test_scaling_by_a_power_of_two_is_exact_at_moderate_scales(tri_gold):
    """At 2^0 and 2^+-40 nothing under- or overflows: the barycentrics are the unit-scale bits and the distance is the unit
    distance times 2^k (a rejected row stays at -1, 0, 0, 0)."""
    out = tri_gold["tri_out"]
    unit = out[SCALES.index(0)]
    rejected = (unit[:, 0] == -1) & (unit[:, 1:] == 0).all(1)
    assert 0.1 < rejected.mean() < 0.5 and not np.isnan(unit).any()
    for k in (0, 40, -40):
        o = out[SCALES.index(k)]
        np.testing.assert_array_equal(_nan_bits(o[:, 1:]), _nan_bits(unit[:, 1:]), err_msg=f"k = {k}")
        np.testing.assert_array_equal(_nan_bits(o[:, 0]), _nan_bits(np.where(rejected, F(-1), unit[:, 0] * _pow2(k))), err_msg=f"k = {k}")


def test_fixture_rows_hit_on_both_sides_of_the_short_reciprocals_range(tri_gold):
    out = tri_gold["tri_out"]
    share = {}
    for j, k in enumerate(SCALES):
        det = _row_dets(tri_gold, j)
        hit = out[j, :, 0] >= 0
        share[k] = ((hit & _out_nonzero(det)).mean(), (hit & _in_range(det)).mean())
    for k in (-65, -64, -63, -62):
        assert share[k][0] >= 0.05, (k, share[k])
    for k in (62, 63):
        assert share[k][0] >= 0.01, (k, share[k])
    for k in (-64, -63, -62, 62, 63):
        assert share[k][1] >= 0.01, (k, share[k])
    # the control scales never leave the range except through det == 0 (the collinear rows)
    for k in (-40, 0, 40):
        assert share[k][0] == 0


# ---------------------------------------------------------------------------- 2. the leaf loop itself
# Mixed leaves. A leaf holds m distinct (row, scale) triangles of one family, each twice (an exact duplicate with its own id), in a
# shuffled order behind a non-identity reference list; its rays are the m rows' rays at their own scales, each once with max_dist = +inf
# and once with a finite max_dist: the nearest distance itself (`<=` keeps it) for every other ray, the float just below it (the nearest
# hit is excluded, and with it every hit) for the rest. Families: "in" = scales where every non-degenerate determinant is in range, "out" =
# scales where every determinant is below it, "mix" = scales on both sides of both ends.
FAMILIES = {"in": (-40, 0, 40), "out": (-66, -65), "mix": (-65, -64, -63, -62, -61, -40, 0, 62, 63)}
LEAVES = {2: {"in": 250, "out": 1200, "mix": 300}, 8: {"in": 100, "out": 250, "mix": 350}, 64: {"in": 30, "out": 40, "mix": 60}}
_mixed_cache = {}


def _mixed_cases(ora, g, n_tri):
    """-> list of leaves: dict(corners [n_tri, 9], refs [n_tri], rays [2m, 7], want = (t, beta, gamma [2m], triangle [2m]),
    win_in / others_in / others_out [2m] bool, family). Expected values from the oracle's tri_intersect alone."""
    if n_tri in _mixed_cache:
        return _mixed_cache[n_tri]
    m = n_tri // 2
    rng = np.random.default_rng(1000 + n_tri)
    rows = {k: _rows_at(g, SCALES.index(k)) for fam in FAMILIES.values() for k in fam}
    leaves = []
    for fam, ks in FAMILIES.items():
        pool = [(i, k) for k in ks for i in range(256)]
        for _ in range(LEAVES[n_tri][fam]):
            pick = [pool[p] for p in rng.choice(len(pool), m, replace=False)]
            own = np.stack([rows[k][i] for i, k in pick])                        # [m, 15]
            corners = np.concatenate([own[:, :9], own[:, :9]])                   # triangle t and its duplicate t + m
            refs = rng.permutation(n_tri).astype(np.uint32)
            while (refs == np.arange(n_tri)).all():
                refs = rng.permutation(n_tri).astype(np.uint32)
            leaves.append(dict(family=fam, corners=corners.astype(F), refs=refs, ray6=own[:, 9:15]))
    # one oracle call for every (ray, triangle in test order) pair of every leaf
    pairs = np.concatenate([np.concatenate([np.repeat(L["corners"][L["refs"]][None], m, 0), np.repeat(L["ray6"][:, None], n_tri, 1)], 2).reshape(-1, 15)
                            for L in leaves])
    res = ora.tri_intersect(pairs).reshape(len(leaves), m, n_tri, 4)
    det = _det32(pairs[:, 0:3], pairs[:, 3:6], pairs[:, 6:9], pairs[:, 12:15]).reshape(len(leaves), m, n_tri)
    for li, L in enumerate(leaves):
        t = res[li, :, :, 0]
        with np.errstate(invalid="ignore"):
            ok = t >= 0
        near = np.where(ok, t, np.inf).min(1)                                    # nearest hit distance per ray, inf = none
        finite = np.where((np.arange(m) + li) % 2 == 0, near, np.nextafter(near.astype(F), F(-1))).astype(F)
        max_dist = np.concatenate([np.full(m, np.inf, F), finite])
        tt, rr, dd = np.concatenate([t, t]), np.concatenate([res[li], res[li]]), np.concatenate([det[li], det[li]])
        with np.errstate(invalid="ignore"):
            valid = (tt >= 0) & (tt <= max_dist[:, None])
        cand = np.where(valid, tt, np.inf)                                       # a valid hit may itself lie at +inf (0 * inf = NaN barycentrics pass)
        pos = (valid & (cand == cand.min(1, keepdims=True))).argmax(1)           # the first valid triangle at the nearest distance
        hit = valid.any(1)
        r = np.arange(2 * m)
        L["rays"] = np.concatenate([np.concatenate([L["ray6"], L["ray6"]]), max_dist[:, None]], 1).astype(F)
        L["want"] = (np.where(hit, rr[r, pos, 0], F(-1)), np.where(hit, rr[r, pos, 2], F(0)), np.where(hit, rr[r, pos, 3], F(0)),
                     np.where(hit, L["refs"][pos].astype(np.int64), -1).astype(np.int32))
        inr = _in_range(dd)
        others = np.ones_like(inr)
        others[r, pos] = False
        dup = L["refs"][None, :] % m == (L["refs"][pos] % m)[:, None]            # the winner's own duplicate is not "another triangle"
        others &= ~dup
        L["hit"] = hit
        L["win_in"] = inr[r, pos]
        L["others_in"], L["others_out"] = (others & inr).any(1), (others & ~inr).any(1)
        L["all_in"], L["all_out"] = inr.all(1), (~inr).all(1)
    _mixed_cache[n_tri] = leaves
    return leaves


def _class_counts(leaves):
    c = np.zeros(4, np.int64)
    for L in leaves:
        h = L["hit"]
        c[0] += (h & L["win_in"] & L["others_out"]).sum()       # 1. the winner in range, another triangle of the leaf out of range
        c[1] += (h & ~L["win_in"] & L["others_in"]).sum()       # 2. the winner out of range, others in range
        c[2] += (h & L["all_out"]).sum()                        # 3. every triangle out of range
        c[3] += (h & L["all_in"]).sum()                         # 4. every triangle in range
    return c


@pytest.mark.parametrize("n_tri", [2, 8, 64])
def test_mixed_leaves_cover_the_four_ray_classes(ora, tri_gold, n_tri):
    """From the oracle alone: at least 200 rays with a hit in each class. A leaf of 2 is a triangle and its duplicate, so only the
    classes "every triangle out of range" and "every triangle in range" exist there."""
    leaves = _mixed_cases(ora, tri_gold, n_tri)
    c = _class_counts(leaves)
    assert (c[2:] >= 200).all(), c
    if n_tri > 2:
        assert (c[:2] >= 200).all(), c
    # the finite max_dist does exclude hits: rays whose nearest hit (and with it every hit) lies just beyond it, and rays that keep a
    # hit exactly at max_dist
    lost = sum(int((L["hit"][:n_tri // 2] & ~L["hit"][n_tri // 2:]).sum()) for L in leaves)
    kept = sum(int((L["hit"][n_tri // 2:] & (L["want"][0][n_tri // 2:] == L["rays"][n_tri // 2:, 6])).sum()) for L in leaves)
    assert lost >= 100 and kept >= 100, (lost, kept)
    # ties: every hit has an exact duplicate later in the leaf, and the expected id is the first one's
    for L in leaves[:: max(1, len(leaves) // 50)]:
        m = n_tri // 2
        order = {int(t): p for p, t in enumerate(L["refs"])}
        for tri in L["want"][3][L["hit"]]:
            assert order[int(tri)] < order[(int(tri) + m) % n_tri]


@pytest.mark.gpu
@pytest.mark.parametrize("leaf_ordered", [False, True], ids=["refs", "leaf-ordered"])
def test_leaf_of_one_triangle_against_reference_at_every_scale(ctx, tri_gold, leaf_ordered):
    """tri_test_pk<true>, the re-test and the host-built record, one triangle at a time: every fixture row at every scale."""
    n_fallback_hits = 0
    for j, k in enumerate(SCALES):
        rows, ref = _rows_at(tri_gold, j), tri_gold["tri_out"][j]
        got = {f: np.zeros(256, F) for f in ("t", "beta", "gamma")}
        tri = np.zeros(256, np.int32)
        for i in range(256):
            h = ctx.leaf_intersect(rows[i, :9], np.concatenate([rows[i, 9:15], [np.inf]]), leaf_ordered=leaf_ordered)
            for f in got:
                got[f][i] = h[f][0]
            tri[i] = h["triangle"][0]
        with np.errstate(invalid="ignore"):
            hit = ref[:, 0] >= 0
        np.testing.assert_array_equal(tri, np.where(hit, 0, -1), err_msg=f"k = {k}")
        np.testing.assert_array_equal(_nan_bits(got["t"]), _nan_bits(np.where(hit, ref[:, 0], F(-1))), err_msg=f"k = {k}")
        np.testing.assert_array_equal(_nan_bits(got["beta"]), _nan_bits(np.where(hit, ref[:, 2], F(0))), err_msg=f"k = {k}")
        np.testing.assert_array_equal(_nan_bits(got["gamma"]), _nan_bits(np.where(hit, ref[:, 3], F(0))), err_msg=f"k = {k}")
        n_fallback_hits += int((hit & ~_in_range(_row_dets(tri_gold, j))).sum())
    assert n_fallback_hits >= 300      # hits that only the IEEE re-test can produce


@pytest.mark.gpu
@pytest.mark.parametrize("leaf_ordered", [False, True], ids=["refs", "leaf-ordered"])
@pytest.mark.parametrize("n_tri", [2, 8, 64])
def test_mixed_leaves_against_oracle(ctx, ora, tri_gold, n_tri, leaf_ordered):
    leaves = _mixed_cases(ora, tri_gold, n_tri)
    got = [ctx.leaf_intersect(L["corners"], L["rays"], refs=L["refs"], leaf_ordered=leaf_ordered) for L in leaves]
    fam = np.concatenate([[L["family"]] * len(L["rays"]) for L in leaves])
    for f, w in (("triangle", 3), ("t", 0), ("beta", 1), ("gamma", 2)):
        a = np.concatenate([h[f] for h in got])
        b = np.concatenate([L["want"][w] for L in leaves])
        if f != "triangle":
            a, b = _nan_bits(a), _nan_bits(b)
        bad = np.flatnonzero(a != b)
        assert len(bad) == 0, f"{f}: {len(bad)} of {len(a)} rays differ, first {bad[:5]} (families {fam[bad[:5]]}): got {a[bad[:5]]} want {b[bad[:5]]}"


@pytest.mark.gpu
def test_leaf_intersect_refusals_and_edges(ptx, ctx, tri_gold):
    L = ptx.lib()
    rows = _rows_at(tri_gold, SCALES.index(0))
    corners = np.ascontiguousarray(rows[:4, :9])
    rays = np.ascontiguousarray(np.concatenate([rows[:4, 9:15], np.full((4, 1), np.inf, F)], 1))
    out, tri = np.zeros((4, 3), F), np.zeros(4, np.int32)
    call = lambda c, n_tri, refs, r, n, o, t: L.ptx_leaf_intersect_batch(ctx.h, c, n_tri, refs, 0, r, n, o, t)
    P = lambda a: a.ctypes.data
    assert call(P(corners), 4, None, P(rays), 4, P(out), P(tri)) == ptx.OK
    assert call(P(corners), 4, None, P(rays), 0, None, None) == ptx.OK                        # an empty batch is a no-op
    assert call(None, 4, None, P(rays), 4, P(out), P(tri)) == ptx.ERR_INVALID
    assert call(P(corners), 4, None, None, 4, P(out), P(tri)) == ptx.ERR_INVALID
    assert call(P(corners), 4, None, P(rays), 4, None, P(tri)) == ptx.ERR_INVALID
    assert call(P(corners), 4, None, P(rays), 4, P(out), None) == ptx.ERR_INVALID
    assert call(P(corners), 0, None, P(rays), 4, P(out), P(tri)) == ptx.ERR_INVALID           # a leaf holds at least one triangle
    assert call(P(corners), 257, None, P(rays), 4, P(out), P(tri)) == ptx.ERR_INVALID         # and at most 256
    assert call(P(corners), 4, None, P(rays), 2 ** 31, P(out), P(tri)) == ptx.ERR_INVALID
    for bad in ([0, 1, 2, 4], [0, 1, 1, 2], [0xFFFFFFFF, 1, 2, 3]):                             # out of bounds, repeated
        assert call(P(corners), 4, P(np.array(bad, np.uint32)), P(rays), 4, P(out), P(tri)) == ptx.ERR_INVALID
    assert L.ptx_leaf_intersect_batch(None, P(corners), 4, None, 0, P(rays), 4, P(out), P(tri)) == ptx.ERR_NO_DEVICE
    with pytest.raises(ValueError):
        ctx.leaf_intersect(corners, rays, refs=[0, 1, 2])
    # 256 triangles, more rays than one workgroup, a ragged count; max_dist = 0, negative and NaN admit nothing but a hit at distance 0
    big = np.ascontiguousarray(np.tile(rows[:, :9], (1, 1)))
    n = 256 * 5 + 37
    rr = np.zeros((n, 7), F)
    rr[:, :6] = rows[np.arange(n) % 256, 9:15]
    rr[:, 6] = np.where(np.arange(n) % 3 == 0, np.inf, np.where(np.arange(n) % 3 == 1, F(-1), np.nan))
    for lo in (False, True):
        h = ctx.leaf_intersect(big, rr, refs=np.arange(256)[::-1].copy(), leaf_ordered=lo)
        assert (h["triangle"][np.arange(n) % 3 != 0] == -1).all() and (h["t"][np.arange(n) % 3 != 0] == -1).all()
        assert (h["triangle"][::3] >= 0).mean() > 0.5


# ---------------------------------------------------------------------------- 3. scaled scenes on every route
SCENE_SCALES = (-65, -64, -63, -62, -61, -60)
RW, RH, RSPP, RB = 64, 36, 2, 2
# Without switches the level-1 plaza (322 triangles) is LDS-resident; of the level-3 plaza (1 602) the ground and the small sphere are,
# and the large sphere stays in global memory with leaf-ordered records: the fused kernel then runs both copies of the leaf loop in one
# launch (lds_resident = 2). The other two routes are the forced routes of tests/_routes.py.
DEFAULT_ROUTE = {1: ("lds fused", 1), 3: ("hybrid fused", 2)}
_scene_cache = {}


def _scaled_plaza(level, k):
    d = _proc().plaza_scene(level=level, sun=True, alpha=False)
    s = _pow2(k)
    d["vertices"] = d["vertices"].copy(); d["vertices"][:, :3] *= s
    d["model_xform"] = d["model_xform"].copy(); d["model_xform"][:, :3] *= s
    d["camera"] = d["camera"].copy(); d["camera"][:3] *= s
    return d


def _scene_rays(ora, level, k):
    """(scene dict, oracle scene, rays [10 000, 6], oracle hit records, surface ids): 5 000 camera rays and 5 000 rays leaving the
    oracle's hit points, no offset, into the hemisphere of the shading normal."""
    if (level, k) not in _scene_cache:
        d = _scaled_plaza(level, k)
        o = oracle_from_dict(ora, d)
        prim = o.primary_rays(ora.make_cfg(100, 50, 1, RB), 0).reshape(-1, 6)
        out, idx = o.intersect(prim)
        rng = np.random.default_rng(100 * level + k + 70)
        sel = rng.choice(np.flatnonzero(idx >= 0), 5000, replace=True)
        dd = rng.standard_normal((5000, 3)).astype(F)
        dd /= np.linalg.norm(dd, axis=1, keepdims=True).astype(F)
        dd = np.where((dd * out[sel, 11:14]).sum(1, keepdims=True) < 0, -dd, dd).astype(F)
        rays = np.concatenate([prim, np.concatenate([out[sel, :3], dd], 1)]).astype(F)
        out, idx = o.intersect(rays)
        _scene_cache[(level, k)] = (d, o, rays, out, idx)
    return _scene_cache[(level, k)]


def _winner_dets(d, o, rays, idx):
    """The determinant of every winning triangle test: the ray's direction in the winning model's space (ray.cpp:10-15: normalize(inverse
    basis * dir), here in double, rounded once) against the winning triangle of model_intersect. One surface per model in these scenes."""
    hit = np.flatnonzero(idx >= 0)
    det = np.zeros(len(hit), F)
    for m in range(o.n_models):
        mo, mi = o.model_intersect(m, rays)
        sel = np.flatnonzero(idx[hit] == m)
        r = hit[sel]
        assert (mi[r, 0] == m).all()
        x = np.asarray(d["model_xform"][m], np.float64)
        dl = rays[r, 3:].astype(np.float64) @ np.linalg.inv(x[3:].reshape(3, 3).T).T
        dl = (dl / np.linalg.norm(dl, axis=1, keepdims=True)).astype(F)
        v0, _, t0, _ = (int(v) for v in d["surf_range"][m][:4])
        p = d["vertices"][v0 + d["triangles"][t0 + mi[r, 1]].astype(np.int64), :3]        # [n, 3 corners, 3]
        det[sel] = _det32(p[:, 0], p[:, 1], p[:, 2], dl)
    return det


@pytest.mark.parametrize("level", [1, 3])
def test_scaled_plaza_host_trees_and_oracle_coverage(ptx, ora, level):
    """The product's boxes and KD streams are the oracle's at every scale; the oracle still hits on more than half of the rays, and on
    at least three of the six scales at least 0.5 % of the winning hits go through a non-zero determinant outside rcp_core's range."""
    enough = 0
    for k in SCENE_SCALES + (0,):
        d, o, rays, out, idx = _scene_rays(ora, level, k)
        s = product_from_dict(ptx, None, d)
        assert s.info()["lds_resident"] == DEFAULT_ROUTE[level][1]
        mb, sb = o.boxes()
        np.testing.assert_array_equal(_nan_bits(s.array(ptx.ARR_MODEL_AABB)), _nan_bits(mb))
        np.testing.assert_array_equal(_nan_bits(s.array(ptx.ARR_MESH_AABB)), _nan_bits(sb))
        nodes, refs, rg = s.array(ptx.ARR_KD_NODES), s.array(ptx.ARR_KD_REFS), s.array(ptx.ARR_SURF_RANGE)
        for u in range(len(rg)):
            np.testing.assert_array_equal(kd_stream_packed(nodes, refs, rg[u, 4], int(rg[u, 2])), kd_stream_preorder(o.kd(u)), err_msg=f"k = {k}, surface {u}")
        assert (idx >= 0).mean() >= 0.5, (k, (idx >= 0).mean())
        assert np.isfinite(out[idx >= 0]).all()
        share = _out_nonzero(_winner_dets(d, o, rays, idx)).mean()
        if k == 0:
            assert share == 0
        elif share >= 0.005:
            enough += 1
    assert enough >= 3, enough


def _nan_class(h):
    """Hit records with every NaN replaced by one pattern: where the reference itself yields NaN, the class is compared, not the payload."""
    return {k: (np.where(np.isnan(v), F(np.nan), v).astype(F) if v.dtype == np.float32 else v) for k, v in h.items()}


@pytest.mark.gpu
@pytest.mark.parametrize("k", SCENE_SCALES + (0,))
@pytest.mark.parametrize("level", [1, 3])
def test_scaled_plaza_every_route_against_oracle(ptx, ctx, ora, clean_env, level, k):
    mp = clean_env
    d, o, rays, out, idx = _scene_rays(ora, level, k)
    out = np.where(np.isnan(out), F(np.nan), out).astype(F)
    hits0, frames0, rays0 = None, {}, {}
    for name, force_global, env, mode, pipeline in forced_routes(3):
        if not force_global:
            name, mode = DEFAULT_ROUTE[level]
        mp.setenv("PTX_WAVEFRONT", env["PTX_WAVEFRONT"])
        s = under_force_global(mp, force_global, lambda: product_from_dict(ptx, ctx, d))
        assert s.info()["lds_resident"] == mode, name
        hits = _nan_class(s.intersect(rays[:, :3], rays[:, 3:]))
        _check_records(hits, o, rays, out, idx)
        if hits0 is None:
            hits0 = hits
        else:
            _same_hits(hits, hits0, name)
        for ig in (0, 1):
            frame, st = s.render(RW, RH, RSPP, RB, integrator=ig)
            assert ctx.timing()["pipeline"] == pipeline, name
            assert np.isfinite(frame).all(), (name, ig)
            if ig not in frames0:
                frames0[ig], rays0[ig] = frame, st["rays"]
            else:
                np.testing.assert_array_equal(frame.view(np.uint32), frames0[ig].view(np.uint32), err_msg=f"{name} integrator {ig}")
                assert st["rays"] == rays0[ig], name
        s.close()
