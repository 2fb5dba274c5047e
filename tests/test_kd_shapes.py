"""Short walks for small LDS-resident KD trees (plan_residency's shape bits in SurfaceRec::lds_root, device_core.hpp: mesh_traverse_leaf and
mesh_traverse_complete).

A resident, leaf-ordered surface whose tree is a single leaf, or a complete tree (no branch lacks a child) of at most three branch levels,
is walked by a loop with the shape's constants folded in. The short walks compute what the general walk computes, expression for
expression, so everything is bit-identical between PTX_KD_SHAPES=0 (no shape bit is set: every walk is the general one) and =1.

  1. Host, no GPU: the bits against a brute-force recomputation from the node arrays, on the Cornell box and on a boundary set of small
     grids (the same meshes as tools/kd_shapes_check.cpp, where they were chosen) that must contain a qualifying tree at exactly three
     branch levels, a complete one at four, a shallow one with a missing child and a single leaf.
  2. GPU: Cornell frames and ray batches, a sun-lit half-transparent scene of the boundary meshes (shadow sweeps, eleven surfaces in one
     model: surface units), a hybrid scene (the boundary meshes resident, a sphere in global memory), under both settings; the boundary
     meshes and rays on the split planes / through the box corners of Cornell's white-wall tree also against the oracle's walk; rays
     along a strip with real volume whose tree has exactly three branch levels, which by the oracle's walk hold two and three pending
     entries and pop with three pending (the flat grids' boxes are 2e-4 thick: their walks set next to nothing aside).
"""
import functools

import numpy as np
import pytest

from _checks import _check_records, _same_hits
from _common import _proc
from _routes import ctx  # noqa: F401  (a fixture)
from conftest import CORNELL, oracle_from_dict, product_from_dict

F = np.float32
NOT_RESIDENT = 0xFFFFFFFF
VARS = ("PTX_KD_SHAPES", "PTX_LDS_LEAF_ORDER", "PTX_LDS_BUDGET", "PTX_WAVEFRONT", "PTX_FORCE_GLOBAL", "PTX_SURFACE_UNITS", "PTX_NO_HYBRID", "PTX_NO_HOT_HITREC")
FLAT, L, FIN, ZIG = 0, 1, 2, 3
# (nx, nz, kind): nx x nz quads of side 0.5 in a plane y = const; L: the quarter i >= nx // 2, j >= nz // 2 left out; FIN: one more quad 2 above
# the first cell; ZIG: the quads of a strip rise and fall by 0.5 in turn along z. Surface k lies at y = 4 k. A flat grid's box is 2e-4 thick,
# so the split distances of its tree hardly ever fall inside a ray's interval and its walks set next to nothing aside; the zigzag strips have
# boxes (and leaf boxes) of full extent on all axes: surface ZIG3 is the complete tree of exactly three branch levels whose walks hold one,
# two and three pending entries, ZIG4 its neighbour with one level more (general walk).
BOUNDARY = ((1, 1, FLAT), (1, 2, FLAT), (1, 4, FLAT), (1, 7, FLAT), (1, 8, FLAT), (2, 2, FLAT), (1, 1, FIN), (2, 2, L), (4, 4, FLAT), (1, 7, ZIG), (1, 8, ZIG))
ZIG3, ZIG4 = 9, 10
CORNELL_SHAPES = ("leaf", "leaf", "complete", None, "leaf", "complete", None)     # boxes, white walls, red wall, green wall, light, sphere


@pytest.fixture
def env(monkeypatch):
    for v in VARS:
        monkeypatch.delenv(v, raising=False)
    return monkeypatch


# ---------------------------------------------------------------------------- scenes (built once, never modified)
def _mesh(nx, nz, kind, y):
    quads = [(0.5 * i, y + (0.5 * (j % 2) if kind == ZIG else 0), 0.5 * j, 0.5 * (i + 1), y + (0.5 * (1 - j % 2) if kind == ZIG else 0), 0.5 * (j + 1))
             for i in range(nx) for j in range(nz) if not (kind == L and i >= nx // 2 and j >= nz // 2)]
    if kind == FIN:
        quads.append((0.0, y + 2.0, 0.0, 0.5, y + 2.0, 0.5))
    v = np.zeros((4 * len(quads), 11), F)
    v[:, 6] = 1.0                                       # normal +y
    v[:, 8] = 1.0                                       # tangent +x
    t = np.zeros((2 * len(quads), 3), np.uint32)
    for q, (x0, y0, z0, x1, y1, z1) in enumerate(quads):
        v[4 * q:4 * q + 4, :3] = [[x0, y0, z0], [x1, y0, z0], [x1, y1, z1], [x0, y1, z1]]
        t[2 * q:2 * q + 2] = np.array([[0, 2, 1], [0, 3, 2]]) + 4 * q
    return v, t


@functools.lru_cache(maxsize=None)
def _boundary(lit=False, sphere=False):
    """The boundary meshes as the surfaces of one model. lit: a sun, every second surface half-transparent and the lowest a shadow catcher.
    sphere: a second model, a 1280-triangle displaced icosphere beside the stack, too large for LDS beside the grids."""
    proc = _proc()
    vs, ts, rg, v0, t0 = [], [], [], 0, 0
    for k, (nx, nz, kind) in enumerate(BOUNDARY):
        v, t = _mesh(nx, nz, kind, 4.0 * k)
        vs.append(v); ts.append(t); rg.append([v0, len(v), t0, len(t)])
        v0 += len(v); t0 += len(t)
    mats = np.tile(np.array([0.8, 0.8, 0.8, 1, 0.5, 0, 0, 0, 0, 1.5, 0], F), (len(BOUNDARY), 1))
    xf, ms = [[0, 0, 0, 1, 0, 0, 0, 1, 0, 0, 0, 1]], [[0, len(BOUNDARY)]]
    if lit:
        mats[1::2, 3] = 0.55
        mats[0, 10] = 1.0
    if sphere:
        v, t = proc.displaced_icosphere(3, 4, 0.2)
        vs.append(v); ts.append(t); rg.append([v0, len(v), t0, len(t)])
        mats = np.concatenate([mats, [[0.95, 0.64, 0.54, 1.0, 0.25, 1.0, 0, 0, 0, 1.33, 0.0]]]).astype(F)
        xf.append([3.5, 14.0, 1.0, 2.0, 0, 0, 0, 2.0, 0, 0, 0, 2.0]); ms.append([len(BOUNDARY), 1])
    sun = None
    if lit:
        d = np.array([0.2, 0.9, 0.3]); d /= np.linalg.norm(d)
        x = np.cross([0, 1, 0], d); x /= np.linalg.norm(x)
        sun = np.concatenate([x, np.cross(d, x), d, [3.0, 2.7, 2.2], [0.004732]]).astype(F)
    cam = np.concatenate([proc._look_at([4.0, 52.0, 7.0], [1.0, 18.0, 1.5]), [F(0.5)]]).astype(F)
    out = dict(model_xform=np.array(xf, F), model_surf=np.array(ms, np.int32), surf_range=np.array(rg, np.int32), vertices=np.concatenate(vs).astype(F),
               triangles=np.concatenate(ts).astype(np.uint32), materials=mats.astype(F), camera=cam, sun=sun)
    for a in out.values():
        if a is not None:
            a.setflags(write=False)
    return out


def _brute(nodes, root):
    """-> (every branch has both children, branch nodes on the longest root-to-leaf path) by recursion over the packed nodes."""
    w1 = int(nodes[root, 1])
    if w1 & 3 == 3:
        return True, 0
    hl, hr, li = bool(w1 & 4), bool(w1 & 8), w1 >> 4
    kids = ([li] if hl else []) + ([li + (1 if hl else 0)] if hr else [])
    sub = [_brute(nodes, k) for k in kids]
    return hl and hr and all(c for c, _ in sub), 1 + max(l for _, l in sub)


def _classes(ptx, s, on=True):
    """Per surface: (shape bits as a name or None, complete, branch levels, leaf-ordered, resident), bits checked against the brute force
    (on: the scene was made with the shapes switched on and leaf-ordered layouts allowed; else no bit may be set)."""
    nodes, rg, shape, root = s.array(ptx.ARR_KD_NODES), s.array(ptx.ARR_SURF_RANGE), s.array(ptx.ARR_LDS_SHAPE), s.array(ptx.ARR_LDS_ROOT)
    out = []
    for u in range(len(rg)):
        w = int(shape[u])
        complete, levels = _brute(nodes, int(rg[u, 4]))             # a surface's root is its first node
        if w == NOT_RESIDENT:
            assert int(root[u]) == NOT_RESIDENT
            out.append((None, complete, levels, False, False))
            continue
        assert int(root[u]) == w & (ptx.LDS_ROOT_MASK | ptx.LDS_LEAF_ORDER_BIT), u          # ARR_LDS_ROOT stays the root and the layout bit
        lo = bool(w & ptx.LDS_LEAF_ORDER_BIT)
        want = None if not (lo and on) else "leaf" if levels == 0 else "complete" if complete and levels <= ptx.KD_SHAPE_MAX_BRANCH_LEVELS else None
        got = {0: None, ptx.LDS_LEAF_ONLY_BIT: "leaf", ptx.LDS_COMPLETE_BIT: "complete"}[w & (ptx.LDS_LEAF_ONLY_BIT | ptx.LDS_COMPLETE_BIT)]
        assert got == want, (u, hex(w), complete, levels)
        out.append((got, complete, levels, lo, True))
    return out


def _need_four_classes(cl):
    lim = 3
    lo = [c for c in cl if c[3]]                                     # a class counts only where the layout allows a shape bit
    assert any(c[0] == "complete" and c[2] == lim for c in lo), "no qualifying tree at exactly three branch levels"
    assert any(c[0] is None and c[1] and c[2] == lim + 1 for c in lo), "no complete tree at four branch levels"
    assert any(c[0] is None and not c[1] and 1 <= c[2] <= lim for c in lo), "no shallow tree with a missing child"
    assert any(c[0] == "leaf" and c[2] == 0 for c in lo), "no leaf-only tree"


def _pair(ptx, ctx, env, make, hybrid=False):
    """The scene made fresh under PTX_KD_SHAPES=0 and =1 -> {"0": scene, "1": scene}; the setting that was asked for is in effect."""
    out = {}
    env.setenv("PTX_WAVEFRONT", "0")                                  # the fused kernels: they hold the walks
    for v in ("0", "1"):
        env.setenv("PTX_KD_SHAPES", v)
        s = make()
        env.delenv("PTX_KD_SHAPES")
        cl = _classes(ptx, s, v == "1")
        assert any(c[0] for c in cl) == (v == "1"), (v, cl)
        assert s.info()["lds_resident"] == (2 if hybrid else 1)
        out[v] = s
    return out


def _render_and_batch(ptx, ctx, pair, W, H, spp, bounces, rays):
    res = {}
    for v, s in pair.items():
        frame, st = s.render(W, H, spp, bounces)
        assert ctx.timing()["pipeline"] == 0                          # the fused kernel, not the queue pipeline
        res[v] = (frame.copy(), st["rays"], s.intersect(rays[:, :3], rays[:, 3:]))
    assert res["0"][0].tobytes() == res["1"][0].tobytes() and res["0"][1] == res["1"][1]
    _same_hits(res["0"][2], res["1"][2], "PTX_KD_SHAPES=0 against =1")
    assert np.isfinite(res["1"][0]).all() and res["1"][1] > W * H * spp
    return res["1"]


def _stack_rays(n, seed, lo=(-0.5, -2.0, -0.5), hi=(4.5, 44.0, 4.5)):
    """Seeded rays among and around the stacked boundary meshes: origins in the box; three quarters aim at a point of a randomly chosen mesh's
    grid (and go on through the layers behind it), the rest anywhere."""
    rng = np.random.default_rng(seed)
    o = rng.uniform(lo, hi, (n, 3))
    d = rng.standard_normal((n, 3))
    k = rng.integers(0, len(BOUNDARY), n)
    ext = np.array([[0.5 * nx, 0.5 * nz] for nx, nz, _ in BOUNDARY])[k]
    aim = np.stack([ext[:, 0] * rng.random(n), 4.0 * k + 0.25 * (np.array([b[2] for b in BOUNDARY])[k] == ZIG), ext[:, 1] * rng.random(n)], 1)
    m = 3 * n // 4
    d[:m] = aim[:m] - o[:m]
    d /= np.linalg.norm(d, axis=1, keepdims=True)
    return np.concatenate([o, d], 1).astype(F)


def _strip_rays(n, seed, surface):
    """Seeded rays along a zigzag strip: origins in and just around its box, directions mostly along +z or -z with a small sideways part, so that
    a ray's interval in the box spans the split planes (all on z) of several levels and many rays pass under a rising quad without hitting it."""
    rng = np.random.default_rng(seed)
    nz, y = BOUNDARY[surface][1], 4.0 * surface
    o = rng.uniform((-0.1, y - 0.05, -0.3), (0.6, y + 0.55, 0.5 * nz + 0.3), (n, 3))
    d = 0.12 * rng.standard_normal((n, 3))
    d[:, 2] = np.where(rng.random(n) < 0.5, 1.0, -1.0)
    d /= np.linalg.norm(d, axis=1, keepdims=True)
    return np.concatenate([o, d], 1).astype(F)


def _strip_walk_facts(ptx, s, o, surface, rays):
    """What the oracle's walk (core::mesh::intersect with its stack) does on a zigzag strip: -> (most entries pending at once per ray, rays that
    popped while three were pending). Every split of the strip's tree is on z, so a leaf is an interval of z. A three-level tree holds three
    entries only at the first leaf it reaches, the one the ray's entry point lies in: a ray that held three and whose hit is none of that
    leaf's triangles, or that misses, has popped with three pending."""
    nodes, refs, rg, box = s.array(ptx.ARR_KD_NODES), s.array(ptx.ARR_KD_REFS), s.array(ptx.ARR_SURF_RANGE)[surface], s.array(ptx.ARR_MESH_AABB)[surface].astype(np.float64)
    leaves = []                                                     # (z from, z to, local triangle ids)

    def down(n, lo, hi):
        w0, w1 = int(nodes[n, 0]), int(nodes[n, 1])
        if w1 & 3 == 3:
            leaves.append((lo, hi, set((refs[w0:w0 + (w1 >> 2)].astype(np.int64) - int(rg[2])).tolist())))
            return
        assert w1 & 3 == 2 and w1 & 12 == 12, "a split off z, or a missing child"
        split = float(np.array([w0], np.uint32).view(F)[0])
        down(w1 >> 4, lo, split); down((w1 >> 4) + 1, split, hi)
    down(int(rg[4]), box[2], box[5])
    _, tri, depth, _ = o.mesh_intersect(surface, rays, stats=True)
    r = rays.astype(np.float64)
    with np.errstate(divide="ignore", invalid="ignore"):
        t0, t1 = (box[:3] - r[:, :3]) / r[:, 3:], (box[3:] - r[:, :3]) / r[:, 3:]
    z = r[:, 2] + np.maximum(np.minimum(t0, t1).max(1), 0.0) * r[:, 5]                                # where the ray enters the box, or starts in it
    popped3 = np.zeros(len(rays), bool)
    for lo, hi, tris in leaves:
        inside = (z > lo + 0.01) & (z < hi - 0.01)                                                   # the first leaf is not in doubt
        popped3 |= inside & (depth == 3) & ~np.isin(tri, list(tris))
    return depth, popped3


# ---------------------------------------------------------------------------- 1. the bits (no GPU)
def test_cornell_shape_bits(ptx, env):
    s = ptx.Scene.load_gltf(None, CORNELL)
    assert tuple(c[0] for c in _classes(ptx, s)) == CORNELL_SHAPES
    env.setenv("PTX_KD_SHAPES", "0")
    off = ptx.Scene.load_gltf(None, CORNELL)
    assert all(c[0] is None for c in _classes(ptx, off, False))
    for a in (ptx.ARR_LDS_ROOT, ptx.ARR_RES_NODES, ptx.ARR_RES_REFS, ptx.ARR_RES_TRIS, ptx.ARR_RES_PLAN):
        assert np.array_equal(s.array(a), off.array(a))                # the switch changes the bits and nothing else of the plan
    env.setenv("PTX_KD_SHAPES", "1")
    env.setenv("PTX_LDS_LEAF_ORDER", "0")
    assert all(c[0] is None for c in _classes(ptx, ptx.Scene.load_gltf(None, CORNELL), False))     # ref-indexed surfaces carry no shape


def test_boundary_meshes_contain_all_four_classes(ptx, env):
    cl = _classes(ptx, product_from_dict(ptx, None, _boundary()))
    assert all(c[4] for c in cl)
    _need_four_classes(cl)
    assert [(c[0], c[2]) for c in cl[:8]] == [("leaf", 0), ("complete", 2), ("complete", 3), ("complete", 3), (None, 4), (None, 4), (None, 2), (None, 4)]
    env.setenv("PTX_KD_SHAPES", "0")
    assert all(c[0] is None for c in _classes(ptx, product_from_dict(ptx, None, _boundary()), False))


# ---------------------------------------------------------------------------- 2. the kernels
def _cornell_rays(ptx, s, n=4096):
    """Seeded rays that start inside the room (the world box of the model with the three wall surfaces, shrunk by a tenth)."""
    ms, box, xf = s.array(ptx.ARR_MODEL_SURF), s.array(ptx.ARR_MODEL_AABB), s.array(ptx.ARR_MODEL_XFORM)
    room = int(np.argmax(ms[:, 1]))
    x = xf[room].astype(np.float64)
    corners = np.array([[box[room][3 * ((c >> a) & 1) + a] for a in range(3)] for c in range(8)], np.float64)
    world = corners @ x[3:].reshape(3, 3) + x[:3]
    lo, hi = world.min(0), world.max(0)
    mid, half = (lo + hi) / 2, (hi - lo) / 2 * 0.9
    rng = np.random.default_rng(4096)
    d = rng.standard_normal((n, 3))
    return np.concatenate([mid + half * rng.uniform(-1, 1, (n, 3)), d / np.linalg.norm(d, axis=1, keepdims=True)], 1).astype(F)


@pytest.mark.gpu
def test_cornell_frame_and_batch_are_the_same_with_and_without_shapes(ptx, ctx, env):
    pair = _pair(ptx, ctx, env, lambda: ptx.Scene.load_gltf(ctx, CORNELL))
    frame, rays, hits = _render_and_batch(ptx, ctx, pair, 96, 64, 2, 8, _cornell_rays(ptx, pair["1"]))
    assert (hits["surface"] >= 0).mean() > 0.95 and len(np.unique(hits["surface"])) >= 6


@pytest.mark.gpu
def test_sunlit_half_transparent_scene_is_the_same(ptx, ctx, env):
    d = _boundary(lit=True)
    pair = _pair(ptx, ctx, env, lambda: product_from_dict(ptx, ctx, d))
    assert pair["1"].info()["has_sun"] == 1
    frame, rays, hits = _render_and_batch(ptx, ctx, pair, 96, 64, 2, 8, _stack_rays(4096, 7))
    assert len(np.unique(hits["surface"][hits["surface"] >= 0])) == len(BOUNDARY)
    env.setenv("PTX_SURFACE_UNITS", "0")                              # and with whole models as the set-aside units
    _render_and_batch(ptx, ctx, pair, 96, 64, 2, 8, _stack_rays(512, 8))


@pytest.mark.gpu
def test_hybrid_scene_is_the_same(ptx, ctx, env):
    d = _boundary(lit=True, sphere=True)
    pair = _pair(ptx, ctx, env, lambda: product_from_dict(ptx, ctx, d), hybrid=True)
    cl = _classes(ptx, pair["1"])
    assert [c[4] for c in cl] == [True] * len(BOUNDARY) + [False]
    frame, rays, hits = _render_and_batch(ptx, ctx, pair, 96, 64, 2, 8, _stack_rays(4096, 9, hi=(6.0, 44.0, 4.5)))
    assert len(np.unique(hits["surface"][hits["surface"] >= 0])) == len(BOUNDARY) + 1


@pytest.mark.gpu
def test_boundary_meshes_against_the_oracle(ptx, ctx, ora, env):
    d = _boundary()
    pair = _pair(ptx, ctx, env, lambda: product_from_dict(ptx, ctx, d))
    _need_four_classes(_classes(ptx, pair["1"]))
    o = oracle_from_dict(ora, d)
    # seeded rays, and rays along the grid lines (x or z a multiple of 0.5: the split planes of these trees) straight down and up
    g = np.arange(0, 4.5, 0.5)
    gx, gz = np.meshgrid(g, g + 0.125, indexing="ij")
    down = np.stack([gx.ravel(), np.full(gx.size, 40.0), gz.ravel(), np.zeros(gx.size), np.full(gx.size, -1.0), np.zeros(gx.size)], 1)
    up = down * [1, 0, 1, 0, -1, 0] + [0, -3.0, 0, 0, 0, 0]
    side = down[:, [2, 1, 0, 3, 4, 5]]
    rays = np.concatenate([_stack_rays(4096, 11), down, up, side, side * [1, 0, 1, 0, -1, 0] + [0, -3.0, 0, 0, 0, 0]]).astype(F)
    out, idx = o.intersect(rays)
    assert len(np.unique(idx[idx >= 0])) == len(BOUNDARY)
    hits = {v: s.intersect(rays[:, :3], rays[:, 3:]) for v, s in pair.items()}
    _same_hits(hits["0"], hits["1"], "PTX_KD_SHAPES=0 against =1")
    _check_records(hits["1"], o, rays, out, idx)


@pytest.mark.gpu
def test_three_pending_entries_on_the_strip_at_exactly_three_levels(ptx, ctx, ora, env):
    """mesh_traverse_complete's register stack at the depth the shape allows: rays along the zigzag strip whose tree has exactly kRegStack
    branch levels. By the oracle's own walk, some of these rays hold two entries, some three, and some pop while three are pending (the
    rebuilt max_dist with the stack full); the test fails unless they do. The same rays on the strip with one level more take the general
    walk (up to four entries: the first spill row). Records bitwise between the settings and the oracle's."""
    d = _boundary()
    pair = _pair(ptx, ctx, env, lambda: product_from_dict(ptx, ctx, d))
    cl = _classes(ptx, pair["1"])
    assert cl[ZIG3][:3] == ("complete", True, 3) and cl[ZIG4][:4] == (None, True, 4, True)
    o = oracle_from_dict(ora, d)
    rays3, rays4 = _strip_rays(4096, 30, ZIG3), _strip_rays(4096, 31, ZIG4)
    depth3, popped3 = _strip_walk_facts(ptx, pair["1"], o, ZIG3, rays3)
    depth4, _ = _strip_walk_facts(ptx, pair["1"], o, ZIG4, rays4)
    print(f"pending entries on the three-level strip {np.bincount(depth3).tolist()}, popped with three pending {int(popped3.sum())}; "
          f"on the four-level strip {np.bincount(depth4).tolist()}")
    assert depth3.max() == 3 and (depth3 == 3).sum() >= 64 and (depth3 == 2).sum() >= 256 and (depth3 == 1).sum() >= 256
    assert popped3.sum() >= 16
    assert depth4.max() == 4 and (depth4 == 4).sum() >= 16
    rays = np.concatenate([rays3, rays4])
    out, idx = o.intersect(rays)
    assert (idx[:4096] == ZIG3).mean() > 0.4 and (idx[4096:] == ZIG4).mean() > 0.4
    hits = {v: s.intersect(rays[:, :3], rays[:, 3:]) for v, s in pair.items()}
    _same_hits(hits["0"], hits["1"], "PTX_KD_SHAPES=0 against =1")
    _check_records(hits["1"], o, rays, out, idx)
    # the rays that popped with three pending: what they went on to hit is the oracle's too (they are part of the comparison above)
    assert (hits["1"]["surface"][:4096][popped3] == idx[:4096][popped3]).all()


def _white_wall_planes(ptx, s):
    """The split planes of Cornell's white-wall tree (surface 2: seven nodes, two branch levels) as (axis, value), its box, and its model's
    transform, which must be the identity for local planes to be world planes."""
    nodes, rg, box = s.array(ptx.ARR_KD_NODES), s.array(ptx.ARR_SURF_RANGE), s.array(ptx.ARR_MESH_AABB)
    n0, nn = int(rg[2, 4]), int(rg[2, 5])
    assert nn == 7
    br = [(int(w1) & 3, float(np.array([w0], np.uint32).view(F)[0])) for w0, w1 in nodes[n0:n0 + nn] if int(w1) & 3 != 3]
    assert len(br) == 3
    return br, box[2].astype(np.float64)


def _plane_and_corner_rays(planes, box):
    rng = np.random.default_rng(12)
    lo, hi = box[:3], box[3:]
    rays = []
    for axis, value in planes:
        n = 256
        o = rng.uniform(lo + 0.05 * (hi - lo), hi - 0.05 * (hi - lo), (n, 3))
        dd = rng.standard_normal((n, 3))
        dd /= np.linalg.norm(dd, axis=1, keepdims=True)
        on = o.copy(); on[:, axis] = value                              # origin exactly on the plane
        for sign in (0.0, -0.0):
            flat = dd.copy(); flat[:, axis] = sign                      # direction parallel to the plane, +0 and -0 (normalising keeps the zero)
            flat /= np.linalg.norm(flat, axis=1, keepdims=True); flat[:, axis] = sign
            rays += [np.concatenate([o, flat], 1), np.concatenate([on, flat], 1)]          # the second: 0 / 0
        rays.append(np.concatenate([on, dd], 1))
        ax = np.zeros((n, 3)); ax[:, axis] = np.where(rng.random(n) < 0.5, 1.0, -1.0)
        rays.append(np.concatenate([on, ax], 1))                        # along the split axis from the plane: zeros on both other axes
    corners = np.array([[box[3 * ((c >> a) & 1) + a] for a in range(3)] for c in range(8)])
    mid = (lo + hi) / 2
    for c in corners:
        for back in (1.0, 3.0):
            for toward in (mid, lo + (hi - lo) * rng.random(3), lo + (hi - lo) * rng.random(3)):
                dirn = toward - c
                dirn /= np.linalg.norm(dirn)
                rays.append(np.concatenate([c - back * dirn, dirn])[None])       # from outside, through the corner, into the box
        for a in range(3):                                             # along the box edges that meet in the corner
            e = np.zeros(3); e[a] = 1.0 if c[a] == lo[a] else -1.0
            rays.append(np.concatenate([c - 2.0 * e, e])[None])
    rays = np.concatenate(rays).astype(F)
    for axis, value in planes:
        assert ((rays[:, axis] == F(value)) & (rays[:, 3 + axis] == 0)).sum() >= 512          # the 0 / 0 rays are in the set
        assert (np.signbit(rays[:, 3 + axis]) & (rays[:, 3 + axis] == 0)).sum() >= 256        # ... and the -0 directions
    return rays


@pytest.mark.gpu
def test_rays_on_the_split_planes_and_through_the_corners_of_the_white_walls(ptx, ctx, ora, cornell_oracle, env):
    """Where a folded constant could hide a difference: origins exactly on a split plane, directions with +0 or -0 on the split axis, both at
    once (split_dist = 0 / 0), and rays that enter the surface's box through its corners and edges."""
    pair = _pair(ptx, ctx, env, lambda: ptx.Scene.load_gltf(ctx, CORNELL))
    s = pair["1"]
    planes, box = _white_wall_planes(ptx, s)
    xf = s.array(ptx.ARR_MODEL_XFORM)[int(np.flatnonzero([a <= 2 < a + b for a, b in s.array(ptx.ARR_MODEL_SURF)])[0])]
    assert xf.tolist() == [0, 0, 0, 1, 0, 0, 0, 1, 0, 0, 0, 1]          # the room is not transformed: its local planes are world planes
    assert sorted(round(v, 4) for _, v in planes)[0] > 0 and {round(v, 5) for _, v in planes} >= {5.35352, 2.15235}
    rays = _plane_and_corner_rays(planes, box)
    out, idx = cornell_oracle.intersect(rays)
    assert (idx == 2).sum() > 200
    hits = {v: sc.intersect(rays[:, :3], rays[:, 3:]) for v, sc in pair.items()}
    _same_hits(hits["0"], hits["1"], "PTX_KD_SHAPES=0 against =1")
    _check_records(hits["1"], cornell_oracle, rays, out, idx)
