"""The stackless walk of chain trees (kd_chain_shape's flag in the auxiliary surface table, device_core.hpp: mesh_traverse_chain).

A resident, leaf-ordered surface whose tree is a chain — every node from the root down is a branch with exactly one child, a leaf at the end;
zero branches is the single leaf — is walked level by level without a stack. The walk computes what the general walk computes on such a tree,
so everything is bit-identical between PTX_KD_SHAPES=0 (no flag, no shape bit: every walk is the general one) and =1.

Which chains the reference's builder makes. A one-child branch is an empty-space cut at an end of the event list (mesh.cpp:148-241). The cut
below all triangles is `min - epsilon`, which IS the root box's lower bound and is refused (`split <= box.lo`), and the same holds in the one
child of every chain level: its box keeps that bound. So no chain of this builder has a branch that keeps only its RIGHT child (checked below
on every mesh tried here; the walk reads the side from the node all the same). Cuts above all triangles exist where aabb::clear()'s upper
bound, the smallest positive float, stays above a mesh at negative coordinates: the box then reaches up to 0 and the cut keeps only the LEFT
child, once per axis on which the whole mesh is negative. Hence chains of one level (Cornell's red wall, the walls below), of two and of
three (the tilted quads in a negative quadrant and octant); deeper ones do not occur at these sizes. Both outcomes of `child is first` /
`child is second` are reached from the two sides of the cut plane.

  1. Host, no GPU: the flag against a brute-force reading of ARR_KD_NODES on Cornell and on the small meshes.
  2. GPU: hit records under both settings, bitwise, and against the oracle, on 4096-ray batches with origins on the cut planes, +-0 on the cut
     axis, split distances equal to the walk's bounds, rays through the boxes' corners and along their edges; a restatement of the
     three-way decision on the CPU proves that each (child side, case) outcome is taken by at least 16 rays. One Cornell frame per setting.
"""
import functools

import numpy as np
import pytest

from _checks import _check_records, _same_hits
from _routes import ctx  # noqa: F401  (a fixture)
from conftest import CORNELL, oracle_from_dict, product_from_dict

F = np.float32
NOT_RESIDENT = 0xFFFFFFFF
VARS = ("PTX_KD_SHAPES", "PTX_LDS_LEAF_ORDER", "PTX_LDS_BUDGET", "PTX_WAVEFRONT", "PTX_FORCE_GLOBAL", "PTX_SURFACE_UNITS", "PTX_NO_HYBRID", "PTX_NO_HOT_HITREC")
CORNELL_CHAINS = (0, 0, None, 1, 0, None, None)      # boxes, white walls, red wall, green wall, light, sphere: chain levels, None = no chain
# the small meshes: (corners of a quad a b c d, expected chain levels). Walls on each axis at negative coordinates; a tilted quad negative
# on two axes and one negative on all three; walls at positive coordinates (single leaves); a two-quad mesh whose tree is no chain.
QUADS = ((((-1, 0, 0), (-1, 2, 0), (-1, 2, 3), (-1, 0, 3)), 1),
         (((0, -2, 0), (0, -2, 3), (2, -2, 3), (2, -2, 0)), 1),
         (((0, 0, -1.5), (2, 0, -1.5), (2, 3, -1.5), (0, 3, -1.5)), 1),
         (((-3, -3, 1), (-1, -3, 1), (-1, -1, 2), (-3, -1, 2)), 2),
         (((-3, -3, -3), (-1, -3, -2.5), (-1, -1, -1), (-3, -1, -1.5)), 3),
         (((1, 0, 0), (1, 2, 0), (1, 2, 3), (1, 0, 3)), 0),
         (((0.5, 1, 0.5), (2.5, 1, 0.5), (2.5, 1.5, 2.5), (0.5, 1.5, 2.5)), 0))
# (the meshes keep these coordinates — the chains depend on them — and share one model, where they cross each other harmlessly)


@pytest.fixture
def env(monkeypatch):
    for v in VARS:
        monkeypatch.delenv(v, raising=False)
    return monkeypatch


@functools.lru_cache(maxsize=None)
def _meshes():
    """The quads as the surfaces of one untransformed model, and a last surface of two far-apart quads (a tree with a two-child root)."""
    vs, ts, rg, v0, t0 = [], [], [], 0, 0
    sets = [[q] for q, _ in QUADS] + [[((-4, -4, -4), (-3.5, -4, -4), (-3.5, -3.5, -4), (-4, -3.5, -4)), ((-1, -1, -0.5), (-0.5, -1, -0.5), (-0.5, -0.5, -0.5), (-1, -0.5, -0.5))]]
    for quads in sets:
        v = np.zeros((4 * len(quads), 11), F)
        v[:, 6] = 1.0
        v[:, 8] = 1.0
        t = np.zeros((2 * len(quads), 3), np.uint32)
        for q, corners in enumerate(quads):
            v[4 * q:4 * q + 4, :3] = corners
            t[2 * q:2 * q + 2] = np.array([[0, 2, 1], [0, 3, 2]]) + 4 * q
        vs.append(v); ts.append(t); rg.append([v0, len(v), t0, len(t)])
        v0 += len(v); t0 += len(t)
    n = len(sets)
    mats = np.tile(np.array([0.8, 0.8, 0.8, 1, 0.5, 0, 0, 0, 0, 1.5, 0], F), (n, 1))
    cam = np.array([0, 0, 10, 1, 0, 0, 0, 1, 0, 0, 0, 1, 0.5], F)
    out = dict(model_xform=np.array([[0, 0, 0, 1, 0, 0, 0, 1, 0, 0, 0, 1]], F), model_surf=np.array([[0, n]], np.int32), surf_range=np.array(rg, np.int32),
               vertices=np.concatenate(vs), triangles=np.concatenate(ts), materials=mats, camera=cam, sun=None)
    for a in out.values():
        if a is not None:
            a.setflags(write=False)
    return out


def _brute_chain(nodes, root):
    """-> [(keeps 'L' or 'R', axis, split)] per branch level when the tree at `root` is a chain, else None."""
    n, levels = root, []
    while True:
        w0, w1 = int(nodes[n, 0]), int(nodes[n, 1])
        if w1 & 3 == 3:
            return levels
        if w1 & 12 not in (4, 8):
            return None
        levels.append(("L" if w1 & 12 == 4 else "R", w1 & 3, float(np.array([w0], np.uint32).view(F)[0])))
        n = w1 >> 4


def _chains(ptx, s, on=True):
    """Per surface the brute-force chain (or None), with the flag of ARR_SURF_AUX checked against it: set exactly on resident, leaf-ordered
    chains of a scene made with the shapes switched on."""
    nodes, rg, root, aux = s.array(ptx.ARR_KD_NODES), s.array(ptx.ARR_SURF_RANGE), s.array(ptx.ARR_LDS_SHAPE), s.array(ptx.ARR_SURF_AUX)
    out = []
    for u in range(len(rg)):
        ch = _brute_chain(nodes, int(rg[u, 4]))
        w = int(root[u])
        want = on and ch is not None and w != NOT_RESIDENT and bool(w & ptx.LDS_LEAF_ORDER_BIT)
        assert bool(int(aux[u, 0]) & ptx.AUX_CHAIN_BIT) == want, (u, ch, hex(w), int(aux[u, 0]))
        if want and not ch:
            assert w & ptx.LDS_LEAF_ONLY_BIT                       # a chain of zero levels is the single leaf of the shape bits
        out.append(ch)
    return out


# ---------------------------------------------------------------------------- 1. the flag (no GPU)
def test_cornell_chain_flags(ptx, env):
    s = ptx.Scene.load_gltf(None, CORNELL)
    ch = _chains(ptx, s)
    assert tuple(None if c is None else len(c) for c in ch) == CORNELL_CHAINS
    assert ch[3][0][0] == "L"                                        # the red wall: a left child only, above one leaf
    env.setenv("PTX_KD_SHAPES", "0")
    off = ptx.Scene.load_gltf(None, CORNELL)
    _chains(ptx, off, False)
    for a in (ptx.ARR_LDS_ROOT, ptx.ARR_RES_NODES, ptx.ARR_RES_REFS, ptx.ARR_RES_TRIS, ptx.ARR_RES_PLAN):
        assert np.array_equal(s.array(a), off.array(a))                # the switch changes the flags and nothing of the plan
    env.setenv("PTX_KD_SHAPES", "1")
    env.setenv("PTX_LDS_LEAF_ORDER", "0")
    _chains(ptx, ptx.Scene.load_gltf(None, CORNELL), False)            # ref-indexed surfaces carry no flag


def test_small_mesh_chain_flags(ptx, env):
    d = _meshes()
    ch = _chains(ptx, product_from_dict(ptx, None, d))
    assert [None if c is None else len(c) for c in ch] == [lv for _, lv in QUADS] + [None]
    sides = {lv[0] for c in ch if c for lv in c}
    assert sides == {"L"}, sides                                       # the builder makes no right-only cut (module docstring)
    assert {lv[1] for c in ch if c for lv in c} == {0, 1, 2}           # cuts on every axis
    env.setenv("PTX_KD_SHAPES", "0")
    _chains(ptx, product_from_dict(ptx, None, d), False)


# ---------------------------------------------------------------------------- 2. the kernels
def _f32_div(a, b):
    with np.errstate(divide="ignore", invalid="ignore"):
        return (a.astype(F) / b.astype(F)).astype(F)


def _walk_outcomes(ora, box, chain, rays):
    """mesh_traverse's three-way decision restated per chain level, in float32: -> int [n, levels], -1 = the ray never reaches the level (it
    misses the box or an earlier level ended its walk), else 3 * (child is second) + case - 1 with the cases of the decision in its order:
    1 `split_dist < 0 || split_dist > max_dist`, 2 `split_dist < min_dist`, 3 neither. The bounds start as the box's entry and exit."""
    n = len(rays)
    inp = np.concatenate([np.tile(box.astype(F), (n, 1)), rays.astype(F)], 1)
    ab = ora.aabb_intersect(inp)
    alive = ab[:, 0] > 0
    mn, mx = ab[:, 1].astype(F).copy(), ab[:, 2].astype(F).copy()
    out = np.full((n, len(chain)), -1, np.int64)
    for lv, (side, axis, split) in enumerate(chain):
        oa, da = rays[:, axis].astype(F), rays[:, 3 + axis].astype(F)
        sd = _f32_div(F(split) - oa, da)
        left_first = oa < F(split)
        child_first = left_first == (side == "L")
        with np.errstate(invalid="ignore"):
            case = np.where((sd < 0) | (sd > mx), 1, np.where(sd < mn, 2, 3))
        out[alive, lv] = (3 * (~child_first) + case - 1)[alive]
        ends = (child_first & (case == 2)) | (~child_first & (case == 1))
        cut_far, cut_near = alive & child_first & (case == 3), alive & ~child_first & (case == 3)
        mx = np.where(cut_far, sd, mx).astype(F)
        mn = np.where(cut_near, sd, mn).astype(F)
        alive = alive & ~ends
    return out


def _special_rays(box, chain, rng, n):
    """Rays aimed at where a folded constant could hide a difference on one chain surface."""
    lo, hi = box[:3].astype(np.float64), box[3:].astype(np.float64)
    ext = hi - lo
    rays = []

    def unit(d):
        return d / np.linalg.norm(d, axis=1, keepdims=True)
    inside = lambda k: lo + ext * rng.random((k, 3))                     # noqa: E731
    around = lambda k: lo - 0.5 * ext.max() + (ext + ext.max()) * rng.random((k, 3))   # noqa: E731
    # seeded rays from around the box towards points inside it, and from inside it anywhere
    o = around(n); rays.append(np.concatenate([o, unit(inside(n) - o)], 1))
    rays.append(np.concatenate([inside(n), unit(rng.standard_normal((n, 3)))], 1))
    for side, axis, split in chain:
        k = n // 4
        on = inside(k); on[:, axis] = split                               # origin exactly on the cut plane
        dd = unit(rng.standard_normal((k, 3)))
        rays.append(np.concatenate([on, dd], 1))
        for zero in (0.0, -0.0):                                          # +-0 on the cut axis, from beside the plane and from on it (0 / 0)
            flat = dd.copy(); flat[:, axis] = 0; flat = unit(flat); flat[:, axis] = zero
            rays += [np.concatenate([inside(k), flat], 1), np.concatenate([on, flat], 1)]
        ax = np.zeros((k, 3)); ax[:, axis] = np.where(rng.random(k) < 0.5, 1.0, -1.0)
        rays.append(np.concatenate([around(k), ax], 1))                   # along the cut axis: zeros on both other axes
        # the child's side of the cut is a thin slab (an empty-space cut sits 1e-4 beside the triangles). From inside the slab, any direction:
        # the rays that move away from the plane never meet it (child first, case 1). Towards points where the slab meets the box's faces of
        # the other axes, from anywhere: a ray from the far side meets the plane before it enters the box (child second, case 2).
        s0, s1 = (lo[axis], split) if side == "L" else (split, hi[axis])
        slab = inside(4 * k); slab[:, axis] = s0 + (s1 - s0) * rng.random(4 * k)
        rays.append(np.concatenate([slab, unit(rng.standard_normal((4 * k, 3)))], 1))
        for other in ((axis + 1) % 3, (axis + 2) % 3):
            low = rng.random(k) < 0.5                                       # the face the ray enters through; its origin lies outside that face
            p = inside(k); p[:, axis] = s0 + (s1 - s0) * rng.random(k); p[:, other] = np.where(low, lo[other], hi[other])
            o = around(k); o[:, other] = np.where(low, lo[other] - ext.max() * rng.random(k), hi[other] + ext.max() * rng.random(k))
            rays.append(np.concatenate([o, unit(p - o)], 1))
        # split_dist equal to a bound: the ray meets the cut plane exactly where it enters or leaves the box through a face of another axis
        for face in (lo, hi):
            for other in ((axis + 1) % 3, (axis + 2) % 3):
                p = inside(k); p[:, axis] = split; p[:, other] = face[other]     # a point of the cut plane on that face
                o = around(k)
                out = np.arange(k) % 2 == 0                                     # every second origin outside that face: the ray enters there
                o[out, other] = (face[other] + (-1.0 if face is lo else 1.0) * ext.max() * (0.05 + rng.random(k)))[out]
                rays.append(np.concatenate([o, unit(p - o)], 1))
    corners = np.array([[(hi if (c >> a) & 1 else lo)[a] for a in range(3)] for c in range(8)])
    for c in corners:
        for back in (1.0, 3.0):
            for toward in ((lo + hi) / 2, *inside(3)):
                dirn = toward - c; dirn /= np.linalg.norm(dirn)
                rays.append(np.concatenate([c - back * dirn, dirn])[None])         # from outside, through the corner, into the box
        for a in range(3):                                                 # along the box edges that meet in the corner
            e = np.zeros(3); e[a] = 1.0 if c[a] == lo[a] else -1.0
            rays.append(np.concatenate([c - 2.0 * e, e])[None])
    return np.concatenate(rays).astype(F)


def _equal_bound_rays(ora, box, chain, rays):
    """Of `rays`, nudged by a few ulps of the origin along the first cut axis until the first level's split_dist EQUALS the walk's min_dist
    or max_dist in float32: -> (rays whose split_dist == min_dist, rays whose split_dist == max_dist)."""
    side, axis, split = chain[0]
    found = {0: [], 1: []}
    for ulps in range(-6, 7):
        r = rays.copy()
        bits = r[:, axis].view(np.int32) + ulps
        r[:, axis] = bits.view(F)
        ab = ora.aabb_intersect(np.concatenate([np.tile(box.astype(F), (len(r), 1)), r], 1))
        sd = _f32_div(F(split) - r[:, axis], r[:, 3 + axis])
        for which in (0, 1):
            found[which].append(r[(ab[:, 0] > 0) & (sd == ab[:, 1 + which])])
    return np.concatenate(found[0]), np.concatenate(found[1])


@functools.lru_cache(maxsize=None)
def _chain_batch(n_total=4096):
    """-> (rays [n_total, 6], {surface: outcome table}) for the small meshes: special rays per chain surface, filled up with seeded ones."""
    import importlib
    ptx = importlib.import_module("distributed-path-tracer_amd")
    from oracle import pt_oracle as ora
    d = _meshes()
    s = product_from_dict(ptx, None, d)
    box, chains = s.array(ptx.ARR_MESH_AABB), _chains(ptx, s)
    rng = np.random.default_rng(2024)
    parts = []
    for u, ch in enumerate(chains):
        if not ch:
            continue
        sp = _special_rays(box[u], ch, rng, 64)
        eq_min, eq_max = _equal_bound_rays(ora, box[u], ch, sp)
        parts += [sp, eq_min[:32], eq_max[:32]]
    rays = np.concatenate(parts)
    assert len(rays) <= n_total, len(rays)
    lo, hi = box[:, :3].min(0).astype(np.float64), box[:, 3:].max(0).astype(np.float64)
    k = n_total - len(rays)
    o = lo - 1 + (hi - lo + 2) * rng.random((k, 3))
    t = lo + (hi - lo) * rng.random((k, 3))
    fill = np.concatenate([o, (t - o) / np.linalg.norm(t - o, axis=1, keepdims=True)], 1).astype(F)
    rays = np.concatenate([rays, fill])
    rays.setflags(write=False)
    return rays


def test_every_outcome_of_the_decision_is_taken(ptx, ora, env):
    """On the CPU: the batch the kernels are given takes each of the six (child side, case) outcomes at least 16 times on every chain surface's
    first level and over the deeper levels together, holds origins on the cut planes with +-0 directions (0 / 0), and holds rays whose
    split_dist equals min_dist and max_dist."""
    d = _meshes()
    s = product_from_dict(ptx, None, d)
    box, chains, rays = s.array(ptx.ARR_MESH_AABB), _chains(ptx, s), _chain_batch()
    assert len(rays) == 4096
    deeper = np.zeros(6, np.int64)
    for u, ch in enumerate(chains):
        if not ch:
            continue
        oc = _walk_outcomes(ora, box[u], ch, rays)
        first = np.bincount(oc[:, 0][oc[:, 0] >= 0], minlength=6)
        print(f"surface {u}: levels {len(ch)}, first-level outcomes (first 1 2 3, second 1 2 3) {first.tolist()}")
        assert (first >= 16).all(), (u, first.tolist())
        for lv in range(1, len(ch)):
            deeper += np.bincount(oc[:, lv][oc[:, lv] >= 0], minlength=6)
        side, axis, split = ch[0]
        zero = rays[:, 3 + axis] == 0
        assert ((rays[:, axis] == F(split)) & zero).sum() >= 32 and (zero & np.signbit(rays[:, 3 + axis])).sum() >= 32
        ab = ora.aabb_intersect(np.concatenate([np.tile(box[u].astype(F), (len(rays), 1)), rays], 1))
        sd = _f32_div(F(split) - rays[:, axis], rays[:, 3 + axis])
        eq_min, eq_max = ((ab[:, 0] > 0) & (sd == ab[:, 1])).sum(), ((ab[:, 0] > 0) & (sd == ab[:, 2])).sum()
        print(f"  split_dist == min_dist on {eq_min} rays, == max_dist on {eq_max}")
        assert eq_min >= 16 and eq_max >= 16, (u, eq_min, eq_max)
    print(f"deeper levels together {deeper.tolist()}")
    assert (deeper >= 16).all(), deeper.tolist()


def _pair(ptx, ctx, env, make):
    """The scene made fresh under PTX_KD_SHAPES=0 and =1 -> {"0": scene, "1": scene}, all resident, the flags as asked for."""
    out = {}
    env.setenv("PTX_WAVEFRONT", "0")                                  # the fused kernels: they hold the walks
    for v in ("0", "1"):
        env.setenv("PTX_KD_SHAPES", v)
        s = make()
        env.delenv("PTX_KD_SHAPES")
        ch = _chains(ptx, s, v == "1")
        assert any(c is not None and len(c) > 0 for c in ch)
        assert bool((s.array(ptx.ARR_SURF_AUX)[:, 0] & ptx.AUX_CHAIN_BIT).any()) == (v == "1")
        assert s.info()["lds_resident"] == 1
        out[v] = s
    return out


@pytest.mark.gpu
def test_small_mesh_chains_against_the_oracle(ptx, ctx, ora, env):
    d = _meshes()
    pair = _pair(ptx, ctx, env, lambda: product_from_dict(ptx, ctx, d))
    o = oracle_from_dict(ora, d)
    rays = np.array(_chain_batch())
    out, idx = o.intersect(rays)
    assert len(np.unique(idx[idx >= 0])) == len(QUADS) + 1
    hits = {v: s.intersect(rays[:, :3], rays[:, 3:]) for v, s in pair.items()}
    _same_hits(hits["0"], hits["1"], "PTX_KD_SHAPES=0 against =1")
    _check_records(hits["1"], o, rays, out, idx)


def _red_wall_rays(ptx, ora, s):
    """4096 rays for Cornell's red wall (surface 3, whose model is not transformed): the special rays of its chain, the equal-bound rays, and
    seeded rays from inside the room."""
    box, ch = s.array(ptx.ARR_MESH_AABB)[3], _brute_chain(s.array(ptx.ARR_KD_NODES), int(s.array(ptx.ARR_SURF_RANGE)[3, 4]))
    rng = np.random.default_rng(77)
    sp = _special_rays(box, ch, rng, 256)
    eq_min, eq_max = _equal_bound_rays(ora, box, ch, sp)
    rays = np.concatenate([sp, eq_min[:128], eq_max[:128]])
    k = 4096 - len(rays)
    assert k > 0
    room = s.array(ptx.ARR_MESH_AABB)[2].astype(np.float64)
    mid, half = (room[:3] + room[3:]) / 2, (room[3:] - room[:3]) / 2 * 0.9
    dd = rng.standard_normal((k, 3))
    rays = np.concatenate([rays, np.concatenate([mid + half * rng.uniform(-1, 1, (k, 3)), dd / np.linalg.norm(dd, axis=1, keepdims=True)], 1).astype(F)])
    oc = _walk_outcomes(ora, box, ch, rays)[:, 0]
    return rays, np.bincount(oc[oc >= 0], minlength=6), (eq_min, eq_max)


@pytest.mark.gpu
def test_cornell_red_wall_batch_and_frame_with_and_without_shapes(ptx, ctx, ora, cornell_oracle, env):
    pair = _pair(ptx, ctx, env, lambda: ptx.Scene.load_gltf(ctx, CORNELL))
    s = pair["1"]
    xf = s.array(ptx.ARR_MODEL_XFORM)[int(np.flatnonzero([a <= 3 < a + b for a, b in s.array(ptx.ARR_MODEL_SURF)])[0])]
    assert xf.tolist() == [0, 0, 0, 1, 0, 0, 0, 1, 0, 0, 0, 1]          # the room is not transformed: local rays are world rays
    rays, first, (eq_min, eq_max) = _red_wall_rays(ptx, ora, s)
    print(f"red wall outcomes (first 1 2 3, second 1 2 3) {first.tolist()}; split_dist == min_dist on {len(eq_min)} candidates, == max_dist on {len(eq_max)}")
    assert len(rays) == 4096 and (first >= 16).all() and len(eq_min) >= 16 and len(eq_max) >= 16
    out, idx = cornell_oracle.intersect(rays)
    assert (idx == 3).sum() > 200
    res = {}
    for v, sc in pair.items():
        frame, st = sc.render(96, 64, 2, 8)
        assert ctx.timing()["pipeline"] == 0                          # the fused kernel, not the queue pipeline
        res[v] = (frame.copy(), st["rays"], sc.intersect(rays[:, :3], rays[:, 3:]))
    assert res["0"][0].tobytes() == res["1"][0].tobytes() and res["0"][1] == res["1"][1]
    assert np.isfinite(res["1"][0]).all() and res["1"][1] > 96 * 64 * 2
    _same_hits(res["0"][2], res["1"][2], "PTX_KD_SHAPES=0 against =1")
    _check_records(res["1"][2], cornell_oracle, rays, out, idx)
