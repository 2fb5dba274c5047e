"""The light tree over ptx_render_nee's light list on the MI355X (include/ptx.h: LIGHT PICK; csrc/nee_core.hpp light_pick_tree and
light_pmf_tree, which the LTREE variants of nee_candidate and nee_vertex and k_light_pick / k_light_pmf inline). The yardstick is
tests/_nee_light_tree_restatement.py: the tree, the pick, the directed pmf and the tree-mode vertex loop, which tests/test_nee_light_tree.py
pins to the unchanged tests/_nee_estimator.py in CDF mode; that file is the CPU side.

Bars are the project's: bitwise equality against the restatement for the batches, between the two forms, between routes and against the
calls a frame is composed of; the per-sample bar of tests/test_nee_lights.py (_nee_common._err: >= 99.5 % of the samples within 1e-3, the
counts within 0.5 % + 1) against the restated loop; _nee_common's statistic for the expectation; 2 * R0 for the variance.
"""
import json
import os
import subprocess

import numpy as np
import pytest

import _adaptive_restatement as AR
import _nee_light_tree_restatement as LT
from _common import _bits, _proc, _same
from _fused_motion_common import Routed, with_motion
from _motion_common import movers as _movers
from _nee_common import K_BATCH, SAME_STATS, SEED, _batch_stat, _err, _pair, _same_expectation
from _nee_light_tree_scenes import restated, scene_dict
from _nee_lit_scenes import CAND, CLOUDS, ENV, FUSED, LIT_LOADS, NO_LIGHTS, SKY, SPDF, _new_scene, _variance_ratio
from _routes import clean_env, ctx  # noqa: F401  (fixtures)
from _routes import DEFAULT_ROUTES, Scenes, forced_routes, on_route, resident_by_creation, route_named, under_force_global, use_route
from conftest import CORNELL, ROOT, oracle_from_dict, product_from_dict

f32 = np.float32
pytestmark = pytest.mark.gpu
BLACK = (0.0, 0.0, 0.0)
LAMPS = f32([[0.5, 2.0, 1.0, 0, 0, -1, 0, 0, 6, 5, 4, 0, 0, 0, 0, 0], [-1.0, 1.5, 2.0, 0, 0, -1, 0, 0, 2, 3, 4, 0, 0, 0, 0, 0],
             [1.5, 2.5, -1.0, 0, 0, -1, 0, 0, 3, 3, 3, 0, 0, 0, 0, 0]])


def _make(ptx, ctx, name, tree=True):
    """name: a case of tests/test_nee_light_tree.py, "cornell", a load of lit.gltf or an emitter cloud; "+sky" sets the golden sky as the map,
    "+lamps" three punctual lights"""
    base, *opts = name.split("+")
    if base in LIT_LOADS or base in CLOUDS or base == "cornell":
        s = _new_scene(ptx, base, ctx, (SKY, False) if "sky" in opts else None)
    else:
        s = product_from_dict(ptx, ctx, scene_dict(base))
        if "sky" in opts:
            s.set_environment(SKY, srgb=False)
    if "lamps" in opts:
        s.set_punctual_lights(LAMPS)
    if tree:
        s.set_light_pick("tree")
    return s


PRODUCTS = Scenes(_make)                                                    # tree mode
CDF_PRODUCTS = Scenes(lambda ptx, ctx, name: _make(ptx, ctx, name, False))  # the same scenes as the parent renders them


def _route(ptx, ctx, mp, name, route, scenes=PRODUCTS):
    r = route_named(DEFAULT_ROUTES if route == "queue" else forced_routes(1), route)   # the fused routes are asked for: PTX_WAVEFRONT=0
    return on_route(scenes, ptx, ctx, mp, name, r, resident_by_creation), r.pipeline


def _samples(ptx, ctx, s, W, H, spp, b, flags, pipeline, **kw):
    """per-sample radiance [H, W, spp, 3] from one call per sample, the route asserted on every call -> (radiance, summed stats)"""
    got = np.zeros((H, W, spp, 3), f32)
    tot = dict(light_samples=0, light_visible=0, rays=0)
    for k in range(spp):
        acc, st = s.render_nee(W, H, 1, b, seed=SEED, sample0=k, flags=flags, **kw)
        tm = ctx.timing()
        assert tm["pipeline"] == pipeline and tm["fused_launches"] == (1 if pipeline == 0 and flags & FUSED else 0), tm
        got[:, :, k] = acc[..., :3]
        for key in tot:
            tot[key] += st[key]
    return got, tot


# ---------------------------------------------------------------------------- 1. the batches
def _probe_points(T, cen, rng, n=4096):
    """n random positions around the tree's box, then every centroid and the centre of every node's box, with u drawn at random, 0 and the
    largest float below 1"""
    lo, hi = T[0, 0:3].view(f32), T[0, 4:7].view(f32)
    span = np.maximum(hi - lo, f32(1))
    x = (lo - span + rng.random((n, 3)) * (hi - lo + 2 * span)).astype(f32)
    x = np.concatenate([x, cen.astype(f32), LT.branch_centres(T)]).astype(f32)
    x = np.concatenate([x, x[n:], x[n:]])                      # the special positions three times: u random, 0 and just below 1
    m = len(x) - n
    u = rng.random(len(x)).astype(f32)
    u[0], u[1] = 0, LT.ONE_BELOW
    u[n + m // 3:n + 2 * (m // 3)] = 0
    u[n + 2 * (m // 3):] = LT.ONE_BELOW
    return np.concatenate([x, u[:, None]], 1).astype(f32)


@pytest.mark.parametrize("name", ["1 triangle", "3 triangles", "field32", "cloud"])
def test_pick_and_pmf_batches_are_the_restatement_bit_for_bit(ptx, ctx, ora, clean_env, name):
    """ptx_light_pick_batch and ptx_light_pmf_batch (the device functions the integrators inline) against the restatement on lists of 1, 3,
    64 and 271 triangles: the entry and every bit of the pmf, for 4096 random positions plus every centroid and the centre of every node's
    box, u random, 0 and 0x1.fffffep-1; the directed pmf of the picked entry is the pick's pmf, and of a random entry the restated walk;
    host and device pointers; CDF mode against the stored CDF; every refusal."""
    import torch
    s, _ = _route(ptx, ctx, clean_env, name, "lds fused")
    _, a, ll, T, path = restated(ora, name)
    np.testing.assert_array_equal(s.array(ptx.ARR_LIGHT_TREE), T)
    np.testing.assert_array_equal(s.array(ptx.ARR_LIGHT_PATH).reshape(-1), path)
    rng = np.random.default_rng(11)
    pu = _probe_points(T, LT.leaves(a, ll)[0], rng)
    want_k, want_p = LT.pick(T, pu[:, :3], pu[:, 3])
    k, p = s.light_pick_batch(pu)
    print(f"{name}: {len(pu)} picks, {int((k != want_k).sum())} entries differ, {int((_bits(p) != _bits(want_p)).sum())} pmfs differ in a bit; smallest pmf {p.min():.3g}")
    np.testing.assert_array_equal(k, want_k)
    _same(p, want_p, f"{name}: pmf")
    assert (p > 0).all() and (p <= 1).all()
    _same(s.light_pmf_batch(pu[:, :3], k), p, f"{name}: the directed pmf of the picked entry")
    other = rng.integers(0, len(path), len(pu)).astype(np.int32)
    _same(s.light_pmf_batch(pu[:, :3], other), LT.pmf(T, path, other, pu[:, :3]), f"{name}: the directed pmf of a random entry")
    if len(path) == 1:
        assert (k == 0).all() and (p == f32(1)).all()
    # device pointers
    d_in = torch.from_numpy(pu).cuda()
    d_x, d_o = torch.from_numpy(np.ascontiguousarray(pu[:, :3])).cuda(), torch.from_numpy(other).cuda()
    d_k, d_p = torch.zeros(len(pu), dtype=torch.int32, device="cuda"), torch.zeros(len(pu), dtype=torch.float32, device="cuda")
    d_q = torch.zeros(len(pu), dtype=torch.float32, device="cuda")
    torch.cuda.synchronize()   # the copies and fills run on torch's stream, the library on its own
    L = ptx.lib()
    assert L.ptx_light_pick_batch(s.h, d_in.data_ptr(), len(pu), d_k.data_ptr(), d_p.data_ptr()) == 0
    assert L.ptx_light_pmf_batch(s.h, d_x.data_ptr(), d_o.data_ptr(), len(pu), d_q.data_ptr()) == 0
    ctx.synchronize()
    np.testing.assert_array_equal(d_k.cpu().numpy(), want_k)
    _same(d_p.cpu().numpy(), want_p, f"{name}: pmf, device pointers")
    _same(d_q.cpu().numpy(), LT.pmf(T, path, other, pu[:, :3]), f"{name}: directed pmf, device pointers")
    # refusals
    x3, q = np.ascontiguousarray(pu[:, :3]), np.zeros(len(pu), f32)
    assert L.ptx_light_pick_batch(s.h, pu.ctypes.data, len(pu), d_k.data_ptr(), d_p.data_ptr()) == ptx.ERR_INVALID      # mixed kinds
    assert L.ptx_light_pmf_batch(s.h, x3.ctypes.data, d_o.data_ptr(), len(pu), q.ctypes.data) == ptx.ERR_INVALID
    assert L.ptx_light_pick_batch(s.h, None, len(pu), k.ctypes.data, p.ctypes.data) == ptx.ERR_INVALID
    assert L.ptx_light_pick_batch(s.h, pu.ctypes.data, len(pu), None, p.ctypes.data) == ptx.ERR_INVALID
    assert L.ptx_light_pmf_batch(s.h, x3.ctypes.data, None, len(pu), q.ctypes.data) == ptx.ERR_INVALID
    assert L.ptx_light_pmf_batch(s.h, x3.ctypes.data, other.ctypes.data, len(pu), None) == ptx.ERR_INVALID
    assert L.ptx_light_pick_batch(s.h, None, 0, None, None) == 0 and L.ptx_light_pmf_batch(s.h, None, None, 0, None) == 0
    for bad in (-1, len(path)):
        outside = other.copy()
        outside[7] = bad
        assert L.ptx_light_pmf_batch(s.h, x3.ctypes.data, outside.ctypes.data, len(pu), q.ctypes.data) == ptx.ERR_INVALID
    # CDF mode: the position plays no part
    c, _ = _route(ptx, ctx, clean_env, name, "lds fused", CDF_PRODUCTS)
    assert len(c.array(ptx.ARR_LIGHT_TREE)) == 0 and len(c.array(ptx.ARR_LIGHT_PATH)) == 0
    ck, cp = c.light_pick_batch(pu)
    wk, wp = LT.cdf_pick(c.array(ptx.ARR_LIGHT_CDF), pu[:, 3])
    np.testing.assert_array_equal(ck, wk)
    _same(cp, wp, f"{name}: CDF mode")
    _same(c.light_pmf_batch(pu[:, :3], ck), wp, f"{name}: CDF mode, directed")


def test_batches_refuse_an_empty_list(ptx, ctx, clean_env):
    s = product_from_dict(ptx, ctx, _proc().lamp_scene(1)[0])
    s.set_light_pick("tree")
    pu, x, k, p = np.zeros((2, 4), f32), np.zeros((2, 3), f32), np.zeros(2, np.int32), np.zeros(2, f32)
    assert ptx.lib().ptx_light_pick_batch(s.h, pu.ctypes.data, 2, k.ctypes.data, p.ctypes.data) == ptx.ERR_INVALID
    assert ptx.lib().ptx_light_pmf_batch(s.h, x.ctypes.data, k.ctypes.data, 2, p.ctypes.data) == ptx.ERR_INVALID
    s.close()


# ---------------------------------------------------------------------------- 2. per-sample radiance against the restated loop
_refs = {}


def _ref(ora, name, W, H, spp, b, M, spdf):
    key = (name, W, H, spp, b, M, spdf)
    if key not in _refs:
        o, a, ll, T, path = restated(ora, name)
        r = LT.render_samples(ora, o, a, W, H, spp, b, tree=(T, path), M=M, spdf=spdf, seed=SEED)
        r["rad"].setflags(write=False)
        _refs[key] = r
    return _refs[key]


@pytest.mark.parametrize("route", ["lds fused", "global fused", "queue"])
@pytest.mark.parametrize("M,spdf", [(1, False), (1, True), (2, False), (16, True)])
def test_per_sample_radiance_is_the_restated_loop(ptx, ctx, ora, clean_env, route, M, spdf):
    """ptx_render_nee in tree mode on emitter_field_scene(16), 16 x 12, 2 samples, 3 bounces, sample by sample against the restated tree-mode
    loop, in both forms (on the queue route PTX_NEE_FUSED is ignored): tests/test_nee_lights.py's bar (_err: >= 99.5 % of the samples within
    1e-3 relative with a floor of 1e-3, light samples and rays within 0.5 % + 1).
    Measured on the MI355X: every sample within 1e-3 on every route, form and flag set (worst 2.2e-7); light samples, visible ones and
    rays equal to the restated counts."""
    W, H, spp, b = 16, 12, 2, 3
    ref = _ref(ora, "field16", W, H, spp, b, M, spdf)
    s, pipeline = _route(ptx, ctx, clean_env, "field16", route)
    flags = CAND(M) | (SPDF if spdf else 0)
    for form in (0, FUSED):
        got, tot = _samples(ptx, ctx, s, W, H, spp, b, flags | form, pipeline)
        assert np.isfinite(got).all() and (got >= 0).all()
        e = _err(got, ref["rad"])
        share = (e <= 1e-3).mean()
        print(f"{route} / M {M} / spdf {spdf} / form {form}: {share * 100:.3f} % of samples within 1e-3, worst {e.max():.3g}; light samples "
              f"{tot['light_samples']} (restated {ref['light_samples']}), visible {tot['light_visible']} ({ref['light_visible']}), rays {tot['rays']} ({ref['rays']})")
        assert ref["light_samples"] > 0 and share >= 0.995
        assert abs(tot["light_samples"] - ref["light_samples"]) <= 0.005 * ref["light_samples"] + 1
        assert abs(tot["rays"] - ref["rays"]) <= 0.005 * ref["rays"] + 1


@pytest.mark.parametrize("form", [0, FUSED], ids=["unfused", "fused"])
def test_first_triangle_sample_bitwise_in_tree_mode(ptx, ctx, ora, clean_env, form):
    """tests/test_nee.py's construction (2 bounces, black environment, no unlisted emitter, no sun) on emitter_field_scene(16) in tree mode:
    a sample whose vertex 1 is not on a listed emitter is vertex 0's emission plus the vertex-0 light term: the picked triangle, its pmf
    and x enter every bit, and no ocml trigonometry lies on that path. That test's bar: <= 0.5 % of the comparable samples may differ in a
    bit, the counts within 0.5 % + 1."""
    W, H, spp = 32, 24, 4
    o, a, ll, T, path = restated(ora, "field16")
    first = {}
    ref = LT.render_samples(ora, o, a, W, H, spp, 2, tree=(T, path), seed=SEED, env=BLACK, first=first)
    s, pipeline = _route(ptx, ctx, clean_env, "field16", "lds fused")
    # the triangle of every contributing depth-0 sample: the product's pick from the restated vertex position and r.x is the restated
    # (exp_surf, exp_tri), and its pmf the restated one, bit for bit (no entry point returns a sample's exp_surf / exp_tri itself)
    k, p = s.light_pick_batch(np.concatenate([first["pos"], first["u"][:, None]], 1))
    assert len(k) > 500
    np.testing.assert_array_equal(s.array(ptx.ARR_LIGHT_TRIS)[k], np.stack([first["surf"], first["tri"]], 1).astype(np.uint32))
    _same(p, LT.pmf(T, path, k, first["pos"]), "the pmf of the first triangle sample")
    got, tot = _samples(ptx, ctx, s, W, H, spp, 2, form, pipeline, env=BLACK)
    sel = ~ref["v1_listed"]
    assert sel.mean() >= 0.5
    differ = (_bits(got) != _bits(ref["rad"])).any(-1) & sel
    print(f"form {form}: {differ.sum()} of {sel.sum()} comparable samples differ; light samples {tot['light_samples']} (restated {ref['light_samples']}), "
          f"visible {tot['light_visible']} (restated {ref['light_visible']})")
    assert ref["light_visible"] > 0 and differ.sum() <= 0.005 * sel.sum()
    assert abs(tot["light_samples"] - ref["light_samples"]) <= 0.005 * ref["light_samples"] + 1
    assert abs(tot["rays"] - ref["rays"]) <= 0.005 * ref["rays"] + 1


# ---------------------------------------------------------------------------- 3. fused against unfused on the LTREE variants
# the eight TEX x ALPHA x SUN loads, and their twins under a map (a map implies the TEX variants); with and without SPDF, candidates, lamps
FUSED_LOADS = sorted(CLOUDS) + [n for n in sorted(LIT_LOADS) if n != "lit_first"]
PLAIN_SETS = [(0, 1), (SPDF, 1), (0, 4), (SPDF, 3)]        # the four (SPDF, RIS) parts, as test_nee_punctual_gpu.py's LOAD_SETS
MAP_SETS = [(flags | ENV, M) for flags, M in PLAIN_SETS]


@pytest.mark.parametrize("route", ["lds fused", "global fused"])
@pytest.mark.parametrize("name", FUSED_LOADS)
def test_fused_is_unfused_bitwise_in_tree_mode(ptx, ctx, clean_env, name, route):
    """every LTREE variant of k_nee_fused against k_nee_shade's: frame and stats bitwise (_nee_common._pair). The eight loads are the eight
    TEX x ALPHA x SUN scene masks, the lit loads under the sky their four ENV twins: 12 scene masks; each runs the four (SPDF, RIS) parts
    without lamps and the four with three lamps on the scene (PUN): 8 parts, 96 masks, on two places of the geometry (LDS, global); the
    hybrid place runs the cloud's four parts below. V = 237 and 239, which run at 256 threads, are lit_opaque and lit under the sky with
    lamps at (ENV, 4). And the tree-mode frame is not the CDF-mode frame."""
    W, H, spp, b = 24, 16, 2, 3
    for opts, sets in (("", PLAIN_SETS), ("+lamps", PLAIN_SETS)) + ((("+sky", MAP_SETS), ("+sky+lamps", MAP_SETS)) if name in LIT_LOADS else ()):
        s, _ = _route(ptx, ctx, clean_env, name + opts, route)
        assert len(s.array(ptx.ARR_LIGHT_TREE)) == 2 * len(s.array(ptx.ARR_LIGHT_CDF)) - 1 > 0
        for flags, M in sets:
            got, st = _pair(ptx, ctx, s, W, H, spp, b, flags=flags | CAND(M))
            assert st["light_samples"] > 0, (name, opts, flags, M, st)
        if not opts:
            c, _ = _route(ptx, ctx, clean_env, name, route, CDF_PRODUCTS)
            assert (_bits(c.render_nee(W, H, spp, b, seed=SEED, flags=FUSED)[0]) != _bits(s.render_nee(W, H, spp, b, seed=SEED, flags=FUSED)[0])).any()


def test_fused_is_unfused_bitwise_on_a_hybrid_scene_in_tree_mode(ptx, ctx, clean_env):
    """the third place of the geometry: the cloud with one byte too little LDS for all of its surfaces"""
    d = scene_dict("cloud")
    R = Routed(ptx, ctx, clean_env, "hybrid", d)
    s = R.make(d)
    s.set_light_pick("tree")
    for flags, M in PLAIN_SETS:
        _pair(ptx, ctx, s, 24, 16, 2, 3, flags=flags | CAND(M))
    s.close()


# ---------------------------------------------------------------------------- 4. the identities
@pytest.mark.parametrize("route", ["lds fused", "global fused", "queue"])
def test_one_triangle_is_the_cdf_frame_bitwise(ptx, ctx, clean_env, route):
    """with one listed triangle the root is its leaf, pmf = 1.0F, and A_0 == A_total: the tree-mode frame is the CDF-mode frame bit for
    bit, stats included, in both forms"""
    W, H, spp, b = 32, 24, 4, 3
    t, pipeline = _route(ptx, ctx, clean_env, "1 triangle", route)
    c, _ = _route(ptx, ctx, clean_env, "1 triangle", route, CDF_PRODUCTS)
    assert len(t.array(ptx.ARR_LIGHT_TREE)) == 1 and t.get_light_pick() == "tree" and c.get_light_pick() == "cdf"
    for flags in (0, FUSED, SPDF | CAND(4) | FUSED):
        want, st0 = c.render_nee(W, H, spp, b, seed=SEED, flags=flags)
        got, st = t.render_nee(W, H, spp, b, seed=SEED, flags=flags)
        assert ctx.timing()["pipeline"] == pipeline
        _same(got, want, f"{route} / {flags}")
        assert all(st[k] == st0[k] for k in SAME_STATS) and st["light_visible"] > 0, (st, st0)


@pytest.mark.parametrize("route", [r.name for r in DEFAULT_ROUTES])
def test_off_means_off(ptx, ctx, clean_env, route):
    """Set to TREE and back to CDF: bitwise a scene never given the setter, stats included. An empty list in tree mode, and
    PTX_NEE_NO_LIGHT_SAMPLES on a listed scene in tree mode: bitwise the CDF mode's, which is ptx_render's estimator."""
    W, H, spp, b = 32, 24, 4, 3
    r = route_named(DEFAULT_ROUTES, route)
    d, bare_d = scene_dict("field16"), _proc().lamp_scene(1)[0]

    def fresh(dd):
        return under_force_global(clean_env, r.force_global, lambda: product_from_dict(ptx, ctx, dd))
    never, back, bare, bare_tree = fresh(d), fresh(d), fresh(bare_d), fresh(bare_d)
    for k, v in r.env.items():
        clean_env.setenv(k, v)
    back.set_light_pick("tree")
    in_tree, _ = back.render_nee(W, H, spp, b, seed=SEED)
    no_lights_tree, st_t = back.render_nee(W, H, spp, b, seed=SEED, flags=NO_LIGHTS | FUSED)
    back.set_light_pick("cdf")
    bare_tree.set_light_pick("tree")
    plain, st_p = never.render(W, H, spp, b, seed=SEED)
    _same(no_lights_tree, plain, f"{route}: PTX_NEE_NO_LIGHT_SAMPLES in tree mode against ptx_render")
    assert st_t["rays"] == st_p["rays"] and st_t["light_samples"] == 0
    for flags in (0, FUSED, SPDF | CAND(4), SPDF | CAND(4) | FUSED):
        want, st0 = never.render_nee(W, H, spp, b, seed=SEED, flags=flags)
        assert ctx.timing()["pipeline"] == r.pipeline
        got, st = back.render_nee(W, H, spp, b, seed=SEED, flags=flags)
        _same(got, want, f"{route} / {flags}: back in CDF mode")
        assert all(st[k] == st0[k] for k in SAME_STATS), (st, st0)
        if flags == 0:
            assert (_bits(in_tree) != _bits(want)).any()
        want, st0 = bare.render_nee(W, H, spp, b, seed=SEED, flags=flags)
        got, st = bare_tree.render_nee(W, H, spp, b, seed=SEED, flags=flags)
        tm = ctx.timing()
        _same(got, want, f"{route} / {flags}: an empty list, tree mode")
        assert all(st[k] == st0[k] for k in SAME_STATS), (st, st0)
        assert tm["fused_launches"] == (st["passes"] if r.pipeline == 0 and flags & FUSED else 0), tm
        _same(got, bare.render(W, H, spp, b, seed=SEED)[0], f"{route} / {flags}: an empty list against ptx_render")
    for s in (never, back, bare, bare_tree):
        s.close()


# ---------------------------------------------------------------------------- 5. composition
def test_composition_in_tree_mode(ptx, ctx, clean_env):
    """tiles, two sample ranges, passes of 3, 64 and 129 paths, two and three shards, a device buffer and the queue route with a forced
    pool overflow, on emitter_field_scene(16) with SPDF and four candidates in tree mode"""
    import torch
    s, _ = _route(ptx, ctx, clean_env, "field16", "lds fused")
    W, H, spp, b, F = 24, 16, 8, 3, FUSED | SPDF | CAND(4)
    whole, st0 = s.render_nee(W, H, spp, b, seed=SEED, flags=SPDF | CAND(4))
    tiles = np.zeros_like(whole)
    for (x0, y0, w, h) in [(0, 0, 9, 16), (9, 0, 15, 7), (9, 7, 15, 9)]:
        tiles[y0:y0 + h, x0:x0 + w] = s.render_nee(W, H, spp, b, seed=SEED, tile=(x0, y0, w, h), flags=F)[0]
    _same(tiles, whole, "tiles")
    two, _ = s.render_nee(W, H, 3, b, seed=SEED, flags=F)
    two, _ = s.render_nee(W, H, 5, b, seed=SEED, sample0=3, accum=two, flags=F)
    _same(two, whole, "two sample ranges")
    for form in (0, FUSED):
        for (x0, y0, w, h) in [(2, 3, 3, 1), (0, 0, 8, 8), (1, 1, 43, 3)]:      # with one sample a pass: 3, 64 and 129 paths
            one = s.render_nee(W * 2, H, 2, b, seed=SEED, tile=(x0, y0, w, h), spp_per_pass=1, flags=F & ~FUSED | form)[0]
            ref = s.render_nee(W * 2, H, 2, b, seed=SEED, tile=(x0, y0, w, h), flags=SPDF | CAND(4))[0]
            _same(one, ref, f"passes of {w * h} paths, form {form}")
    for n in (2, 3):
        shards = sum(s.render_nee(W, H, spp, b, seed=SEED, shard=(k, n, 8), flags=F)[0] for k in range(n))
        _same(shards, whole, f"{n} shards")
    dev = torch.zeros((H, W, 4), dtype=torch.float32, device="cuda")
    torch.cuda.synchronize()   # the fill runs on torch's stream, the library on its own
    s.render_nee(W, H, spp, b, accum=dev, seed=SEED, flags=F)
    _same(dev.cpu().numpy(), whole, "device buffer")
    q, pipeline = _route(ptx, ctx, clean_env, "field16", "queue")
    assert pipeline == 1
    got, _ = _pair(ptx, ctx, q, W, H, spp, b, fused=False, flags=SPDF | CAND(4))
    _same(got, whole, "queue route")


def test_queue_route_with_a_forced_pool_overflow_in_tree_mode(ptx, ctx, clean_env):
    """the queue frame with a 1 Mi-pair pool that 800 x 600 x 4 camera rays overflow is the 'lds fused' frame bit for bit, stats included
    (the frame is as large as tests/test_nee_punctual_gpu.py's: the pool overflows only with more than 2^20 pairs in a slice)"""
    W, H, spp, b = 800, 600, 4, 2
    s, _ = _route(ptx, ctx, clean_env, "field16", "lds fused")
    want, st0 = s.render_nee(W, H, spp, b, seed=SEED)
    fresh = under_force_global(clean_env, True, lambda: _make(ptx, ctx, "field16"))
    use_route(clean_env, route_named(DEFAULT_ROUTES, "queue"))      # the product's own choice of pipeline: no PTX_WAVEFRONT at the call
    clean_env.setenv("PTX_WF_PAIRS_M", "1")
    clean_env.setenv("PTX_WF_RATIO_GUESS", "0.25")
    forced, st = fresh.render_nee(W, H, spp, b, seed=SEED)
    tm = ctx.timing()
    fresh.close()
    assert tm["pipeline"] == 1 and tm["pool_overflows"] >= 1, tm
    _same(forced, want, "queue, forced overflow, against lds fused")
    assert all(st[k] == st0[k] for k in SAME_STATS) and st0["light_samples"] > 0, (st, st0)


@pytest.mark.parametrize("route,flags", [("lds fused", FUSED), ("queue", CAND(4))])
def test_adaptive_in_tree_mode_is_the_calls_of_the_half_ranges(ptx, ctx, clean_env, route, flags):
    """tests/test_adaptive_nee.py's snapshot method on emitter_field_scene(16) in tree mode, 32 x 24, 3 bounces, 8 samples first, 8 per
    round, cap 24: a pixel with n samples holds, in A and in B, what the ptx_render_nee calls of the same half ranges leave"""
    W, H, b, cap, thr = 32, 24, 3, 24, 0.2
    s, pipeline = _route(ptx, ctx, clean_env, "field16", route)
    a, bb = np.zeros((H, W, 4), f32), np.zeros((H, W, 4), f32)
    snaps, given = [], 0
    for k in AR.round_sizes(cap, 8, 8):
        s.render_nee(W, H, k // 2, b, accum=a, seed=SEED, sample0=given, want_stats=False, flags=flags)
        s.render_nee(W, H, k // 2, b, accum=bb, seed=SEED, sample0=given + k // 2, want_stats=False, flags=flags)
        given += k
        snaps.append((a.copy(), bb.copy()))
    want_a, want_b, want_rounds, want_last = AR.replay(snaps, thr)
    got_a, got_b, st = s.render_adaptive_nee(W, H, cap, b, 8, 8, thr, seed=SEED, flags=flags)
    tm = ctx.timing()
    _same(got_a, want_a, f"{route}: A"), _same(got_b, want_b, f"{route}: B")
    assert st["rounds"] == want_rounds and st["active_last"] == want_last and st["light_samples"] > 0, st
    assert tm["pipeline"] == pipeline and tm["fused_launches"] == (st["passes"] if pipeline == 0 and flags & FUSED else 0), (tm, st)


# ---------------------------------------------------------------------------- 6. under a shutter
def test_under_a_shutter_the_unfused_form_runs_the_tree(ptx, ctx, clean_env):
    """The movers in tree mode. A degenerate shutter (open == close == 1, the motion active) against the static twin: the unfused tree
    frame bit for bit. PTX_NEE_FUSED | PTX_NEE_FUSED_MOTION under an open shutter falls back as PTX_NEE_FUSED alone does
    (fused_launches == 0) and is bitwise the unfused frame; the tree-mode frame is not the CDF-mode frame."""
    d = _movers()
    R = Routed(ptx, ctx, clean_env, "lds fused", d)
    W, H, spp, b = 16, 12, 3, 3
    static = R.make(d)
    static.set_light_pick("tree")
    want, wst = static.render_nee(W, H, spp, b, seed=SEED)
    assert len(static.array(ptx.ARR_LIGHT_TREE)) > 0
    deg = with_motion(R, d, (1.0, 1.0))
    deg.set_light_pick("tree")
    assert deg.array(ptx.ARR_MOTION_MOVED).any()
    got, gst = deg.render_nee(W, H, spp, b, seed=SEED)
    np.testing.assert_array_equal(deg.array(ptx.ARR_LIGHT_TREE), static.array(ptx.ARR_LIGHT_TREE))   # no listed emitter moves
    _same(got, want, "a degenerate shutter against the static twin")
    assert all(gst[k] == wst[k] for k in SAME_STATS) and gst["light_samples"] > 0, (gst, wst)
    a = with_motion(R, d, (0.2, 0.9))
    a.set_light_pick("tree")
    fm = ptx.NEE_FUSED | ptx.NEE_FUSED_MOTION
    for flags in (0, SPDF | CAND(4)):
        want, wst = a.render_nee(W, H, spp, b, seed=SEED, flags=flags)
        assert ctx.timing()["fused_launches"] == 0
        got, gst = a.render_nee(W, H, spp, b, seed=SEED, flags=flags | fm)
        assert ctx.timing()["fused_launches"] == 0                       # ignored: k_nee_fused_motion has no tree variants
        _same(got, want, f"PTX_NEE_FUSED | PTX_NEE_FUSED_MOTION in tree mode / {flags}")
        assert all(gst[k] == wst[k] for k in SAME_STATS) and gst["light_samples"] > 0, (gst, wst)
    tree, _ = a.render_nee(W, H, spp, b, seed=SEED, flags=fm)
    a.set_light_pick("cdf")
    cdf, cst = a.render_nee(W, H, spp, b, seed=SEED, flags=fm)
    assert ctx.timing()["fused_launches"] == cst["passes"] >= 1          # back in CDF mode the motion kernel runs
    assert (_bits(cdf) != _bits(tree)).any()
    for s in (static, deg, a):
        s.close()


# ---------------------------------------------------------------------------- 7. expectation and variance
@pytest.mark.parametrize("name", ["field16", "cornell", "cloud_opaque_nosun+sky+lamps"])
def test_tree_mode_has_the_cdf_modes_expectation(ptx, ctx, clean_env, name):
    """16 batches of 16 spp in tree mode against 16 of other seeds in CDF mode, 32 x 24, 3 bounces, _nee_common's statistic with its own
    bars; the third scene has punctual lights and an environment table beside the tree (ENV, PUN and LTREE together).
    Measured on the MI355X, worst z frame / quadrant: field16 0.75 / 1.30, cornell 0.55 / 0.60, the cloud under the sky with lamps 1.70 / 3.55."""
    W, H, b = 32, 24, 3
    flags = FUSED | (ENV if "sky" in name else 0)
    t, _ = _route(ptx, ctx, clean_env, name, "lds fused")
    c, _ = _route(ptx, ctx, clean_env, name, "lds fused", CDF_PRODUCTS)

    def batches(s, seed0):
        return _batch_stat(np.stack([s.render_nee(W, H, 16, b, seed=seed0 + k, flags=flags)[0][..., :3] / f32(16) for k in range(K_BATCH)]))
    ok, zf, zq = _same_expectation(batches(t, 0xA000), batches(c, 0xB000))
    print(f"{name}: tree against CDF mode, worst z frame {zf:.2f} quadrant {zq:.2f}")
    assert ok, (zf, zq)


def test_variance_against_the_restatements_ratio(ptx, ctx, clean_env):
    """LT.VARIANCE_CASE (emitter_field_scene(64), 32 x 24, 2 bounces, black environment) on the product, 64 samples a pixel: the per-sample
    variance in tree mode over that in CDF mode is at most 2 * R0 (the project's margin for this kind of estimate, as for the punctual
    tree: the restated figure is itself an estimate from 4 samples a pixel) and below 1.
    Measured on the MI355X: 0.2442 (R0 = 0.2347); visible light samples 36055 in tree mode against 34902."""
    v = LT.VARIANCE_CASE
    W, H, spp = v["W"], v["H"], 64
    rad, ls = {}, {}
    for mode, scenes in (("tree", PRODUCTS), ("cdf", CDF_PRODUCTS)):
        s, pipeline = _route(ptx, ctx, clean_env, f"field{v['n']}", "lds fused", scenes)
        rad[mode], tot = _samples(ptx, ctx, s, W, H, spp, v["bounces"], FUSED, pipeline, env=BLACK)
        ls[mode] = tot["light_visible"]
    r = _variance_ratio(rad["tree"], rad["cdf"])
    print(f"per-sample variance tree / CDF on the product: {r:.4f} (R0 = {LT.R0}); visible light samples {ls['tree']} against {ls['cdf']}")
    assert r <= 2 * LT.R0 and r < 1


# ---------------------------------------------------------------------------- 8. mirrors
def test_mirrors_and_cli_in_tree_mode(ptx, ctx, clean_env, tmp_path):
    """the Cornell box in tree mode: Scene.render_nee after the C call against Renderer.set_light_pick + render_nee (python) and
    ptx_render_cli --nee-light-tree (core::renderer::set_light_pick; the switch implies --nee), bit for bit"""
    from PIL import Image
    W, H, spp, b = 24, 16, 8, 3
    s = ptx.Scene.load_gltf(ctx, CORNELL)
    cdf, _ = s.render_nee(W, H, spp, b, seed=SEED)
    assert ptx.lib().ptx_scene_set_light_pick(s.h, ptx.LIGHT_PICK_TREE) == 0
    want, st = s.render_nee(W, H, spp, b, seed=SEED)
    assert (_bits(want) != _bits(cdf)).any() and st["light_samples"] > st["light_visible"] > 0
    _same(s.render_nee(W, H, spp, b, seed=SEED, flags=FUSED)[0], want, "Scene.render_nee, fused")
    r = ptx.Renderer(0)
    r.resolution, r.sample_count, r.bounce_count, r.seed = (W, H), spp, b, SEED
    r.load_gltf(CORNELL)
    r.set_light_pick("tree")
    _same(r.render_nee(), want, "Renderer.render_nee")
    cli = os.path.join(ROOT, "distributed-path-tracer_amd", "ptx_render_cli")
    for switches in (["--nee-light-tree"], ["--nee", "--nee-light-tree"], ["--nee-light-tree", "--nee-fused"]):
        out = subprocess.run([cli, *switches, CORNELL, str(tmp_path / "f.png"), str(W), str(H), str(spp), str(b)], capture_output=True, text=True, timeout=120)
        assert out.returncode == 0, out.stderr
        js = json.loads(out.stdout)
        assert js["nee_light_samples"] == st["light_samples"] and js["nee_light_pick"] == "tree", js
        np.testing.assert_array_equal(np.array(Image.open(tmp_path / "f.png")), ctx.tonemap_encode(want, W, H, spp))
    s.close()
