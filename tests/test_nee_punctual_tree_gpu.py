"""The light tree of ptx_render_nee's punctual lights on the MI355X (include/ptx.h: PUNCTUAL PICK; csrc/nee_core.hpp punctual_pick, which
nee_candidate's PUN branch and k_punctual_pick inline). The yardsticks are tests/_nee_punctual_tree_restatement.py for the pick and the
unchanged tests/_nee_estimator.py for everything else; the CPU side is tests/test_nee_punctual_tree.py.

Scenes are test_nee_punctual_gpu.py's: procedural.lamp_scene and the material chart under six lamps, the golden sky as the map. Bars are the
project's: bitwise equality against the restatement, between the two forms, between routes and against the calls a frame is composed of;
test_nee_punctual_gpu's per-sample bar for construction D; _nee_common's statistic for the expectation; 2 * R0 for the variance.
"""
import json
import os
import subprocess

import numpy as np
import pytest

import _adaptive_restatement as AR
import _nee_punctual_restatement as PU
import _nee_punctual_tree_restatement as PT
from _common import _bits, _proc, _same
from _fused_motion_common import Routed, with_motion
from _motion_common import movers as _movers
from _nee_common import K_BATCH, SAME_STATS, SEED, _batch_stat, _pair, _same_expectation
from _nee_estimator import BLOCK_PUNCTUAL, render_samples
from _nee_lit_scenes import CAND, ENV, FUSED, NO_LIGHTS, SKY, SPDF, _variance_ratio
from _nee_restatement import draws
from _routes import clean_env, ctx  # noqa: F401  (fixtures)
from _routes import DEFAULT_ROUTES, ROUTE_VARS, Scenes, on_route, route_named, under_force_global
from conftest import GOLD, ROOT, oracle_from_dict, product_from_dict

f32 = np.float32
pytestmark = pytest.mark.gpu
LAMPS_FILE = os.path.join(GOLD, "lights", "lamps.gltf")
BLACK = (0.0, 0.0, 0.0)

# name -> (lamp_scene arguments, under the sky map); "chart": the chart with pass-through patches and a sun under six lamps
CASES = {"one": (dict(n_lamps=1, spots=True), False), "three": (dict(n_lamps=3, spots=True, lamp_range=3.0), False),
         "five": (dict(n_lamps=5, spots=True), False), "sixteen": (PT.VARIANCE_CASE["lamps"], False),
         "lamps_emit": (dict(n_lamps=8, emitters=True, spots=True), False), "lamps_emit_map": (dict(n_lamps=8, emitters=True, spots=True), True),
         "many": (dict(n_lamps=64, spots=True), False), "many_range": (dict(n_lamps=64, spots=True, lamp_range=3.0), False),
         "257": (dict(n_lamps=257, spots=True, lamp_range=4.0), False)}
_built = {}


def _dict_and_lights(name):
    if name not in _built:
        if name.startswith("chart"):
            _built[name] = (_proc().chart_scene(facing=True, alpha=True, sun=0.004732), _proc().lamp_scene(6, chart=True, spots=True)[1], name == "chart_map")
        else:
            kw, sky = CASES[name]
            _built[name] = (*_proc().lamp_scene(**kw), sky)
    return _built[name]


def _make(ptx, ctx, name, tree=True):
    d, lights, sky = _dict_and_lights(name)
    s = product_from_dict(ptx, ctx, d)
    if sky:
        s.set_environment(SKY, srgb=False)
    s.set_punctual_lights(lights)
    if tree:
        s.set_punctual_pick(ptx.PUNCTUAL_PICK_TREE)
    return s


PRODUCTS = Scenes(_make)                                                    # tree mode
CDF_PRODUCTS = Scenes(lambda ptx, ctx, name: _make(ptx, ctx, name, False))  # the same scenes as the parent renders them


def _route(ptx, ctx, mp, name, route, scenes=PRODUCTS):
    r = route_named(DEFAULT_ROUTES, route)
    return on_route(scenes, ptx, ctx, mp, name, r), r.pipeline


def _hybrid(ptx, ctx, mp, name):
    """test_nee_punctual_gpu's hybrid scene: one byte too little LDS for all of its surfaces, the fused kernel asked for"""
    budget = int(_make(ptx, None, name).array(ptx.ARR_RES_PLAN)[0]) - 1
    mp.setenv("PTX_LDS_BUDGET", str(budget))
    if _make(ptx, None, name).info()["lds_resident"] == 1:
        mp.delenv("PTX_LDS_BUDGET")
        mp.setenv("PTX_LDS_LEAF_ORDER", "0")
        budget = int(_make(ptx, None, name).array(ptx.ARR_RES_PLAN)[0]) - 1
        mp.delenv("PTX_LDS_LEAF_ORDER")
        mp.setenv("PTX_LDS_BUDGET", str(budget))
    s = _make(ptx, ctx, name)
    for k in ROUTE_VARS:
        mp.delenv(k, raising=False)
    mp.delenv("PTX_LDS_BUDGET")
    mp.setenv("PTX_WAVEFRONT", "0")
    assert s.info()["lds_resident"] == 2, (name, s.info())
    return s


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


# ---------------------------------------------------------------------------- 1. the batch
def _probe_points(lights, T, rng, n=4096):
    """n random positions around the scene, then every light's own position and the centre of every branch's box, with u drawn at random,
    0 and the largest float below 1"""
    x = np.stack([rng.uniform(-4.5, 4.5, n), rng.uniform(-0.5, 3.5, n), rng.uniform(-4.5, 4.5, n)], 1).astype(f32)
    lo, hi = T[:, 0:3].view(f32), T[:, 4:7].view(f32)
    inside = ((lo + hi) * f32(0.5))[(T[:, 7] & PT.LEAF) == 0]
    x = np.concatenate([x, lights[:, 0:3], inside]).astype(f32)
    x = np.concatenate([x, x[n:], x[n:]])                      # the special positions three times: u random, 0 and just below 1
    m = len(x) - n
    u = rng.random(len(x)).astype(f32)
    u[0], u[1] = 0, PT.ONE_BELOW
    u[n + m // 3:n + 2 * (m // 3)] = 0
    u[n + 2 * (m // 3):] = PT.ONE_BELOW
    return np.concatenate([x, u[:, None]], 1).astype(f32)


@pytest.mark.parametrize("name", ["one", "three", "many_range", "257"])
def test_pick_batch_is_the_restatement_bit_for_bit(ptx, ctx, clean_env, name):
    """ptx_punctual_pick_batch (the device function the integrators inline) against the restated pick: the light and every bit of the pmf, for
    4096 random positions plus positions on every light and at the centre of every branch's box, u random, 0 and 0x1.fffffep-1; host and
    device pointers; then CDF mode against the stored CDF; and the refusals.
    Measured on the MI355X: no light and no bit differs in any of the four scenes (4099 / 4111 / 4477 / 5635 picks; smallest pmf 0.00035)."""
    import torch
    s, _ = _route(ptx, ctx, clean_env, name, "lds fused")
    lights = _dict_and_lights(name)[1]
    T = s.array(ptx.ARR_PUNCTUAL_TREE)
    np.testing.assert_array_equal(T, PT.build(lights))
    pu = _probe_points(lights, T, np.random.default_rng(11))
    want_k, want_p = PT.pick(T, lights, pu[:, :3], pu[:, 3])
    k, p = s.punctual_pick_batch(pu)
    print(f"{name}: {len(pu)} picks, {int((k != want_k).sum())} lights differ, {int((_bits(p) != _bits(want_p)).sum())} pmfs differ in a bit; smallest pmf {p.min():.3g}")
    np.testing.assert_array_equal(k, want_k)
    _same(p, want_p, f"{name}: pmf")
    assert (p > 0).all() and (p <= 1).all()
    d_in = torch.from_numpy(pu).cuda()
    d_k, d_p = torch.zeros(len(pu), dtype=torch.int32, device="cuda"), torch.zeros(len(pu), dtype=torch.float32, device="cuda")
    torch.cuda.synchronize()   # the copies and fills run on torch's stream, the library on its own
    L = ptx.lib()
    assert L.ptx_punctual_pick_batch(s.h, d_in.data_ptr(), len(pu), d_k.data_ptr(), d_p.data_ptr()) == 0
    ctx.synchronize()
    np.testing.assert_array_equal(d_k.cpu().numpy(), want_k)
    _same(d_p.cpu().numpy(), want_p, f"{name}: pmf, device pointers")
    # refusals
    assert L.ptx_punctual_pick_batch(s.h, pu.ctypes.data, len(pu), d_k.data_ptr(), d_p.data_ptr()) == ptx.ERR_INVALID      # mixed kinds
    assert L.ptx_punctual_pick_batch(s.h, None, len(pu), k.ctypes.data, p.ctypes.data) == ptx.ERR_INVALID
    assert L.ptx_punctual_pick_batch(s.h, pu.ctypes.data, len(pu), None, p.ctypes.data) == ptx.ERR_INVALID
    assert L.ptx_punctual_pick_batch(s.h, None, 0, None, None) == 0
    # CDF mode: the position plays no part
    c, _ = _route(ptx, ctx, clean_env, name, "lds fused", CDF_PRODUCTS)
    assert len(c.array(ptx.ARR_PUNCTUAL_TREE)) == 0
    ck, cp = c.punctual_pick_batch(pu)
    wk, wp = PT.cdf_pick(c.array(ptx.ARR_PUNCTUAL_CDF), pu[:, 3])
    np.testing.assert_array_equal(ck, wk)
    _same(cp, wp, f"{name}: CDF mode")
    np.testing.assert_array_equal(_bits(c.array(ptx.ARR_PUNCTUAL_CDF)), _bits(PU.cdf_of(lights)))


def test_pick_batch_refuses_a_scene_without_lights(ptx, ctx, clean_env):
    s = product_from_dict(ptx, ctx, _dict_and_lights("one")[0])
    s.set_punctual_pick(ptx.PUNCTUAL_PICK_TREE)
    pu, k, p = np.zeros((2, 4), f32), np.zeros(2, np.int32), np.zeros(2, f32)
    assert ptx.lib().ptx_punctual_pick_batch(s.h, pu.ctypes.data, 2, k.ctypes.data, p.ctypes.data) == ptx.ERR_INVALID
    s.close()


# ---------------------------------------------------------------------------- 2. one lamp
@pytest.mark.parametrize("route", ["lds fused", "global fused", "queue"])
def test_one_lamp_is_the_cdf_frame_bitwise(ptx, ctx, clean_env, route):
    """with one light the root is its leaf, (0, 1.0f): the tree-mode frame is the CDF-mode frame bit for bit, stats included, in both forms"""
    W, H, spp, b = 32, 24, 4, 3
    t, pipeline = _route(ptx, ctx, clean_env, "one", route)
    c, _ = _route(ptx, ctx, clean_env, "one", route, CDF_PRODUCTS)
    assert len(t.array(ptx.ARR_PUNCTUAL_TREE)) == 1 and t.punctual_pick == 1 and c.punctual_pick == 0
    for flags in (0, FUSED, CAND(4) | FUSED):
        want, st0 = c.render_nee(W, H, spp, b, seed=SEED, flags=flags)
        got, st = t.render_nee(W, H, spp, b, seed=SEED, flags=flags)
        assert ctx.timing()["pipeline"] == pipeline
        _same(got, want, f"{route} / {flags}")
        assert all(st[k] == st0[k] for k in SAME_STATS) and st["light_visible"] > 0, (st, st0)


# ---------------------------------------------------------------------------- 3. construction D
_refs = {}


def _construction_d(ora, name, W, H, spp):
    """2 bounces under a black environment without an emitter: a sample's radiance is vertex 0's punctual sample alone. -> dict(X [n_lamps]
    of [H, W, spp, 3]: the unchanged restatement's frame of each lamp alone; pos [H, W, spp, 3], hit, normal, d: vertex 0 from the
    restatement's own hit code; u [H, W, spp]: draws(pixel, sample, 0, 0, 0x200).y), computed once and left unchanged"""
    key = (name, W, H, spp)
    if key not in _refs:
        d, lights, _ = _dict_and_lights(name)
        o = oracle_from_dict(ora, d)
        X = [render_samples(ora, o, o.a, W, H, spp, 2, seed=SEED, env=BLACK, punctual=lights[k:k + 1])["rad"] for k in range(len(lights))]
        pos, nrm, dirs = (np.zeros((H, W, spp, 3), f32) for _ in range(3))
        hit, u = np.zeros((H, W, spp), bool), np.zeros((H, W, spp), f32)
        pixel = np.arange(W * H, dtype=np.uint32)
        for s in range(spp):
            rays = o.primary_rays(ora.make_cfg(W, H, 1, 1, seed=SEED), s).reshape(-1, 6)
            out, surf = o.intersect(rays)
            pos[:, :, s], nrm[:, :, s], dirs[:, :, s] = out[:, 0:3].reshape(H, W, 3), out[:, 11:14].reshape(H, W, 3), rays[:, 3:].reshape(H, W, 3)
            hit[:, :, s] = (surf >= 0).reshape(H, W)
            z = np.zeros(W * H, np.int64)
            u[:, :, s] = draws(ora, pixel, np.full(W * H, s, np.uint32), z, z, BLOCK_PUNCTUAL, SEED)[:, 1].reshape(H, W)
        ref = dict(X=np.stack(X), pos=pos, hit=hit, normal=nrm, d=dirs, u=u)
        for v in ref.values():
            v.setflags(write=False)
        _refs[key] = ref
    return _refs[key]


def _expected_tree_frame(ref, lights, pick_of):
    """the per-sample radiance X_k / pmf of the pick (k, pmf) = pick_of(positions, u), and whether the sample traces a light ray: the
    PUNCTUAL SAMPLE conditions of light k at vertex 0, which faces the camera"""
    shape = ref["hit"].shape
    k, pmf = pick_of(ref["pos"].reshape(-1, 3), ref["u"].reshape(-1))
    k, pmf = k.reshape(shape), pmf.reshape(shape)
    Xk = np.take_along_axis(ref["X"], k[None, ..., None].astype(np.int64), 0)[0]
    with np.errstate(all="ignore"):
        want = np.where(ref["hit"][..., None], Xk / pmf[..., None], f32(0)).astype(f32)
        dist2, dist, w, att, in_range = PT.light_geom(lights[k.reshape(-1)], ref["pos"].reshape(-1, 3))
        n, dd = ref["normal"].reshape(-1, 3), ref["d"].reshape(-1, 3)
        E = (lights[k.reshape(-1), 8:11] * att[:, None]) / dist2[:, None]
        traced = (ref["hit"].reshape(-1) & ((n * -dd).sum(-1) > 0) & (dist2 > 0) & ((n * w).sum(-1) > 0) & (pmf.reshape(-1) > 0) & in_range & (att > 0)
                  & (E.max(-1) > 0))
    return want, int(traced.sum())


@pytest.mark.parametrize("flags", [0, FUSED], ids=["unfused", "fused"])
def test_first_punctual_sample_is_the_picked_lamps_alone_over_its_pmf(ptx, ctx, ora, clean_env, flags):
    """test_nee_punctual_gpu's construction D on lamp_scene(5, spots=True), 48 x 32 x 4: tree mode's per-sample radiance is bitwise X_k / pmf
    (with c_p = 1, c_p * pmf is pmf exactly), X_k the unchanged restatement's frame of lamp k alone and (k, pmf) the restated pick at vertex
    0's position with draws(pixel, sample, 0, 0, 0x200).y. That test's bar: <= 0.5 % of the samples may differ in a bit, the light-ray
    counts within 0.5 % + 1, lit and black shares asserted; both forms. The same construction with the CDF's pick pins the reference itself.
    Measured on the MI355X: none of 6144 samples differs in either form, in tree mode (4393 not black, 4897 light rays, both equal to the
    restated counts) or in CDF mode (2976 and 3425)."""
    W, H, spp = 48, 32, 4
    lights = _dict_and_lights("five")[1]
    ref = _construction_d(ora, "five", W, H, spp)
    T = PT.build(lights)
    cdf = PU.cdf_of(lights)
    for mode, scenes, pick_of in (("tree", PRODUCTS, lambda x, u: PT.pick(T, lights, x, u)), ("cdf", CDF_PRODUCTS, lambda x, u: PT.cdf_pick(cdf, u))):
        want, traced = _expected_tree_frame(ref, lights, pick_of)
        s, pipeline = _route(ptx, ctx, clean_env, "five", "lds fused", scenes)
        got, tot = _samples(ptx, ctx, s, W, H, spp, 2, flags, pipeline, env=BLACK)
        differ = (_bits(got) != _bits(want)).any(-1)
        lit = (want > 0).any(-1)
        print(f"{mode} / {flags}: {differ.sum()} of {differ.size} samples differ ({lit.sum()} of them not black); light samples {tot['light_samples']} "
              f"(restated {traced}), visible {tot['light_visible']} (restated not black {lit.sum()})")
        assert lit.mean() > 0.05 and (~lit).mean() > 0.02 and differ.sum() <= 0.005 * differ.size
        assert abs(tot["light_samples"] - traced) <= 0.005 * traced + 1
        assert abs(tot["light_visible"] - int(lit.sum())) <= 0.005 * lit.sum() + 1
    tree_want, _ = _expected_tree_frame(ref, lights, lambda x, u: PT.pick(T, lights, x, u))
    assert (_bits(tree_want) != _bits(want)).any()               # the two modes are different frames


# ---------------------------------------------------------------------------- 4. fused against unfused
FUSED_SETS = {"lamps_emit": [(0, 1), (SPDF, 1), (0, 4), (SPDF, 3), (NO_LIGHTS, 1), (NO_LIGHTS, 4)],
              "lamps_emit_map": [(ENV, 1), (ENV | SPDF, 1), (ENV, 4), (ENV | SPDF, 16), (ENV | NO_LIGHTS, 2)],
              "chart": [(0, 1), (SPDF, 2), (0, 4)], "chart_map": [(ENV, 1), (ENV | SPDF, 1), (ENV, 4), (ENV | SPDF, 4)]}


@pytest.mark.parametrize("route", ["lds fused", "hybrid", "global fused"])
@pytest.mark.parametrize("name", sorted(FUSED_SETS))
def test_fused_is_unfused_bitwise_in_tree_mode(ptx, ctx, clean_env, name, route):
    """test_nee_punctual_gpu's fused-against-unfused test with the tree set: the same scenes, flag sets and routes, frame and stats bitwise
    (_nee_common._pair); and the tree-mode frame is not the CDF-mode frame"""
    s = _hybrid(ptx, ctx, clean_env, name) if route == "hybrid" else _route(ptx, ctx, clean_env, name, route)[0]
    assert len(s.array(ptx.ARR_PUNCTUAL_TREE)) == 2 * len(_dict_and_lights(name)[1]) - 1
    W, H = (48, 40) if name.startswith("chart") else (40, 28)
    for flags, M in FUSED_SETS[name]:
        got, st = _pair(ptx, ctx, s, W, H, 3, 4, flags=flags | CAND(M))
        assert st["light_samples"] > st["light_visible"] > 0, (flags, M, st)
    flags = FUSED_SETS[name][0][0] | FUSED
    tree, _ = s.render_nee(W, H, 3, 4, seed=SEED, flags=flags)
    s.set_punctual_pick(ptx.PUNCTUAL_PICK_CDF)
    cdf, _ = s.render_nee(W, H, 3, 4, seed=SEED, flags=flags)
    s.set_punctual_pick(ptx.PUNCTUAL_PICK_TREE)
    again, _ = s.render_nee(W, H, 3, 4, seed=SEED, flags=flags)
    assert (_bits(tree) != _bits(cdf)).any()
    _same(again, tree, "the mode set back")
    if route == "hybrid":
        s.close()


def test_queue_route_and_a_forced_pool_overflow_in_tree_mode(ptx, ctx, clean_env):
    """test_nee_punctual_gpu's pool switches on the 64-lamp scene in tree mode: the queue frame, unforced and with a 1 Mi-pair pool that
    800 x 600 x 4 camera rays overflow, is the 'lds fused' frame bit for bit, stats included. The frame is as large as that test's: the
    pool overflows only with more than 2^20 (ray, surface) pairs in a slice."""
    W, H, spp, b = 800, 600, 4, 3
    s, _ = _route(ptx, ctx, clean_env, "many", "lds fused")
    want, st0 = s.render_nee(W, H, spp, b, seed=SEED)
    q, _ = _route(ptx, ctx, clean_env, "many", "queue")
    unforced, st1 = q.render_nee(W, H, spp, b, seed=SEED)
    assert ctx.timing()["pipeline"] == 1 and ctx.timing()["pool_overflows"] == 0
    fresh = under_force_global(clean_env, True, lambda: _make(ptx, ctx, "many"))
    clean_env.setenv("PTX_WF_PAIRS_M", "1")
    clean_env.setenv("PTX_WF_RATIO_GUESS", "0.25")
    forced, st2 = fresh.render_nee(W, H, spp, b, seed=SEED)
    tm = ctx.timing()
    fresh.close()
    assert tm["pipeline"] == 1 and tm["pool_overflows"] >= 1, tm
    for tag, (got, st) in (("queue", (unforced, st1)), ("queue, forced overflow", (forced, st2))):
        _same(got, want, f"{tag} against lds fused")
        assert all(st[k] == st0[k] for k in SAME_STATS), (tag, st, st0)
    assert st0["light_samples"] > 0


MOTION_LAMPS = f32([[0.5, 2.0, 1.0, 0, 0, -1, 0, 0, 6, 5, 4, 0, 0, 0, 0, 0], [-1.0, 1.5, 2.0, 0, 0, -1, 0, 0, 2, 3, 4, 0, 0, 0, 0, 0],
                    [1.5, 2.5, -1.0, 0, 0, -1, 0, 0, 3, 3, 3, 0, 0, 0, 0, 0]])


def test_fused_motion_is_unfused_bitwise_in_tree_mode(ptx, ctx, clean_env):
    """the movers under an open shutter with three lamps in tree mode: PTX_NEE_FUSED | PTX_NEE_FUSED_MOTION against the unfused form, frame
    and stats bitwise; lights do not move under the shutter"""
    d = _movers()
    R = Routed(ptx, ctx, clean_env, "lds fused", d)
    a = with_motion(R, d, (0.2, 0.9))
    a.set_punctual_lights(MOTION_LAMPS)
    a.set_punctual_pick(ptx.PUNCTUAL_PICK_TREE)
    assert a.array(ptx.ARR_MOTION_MOVED).any() and len(a.array(ptx.ARR_PUNCTUAL_TREE)) == 5
    fm = ptx.NEE_FUSED | ptx.NEE_FUSED_MOTION
    tree = {}
    for flags in (0, CAND(4)):
        want, wst = a.render_nee(16, 12, 3, 3, seed=SEED, flags=flags)
        assert ctx.timing()["fused_launches"] == 0
        tree[flags], gst = a.render_nee(16, 12, 3, 3, seed=SEED, flags=flags | fm)
        assert ctx.timing()["fused_launches"] == gst["passes"] >= 1
        _same(tree[flags], want, f"fused motion / {flags}")
        assert all(gst[k] == wst[k] for k in SAME_STATS) and gst["light_samples"] > 0, (gst, wst)
    a.set_punctual_pick(ptx.PUNCTUAL_PICK_CDF)
    cdf, _ = a.render_nee(16, 12, 3, 3, seed=SEED, flags=fm)
    assert (_bits(cdf) != _bits(tree[0])).any()
    a.close()


# ---------------------------------------------------------------------------- 5. composition
def test_composition_in_tree_mode(ptx, ctx, clean_env):
    """test_nee_punctual_gpu's composition on the eight-lamp scene under the map, in tree mode: tiles, two sample ranges, pass sizes that cut
    the frame, two and three shards, a device buffer, and the queue route"""
    import torch
    s, _ = _route(ptx, ctx, clean_env, "lamps_emit_map", "lds fused")
    W, H, spp, b, F = 24, 16, 8, 3, FUSED | ENV | CAND(4)
    whole, _ = s.render_nee(W, H, spp, b, seed=SEED, flags=ENV | CAND(4))
    tiles = np.zeros_like(whole)
    for (x0, y0, w, h) in [(0, 0, 9, 16), (9, 0, 15, 7), (9, 7, 15, 9)]:
        tiles[y0:y0 + h, x0:x0 + w] = s.render_nee(W, H, spp, b, seed=SEED, tile=(x0, y0, w, h), flags=F)[0]
    _same(tiles, whole, "tiles")
    two, _ = s.render_nee(W, H, 3, b, seed=SEED, flags=F)
    two, _ = s.render_nee(W, H, 5, b, seed=SEED, sample0=3, accum=two, flags=F)
    _same(two, whole, "two sample ranges")
    for pp in (1, 3):
        got, st = s.render_nee(W, H, spp, b, seed=SEED, spp_per_pass=pp, flags=F)
        assert st["passes"] == -(-spp // pp) == ctx.timing()["fused_launches"]
        _same(got, whole, f"spp_per_pass {pp}")
    for n in (2, 3):
        shards = sum(s.render_nee(W, H, spp, b, seed=SEED, shard=(k, n, 8), flags=F)[0] for k in range(n))
        _same(shards, whole, f"{n} shards")
    dev = torch.zeros((H, W, 4), dtype=torch.float32, device="cuda")
    torch.cuda.synchronize()   # the fill runs on torch's stream, the library on its own
    s.render_nee(W, H, spp, b, accum=dev, seed=SEED, flags=F)
    _same(dev.cpu().numpy(), whole, "device buffer")
    q, pipeline = _route(ptx, ctx, clean_env, "lamps_emit_map", "queue")
    assert pipeline == 1
    got, _ = _pair(ptx, ctx, q, W, H, spp, b, fused=False, flags=ENV | CAND(4))
    _same(got, whole, "queue route")
    c, _ = _route(ptx, ctx, clean_env, "lamps_emit_map", "lds fused", CDF_PRODUCTS)
    assert (_bits(c.render_nee(W, H, spp, b, seed=SEED, flags=F)[0]) != _bits(whole)).any()


@pytest.mark.parametrize("route,flags", [("lds fused", FUSED), ("queue", CAND(4))])
def test_adaptive_in_tree_mode_is_the_calls_of_the_half_ranges(ptx, ctx, clean_env, route, flags):
    """tests/test_adaptive_nee.py's snapshot method on the eight-lamp scene in tree mode, 48 x 32, 3 bounces, 8 samples first, 8 per round,
    cap 24: a pixel with n samples holds, in A and in B, what the ptx_render_nee calls of the same half ranges leave"""
    W, H, b, cap, thr = 48, 32, 3, 24, 0.2
    s, pipeline = _route(ptx, ctx, clean_env, "lamps_emit", route)
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


# ---------------------------------------------------------------------------- 6. expectation
@pytest.mark.parametrize("name", ["lamps_emit", "many"])
def test_tree_mode_has_the_cdf_modes_expectation(ptx, ctx, clean_env, name):
    """16 batches of 16 spp in tree mode against 16 of other seeds in CDF mode, 32 x 24, 3 bounces, _nee_common's statistic with its own
    bars: eight lamps with an emitter (c_p = 0.5) and 64 lamps alone (c_p = 1).
    Measured on the MI355X, worst z frame / quadrant: lamps_emit 2.06 / 2.30, many 0.48 / 1.43."""
    W, H, b = 32, 24, 3
    t, _ = _route(ptx, ctx, clean_env, name, "lds fused")
    c, _ = _route(ptx, ctx, clean_env, name, "lds fused", CDF_PRODUCTS)

    def batches(s, seed0):
        return _batch_stat(np.stack([s.render_nee(W, H, 16, b, seed=seed0 + k, flags=FUSED)[0][..., :3] / f32(16) for k in range(K_BATCH)]))
    ok, zf, zq = _same_expectation(batches(t, 0xA000), batches(c, 0xB000))
    print(f"{name}: tree against CDF mode, worst z frame {zf:.2f} quadrant {zq:.2f}")
    assert ok, (zf, zq)


# ---------------------------------------------------------------------------- 7. variance
def test_variance_against_the_restatements_ratio(ptx, ctx, clean_env):
    """PT.VARIANCE_CASE (construction D on lamp_scene(16, spots=True), 32 x 24) on the product, 64 samples a pixel: the per-sample variance
    in tree mode over that in CDF mode is at most 2 * R0 (the project's margin for this kind of estimate) and below 1. The per-pixel sample
    variance holds the variance of the vertex under the pixel's jitter too, the same in both modes, so the product's ratio lies above R0.
    Measured on the MI355X: 0.4374 (R0 = 0.4402); light samples 36639 in tree mode against 22938: the tree picks lamps that reach the vertex."""
    v = PT.VARIANCE_CASE
    W, H, spp = v["W"], v["H"], 64
    rad, ls = {}, {}
    for mode, scenes in (("tree", PRODUCTS), ("cdf", CDF_PRODUCTS)):
        s, pipeline = _route(ptx, ctx, clean_env, "sixteen", "lds fused", scenes)
        rad[mode], tot = _samples(ptx, ctx, s, W, H, spp, 2, FUSED, pipeline, env=BLACK)
        ls[mode] = tot["light_samples"]
    r = _variance_ratio(rad["tree"], rad["cdf"])
    print(f"per-sample variance tree / CDF on the product: {r:.4f} (R0 = {PT.R0}); light samples {ls['tree']} against {ls['cdf']}")
    assert r <= 2 * PT.R0 and r < 1


# ---------------------------------------------------------------------------- 8. off means off
@pytest.mark.parametrize("route", [r.name for r in DEFAULT_ROUTES])
def test_off_means_off(ptx, ctx, clean_env, route):
    """After set_punctual_pick(CDF) the frame is bitwise the one of a scene never given the setter, stats included; and a scene without
    lights in tree mode is bitwise the scene nobody touched, in both forms and with flags"""
    W, H, spp, b = 32, 24, 4, 3
    r = route_named(DEFAULT_ROUTES, route)
    d, lights, _ = _dict_and_lights("lamps_emit")

    def fresh():
        def make():
            s = product_from_dict(ptx, ctx, d)
            s.set_environment(SKY, srgb=False)
            return s
        return under_force_global(clean_env, r.force_global, make)
    never, back, bare, bare_tree = fresh(), fresh(), fresh(), fresh()
    for k, v in r.env.items():
        clean_env.setenv(k, v)
    never.set_punctual_lights(lights)
    back.set_punctual_pick(ptx.PUNCTUAL_PICK_TREE)
    back.set_punctual_lights(lights)
    in_tree, _ = back.render_nee(W, H, spp, b, seed=SEED)
    back.set_punctual_pick(ptx.PUNCTUAL_PICK_CDF)
    bare_tree.set_punctual_pick(ptx.PUNCTUAL_PICK_TREE)
    for flags in (0, FUSED, ENV | SPDF | CAND(4), ENV | SPDF | CAND(4) | FUSED):
        want, st0 = never.render_nee(W, H, spp, b, seed=SEED, flags=flags)
        assert ctx.timing()["pipeline"] == r.pipeline
        got, st = back.render_nee(W, H, spp, b, seed=SEED, flags=flags)
        _same(got, want, f"{route} / {flags}: back in CDF mode")
        assert all(st[k] == st0[k] for k in SAME_STATS), (st, st0)
        if flags == 0:
            assert (_bits(in_tree) != _bits(want)).any()
        want, st0 = bare.render_nee(W, H, spp, b, seed=SEED, flags=flags)
        got, st = bare_tree.render_nee(W, H, spp, b, seed=SEED, flags=flags)
        _same(got, want, f"{route} / {flags}: no lights, tree mode")
        assert all(st[k] == st0[k] for k in SAME_STATS), (st, st0)
    for s in (never, back, bare, bare_tree):
        s.close()


# ---------------------------------------------------------------------------- 9. mirrors
def test_mirrors_and_cli_in_tree_mode(ptx, ctx, clean_env, tmp_path):
    """lamps.gltf with its own lamps in tree mode: Scene.render_nee against Renderer.set_punctual_pick + render_nee (python) and
    ptx_render_cli --nee --nee-punctual-tree (core::renderer::set_punctual_pick; the switch implies --nee-punctual), bit for bit"""
    from PIL import Image
    W, H, spp, b = 24, 16, 8, 3
    lamps = ptx.read_punctual_lights(LAMPS_FILE)
    s = ptx.Scene.load_gltf(ctx, LAMPS_FILE)
    s.set_punctual_lights(lamps)
    cdf, _ = s.render_nee(W, H, spp, b, seed=SEED)
    assert ptx.lib().ptx_scene_set_punctual_pick(s.h, ptx.PUNCTUAL_PICK_TREE) == 0
    want, st = s.render_nee(W, H, spp, b, seed=SEED)
    assert (_bits(want) != _bits(cdf)).any() and st["light_samples"] > st["light_visible"] > 0
    assert len(s.array(ptx.ARR_PUNCTUAL_TREE)) == 2 * 3 - 1          # the file's fourth lamp is black
    _same(s.render_nee(W, H, spp, b, seed=SEED, flags=FUSED)[0], want, "Scene.render_nee, fused")
    r = ptx.Renderer(0)
    r.resolution, r.sample_count, r.bounce_count, r.seed = (W, H), spp, b, SEED
    r.load_gltf(LAMPS_FILE)
    r.set_punctual_pick(ptx.PUNCTUAL_PICK_TREE)                       # before the lamps: the mode survives the set
    r.set_punctual_lights(lamps)
    _same(r.render_nee(), want, "Renderer.render_nee")
    cli = os.path.join(ROOT, "distributed-path-tracer_amd", "ptx_render_cli")
    for switches in (["--nee", "--nee-punctual-tree"], ["--nee-punctual-tree", "--nee-fused"], ["--nee", "--nee-punctual", "--nee-punctual-tree"]):
        out = subprocess.run([cli, *switches, LAMPS_FILE, str(tmp_path / "f.png"), str(W), str(H), str(spp), str(b)], capture_output=True, text=True, timeout=120)
        assert out.returncode == 0, out.stderr
        np.testing.assert_array_equal(np.array(Image.open(tmp_path / "f.png")), ctx.tonemap_encode(want, W, H, spp))
        js = json.loads(out.stdout)
        assert js["nee_light_samples"] == st["light_samples"] and js["nee_punctual_lights"] == 4 and js["nee_punctual_pick"] == "tree"
    out = subprocess.run([cli, "--nee-punctual-tree", LAMPS_FILE, str(tmp_path / "g.png"), str(W), str(H), str(spp), str(b)], capture_output=True, text=True, timeout=120)
    assert out.returncode == 1 and "--nee-punctual needs --nee" in out.stderr and not (tmp_path / "g.png").exists()
    s.close()
