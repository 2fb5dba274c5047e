"""Point and spot lights in ptx_render_nee on the MI355X (include/ptx.h: PUNCTUAL LIGHTS; csrc/nee_core.hpp nee_candidate's PUN branch,
the PUN parts of nee.hip and nee_fused.hip). The yardstick is tests/_nee_estimator.py; the CPU side of it is tests/test_nee_punctual.py.

Scenes: procedural.lamp_scene (a floor, a blocker, optionally an emitter, lamps above) and the material chart with pass-through patches and a
sun under six lamps; the golden sky as the map. Bars are the project's: the per-sample bar of test_nee.py / test_nee_lights.py, bitwise
equality between the two forms, between routes and against the calls an adaptive frame is made of.
"""
import ctypes as C
import json
import os
import subprocess

import numpy as np
import pytest

import _adaptive_restatement as AR
from _common import _bits, _proc, _same
from _nee_common import SAME_STATS, SEED, _err, _pair
from _nee_estimator import render_samples
from _nee_lit_scenes import CAND, CLOUDS, ENV, FUSED, LIT, LIT_LOADS, NO_LIGHTS, SKY, SPDF, _table
from _nee_lit_scenes import _dict as _lit_dict
from _routes import clean_env, ctx  # noqa: F401  (fixtures)
from _routes import DEFAULT_ROUTES, ROUTE_VARS, Scenes, on_route, route_named, under_force_global
from conftest import GOLD, ROOT, oracle_from_dict, product_from_dict

f32 = np.float32
LAMPS = os.path.join(GOLD, "lights", "lamps.gltf")


# name -> (lamp_scene arguments, under the sky map)
CASES = {"point": (dict(n_lamps=1, blocker=False), False), "spot": (dict(n_lamps=1, spots=True, blocker=False), False),
         "blocked": (dict(n_lamps=1), False), "range": (dict(n_lamps=1, lamp_range=2.6), False),
         "lamps_emit": (dict(n_lamps=8, emitters=True, spots=True), False), "lamps_emit_map": (dict(n_lamps=8, emitters=True, spots=True), True),
         "many": (dict(n_lamps=64, spots=True), False)}
# the eight loads of tests/test_nee_lights.py that span TEX x ALPHA x SUN (lit.gltf four times, the emitter cloud four times); "<load>_map":
# the same under the sky map, which makes every kernel a TEX one and, with PTX_NEE_ENV_SAMPLES, an ENV one
LOADS = ["lit", "lit_nosun", "lit_opaque", "lit_opaque_nosun"] + sorted(CLOUDS)
_built = {}


def _load_of(name):
    """the load a name stands for, or None: 'lit_nosun_map' -> 'lit_nosun'"""
    base = name[:-4] if name.endswith("_map") else name
    return base if base in LOADS else None


def _new_product(ptx, ctx, name):
    load = _load_of(name)
    if load in LIT_LOADS:
        sun, work = LIT_LOADS[load]
        return ptx.Scene.load_gltf(ctx, LIT, sun_light_index=sun, work=work)
    return product_from_dict(ptx, ctx, _lit_dict(load) if load else _dict_and_lights(name)[0])


def _box_lamps(ptx, name, n=6, seed=41):
    """n lamps scattered (seeded) through the middle of the scene's box, odd ones spots aimed at its centre with wide cones, intensities
    scaled with the box so that a lamp's irradiance across the scene is of order 1"""
    box = _new_product(ptx, None, name).array(ptx.ARR_MODEL_AABB).reshape(-1, 6).astype(np.float64)
    lo, hi = box[:, :3].min(0), box[:, 3:].max(0)
    rng = np.random.default_rng(seed)
    lights = np.zeros((n, 16), f32)
    for k in range(n):
        pos = lo + rng.uniform(0.15, 0.85, 3) * (hi - lo)
        aim = 0.5 * (lo + hi) + rng.uniform(-0.1, 0.1, 3) * (hi - lo) - pos
        lights[k, 0:3] = pos
        lights[k, 4:7] = aim / np.linalg.norm(aim)
        lights[k, 7] = k % 2
        lights[k, 8:11] = rng.uniform(0.4, 1.0, 3) * 0.3 * float(((hi - lo) ** 2).sum()) * 10.0 ** rng.uniform(-0.5, 0.5)
        lights[k, 11], lights[k, 12] = (np.cos(0.7), np.cos(1.2)) if k % 2 else (1.0, np.cos(np.pi / 4))
    return lights


def _dict_and_lights(name, ptx=None):
    """-> (scene dict, or None for a load of lit.gltf; lights [n, 16]; whether the sky map is set). ptx: needed the first time a load is asked for"""
    if name not in _built:
        load = _load_of(name)
        if load is not None:
            _built[name] = (None if load in LIT_LOADS else _lit_dict(load), _box_lamps(ptx, name), name.endswith("_map"))
        elif name.startswith("chart"):     # pass-through patches and a sun: the (ALPHA, SUN) kernels; "chart_map": the (TEX, ALPHA, SUN) ENV ones
            d = _proc().chart_scene(facing=True, alpha=True, sun=0.004732)
            _built[name] = (d, _proc().lamp_scene(6, chart=True, spots=True)[1], name == "chart_map")
        else:
            kw, sky = CASES[name]
            _built[name] = (*_proc().lamp_scene(**kw), sky)
    return _built[name]


def _make(ptx, ctx, name):
    d, lights, sky = _dict_and_lights(name, ptx)
    s = _new_product(ptx, ctx, name)
    if sky:
        s.set_environment(SKY, srgb=False)
    s.set_punctual_lights(lights)
    return s


PRODUCTS = Scenes(_make)
_oracles, _refs = {}, {}


def _oracle_and_table(ptx, ora, name, flags):
    key = (name, bool(flags & ENV))
    if key not in _oracles:
        d, _, sky = _dict_and_lights(name, ptx)
        if d is None:
            sun, work = LIT_LOADS[_load_of(name)]
            o = ora.OracleScene(ora.load_gltf(LIT, sun_light_index=sun, work=work))
        else:
            o = oracle_from_dict(ora, d)
        tab = None
        if sky:
            o.set_environment(SKY, srgb=False)
            if flags & ENV:
                s = _make(ptx, None, name)
                tab = _table(ptx, s)
        _oracles[key] = (o, tab)
    return _oracles[key]


def _restated(ptx, ora, name, flags, M, W, H, spp, b, **kw):
    """the restated per-sample radiance of a case, computed once and left unchanged"""
    key = (name, flags, M, W, H, spp, b, tuple(sorted(kw.items())))
    if key not in _refs:
        o, tab = _oracle_and_table(ptx, ora, name, flags)
        ref = render_samples(ora, o, o.a, W, H, spp, b, tab=tab, M=M, spdf=bool(flags & SPDF), seed=SEED, punctual=_dict_and_lights(name)[1], **kw)
        ref["rad"].setflags(write=False)
        _refs[key] = ref
    return _refs[key]


def _route(ptx, ctx, mp, name, route):
    r = route_named(DEFAULT_ROUTES, route)
    return on_route(PRODUCTS, ptx, ctx, mp, name, r), r.pipeline


def _samples(ptx, ctx, s, W, H, spp, b, flags, M, pipeline, **kw):
    """per-sample radiance [H, W, spp, 3] from one call per sample, the route asserted on every call -> (radiance, summed stats)"""
    got = np.zeros((H, W, spp, 3), f32)
    tot = dict(light_samples=0, light_visible=0, rays=0)
    for k in range(spp):
        acc, st = s.render_nee(W, H, 1, b, seed=SEED, sample0=k, flags=flags, candidates=M, **kw)
        tm = ctx.timing()
        assert tm["pipeline"] == pipeline and tm["fused_launches"] == (1 if pipeline == 0 and flags & FUSED else 0), tm
        assert (acc[..., 3] == 1).all()
        got[:, :, k] = acc[..., :3]
        for key in tot:
            tot[key] += st[key]
    return got, tot


# ---------------------------------------------------------------------------- per-sample radiance
A_CASES = [("chart", 0, 1), ("cloud", 0, 1), ("cloud_opaque_nosun", SPDF, 4), ("lit", 0, 1), ("lit_opaque_nosun_map", ENV, 2), ("point", 0, 1), ("spot", 0, 1), ("blocked", 0, 1), ("range", 0, 1), ("lamps_emit", 0, 1), ("lamps_emit_map", ENV, 1),
           ("lamps_emit_map", ENV | SPDF, 1), ("lamps_emit_map", ENV, 2), ("lamps_emit_map", ENV | SPDF, 16), ("lamps_emit", 0, 16)]


@pytest.mark.gpu
@pytest.mark.parametrize("route", [r.name for r in DEFAULT_ROUTES])
@pytest.mark.parametrize("name,flags,M", A_CASES, ids=lambda v: str(v))
def test_per_sample_radiance_against_the_restatement(ptx, ctx, ora, clean_env, name, flags, M, route):
    """The bar of test_nee.py and test_nee_lights.py, unchanged: every sample finite and >= 0, >= 99.5 % within 1e-3 relative (floor 1e-3),
    light samples and rays within 0.5 % + 1. A point light alone (c_p = 1); a spot whose cone edge crosses the frame; a lamp behind the
    blocker; a lamp whose range ends on the floor; eight lamps with an emitter (c_p = 0.5); the same under the sky map with
    PTX_NEE_ENV_SAMPLES, with PTX_NEE_SAMPLER_PDF and with 2 and 16 candidates. And lamps on the scenes of the older tests: the chart with
    pass-through patches and a sun, the emitter cloud (four rotated, non-uniformly scaled models: the hit distance of the visibility rule is
    a world distance there), and lit.gltf (textures, an instance turned and scaled), alone and under the map. The fused routes run k_nee_fused's PUN variants, the queue route
    k_nee_shade's.
    Measured on the MI355X, the same on the three routes: light samples, visible ones and rays equal to the restated counts in all fifteen
    cases (blocked: 1287 / 1100 / 4106; cloud: 810 / 421 / 5252). 100 % of the samples within 1e-3 in thirteen: worst error 3.7e-7 on
    lamp_scene without a map, 1.8e-5 under it, 3.5e-6 on the chart, 2.1e-6 on the cloud. lit.gltf: 99.935 % (worst 3.6e-3), under the map
    99.870 % (worst 3.6e-3): its float sRGB emitter's powf differs between the device's and the host's library, as test_nee_lights notes."""
    W, H, spp, b = 32, 24, 2, 3
    _dict_and_lights(name, ptx)
    ref = _restated(ptx, ora, name, flags, M, W, H, spp, b)
    s, pipeline = _route(ptx, ctx, clean_env, name, route)
    got, tot = _samples(ptx, ctx, s, W, H, spp, b, flags | FUSED, M, pipeline)
    assert np.isfinite(got).all() and (got >= 0).all()
    e = _err(got, ref["rad"])
    share = (e <= 1e-3).mean()
    print(f"{name} / {flags} / M {M} / {route}: {share * 100:.3f} % of samples within 1e-3, worst {e.max():.3g}; light samples {tot['light_samples']} "
          f"(restated {ref['light_samples']}), visible {tot['light_visible']} (restated {ref['light_visible']}), rays {tot['rays']} (restated {ref['rays']})")
    assert ref["light_samples"] > 0 and 0 < ref["light_visible"] and share >= 0.995
    if name == "blocked":
        assert ref["light_visible"] < ref["light_samples"]
    assert abs(tot["light_samples"] - ref["light_samples"]) <= 0.005 * ref["light_samples"] + 1
    assert abs(tot["rays"] - ref["rays"]) <= 0.005 * ref["rays"] + 1
    # the lamps change the frame: ptx_render, which ignores them, gives another
    plain, _ = s.render(W, H, 1, b, seed=SEED)
    assert (_bits(plain[..., :3]) != _bits(got[:, :, 0])).any()


@pytest.mark.gpu
@pytest.mark.parametrize("name", ["blocked", "spot"])
def test_first_punctual_sample_bitwise(ptx, ctx, ora, clean_env, name):
    """test_nee_lights' construction D: 2 bounces under a black environment, so that a sample's radiance is the punctual sample of vertex 0
    alone, x = ((T * b) * E) / (c_p * pmf) or nothing: its direction (through b and the shadow ray), E and its visibility. <= 0.5 % of the
    samples may differ in a bit; both forms.
    Measured on the MI355X: none of 6144 differs in either form (blocked: 4201 not black, 4897 light rays; spot: 603 and 603)."""
    W, H, spp, b = 48, 32, 4, 2
    ref = _restated(ptx, ora, name, 0, 1, W, H, spp, b, env=(0.0, 0.0, 0.0))
    s, pipeline = _route(ptx, ctx, clean_env, name, "lds fused")
    for flags in (0, FUSED):
        got, tot = _samples(ptx, ctx, s, W, H, spp, b, flags, 1, pipeline, env=(0.0, 0.0, 0.0))
        differ = (_bits(got) != _bits(ref["rad"])).any(-1)
        lit = (ref["rad"] > 0).any(-1)
        print(f"{name} / {flags}: {differ.sum()} of {differ.size} samples differ ({lit.sum()} of them not black); light samples {tot['light_samples']} "
              f"(restated {ref['light_samples']}), visible {tot['light_visible']} (restated {ref['light_visible']})")
        assert lit.mean() > 0.05 and (~lit).mean() > 0.02 and differ.sum() <= 0.005 * differ.size   # the spot's cone covers a tenth of the frame
        assert abs(tot["light_samples"] - ref["light_samples"]) <= 0.005 * ref["light_samples"] + 1
        assert abs(tot["light_visible"] - ref["light_visible"]) <= 0.005 * ref["light_visible"] + 1


# ---------------------------------------------------------------------------- fused against unfused
def _hybrid(ptx, ctx, mp, name):
    """the scene with one byte too little LDS for all of its surfaces (tests/_nee_lit_scenes._hybrid_budget's rule), the fused kernel asked for"""
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


FUSED_SETS = {"lamps_emit": [(0, 1), (SPDF, 1), (0, 4), (SPDF, 3), (NO_LIGHTS, 1), (NO_LIGHTS, 4)],
              "lamps_emit_map": [(ENV, 1), (ENV | SPDF, 1), (ENV, 4), (ENV | SPDF, 16), (ENV | NO_LIGHTS, 2)],
              "chart": [(0, 1), (SPDF, 2), (0, 4)], "chart_map": [(ENV, 1), (ENV | SPDF, 1), (ENV, 4), (ENV | SPDF, 4)]}


@pytest.mark.gpu
@pytest.mark.parametrize("route", ["lds fused", "hybrid", "global fused"])
@pytest.mark.parametrize("name", sorted(FUSED_SETS))
def test_fused_is_unfused_bitwise_with_lamps(ptx, ctx, clean_env, name, route):
    """PTX_NEE_FUSED against the unflagged call, bitwise with equal stats (_nee_common._pair), on the three places of the geometry: the floor
    scene (no texture, alpha or sun code), the same under the map (TEX, ENV), the chart with pass-through patches and a sun, and that under
    the map, each with and without PTX_NEE_SAMPLER_PDF and candidates: the PUN variants of all four pairs of translation units, the
    256-thread ones (ENV, SUN, RIS and SPDF together) included. With PTX_NEE_NO_LIGHT_SAMPLES the lamps are the only strategy but the map."""
    if route == "hybrid":
        s = _hybrid(ptx, ctx, clean_env, name)
    else:
        s = _route(ptx, ctx, clean_env, name, route)[0]
    W, H = (48, 40) if name.startswith("chart") else (40, 28)
    for flags, M in FUSED_SETS[name]:
        got, st = _pair(ptx, ctx, s, W, H, 3, 4, flags=flags | CAND(M))
        assert st["light_samples"] > st["light_visible"] > 0, (flags, M, st)
    dark, _ = s.render_nee(W, H, 3, 4, seed=SEED, flags=FUSED)
    s.set_punctual_lights(None)
    unlit, _ = s.render_nee(W, H, 3, 4, seed=SEED, flags=FUSED)
    s.set_punctual_lights(_dict_and_lights(name)[1])
    assert (_bits(dark) != _bits(unlit)).any()
    if route == "hybrid":
        s.close()


LOAD_SETS = [(0, 1), (SPDF, 1), (0, 4), (SPDF, 3)]


@pytest.mark.gpu
@pytest.mark.parametrize("route", ["lds fused", "hybrid", "global fused"])
@pytest.mark.parametrize("name", LOADS + [n + "_map" for n in LOADS[:4]])
def test_every_pun_variant_of_the_fused_form_bitwise(ptx, ctx, clean_env, name, route):
    """test_nee_lights' B with lamps set. Its eight loads span TEX x ALPHA x SUN; the four loads of lit.gltf under the sky map with
    PTX_NEE_ENV_SAMPLES span ENV x ALPHA x SUN: the twelve (TEX, ALPHA, SUN, ENV) combinations the launchers know. Each on the three places of
    the geometry, each plain, with PTX_NEE_SAMPLER_PDF, with candidates and with both: all 144 PUN variants of k_nee_fused against the 48 PUN
    variants of k_nee_shade, bitwise with equal stats and one launch per pass (_nee_common._pair). 48 x 32, 3 spp, 4 bounces.
    Measured on the MI355X: all 36 pass."""
    _dict_and_lights(name, ptx)
    if route == "hybrid":
        s = _hybrid(ptx, ctx, clean_env, name)
    else:
        s = _route(ptx, ctx, clean_env, name, route)[0]
    env = ENV if name.endswith("_map") else 0
    for flags, M in LOAD_SETS:
        got, st = _pair(ptx, ctx, s, 48, 32, 3, 4, flags=flags | env | CAND(M))
        assert st["light_samples"] > 0 and st["light_visible"] > 0 and st["n_lights"] > 0, (flags, M, st)
    lamps, _ = s.render_nee(48, 32, 3, 4, seed=SEED, flags=FUSED | env)
    s.set_punctual_lights(None)
    unlit, _ = s.render_nee(48, 32, 3, 4, seed=SEED, flags=FUSED | env)
    s.set_punctual_lights(_dict_and_lights(name)[1])
    assert (_bits(lamps) != _bits(unlit)).any()
    if route == "hybrid":
        s.close()


@pytest.mark.gpu
def test_fused_composition_and_queue_fallback_with_lamps(ptx, ctx, clean_env):
    """test_nee_fused's composition on the eight-lamp scene under the map: a 5 x 3 frame at 3 spp, tiles, two sample ranges, pass sizes that
    cut the frame, two and three shards summing to the unsharded frame, host and device buffers, and the queue route, where PTX_NEE_FUSED is
    ignored. 24 x 16 at 8 spp, as test_nee_fused's and test_nee_ris' composition tests have it: the sample ranges 3 + 5 and the pass sizes 1
    and 3 need more than the 2 to 4 samples of the other tests here."""
    s, _ = _route(ptx, ctx, clean_env, "lamps_emit_map", "lds fused")
    small, _ = _pair(ptx, ctx, s, 5, 3, 3, 3, flags=ENV | CAND(4))
    assert np.isfinite(small).all()
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
    import torch
    dev = torch.zeros((H, W, 4), dtype=torch.float32, device="cuda")
    s.render_nee(W, H, spp, b, accum=dev, seed=SEED, flags=F)
    _same(dev.cpu().numpy(), whole, "device buffer")
    q, pipeline = _route(ptx, ctx, clean_env, "lamps_emit_map", "queue")
    assert pipeline == 1
    got, _ = _pair(ptx, ctx, q, W, H, spp, b, fused=False, flags=ENV | CAND(4))
    _same(got, whole, "queue route")


@pytest.mark.gpu
def test_queue_route_with_a_forced_pool_overflow_with_lamps(ptx, ctx, clean_env):
    """test_nee_lights' pool switches on the 64-lamp scene: a 1 Mi-pair pool and a guess of 0.25 pairs per ray; 800 x 600 x 4 camera rays
    overflow it. The frame is the unforced queue frame and the 'lds fused' frame, bit for bit, stats included. The frame is as large as
    test_nee_lights': the pool overflows only with more than 2^20 (ray, surface) pairs in a slice, which no small frame has."""
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


# ---------------------------------------------------------------------------- no punctual lights
@pytest.mark.gpu
@pytest.mark.parametrize("route", [r.name for r in DEFAULT_ROUTES])
def test_without_punctual_lights_no_bit_changes(ptx, ctx, clean_env, route):
    """A scene on which lights were set with n = 0, a scene on which they were set, used and cleared, and a scene on which all-black lights
    were set: each is bitwise, stats included, the call on the scene nobody touched, in both forms and with flags; and with the emitters
    switched off and no lamps the frame is ptx_render's."""
    W, H, spp, b = 32, 24, 4, 3
    r = route_named(DEFAULT_ROUTES, route)
    d, lights, _ = _dict_and_lights("lamps_emit")

    def fresh():
        def make():      # the map goes up with the scene: set_environment uploads again, under the switches of that moment
            s = product_from_dict(ptx, ctx, d)
            s.set_environment(SKY, srgb=False)
            return s
        return under_force_global(clean_env, r.force_global, make)
    untouched, zero, cleared, black = fresh(), fresh(), fresh(), fresh()
    for k, v in r.env.items():
        clean_env.setenv(k, v)
    zero.set_punctual_lights(np.zeros((0, 16), f32))
    cleared.set_punctual_lights(lights)
    lit, _ = cleared.render_nee(W, H, spp, b, seed=SEED)
    cleared.set_punctual_lights(None)
    black.set_punctual_lights(lights * f32([1] * 8 + [0] * 3 + [1] * 5))
    for flags in (0, FUSED, ENV | SPDF | CAND(4), ENV | SPDF | CAND(4) | FUSED, NO_LIGHTS | FUSED):
        want, st0 = untouched.render_nee(W, H, spp, b, seed=SEED, flags=flags)
        assert ctx.timing()["pipeline"] == r.pipeline
        for tag, s in (("n = 0", zero), ("cleared", cleared), ("black", black)):
            got, st = s.render_nee(W, H, spp, b, seed=SEED, flags=flags)
            _same(got, want, f"{route} / {flags} / {tag}")
            assert all(st[k] == st0[k] for k in SAME_STATS), (tag, st, st0)
        if flags == 0:
            assert (_bits(lit) != _bits(want)).any()
        if flags == NO_LIGHTS | FUSED:
            _same(want, untouched.render(W, H, spp, b, seed=SEED)[0], "ptx_render")
    for s in (untouched, zero, cleared, black):
        s.close()


# ---------------------------------------------------------------------------- adaptive
@pytest.mark.gpu
@pytest.mark.parametrize("route,flags", [("lds fused", FUSED), ("lds fused", 0), ("queue", CAND(4))])
def test_adaptive_with_lamps_is_the_calls_of_the_half_ranges(ptx, ctx, clean_env, route, flags):
    """tests/test_adaptive_nee.py's snapshot method on the eight-lamp scene, 48 x 32, 3 bounces, 8 samples first, 8 per round, cap 24: a pixel
    with n samples holds, in A and in B, what the ptx_render_nee calls of the same half ranges leave, and the counts are the replayed decision's.
    The cap of 24 samples is test_adaptive_nee's and test_nee_ris': three rounds need it."""
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
    s.set_punctual_lights(None)
    plain_a, _, _ = s.render_adaptive_nee(W, H, cap, b, 8, 8, thr, seed=SEED, flags=flags)
    s.set_punctual_lights(_dict_and_lights("lamps_emit")[1])
    assert (_bits(plain_a) != _bits(got_a)).any()


# ---------------------------------------------------------------------------- mirrors
@pytest.mark.gpu
def test_mirrors_and_cli_on_the_lamps_file(ptx, ctx, clean_env, tmp_path):
    """lamps.gltf with its own lamps set: the C call against Scene.render_nee, Renderer.set_punctual_lights + render_nee (python) and
    ptx_render_cli --nee --nee-punctual (core::renderer's read_punctual_lights and set_punctual_lights), bit for bit; --nee-punctual without
    --nee is an error message"""
    from PIL import Image
    W, H, spp, b = 24, 16, 8, 3
    lamps = ptx.read_punctual_lights(LAMPS)
    s = ptx.Scene.load_gltf(ctx, LAMPS)
    unlit, _ = s.render_nee(W, H, spp, b, seed=SEED)
    assert ptx.lib().ptx_scene_set_punctual_lights(s.h, lamps.ctypes.data, len(lamps)) == 0
    cfg = ptx.RenderCfg(W, H, spp, b, (C.c_float * 3)(1, 1, 1), SEED, 0, 0, 0, W, H, 0, 0, 0, 0, 0, 0)
    want = np.zeros((H, W, 4), f32)
    st = ptx.NeeStats()
    assert ptx.lib().ptx_render_nee(s.h, C.byref(cfg), C.byref(ptx.NeeCfg(0)), want.ctypes.data, C.byref(st)) == 0
    assert st.light_samples > st.light_visible > 0 and st.n_lights == 0 and (_bits(unlit) != _bits(want)).any()
    _same(s.render_nee(W, H, spp, b, seed=SEED)[0], want, "Scene.render_nee")
    _same(s.render_nee(W, H, spp, b, seed=SEED, flags=FUSED)[0], want, "Scene.render_nee, fused")
    r = ptx.Renderer(0)
    r.resolution, r.sample_count, r.bounce_count, r.seed = (W, H), spp, b, SEED
    r.load_gltf(LAMPS)
    _same(r.render_nee(), unlit, "Renderer.render_nee before the lamps are set")
    r.set_punctual_lights(lamps)
    _same(r.render_nee(), want, "Renderer.render_nee")
    assert r.last_nee_stats["light_samples"] == st.light_samples and r.last_nee_stats["light_visible"] == st.light_visible
    cli = os.path.join(ROOT, "distributed-path-tracer_amd", "ptx_render_cli")
    for switches in (["--nee", "--nee-punctual"], ["--nee-punctual", "--nee-fused"]):
        out = subprocess.run([cli, *switches, LAMPS, str(tmp_path / "f.png"), str(W), str(H), str(spp), str(b)], capture_output=True, text=True, timeout=120)
        assert out.returncode == 0, out.stderr
        np.testing.assert_array_equal(np.array(Image.open(tmp_path / "f.png")), ctx.tonemap_encode(want, W, H, spp))
        js = json.loads(out.stdout)
        assert js["nee_light_samples"] == st.light_samples and js["nee_light_visible"] == st.light_visible and js["nee_punctual_lights"] == 4
    out = subprocess.run([cli, "--nee-punctual", LAMPS, str(tmp_path / "g.png"), str(W), str(H), str(spp), str(b)], capture_output=True, text=True, timeout=120)
    assert out.returncode == 1 and "--nee-punctual needs --nee" in out.stderr and not (tmp_path / "g.png").exists()
    s.close()
