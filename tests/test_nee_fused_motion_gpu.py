"""PTX_NEE_FUSED | PTX_NEE_FUSED_MOTION on the GPU (include/ptx.h): under active motion the fused kernel with a time per lane
(csrc/nee_fused_motion.hip) renders, bit for bit, what the unfused form renders under the same motion — frame and stats.

Every comparison is bitwise. "Unfused" is the same call without the two bits on the same scene under the same motion;
tests/test_motion_blur_gpu.py ties that form, sample by sample, to the static scene at the sample's own time, and equality of bits carries
it over. Frames are 16 x 12 or smaller at 3 to 4 spp and 3 bounces. One shape is not a 16 x 12 frame: a tile of exactly 129 paths
(two waves and one path) needs 43 pixels at 3 spp, and 43 is prime, so that tile is one row of a 43 x 3 frame (129 pixels, fewer than 192).
"""
import os

import numpy as np
import pytest

from _common import _bits, _same
from _fused_motion_common import FUSED_ROUTES, Routed, turned, with_motion
from _motion_common import begin_camera as _begin_camera, movers as _movers
from _nee_env_restatement import write_hdr
from _routes import clean_env, ctx  # noqa: F401  (fixtures)
from conftest import GOLD

f32 = np.float32
pytestmark = pytest.mark.gpu

W, H, SPP, B, SEED = 16, 12, 3, 3, 0x5EED
OPEN = (0.2, 0.9)
SAME_STATS = ("rays", "samples", "n_lights", "light_area", "light_samples", "light_visible")
LIT = os.path.join(GOLD, "textures", "lit.gltf")
LAMPS = f32([[0.5, 2.0, 1.0, 0, 0, -1, 0, 0, 6, 5, 4, 0, 0, 0, 0, 0], [-1.0, 1.5, 2.0, 0, 0, -1, 0, 0, 2, 3, 4, 0, 0, 0, 0, 0]])


def _fm(ptx):
    return ptx.NEE_FUSED | ptx.NEE_FUSED_MOTION


@pytest.fixture(scope="module")
def env_map(tmp_path_factory):
    """a small Radiance map: grey with one hot texel"""
    rgb = np.full((8, 16, 3), 0.5)
    rgb[1, 3] = [40.0, 36.0, 24.0]
    return write_hdr(str(tmp_path_factory.mktemp("fused_motion_env") / "hot.hdr"), rgb)


def _pair(ptx, ctx, s, what, w=W, h=H, spp=SPP, bounces=B, flags=0, **kw):
    """the call with FM and without on scene `s`: frames and the six stats equal, one fused launch per pass -> (frame, stats)"""
    want, wst = s.render_nee(w, h, spp, bounces, seed=SEED, flags=flags, **kw)
    t = ctx.timing()
    assert t["fused_launches"] == 0 and t["pipeline"] == 0, (what, t)
    got, gst = s.render_nee(w, h, spp, bounces, seed=SEED, flags=flags | _fm(ptx), **kw)
    t = ctx.timing()
    assert t["pipeline"] == 0 and t["fused_launches"] == gst["passes"] >= 1 and t["fused_ms"] == gst["kernel_ms"], (what, t, gst)
    _same(got, want, f"{what}: the frame of the fused motion kernel against the unfused form's")
    assert all(gst[k] == wst[k] for k in SAME_STATS), (what, gst, wst)
    return got, gst


# ---------------------------------------------------------------------------- 1. routes and shutters
@pytest.mark.parametrize("moving", ["models and camera", "camera alone", "models alone"])
@pytest.mark.parametrize("shutter", [OPEN, (0.3, 0.3)], ids=["open", "degenerate"])
@pytest.mark.parametrize("route", FUSED_ROUTES)
def test_routes_and_shutters(ptx, ctx, clean_env, route, shutter, moving):
    """The movers on the three fused routes. With the camera alone models_moved == 0 and the static traversal runs; with the models alone
    the camera is the scene's. 576 samples put many times into every wave: a time taken wave-uniformly fails under the open shutter.
    Fails on the parent, which refuses the flag."""
    d = _movers()
    R = Routed(ptx, ctx, clean_env, route, d)
    a = with_motion(R, d, shutter, models=moving != "camera alone", camera=moving != "models alone")
    moved = a.array(ptx.ARR_MOTION_MOVED)
    assert bool(moved.any()) == (moving != "camera alone")
    got, st = _pair(ptx, ctx, a, f"{route}, {shutter}, {moving}")
    assert st["light_samples"] > 0 and st["n_lights"] == 2
    a.clear_motion()
    still, _ = a.render_nee(W, H, SPP, B, seed=SEED)
    assert (_bits(got) != _bits(still)).any(), "the frame under motion is not the frame of the scene at u = 1"
    a.close()


# ---------------------------------------------------------------------------- 2. variants
# tests/test_motion_blur_gpu.py's table, and the fullest combination: the smallest workgroup
VARIANTS = {
    "lens": dict(lens=(0.08, 5.0, 6, 0.3)),
    "sun and pass-through": dict(scene=(False, True, True)),
    "env samples": dict(flags="NEE_ENV_SAMPLES", env_map=True),
    "sampler pdf": dict(flags="NEE_SAMPLER_PDF"),
    "candidates": dict(candidates=4),
    "punctual": dict(punctual=True),
    "emissive mover, no light samples": dict(scene=(True, False, False), flags="NEE_NO_LIGHT_SAMPLES"),
    "emissive mover": dict(scene=(True, False, False)),
    "fullest": dict(scene=(False, True, False), flags="NEE_ENV_SAMPLES|NEE_SAMPLER_PDF", env_map=True, candidates=4, punctual=True),
}


def _flags(ptx, names):
    f = 0
    for n in names.split("|") if names else ():
        f |= getattr(ptx, n)
    return f


def _variant_scene(ptx, R, v, env_map):
    d = _movers(*v.get("scene", ()))
    a = with_motion(R, d, OPEN, lens=v.get("lens"))
    if v.get("env_map"):
        R.creating(lambda: a.set_environment(env_map, srgb=False))   # the scene goes up again: under the route's creation switches
    if v.get("punctual"):
        a.set_punctual_lights(LAMPS)
    assert a.info()["lds_resident"] == R.resident, (R.route, a.info())
    assert a.array(R.ptx.ARR_MOTION_MOVED).any(), "the motion outlives the upload"
    return d, a


def _strategy_ran(ptx, a, v, got, st, what):
    """from the stats and the scene that the intended strategy ran, and that it changes the frame"""
    info = a.info()
    flags = v.get("flags", "")
    assert info["has_sun"] == (1 if len(v.get("scene", ())) > 1 and v["scene"][1] else 0), (what, info)
    assert (info["n_textures"] > 0) == bool(v.get("env_map")), (what, info)
    if "NO_LIGHT" in flags:
        assert st["light_samples"] == 0 and st["n_lights"] == 2, (what, st)
        return
    assert st["light_samples"] > 0 and st["light_visible"] > 0 and st["n_lights"] == 2, (what, st)   # a moving emitter is not listed
    if flags or v.get("candidates", 1) > 1 or v.get("punctual"):
        if v.get("punctual"):
            a.set_punctual_lights(None)
        plain, pst = a.render_nee(W, H, SPP, B, seed=SEED)
        assert (_bits(plain) != _bits(got)).any(), f"{what}: the frame does not depend on the variant's flags"
        if v.get("punctual") and not flags and v.get("candidates", 1) == 1:
            assert st["light_samples"] >= pst["light_samples"], (what, st, pst)


@pytest.mark.parametrize("name", list(VARIANTS))
def test_variants(ptx, ctx, clean_env, env_map, name):
    """each row once under the open shutter on the LDS route, against unfused with the same flags"""
    v = VARIANTS[name]
    R = Routed(ptx, ctx, clean_env, "lds fused", _movers(*v.get("scene", ())))
    d, a = _variant_scene(ptx, R, v, env_map)
    got, st = _pair(ptx, ctx, a, name, flags=_flags(ptx, v.get("flags")), candidates=v.get("candidates", 1))
    _strategy_ran(ptx, a, v, got, st, name)
    a.close()


# Coverage: each of the 8 parts (SPDF = 1, RIS = 2, PUN = 4: the high bits of the variant mask) in each of the three modes, with scene bits
# chosen so that TEX, ALPHA, SUN and ENV are each on and off at least once in each mode. A map on the scene is TEX; with NEE_ENV_SAMPLES, ENV.
#        part: (emissive, sun, alpha), map, env samples          scene mask (ENV SUN ALPHA TEX)
PART_SCENES = {0: ((False, False, False), False, False),       # 0000
               1: ((False, False, False), True, True),         # 1001
               2: ((False, True, True), False, False),         # 0110
               3: ((False, True, False), True, False),         # 0101
               4: ((False, False, True), False, False),        # 0010
               5: ((False, True, True), True, True),           # 1111
               6: ((False, True, False), False, False),        # 0100
               7: ((False, True, False), True, True)}          # 1101


def test_part_table_covers_every_scene_bit():
    """no GPU work: the table above has each scene bit on and off (runs with the GPU file because the table lives here)"""
    for bit in ("tex", "alpha", "sun", "env"):
        on = {p: {"tex": m, "alpha": s[2], "sun": s[1], "env": e}[bit] for p, (s, m, e) in PART_SCENES.items()}
        assert any(on.values()) and not all(on.values()), bit
    assert sorted(PART_SCENES) == list(range(8))


@pytest.mark.parametrize("part", sorted(PART_SCENES))
@pytest.mark.parametrize("route", FUSED_ROUTES)
def test_every_part_in_every_mode(ptx, ctx, clean_env, env_map, route, part):
    scene, has_map, env_samples = PART_SCENES[part]
    flags = ("NEE_SAMPLER_PDF" if part & 1 else "") + ("|NEE_ENV_SAMPLES" if env_samples else "")
    v = dict(scene=scene, flags=flags.strip("|"), env_map=has_map, candidates=4 if part & 2 else 1, punctual=bool(part & 4))
    R = Routed(ptx, ctx, clean_env, route, _movers(*scene))
    d, a = _variant_scene(ptx, R, v, env_map)
    assert a.info()["lds_resident"] == R.resident
    what = f"part {part} on {route}"
    got, st = _pair(ptx, ctx, a, what, flags=_flags(ptx, v["flags"]), candidates=v["candidates"])
    info = a.info()
    assert info["has_sun"] == int(scene[1]) and (info["n_textures"] > 0) == has_map, (what, info)
    assert st["light_samples"] > 0 and st["light_visible"] > 0, (what, st)
    a.close()


def test_textured_model_moves(ptx, ctx, clean_env):
    """lit.gltf (textures, normal maps, an instance turned and scaled, blended surfaces, a sun) with the begin transforms of its models a few
    degrees and centimetres off: hit_attributes_at on textured moving surfaces"""
    clean_env.setenv("PTX_WAVEFRONT", "0")
    a = ptx.Scene.load_gltf(ctx, LIT)
    info = a.info()
    assert info["lds_resident"] == 1 and info["n_textures"] > 0 and info["has_sun"] == 1, info
    cur = a.array(ptx.ARR_MODEL_XFORM)
    a.set_motion(turned(cur, 4.0, (0.03, -0.02, 0.05)), None, OPEN)
    assert a.array(ptx.ARR_MOTION_MOVED).all()
    got, st = _pair(ptx, ctx, a, "lit.gltf, every model moving", flags=ptx.NEE_NO_LIGHT_SAMPLES)
    assert st["rays"] > st["samples"]
    a.clear_motion()
    still, _ = a.render_nee(W, H, SPP, B, seed=SEED, flags=ptx.NEE_NO_LIGHT_SAMPLES)
    assert (_bits(got) != _bits(still)).any()
    a.close()


# ---------------------------------------------------------------------------- 3. work distribution and composition
@pytest.fixture
def movers_lds(ptx, ctx, clean_env):
    d = _movers()
    R = Routed(ptx, ctx, clean_env, "lds fused", d)
    a = with_motion(R, d, OPEN)
    yield a
    a.close()


@pytest.mark.parametrize("shape", ["1 x 1", "64 paths", "129 paths"])
def test_tiles_below_at_and_above_a_wave(ptx, ctx, movers_lds, shape):
    """fewer paths than a wave (3), one wave exactly (a 4 x 4 tile at 4 spp), two waves and one path (43 pixels at 3 spp: see the module's text)"""
    w, h, spp, tile = {"1 x 1": (W, H, 3, (5, 7, 1, 1)), "64 paths": (W, H, 4, (3, 2, 4, 4)), "129 paths": (43, 3, 3, (0, 1, 43, 1))}[shape]
    got, st = _pair(ptx, ctx, movers_lds, shape, w=w, h=h, spp=spp, tile=tile)
    assert st["samples"] == {"1 x 1": 3, "64 paths": 64, "129 paths": 129}[shape] and st["passes"] == 1


def test_passes_and_bounces(ptx, ctx, movers_lds):
    a = movers_lds
    full, fst = _pair(ptx, ctx, a, "one pass", spp=4)
    one, ost = _pair(ptx, ctx, a, "spp_per_pass = 1", spp=4, spp_per_pass=1)
    assert ost["passes"] == 4 and fst["passes"] == 1
    _same(one, full, "spp_per_pass = 1 against one pass")
    black, bst = _pair(ptx, ctx, a, "bounces = 0", spp=4, bounces=0)
    assert (black[..., :3] == 0).all() and (black[..., 3] == 4).all() and bst["rays"] == 0
    first, _ = _pair(ptx, ctx, a, "bounces = 1", spp=4, bounces=1)
    assert (first[..., 3] == 4).all() and (_bits(first) != _bits(full)).any()


def test_composition(ptx, ctx, movers_lds):
    torch = pytest.importorskip("torch")
    a, FM, spp = movers_lds, _fm(ptx), 4
    full, _ = a.render_nee(W, H, spp, B, seed=SEED)   # unfused
    kw = dict(seed=SEED, flags=FM, want_stats=False)
    tiles = np.zeros_like(full)
    for (x0, y0, w, h) in ((0, 0, 7, 12), (7, 0, 9, 5), (7, 5, 9, 7)):
        t, _ = a.render_nee(W, H, spp, B, tile=(x0, y0, w, h), **kw)
        tiles[y0:y0 + h, x0:x0 + w] = t
    _same(tiles, full, "three tile rectangles")
    acc = np.zeros_like(full)
    for s0, n in ((0, 1), (1, 2), (3, 1)):
        a.render_nee(W, H, n, B, accum=acc, sample0=s0, **kw)
    _same(acc, full, "ascending sample ranges into one buffer")
    for count in (2, 3):
        acc = np.zeros_like(full)
        for k in range(count):
            a.render_nee(W, H, spp, B, accum=acc, shard=(k, count, 4), **kw)
        _same(acc, full, f"{count} shards")
    dev = torch.zeros((H, W, 4), dtype=torch.float32, device="cuda")
    torch.cuda.synchronize()   # the fill runs on torch's stream, the library on its own
    a.render_nee(W, H, spp, B, accum=dev, **kw)
    ctx.synchronize()
    _same(dev.cpu().numpy(), full, "device buffer")


def test_adaptive_rounds_run_fused(ptx, ctx, movers_lds):
    """ptx_render_adaptive_nee with FM against the unfused adaptive call: a threshold nothing exceeds, and a finite one that leaves some
    pixels active after the first round. The finite threshold is the first of a descending list for which the UNFUSED call reports
    0 < active_last < every pixel: chosen from the reference form, never from the code under test."""
    a, FM = movers_lds, _fm(ptx)
    kw = dict(min_spp=2, step_spp=2, seed=SEED)
    finite = None
    for thr in (1.0, 0.5, 0.3, 0.2, 0.1, 0.05, 0.02, 0.01):
        _, _, st = a.render_adaptive_nee(W, H, 4, B, threshold=thr, **kw)
        if 0 < st["active_last"] < W * H and st["rounds"] == 2:
            finite = thr
            break
    assert finite is not None, "no threshold of the list leaves some pixels active"
    for thr in (float("inf"), finite):
        wa, wb, wst = a.render_adaptive_nee(W, H, 4, B, threshold=thr, **kw)
        assert ctx.timing()["fused_launches"] == 0
        ga, gb, gst = a.render_adaptive_nee(W, H, 4, B, threshold=thr, flags=FM, **kw)
        t = ctx.timing()
        assert t["pipeline"] == 0 and t["fused_launches"] == gst["passes"] >= gst["rounds"] and t["fused_ms"] == gst["kernel_ms"], (thr, t, gst)
        _same(ga, wa, f"threshold {thr}: first half")
        _same(gb, wb, f"threshold {thr}: second half")
        assert all(gst[k] == wst[k] for k in SAME_STATS + ("rounds", "active_last")), (thr, gst, wst)
    assert wst["rounds"] == 2 and 0 < wst["active_last"] < W * H


# ---------------------------------------------------------------------------- 4. flag semantics
def test_flag_semantics(ptx, ctx, clean_env):
    d = _movers()
    FM = _fm(ptx)
    R = Routed(ptx, ctx, clean_env, "lds fused", d)
    never, a = R.make(d), R.make(d)
    kw = dict(seed=SEED)
    base, bst = never.render_nee(W, H, SPP, B, flags=ptx.NEE_FUSED, **kw)
    passes = ctx.timing()["fused_launches"]
    assert passes == bst["passes"] >= 1

    def is_the_fused_call(s, what):
        got, st = s.render_nee(W, H, SPP, B, flags=FM, **kw)
        assert ctx.timing()["fused_launches"] == passes and ctx.timing()["pipeline"] == 0, what
        _same(got, base, f"{what}: FM is the NEE_FUSED call")
        assert all(st[k] == bst[k] for k in SAME_STATS + ("passes",)), (what, st, bst)

    is_the_fused_call(never, "never given motion")
    a.set_motion(d["model_xform"], (d["camera"][:3], d["camera"][3:12], d["camera"][12]), OPEN)
    assert not a.array(ptx.ARR_MOTION_MOVED).any()
    is_the_fused_call(a, "all keys equal")
    # under active motion: the bit alone does nothing
    a.set_motion(d["begin_model_xform"], _begin_camera(d), OPEN)
    plain, _ = a.render_nee(W, H, SPP, B, **kw)
    alone, _ = a.render_nee(W, H, SPP, B, flags=ptx.NEE_FUSED_MOTION, **kw)
    assert ctx.timing()["fused_launches"] == 0 and ctx.timing()["pipeline"] == 0
    _same(alone, plain, "NEE_FUSED_MOTION without NEE_FUSED under motion")
    assert (_bits(plain) != _bits(base)).any()
    # the refused entry points still refuse while FM renders
    flagged, _ = a.render_nee(W, H, SPP, B, flags=FM, **kw)
    assert ctx.timing()["fused_launches"] >= 1
    _same(flagged, plain, "FM under motion")
    refused = {
        "ptx_render": lambda s: s.render(W, H, 1, B, **kw),
        "ptx_render_transparent": lambda s: s.render_transparent(W, H, 1, B, **kw),
        "ptx_render_adaptive": lambda s: s.render_adaptive(W, H, 2, B, min_spp=2, **kw),
        "ptx_render_motion": lambda s: s.render_motion(W, H, 1, **kw),
        "ptx_render_emission": lambda s: s.render_emission(W, H, 1, **kw),
        "worker ptx_render_nee": lambda s: s.render_nee(W, H, 1, B, integrator=ptx.INTEGRATOR_WORKER, flags=FM, **kw),
    }
    for k, f in refused.items():
        with pytest.raises(ptx.PtxError) as e:
            f(a)
        assert e.value.code == ptx.ERR_UNSUPPORTED, k
    a.clear_motion()
    is_the_fused_call(a, "cleared")
    for setter in ("set_model_xforms", "set_camera"):
        a.set_motion(d["begin_model_xform"], _begin_camera(d), OPEN)
        if setter == "set_model_xforms":
            a.set_model_xforms(d["model_xform"])
        else:
            a.set_camera(d["camera"][:3], d["camera"][3:12], d["camera"][12])
        is_the_fused_call(a, f"after {setter}")
    a.close(), never.close()


def test_queue_route_ignores_the_bits(ptx, ctx, clean_env):
    d = _movers()
    R = Routed(ptx, ctx, clean_env, "queue", d)
    a = with_motion(R, d, OPEN)
    plain, pst = a.render_nee(W, H, SPP, B, seed=SEED)
    got, gst = a.render_nee(W, H, SPP, B, seed=SEED, flags=_fm(ptx))
    t = ctx.timing()
    assert t["pipeline"] == 1 and t["fused_launches"] == 0, t
    _same(got, plain, "queue route: FM is ignored")
    assert all(gst[k] == pst[k] for k in SAME_STATS + ("passes",)), (gst, pst)
    a.close()
