"""The fused kernel's stream addressing: every array of a wave's stream area is reached as the area's wave-uniform base plus a 32-bit byte
offset (Q4 / Q2, csrc/device_core.hpp). What that form can break and tests/test_stream_prefetch.py does not reach:

  1. The base of EVERY wave slot. A pass of 512 x 256 pixels x 4 samples at 2 bounces is 524 288 camera paths; with chunks that shrink to
     the 128-path minimum (guided self-scheduling, kernels.hip) that is one chunk for each of the 4096 wave slots of a 256-CU grid, the
     last slot included, so a base that is wrong for some slot (the slot index is made wave-uniform by hand) lands in a neighbour's area.
     The pass must be bitwise the same samples rendered in 16 small passes, which use the first slots only.
  2. The far end of the area: the shadow requests (`sreq`, SUN kernels), the read-modify-write of single words in them and in the outgoing
     stream (SHADOW sweep, pass-through), and the deferred lists up to unit 63 (`lists`, the last array of the area). A sun-lit cloud of
     64 models of one surface each — as many units as the deferral allows (kMaxDeferModels), in both unit kinds — with half-transparent
     surfaces and a shadow catcher, so that the SUN / ALPHA kernels run. 64 x 64 pixels, 4 samples, 3 bounces. Model units and surface
     units must give bitwise the same frame, samples and ray count; against the oracle the samples meet the bars of
     tests/test_gpu_parity.py (a path of three bounces goes through libm's cosf / acosf on both sides, so agreement with the oracle is
     not bitwise at any revision; the share of samples that is, is printed). What CAN be bitwise the oracle's is: the same cloud under a
     sun of angular radius 0 at one bounce, where no sample depends on libm (tests/test_material_chart.py, check 1) while shadow
     requests, catcher and pass-through entries and the lists are all in use. Every sample, both unit kinds.
Routes come from the shared harness (tests/_routes.py): residency and pipeline are asserted, so a fallback cannot pass.
"""
import numpy as np
import pytest

from _common import _bits, _proc
from _routes import Route, Scenes, clean_env, ctx, on_route  # noqa: F401  (clean_env and ctx are fixtures)
from conftest import CORNELL, oracle_from_dict, product_from_dict

BW, BH, BSPP, BB = 512, 256, 4, 2           # 1: the pass that fills every wave slot
BANDS = [(0, 64 * k, BW, 64) for k in range(4)]
W, H, SPP, B = 64, 64, 4, 3                 # 2: the cloud
MAX_UNITS = 64                              # kMaxDeferModels (csrc/kernels.hpp)

UNIT_ROUTES = [Route(f"lds fused, {kind} units", False, {"PTX_WAVEFRONT": "0", "PTX_SURFACE_UNITS": v}, 1, 0) for kind, v in (("model", "0"), ("surface", "1"))]


def _cloud(sharp=False):
    """cloud_scene's 64 scattered one-surface models under its sun, with every fourth surface half transparent and one a shadow catcher.
    sharp: a sun of angular radius 0, whose sample involves no libm call (rand_cone_vec multiplies the azimuth's sin / cos by an exact 0)."""
    d = _proc().cloud_scene(MAX_UNITS, 1, 16, layout="scattered")
    m = d["materials"].copy()
    m[1::4, 3] = 0.5
    m[2, 10] = 1.0
    d["materials"] = m
    if sharp:
        d["sun"] = d["sun"].copy()
        d["sun"][12] = 0.0
    return d


def _make(ptx, ctx, name):
    return ptx.Scene.load_gltf(ctx, CORNELL) if name == "cornell" else product_from_dict(ptx, ctx, _cloud(sharp=name == "sharp cloud"))


SCENES = Scenes(_make)


# ---------------------------------------------------------------------------- no GPU
def test_shapes_are_what_they_claim(ptx):
    assert BW * BH * BSPP == 524288 == 4096 * 128          # 256 CUs x 16 waves, the minimum chunk
    cover = np.zeros((BH, BW), int)
    for x, y, w, h in BANDS:
        cover[y:y + h, x:x + w] += 1
    assert (cover == 1).all()
    d = _cloud()
    info = product_from_dict(ptx, None, d).info()
    assert info["n_models"] == MAX_UNITS and info["n_surfaces"] == MAX_UNITS and info["lds_resident"] == 1
    assert info["has_sun"] == 1 and (d["materials"][:, 3] == 0.5).sum() == 16 and d["materials"][:, 10].sum() == 1


# ---------------------------------------------------------------------------- GPU
@pytest.mark.gpu
def test_a_pass_over_every_wave_slot_equals_small_passes(ptx, ctx, clean_env):
    route = Route("lds fused", False, {"PTX_WAVEFRONT": "0"}, 1, 0)
    s = on_route(SCENES, ptx, ctx, clean_env, "cornell", route)
    big, st = s.render(BW, BH, BSPP, BB, spp_per_pass=BSPP)
    assert ctx.timing()["pipeline"] == 0, route.name
    assert st["passes"] == 1 and st["samples"] == BW * BH * BSPP
    assert np.isfinite(big).all() and (big[..., 3] == BSPP).all()
    rays = 0
    for x, y, w, h in BANDS:
        got, gst = s.render(BW, BH, BSPP, BB, tile=(x, y, w, h), spp_per_pass=1)
        assert gst["passes"] == BSPP and ctx.timing()["pipeline"] == 0
        np.testing.assert_array_equal(_bits(got), _bits(np.ascontiguousarray(big[y:y + h, x:x + w])), err_msg=f"band at y = {y}")
        rays += gst["rays"]
    assert rays == st["rays"] and st["rays"] > BW * BH * BSPP


@pytest.mark.gpu
def test_sun_and_pass_through_at_the_unit_limit_in_both_unit_kinds(ptx, ctx, ora, clean_env):
    d = _cloud()
    ref = oracle_from_dict(ora, d).render_samples(ora.make_cfg(W, H, SPP, B), threads=0)
    assert np.isfinite(ref).all()
    first = None
    for route in UNIT_ROUTES:
        s = on_route(SCENES, ptx, ctx, clean_env, "cloud", route)
        assert s.info()["n_models"] == MAX_UNITS and s.info()["has_sun"] == 1, route.name
        frame, st = s.render(W, H, SPP, B)
        assert ctx.timing()["pipeline"] == 0 and st["passes"] == 1, route.name
        smp = np.zeros((H, W, SPP, 3), np.float32)
        for k in range(SPP):
            a, _ = s.render(W, H, 1, B, sample0=k)
            assert ctx.timing()["pipeline"] == 0, route.name
            smp[:, :, k] = a[..., :3]
        assert np.isfinite(frame).all() and np.isfinite(smp).all(), route.name
        assert st["rays"] > W * H * SPP, route.name                      # shadow rays and pass-through on top of the camera rays
        err = np.abs(smp - ref).max(-1) / np.maximum(np.abs(ref).max(-1), 1e-3)
        same = (_bits(smp) == _bits(ref)).all(-1).mean()
        print(f"{route.name}: {(err < 1e-3).mean():.4%} of samples within 1e-3, {(err < 1e-5).mean():.4%} within 1e-5, {same:.4%} bitwise the oracle's")
        assert (err < 1e-3).mean() > 0.995, route.name
        assert (err < 1e-5).mean() > 0.98, route.name
        if first is None:
            first = (frame, smp, st["rays"])
        else:
            np.testing.assert_array_equal(_bits(frame), _bits(first[0]), err_msg=route.name)
            np.testing.assert_array_equal(_bits(smp), _bits(first[1]), err_msg=route.name)
            assert st["rays"] == first[2], route.name


@pytest.mark.gpu
def test_sharp_sun_at_one_bounce_is_bitwise_the_oracle_in_both_unit_kinds(ptx, ctx, ora, clean_env):
    ref = oracle_from_dict(ora, _cloud(sharp=True)).render_samples(ora.make_cfg(W, H, SPP, 1), threads=0)
    assert np.isfinite(ref).all() and len(np.unique(ref.reshape(-1, 3), axis=0)) > 100      # lit, shadowed, passed through, missed
    for route in UNIT_ROUTES:
        s = on_route(SCENES, ptx, ctx, clean_env, "sharp cloud", route)
        smp = np.zeros((H, W, SPP, 3), np.float32)
        for k in range(SPP):
            a, _ = s.render(W, H, 1, 1, sample0=k)
            assert ctx.timing()["pipeline"] == 0, route.name
            smp[:, :, k] = a[..., :3]
        print(f"{route.name}: {(_bits(smp) == _bits(ref)).all(-1).mean():.4%} of samples bitwise the oracle's")
        np.testing.assert_array_equal(_bits(smp), _bits(ref), err_msg=route.name)
