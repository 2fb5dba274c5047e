"""PTX_NEE_SAMPLER_PDF: ptx_render_nee's MIS weights built on the density of LIB's BSDF sampler in place of LIB's pdf value (include/ptx.h has
the density and the three places; csrc/nee_core.hpp sampler_pdf and nee_vertex's SPDF parameter).

The yardstick is tests/_nee_pdf_restatement.py, the density, and tests/_nee_estimator.py, the estimator for both light kinds, whose spdf=False
puts pe back. Maps: _nee_lit_scenes' uniform 16 x 8 map of value 1 and its hot-texel map, written into tmp.

Without a GPU: the flag's value and the refusals, the density against the oracle's importance_specular draws (and LIB's pdf_specular failing
the same check), the expectation under a map and under the triangle list alone with the power of both checks, the bitwise LIB frame where no
light sample is possible.
On the GPU: per-sample radiance against the restatement on three routes, fused against unfused with the flag on every flagged variant of
k_nee_fused, composition and the queue fallback, the flag without a possible light sample, the product's expectation against ptx_render,
ptx_render_adaptive_nee with the flag, the mirrors.
"""
import ctypes as C
import json
import os
import subprocess

import numpy as np
import pytest

import _adaptive_restatement as AR
import _nee_pdf_restatement as P
import _nee_restatement as R
from _common import _bits, _same
from _nee_common import K_BATCH, SAME_STATS, SEED, _batch_stat, _err, _pair, _same_expectation
from _nee_estimator import render_samples
from _nee_lit_scenes import CLOUDS, ENV, FUSED, LIT, LIT_LOADS, NO_LIGHTS, SPDF, _hybrid_budget, _new_oracle, _new_scene, _table
from _nee_lit_scenes import maps  # noqa: F401  (fixture)
from _routes import clean_env, ctx  # noqa: F401  (fixtures)
from _routes import DEFAULT_ROUTES, ROUTE_VARS, Scenes, on_route, route_named
from conftest import ROOT

f32 = np.float32


# ---------------------------------------------------------------------------- no GPU
def test_flag_value_and_refusals_without_a_device(ptx):
    """A known flag combination on a host-only scene ends at PTX_ERR_NO_DEVICE, an unknown one at PTX_ERR_INVALID: 2, 8 and 32 stay unassigned."""
    assert ptx.NEE_SAMPLER_PDF == SPDF
    s = _new_scene(ptx, "chart")
    cfg = ptx.RenderCfg(8, 8, 8, 2, (C.c_float * 3)(1, 1, 1), 1, 0, 0, 0, 8, 8, 0, 0, 0, 0, 0, 0)
    acc, acc_b = np.zeros((8, 8, 4), np.float32), np.zeros((8, 8, 4), np.float32)
    ad = ptx.AdaptiveCfg(8, 0, 0.1)

    def nee(flags):
        return ptx.lib().ptx_render_nee(s.h, C.byref(cfg), C.byref(ptx.NeeCfg(flags)), acc.ctypes.data, None)

    def adaptive(flags):
        return ptx.lib().ptx_render_adaptive_nee(s.h, C.byref(cfg), C.byref(ad), C.byref(ptx.NeeCfg(flags)), acc.ctypes.data, acc_b.ctypes.data, None)
    for call in (nee, adaptive):
        for ok in (64, 64 | 1, 64 | 4, 64 | 16, 64 | 16 | 4 | 1):
            assert call(ok) == ptx.ERR_NO_DEVICE, (call.__name__, ok)
        for bad in (64 | 2, 64 | 8, 64 | 32, 128):
            assert call(bad) == ptx.ERR_INVALID and "unknown flag" in ptx.lib().ptx_last_error().decode(), (call.__name__, bad)
    assert (acc == 0).all() and (acc_b == 0).all()


N_DRAWS = 1 << 20
Q_GRID = 2048


def _specular_draws(ora, rough, n_dot_o, seed):
    """The oracle's importance_specular for N_DRAWS uniform (u1, u2) at normal (0, 1, 0) and an outcoming direction of the given cosine
    -> (normal, outcoming, directions), each [N_DRAWS, 3] float32"""
    rng = np.random.default_rng(seed)
    n = np.tile(np.array([[0, 1, 0]], f32), (N_DRAWS, 1))
    outc = np.tile(np.array([[np.sqrt(1 - n_dot_o * n_dot_o), n_dot_o, 0]], f32), (N_DRAWS, 1))
    u = rng.random((N_DRAWS, 2)).astype(f32)
    w = R._pbr(ora, n, outc, n, u[:, 0], u[:, 1], f32(rough), 1, 1.5)[:, 6:9]
    return n, outc, np.ascontiguousarray(w)


def _mass_above_by_quadrature(rough, n_dot_o):
    """The integral of ps_spec over the directions above the surface, midpoint rule on a Q_GRID x Q_GRID grid of half vectors: w = reflect(-o, h),
    dw = 4 (o.h) dh, dh = sin(t) dt dphi, and t = atan(a sqrt(s / (1 - s))) with s = 1 - (1 - v)^2, v uniform, spreads the lobe evenly over the grid. Where ps_spec is
    the sampler's density the integrand is 1 / (2 pi) on the part of the grid whose w lies above the surface and 0 elsewhere."""
    a = float(rough) ** 2
    v = (np.arange(Q_GRID) + 0.5) / Q_GRID
    s = 1 - (1 - v) ** 2                      # finer towards s = 1, where the directions below the surface of a narrow lobe lie
    g = a * np.sqrt(s / (1 - s))
    t = np.arctan(g)
    dt_ds = a / (2 * np.sqrt(s / (1 - s)) * (1 - s) ** 2) / (1 + g * g) * 2 * (1 - v)   # dt / dv
    phi = (np.arange(Q_GRID) + 0.5) / Q_GRID * 2 * np.pi
    tt, pp = np.meshgrid(t, phi, indexing="ij")
    h = np.stack([np.sin(tt) * np.cos(pp), np.cos(tt), np.sin(tt) * np.sin(pp)], -1).reshape(-1, 3)
    o = np.array([np.sqrt(1 - n_dot_o * n_dot_o), n_dot_o, 0.0])
    oh = h @ o
    w = 2 * oh[:, None] * h - o
    ps = P.ggx_density(np.tile(np.array([[0.0, 1.0, 0.0]]), (len(w), 1)), np.tile(o, (len(w), 1)), w, np.full(len(w), float(rough)))   # in float64
    above = (w[:, 1] > 0) & (oh > 0)
    integrand = np.where(above, ps * 4 * oh * np.sin(tt.ravel()) * np.repeat(dt_ds, Q_GRID), 0.0)
    return float(integrand.sum() * (1.0 / Q_GRID) * (2 * np.pi / Q_GRID))


@pytest.mark.parametrize("n_dot_o", [0.9, 0.3])
@pytest.mark.parametrize("rough", [0.05, 0.2, 0.5, 1.0])
def test_the_density_is_the_specular_samplers(ora, rough, n_dot_o):
    """Over the oracle's importance_specular draws, the mean of cos(w) / p(w) over the draws above the surface and 0 over the others (those
    paths end) is the integral of the cosine over the hemisphere, pi, iff p is the sampler's density there. With ps_spec it is within 4
    standard errors of pi; with LIB's pdf_specular for p it is not (asserted at roughness 0.2; measured 3.52 for n.o = 0.9 and 54 at roughness 0.05). The share of draws below the surface
    is 1 - the integral of ps_spec above it, by quadrature, within 4 binomial standard errors (plus one draw: the share is a multiple of
    1 / N_DRAWS)."""
    n, outc, w = _specular_draws(ora, rough, n_dot_o, 1234)
    up = w[:, 1] > 0
    cos = w[up, 1].astype(np.float64)
    ps = P.ggx_density(n[up], outc[up], w[up], np.full(int(up.sum()), rough, f32)).astype(np.float64)
    assert (ps > 0).all()
    x = np.zeros(N_DRAWS)
    x[up] = cos / ps
    mean, se = x.mean(), x.std(ddof=1) / np.sqrt(N_DRAWS)
    lib_pdf = R._pbr(ora, n[up], outc[up], w[up], 0, 0, f32(rough), 1, 1.5)[:, 10].astype(np.float64)
    y = np.zeros(N_DRAWS)
    y[up] = cos / np.maximum(lib_pdf, 1e-4)
    mean_lib, se_lib = y.mean(), y.std(ddof=1) / np.sqrt(N_DRAWS)
    below = 1 - up.mean()
    mass = _mass_above_by_quadrature(rough, n_dot_o)
    se_b = np.sqrt(max(mass * (1 - mass), 0) / N_DRAWS)
    print(f"roughness {rough}, n.o {n_dot_o}: E[cos / ps_spec] = {mean:.5f} +- {se:.5f}, with pdf_specular {mean_lib:.4f} +- {se_lib:.4f}; "
          f"below the surface {below:.6f}, 1 - quadrature {1 - mass:.6f} (se {se_b:.2e})")
    assert abs(mean - np.pi) <= 4 * se, (mean, se)
    if rough == 0.2:
        assert abs(mean_lib - np.pi) > 4 * se_lib, (mean_lib, se_lib)
    assert abs(below - (1 - mass)) <= 4 * se_b + 1.0 / N_DRAWS, (below, 1 - mass, se_b)


def _batches(ora, render, seed0, K=K_BATCH, spp=16, **kw):
    return _batch_stat(np.stack([render(seed=seed0 + k, spp=spp, **kw)["rad"].mean(2) for k in range(K)]))


@pytest.mark.parametrize("map_name", ["uniform", "hot"])
def test_expectation_under_a_map_on_the_restatement(ptx, ora, maps, map_name):
    """The open chart scene (12 listed triangles, c_env = 0.5), 24 x 16, 3 bounces, 16 batches of 16 spp, _nee_common's statistic (|z| <= 4 on
    the frame, 5 on the quadrants) against the unflagged estimator without a table. Under the uniform map of value 1 the flagged frame passes
    and the same estimator with pe put back fails (measured: 0.28 / 1.37 against 27.4 / 69.3). Under the hot-texel map the flagged frame
    passes (0.65 / 1.30); the pe form's shift there is below what 16 x 16 resolves (0.68 / 1.33), so only its figure is printed."""
    W, H, b = 24, 16, 3
    o = _new_oracle(ora, "chart", maps[map_name])
    tab = _table(ptx, _new_scene(ptx, "chart", env_map=maps[map_name]))

    def flagged(seed, spp, spdf=True):
        return render_samples(ora, o, o.a, W, H, spp, b, tab=tab, spdf=spdf, seed=seed)

    def unflagged(seed, spp):
        return render_samples(ora, o, o.a, W, H, spp, b, seed=seed)
    ref = _batches(ora, unflagged, 0xB000)
    ok, zf, zq = _same_expectation(_batches(ora, flagged, 0xA000), ref)
    print(f"{map_name}: weights on the sampler's density against unflagged: worst z frame {zf:.2f} quadrant {zq:.2f}")
    assert ok, (zf, zq)
    pe_ok, zf, zq = _same_expectation(_batches(ora, flagged, 0xA000, spdf=False), ref)
    print(f"{map_name}: weights on pe against unflagged: worst z frame {zf:.2f} quadrant {zq:.2f}")
    if map_name == "uniform":
        assert not pe_ok, (zf, zq)


TRI_K, TRI_SPP = 16, 16


def test_expectation_under_the_triangle_list_alone_on_the_restatement(ora):
    """The chart scene's own 12 listed triangles, no map (lights=True, tab=None), 24 x 16, 3 bounces, against LIB's estimator (lights=False)
    with other seeds: the flagged frame passes _nee_common's statistic.
    No size of at most 64 batches of 64 spp separates the two forms on this scene, so the pe form is not asserted to fail: the 12 patches are
    small and most of the frame's radiance is the constant environment, which no light sample competes for. Measured, worst z frame / quadrant
    against LIB, weights on the sampler's density | weights on pe: 16 x 16: 0.53 / 0.78 | 0.43 / 0.83; 32 x 32: 1.21 / 1.34 | 1.19 / 1.27;
    64 x 64: 0.62 / 1.59 | 0.60 / 1.59 (frame means within 0.1 % of LIB's in both forms). The triangle weights' defect is resolved where it
    is large: under a map (the test above), and per sample against the restatement on the GPU."""
    W, H, b = 24, 16, 3
    o = _new_oracle(ora, "chart")

    def nee(seed, spp):
        return render_samples(ora, o, o.a, W, H, spp, b, spdf=True, seed=seed)

    def lib(seed, spp):
        return render_samples(ora, o, o.a, W, H, spp, b, seed=seed, lights=False)
    ref = _batches(ora, lib, 0xB000, TRI_K, TRI_SPP)
    ok, zf, zq = _same_expectation(_batches(ora, nee, 0xA000, TRI_K, TRI_SPP), ref)
    print(f"triangle list, weights on the sampler's density against LIB: worst z frame {zf:.2f} quadrant {zq:.2f}")
    assert ok, (zf, zq)


def test_without_a_possible_light_sample_the_restatement_is_lib_bitwise(ora):
    """lights=False, tab=None: every weight is 1, so the flagged restatement (spdf) is the unflagged one's LIB frame bit for bit"""
    o = _new_oracle(ora, "chart")
    got = render_samples(ora, o, o.a, 24, 16, 4, 3, spdf=True, seed=SEED, lights=False)
    want = render_samples(ora, o, o.a, 24, 16, 4, 3, seed=SEED, lights=False)
    _same(got["rad"], want["rad"], "flagged restatement without lights against LIB")
    assert got["light_samples"] == 0 and got["rays"] == want["rays"]


# ---------------------------------------------------------------------------- GPU
PRODUCTS = Scenes(lambda ptx, ctx, key: _new_scene(ptx, key[0], ctx, key[1]))   # key: (scene name, its map as (path, srgb) or None)


def _route(ptx, ctx, mp, name, map_name, maps, route):
    r = route_named(DEFAULT_ROUTES, route)
    return on_route(PRODUCTS, ptx, ctx, mp, (name, maps[map_name] if map_name else None), r), r.pipeline


_refs = {}


def _restated(ptx, ora, maps, name, map_name, flags, W, H, spp, b):
    """the restated per-sample radiance of a case, computed once and left unchanged"""
    key = (name, map_name, flags)
    if key not in _refs:
        o = _new_oracle(ora, name, maps[map_name] if map_name else None)
        tab = _table(ptx, _new_scene(ptx, name, env_map=maps[map_name])) if flags & ENV else None
        ref = render_samples(ora, o, o.a, W, H, spp, b, tab=tab, spdf=True, seed=SEED)
        ref["rad"].setflags(write=False)
        _refs[key] = ref
    return _refs[key]


RADIANCE_CASES = [("chart", "hot", SPDF | ENV), ("lit_opaque_nosun", None, SPDF), ("cornell", None, SPDF)]


@pytest.mark.gpu
@pytest.mark.parametrize("route", [r.name for r in DEFAULT_ROUTES])
@pytest.mark.parametrize("name,map_name,flags", RADIANCE_CASES)
def test_per_sample_radiance_against_the_restatement(ptx, ctx, ora, clean_env, maps, name, map_name, flags, route):
    """test_nee_env's bar: all samples finite and >= 0, >= 99.5 % within 1e-3 relative (floor 1e-3), counts within 0.5 % + 1. The fused
    routes run the flagged variants of k_nee_fused (PTX_NEE_FUSED), the queue route k_nee_shade's.
    Measured on the MI355X, the same on the three routes: 100 % of samples within 1e-3; worst error chart 1.8e-05, lit_opaque_nosun 2.5e-04,
    cornell 2.5e-05; light samples / visible ones 366 / 305 (restated 367 / 306), 589 / 384 and 1103 / 896 (equal to the restated counts)."""
    W, H, spp, b = 24, 16, 4, 3
    ref = _restated(ptx, ora, maps, name, map_name, flags, W, H, spp, b)
    s, pipeline = _route(ptx, ctx, clean_env, name, map_name, maps, route)
    got = np.zeros((H, W, spp, 3), np.float32)
    tot = dict(light_samples=0, light_visible=0, rays=0)
    for k in range(spp):
        acc, st = s.render_nee(W, H, 1, b, seed=SEED, sample0=k, flags=flags | FUSED)
        tm = ctx.timing()
        assert tm["pipeline"] == pipeline and tm["fused_launches"] == (1 if pipeline == 0 else 0), (route, tm)
        assert (acc[..., 3] == 1).all()
        got[:, :, k] = acc[..., :3]
        for key in tot:
            tot[key] += st[key]
    assert np.isfinite(got).all() and (got >= 0).all()
    e = _err(got, ref["rad"])
    share = (e <= 1e-3).mean()
    print(f"{name} / {map_name} / {flags} / {route}: {share * 100:.3f} % of samples within 1e-3, worst {e.max():.3g}; light samples {tot['light_samples']} "
          f"(restated {ref['light_samples']}), visible {tot['light_visible']} (restated {ref['light_visible']})")
    assert ref["light_samples"] > 0 and share >= 0.995
    for key in tot:
        assert abs(tot[key] - ref[key]) <= 0.005 * ref[key] + 1, key
    # the flag changes the frame: the unflagged call's samples differ
    plain, _ = s.render_nee(W, H, 1, b, seed=SEED, sample0=0, flags=(flags & ~SPDF) | FUSED)
    assert (_bits(plain[..., :3]) != _bits(got[:, :, 0])).any()


def _fused_scene(ptx, ctx, mp, name, map_name, maps, route):
    """the scene on one of the three places of the geometry, the fused kernel in charge -> (scene, whether to close it)"""
    if route == "hybrid":   # some surface stays in global memory; the fused kernel is asked for at the call (as tests/test_nee_env.py)
        mp.setenv("PTX_LDS_BUDGET", str(_hybrid_budget(ptx, mp, name)))
        s = _new_scene(ptx, name, ctx, maps[map_name] if map_name else None)
        for k in ROUTE_VARS:
            mp.delenv(k, raising=False)
        mp.delenv("PTX_LDS_BUDGET")
        mp.setenv("PTX_WAVEFRONT", "0")
        assert s.info()["lds_resident"] == 2, (name, s.info())
        return s, True
    return _route(ptx, ctx, mp, name, map_name, maps, route)[0], False


@pytest.mark.gpu
@pytest.mark.parametrize("route", ["lds fused", "hybrid", "global fused"])
@pytest.mark.parametrize("name", ["lit", "lit_nosun", "lit_opaque", "lit_opaque_nosun"] + sorted(CLOUDS))
def test_fused_is_unfused_bitwise_with_the_flag(ptx, ctx, clean_env, maps, name, route):
    """8 loads x 3 places of the geometry = the 24 flagged variants MODE x TEX x ALPHA x SUN of k_nee_fused, each against k_nee_shade's flagged
    variant: bitwise equal frames, equal stats, one launch per pass (_nee_common._pair). The frame is not the unflagged one."""
    s, close = _fused_scene(ptx, ctx, clean_env, name, None, maps, route)
    W, H = (48, 32) if name in LIT_LOADS else (64, 36)
    got, st = _pair(ptx, ctx, s, W, H, 4, 4, flags=SPDF)
    assert st["light_samples"] > 0 and st["n_lights"] > 0
    plain, _ = s.render_nee(W, H, 4, 4, seed=SEED, flags=FUSED)
    assert (_bits(plain) != _bits(got)).any()
    if close:
        s.close()


@pytest.mark.gpu
@pytest.mark.parametrize("route", ["lds fused", "hybrid", "global fused"])
@pytest.mark.parametrize("name", ["lit", "lit_nosun", "lit_opaque", "lit_opaque_nosun"])
def test_fused_is_unfused_bitwise_with_the_flag_under_a_map(ptx, ctx, clean_env, maps, name, route):
    """3 places x ALPHA x SUN: the twelve flagged ENV variants of k_nee_fused against k_nee_shade's four, with and without the triangle list"""
    s, close = _fused_scene(ptx, ctx, clean_env, name, "sky", maps, route)
    for extra in (0, NO_LIGHTS):
        got, st = _pair(ptx, ctx, s, 24, 16, 4, 4, flags=SPDF | ENV | extra)
        assert st["light_samples"] > 0
        plain, _ = s.render_nee(24, 16, 4, 4, seed=SEED, flags=ENV | extra | FUSED)
        assert (_bits(plain) != _bits(got)).any()
    if close:
        s.close()


@pytest.mark.gpu
def test_fused_composition_and_queue_fallback_with_the_flag(ptx, ctx, clean_env, maps):
    s, _ = _route(ptx, ctx, clean_env, "lit_opaque_nosun", "hot", maps, "lds fused")
    W, H, spp, b, F = 24, 16, 8, 3, FUSED | ENV | SPDF
    whole, _ = s.render_nee(W, H, spp, b, seed=SEED, flags=ENV | SPDF)          # the unfused flagged frame
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
    shards = sum(s.render_nee(W, H, spp, b, seed=SEED, shard=(k, 3, 8), flags=F)[0] for k in range(3))
    _same(shards, whole, "three shards")
    q, pipeline = _route(ptx, ctx, clean_env, "lit_opaque_nosun", "hot", maps, "queue")
    assert pipeline == 1
    got, _ = _pair(ptx, ctx, q, W, H, spp, b, fused=False, flags=ENV | SPDF)   # fused_launches == 0: the flag is ignored, not refused
    _same(got, whole, "queue route")


@pytest.mark.gpu
@pytest.mark.parametrize("route", [r.name for r in DEFAULT_ROUTES])
def test_without_a_possible_light_sample_the_flag_changes_no_bit(ptx, ctx, clean_env, maps, route):
    """An emptied list and no table (no map; a map with PTX_NEE_ENV_SAMPLES unset): the flagged call is the unflagged call and ptx_render"""
    W, H, spp, b = 24, 16, 4, 3
    for map_name in (None, "hot"):
        s, pipeline = _route(ptx, ctx, clean_env, "chart", map_name, maps, route)
        lib, _ = s.render(W, H, spp, b, seed=SEED)
        for extra in (NO_LIGHTS, NO_LIGHTS | FUSED) + ((NO_LIGHTS | ENV,) if map_name is None else ()):
            want, st0 = s.render_nee(W, H, spp, b, seed=SEED, flags=extra)
            got, st = s.render_nee(W, H, spp, b, seed=SEED, flags=extra | SPDF)
            _same(got, want, f"{map_name} / {route} / {extra}")
            _same(got, lib, f"{map_name} / {route} / {extra}: ptx_render")
            assert all(st[k] == st0[k] for k in SAME_STATS) and st["light_samples"] == 0 and ctx.timing()["pipeline"] == pipeline


@pytest.mark.gpu
def test_the_products_expectation_is_ptx_renders(ptx, ctx, clean_env, maps):
    """The chart under the uniform map, 24 x 16, 3 bounces, 16 batches of 16 spp: the frame of PTX_NEE_SAMPLER_PDF | ENV_SAMPLES | FUSED has
    ptx_render's expectation by _nee_common's statistic; the same sizes without the flag fail it (the restatement's gap is z = 27).
    Measured on the MI355X, worst z frame / quadrant: 0.16 / 1.44 with the flag, 24.2 / 61.8 without."""
    W, H, b = 24, 16, 3
    s, _ = _route(ptx, ctx, clean_env, "chart", "uniform", maps, "lds fused")

    def batches(render, seed0):
        return _batch_stat(np.stack([render(seed0 + k)[..., :3] / f32(16) for k in range(K_BATCH)]))
    lib = batches(lambda seed: s.render(W, H, 16, b, seed=seed)[0], 0xB000)
    ok, zf, zq = _same_expectation(batches(lambda seed: s.render_nee(W, H, 16, b, seed=seed, flags=SPDF | ENV | FUSED)[0], 0xA000), lib)
    print(f"flags 64|16|4 against ptx_render: worst z frame {zf:.2f} quadrant {zq:.2f}")
    assert ok, (zf, zq)
    bad, zf, zq = _same_expectation(batches(lambda seed: s.render_nee(W, H, 16, b, seed=seed, flags=ENV | FUSED)[0], 0xA000), lib)
    print(f"flags 16|4 against ptx_render: worst z frame {zf:.2f} quadrant {zq:.2f}")
    assert not bad, (zf, zq)


@pytest.mark.gpu
@pytest.mark.parametrize("route,flags", [("lds fused", SPDF | FUSED), ("queue", SPDF)])
def test_adaptive_with_the_flag_is_the_flagged_calls_of_the_half_ranges(ptx, ctx, clean_env, maps, route, flags):
    """tests/test_adaptive_nee.py's snapshot method on Cornell, 48 x 32, 3 bounces, 8 samples first, 8 per round, cap 24: a pixel with n samples
    holds, in A and in B, what the flagged ptx_render_nee calls of the same half ranges leave, and the counts are the replayed decision's."""
    W, H, b, cap, thr = 48, 32, 3, 24, 0.2
    s, pipeline = _route(ptx, ctx, clean_env, "cornell", None, maps, route)
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
    assert tm["pipeline"] == pipeline and tm["fused_launches"] == (st["passes"] if pipeline == 0 else 0), (tm, st)
    plain_a, _, _ = s.render_adaptive_nee(W, H, cap, b, 8, 8, thr, seed=SEED, flags=flags & ~SPDF)
    assert (_bits(plain_a) != _bits(got_a)).any()


@pytest.mark.gpu
def test_mirrors_give_the_flagged_frame_bitwise(ptx, ctx, clean_env, tmp_path):
    """Scene.render_nee and Renderer.render_nee (python), ptx_render_cli --nee --nee-sampler-pdf (core::renderer::render_nee) against the C
    call; ptx_ctx_get_timing reports the fused form as for the other flags."""
    from PIL import Image
    W, H, spp, b = 24, 16, 8, 3
    s = ptx.Scene.load_gltf(ctx, LIT)
    cfg = ptx.RenderCfg(W, H, spp, b, (C.c_float * 3)(1, 1, 1), SEED, 0, 0, 0, W, H, 0, 0, 0, 0, 0, 0)
    want = np.zeros((H, W, 4), np.float32)
    st = ptx.NeeStats()
    assert ptx.lib().ptx_render_nee(s.h, C.byref(cfg), C.byref(ptx.NeeCfg(SPDF)), want.ctypes.data, C.byref(st)) == 0
    assert ctx.timing()["fused_launches"] == 0
    plain, _ = s.render_nee(W, H, spp, b, seed=SEED)
    assert (_bits(plain) != _bits(want)).any()
    _same(s.render_nee(W, H, spp, b, seed=SEED, flags=ptx.NEE_SAMPLER_PDF)[0], want, "Scene.render_nee")
    got, fst = s.render_nee(W, H, spp, b, seed=SEED, flags=ptx.NEE_SAMPLER_PDF | ptx.NEE_FUSED)
    tm = ctx.timing()
    _same(got, want, "Scene.render_nee, fused")
    assert tm["pipeline"] == 0 and tm["fused_launches"] == fst["passes"] > 0 and tm["fused_ms"] == fst["kernel_ms"], (tm, fst)
    r = ptx.Renderer(0)
    r.resolution, r.sample_count, r.bounce_count, r.seed = (W, H), spp, b, SEED
    r.load_gltf(LIT)
    _same(r.render_nee(flags=ptx.NEE_SAMPLER_PDF), want, "Renderer.render_nee")
    assert r.last_nee_stats["light_samples"] == st.light_samples and r.last_nee_stats["light_visible"] == st.light_visible
    cli = os.path.join(ROOT, "distributed-path-tracer_amd", "ptx_render_cli")
    for switches in (["--nee", "--nee-sampler-pdf"], ["--nee-fused", "--nee-sampler-pdf"]):
        out = subprocess.run([cli, *switches, LIT, str(tmp_path / "f.png"), str(W), str(H), str(spp), str(b)], capture_output=True, text=True, timeout=120)
        assert out.returncode == 0, out.stderr
        np.testing.assert_array_equal(np.array(Image.open(tmp_path / "f.png")), ctx.tonemap_encode(want, W, H, spp))
        js = json.loads(out.stdout)
        assert js["nee_light_samples"] == st.light_samples and js["nee_light_visible"] == st.light_visible
    s.close()
