"""The per-material constants of the shade records (csrc/flat_scene.hpp: RoughConsts, fresnel_f0sq, fill_shade_consts).

What a path vertex needs of the material's roughness and ior alone — roughness^4 of the clamped roughness, that minus 1, the Smith k,
the squared Fresnel f0 — is computed once per surface by the scene builder and read from the record by the untextured kernels
(shade_vertex<.., TEX = false, ..>); textured kernels compute it per vertex from the scaled roughness. The record must hold the very bits
the vertex would compute, or frames change.

  1. ptx_shade_consts_check: the builder's function on the host against the vertex's expressions on the device, over a grid of a few
     thousand materials at the corners: roughness 0, -0, just below / at the 0.05 clamp, 0.5, 1; ior 1, 1.45, 0 and -1 (a zero
     denominator); metallic 0, 0.5, 1; denormals, infinities and NaN in each field. Expected: 0 words differ (a NaN equals any NaN).
  2. A chart of tests/test_material_chart.py's kind with the corner values as materials: procedural.chart_scene(alpha=False) with the
     (roughness, metallic, ior) of its 22 patches replaced by CORNERS, two bounces, no sun, per-sample radiance per patch against the
     oracle on the three default routes, with that file's bars. Only materials whose oracle samples are all finite are judged:
     NOT_FINITE lists the ones left out (a NaN roughness, metallic or ior, and ior -1, whose f0 is infinite), checked against the oracle on
     the CPU by test_the_oracle_is_finite_on_all_corners_but_the_listed; their patches are still rendered, and every route must agree on
     them bitwise (a NaN equals any NaN).
"""
import itertools

import numpy as np
import pytest

from _common import _bits, _proc
from _routes import Scenes, clean_env, ctx, each_route  # noqa: F401  (clean_env and ctx are fixtures)
from conftest import oracle_from_dict, product_from_dict

W, H, SPP, BOUNCES = 192, 160, 4, 2
ENV = (0.5, 0.25, 1.0)
DN = 1e-40                                   # a denormal binary32

# (roughness, metallic, ior) of the chart's 22 opaque patches, in patch order
CORNERS = [
    (0.0, 0.0, 1.45), (-0.0, 0.5, 1.45), (0.0499, 1.0, 1.45), (0.05, 0.0, 1.45), (0.5, 0.5, 1.45), (1.0, 1.0, 1.45),
    (0.5, 0.0, 1.0), (0.5, 0.0, 0.0), (0.5, 0.0, -1.0), (0.05, 0.5, 1.0), (1.0, 0.0, 0.0), (0.0499, 0.0, 0.0),
    (DN, 0.0, 1.45), (0.5, DN, 1.45), (0.5, 0.0, DN), (0.05, 1.0, DN),
    (float("nan"), 0.0, 1.45), (0.5, float("nan"), 1.45), (0.5, 0.0, float("nan")),
    (1.0, 1.0, -1.0), (0.0, 1.0, 1.0), (-0.0, 0.0, 0.0),
]
NOT_FINITE = [8, 16, 17, 18, 19]             # indices into CORNERS whose oracle samples are not all finite


def _grid():
    f = np.float32
    rough = [0.0, -0.0, 0.0499, 0.05, 0.5, 1.0, DN, -DN, np.inf, np.nan]
    metal = [0.0, 0.5, 1.0, DN, np.nan]
    ior = [1.0, 1.45, 0.0, -1.0, DN, -DN, np.inf, np.nan]
    tint = [(0.9, 0.6, 0.3, 0.0, 0.0, 0.0), (0.0, 1.0, DN, 0.5, np.nan, DN), (np.nan, 0.3, 0.3, DN, 0.2, 1.0)]   # albedo, emissive
    rows = [(r, m, i, *t) for r, m, i, t in itertools.product(rough, metal, ior, tint)]
    return np.array(rows, f)


_kept = {}


def _chart():
    if "d" not in _kept:
        d = _proc().chart_scene(alpha=False)
        m = d["materials"].copy()
        assert len(m) == len(CORNERS)
        m[:, 4], m[:, 5], m[:, 9] = [np.float32([c[k] for c in CORNERS]) for k in range(3)]
        d["materials"] = m
        _kept["d"] = d
    return _kept["d"]


def _oracle_samples(ora):
    """[H, W, SPP, 3] per-sample radiance and [H, W, SPP] primary-hit surface from the oracle, once."""
    if "ref" not in _kept:
        o = oracle_from_dict(ora, _chart())
        with np.errstate(all="ignore"):
            ref = o.render_samples(ora.make_cfg(W, H, SPP, BOUNCES, env=ENV), threads=0)
        member = np.zeros((H, W, SPP), np.int32)
        for s in range(SPP):
            _, idx = o.intersect(o.primary_rays(ora.make_cfg(W, H, SPP, 1), s).reshape(-1, 6))
            member[:, :, s] = idx.reshape(H, W)
        ref.setflags(write=False); member.setflags(write=False)
        _kept["ref"] = (ref, member)
    return _kept["ref"]


# ---------------------------------------------------------------------------- no GPU
def test_grid_covers_the_corners():
    g = _grid()
    assert g.shape == (10 * 5 * 8 * 3, 9) and 1000 < len(g) < 10000
    assert np.isnan(g[:, 0]).any() and np.isnan(g[:, 2]).any() and (g[:, 2] == -1).any() and (np.abs(g[:, 0]) == np.float32(DN)).any()
    assert np.float32(DN) > 0 and np.float32(DN) < np.finfo(np.float32).tiny
    assert np.signbit(g[:, 0][g[:, 0] == 0]).any()


def test_the_oracle_is_finite_on_all_corners_but_the_listed(ora):
    ref, member = _oracle_samples(ora)
    bad = [k for k in range(len(CORNERS)) if not np.isfinite(ref[member == k]).all()]
    count = np.bincount(member[member >= 0], minlength=len(CORNERS))
    assert count.min() >= 2000, count.tolist()
    assert bad == NOT_FINITE, bad
    assert np.isfinite(ref[member < 0]).all()


# ---------------------------------------------------------------------------- GPU
@pytest.mark.gpu
def test_record_constants_are_the_vertex_expressions_bit_for_bit(ctx):
    assert ctx.shade_consts_check(_grid()) == 0
    assert ctx.shade_consts_check(np.zeros((0, 9), np.float32)) == 0


PRODUCTS = Scenes(lambda ptx, ctx, name: product_from_dict(ptx, ctx, _chart()))


def _nan_aware_bits(a):
    b = _bits(a).copy()
    b[np.isnan(a)] = 0x7FC00000
    return b


@pytest.mark.gpu
def test_corner_materials_on_the_chart_against_the_oracle(ptx, ctx, ora, clean_env):
    ref, member = _oracle_samples(ora)
    judged = [k for k in range(len(CORNERS)) if k not in NOT_FINITE]
    bad, first = [], None
    for route, s in each_route(PRODUCTS, ptx, ctx, clean_env, "corners"):
        got = np.zeros((H, W, SPP, 3), np.float32)
        for k in range(SPP):
            a, _ = s.render(W, H, 1, BOUNCES, env=ENV, sample0=k)
            assert ctx.timing()["pipeline"] == route.pipeline, route.name
            got[:, :, k] = a[..., :3]
        if first is not None:
            np.testing.assert_array_equal(_nan_aware_bits(got), _nan_aware_bits(first), err_msg=route.name)
            continue
        first = got
        with np.errstate(all="ignore"):
            err = np.abs(got - ref).max(-1) / np.maximum(np.abs(ref).max(-1), 1e-3)
        for k in judged:
            sel = member == k
            g, e = got[sel], err[sel]
            s3, s5 = (e < 1e-3).mean(), (e < 1e-5).mean()
            print(f"{route.name} | patch {k:2d} {CORNERS[k]} n {int(sel.sum()):5d}  <1e-3 {s3:.4%}  <1e-5 {s5:.4%}  max {np.nanmax(e):.3e}")
            if not np.isfinite(g).all():
                bad.append(f"patch {k} {CORNERS[k]}: a sample is not finite")
            elif s3 < 0.995 or s5 < 0.98:
                bad.append(f"patch {k} {CORNERS[k]}: {s3:.4%} within 1e-3, {s5:.4%} within 1e-5")
    assert not bad, "\n".join(bad)
