"""Every material regime of the shading vertex (shade_vertex, csrc/device_core.hpp), sample by sample, against the oracle.

procedural.chart_scene lays one patch per regime under a camera that looks straight down (roughness 0 ... 1 x metallic 0 / 0.5 / 1 with
the 0.05 roughness clamp on both sides, opacities 0, 0.5 and three next to 1, emissive dielectric and metal, albedo 0 and 1, ior 1 /
1.33 / 2.5, an opaque and a half-transparent shadow catcher, a back face), so a regime is a block of pixels of its own and is judged on
its own samples: a regime that is wrong cannot hide in a frame-wide share. Frame 192 x 160 (32 x 32 pixels per cell), 4 samples, one
launch per sample; patch membership of a sample comes from the oracle's primary ray of that sample and that integrator.

Routes, each asserted from the scene's residency and the pipeline the render reports: the fused kernel on LDS-resident geometry (the
default), the queue pipeline (scene created under PTX_FORCE_GLOBAL) and the fused kernel on global memory (the same scene, PTX_WAVEFRONT=0).
Compile-time forms of shade_vertex<SUN, ALPHA, TEX, WORKER>: SUN by sun None / set, ALPHA by chart_scene(alpha=False) (no patch can pass
a ray through), WORKER by the integrator. TEX = true stays with tests/test_textures.py: the chart has no texture.

What is asserted:
  1. BITWISE, one bounce, no sun / a sun of angular radius 0 with and without the blocker: nothing on that path depends on libm (with radius
     0 rand_cone_vec multiplies the azimuth's sin / cos by an exact 0), so every sample of every interior pixel is the oracle's, bit for bit.
  2. The three routes give bitwise the same samples, whole frame, in every configuration of 1 and 3.
  3. Bounces 2 and 4, sun None / 0.004732 / 0.5, flat and facing charts, both integrators: the bars of test_gpu_parity PER PATCH — all
     samples finite and >= 0, >= 99.5 % within 1e-3 relative (floor 1e-3), >= 98 % within 1e-5.
  4. ptx_render_transparent and ptx_render_aov on the chart, bitwise the restatements (tests/_transparent_restatement.py,
     tests/_aov_restatement.py).
"""
import numpy as np
import pytest

from _aov_restatement import restate as aov_restatement
from _common import _bits, _proc
from _routes import Scenes, clean_env, ctx, each_route  # noqa: F401  (clean_env and ctx are fixtures)
from _transparent_restatement import _alpha_of, blend_restatement
from conftest import oracle_from_dict, product_from_dict

W, H, SPP = 192, 160, 4
ENV = (0.5, 0.25, 1.0)
RADIUS = 0.004732                    # the reference's sun


def _variant(sun=None, blocker=False, facing=False, alpha=True):
    return (sun, blocker, facing, alpha)


# ---------------------------------------------------------------------------- scenes, oracle results and masks, computed once
_scenes, _oracles, _refs, _members, _interior = {}, {}, {}, {}, {}


def _scene(v):
    if v not in _scenes:
        _scenes[v] = _proc().chart_scene(sun=v[0], blocker=v[1], facing=v[2], alpha=v[3])
    return _scenes[v]


def _oracle(ora, v):
    if v not in _oracles:
        _oracles[v] = oracle_from_dict(ora, _scene(v))
    return _oracles[v]


def _ref(ora, v, ig, bounces, env=ENV):
    """The oracle's per-sample radiance [H, W, SPP, 3], cached per (variant, integrator, bounces, env) and never modified."""
    key = (v, ig, bounces, env)
    if key not in _refs:
        r = _oracle(ora, v).render_samples(ora.make_cfg(W, H, SPP, bounces, env=env, integrator=ig), threads=0)
        r.setflags(write=False)
        _refs[key] = r
    return _refs[key]


def _member(ora, v, ig):
    """[H, W, SPP] surface hit by the primary ray of each sample (-1: none); sample 0 of the worker integrator is not jittered."""
    key = (v, ig)
    if key not in _members:
        o, m = _oracle(ora, v), np.zeros((H, W, SPP), np.int32)
        for s in range(SPP):
            _, idx = o.intersect(o.primary_rays(ora.make_cfg(W, H, SPP, 1, integrator=ig), s).reshape(-1, 6))
            m[:, :, s] = idx.reshape(H, W)
        m.setflags(write=False)
        _members[key] = m
    return _members[key]


def _interior_of(ora, v):
    """[H, W] the surface of the pixels whose footprint, grown by one pixel on every side, lies inside one patch (-1 elsewhere): the rays
    through the four corners of the grown footprint hit the same surface, and a patch is convex."""
    if v not in _interior:
        o = _oracle(ora, v)
        jj, ii = np.meshgrid(np.arange(H + 1), np.arange(W + 1), indexing="ij")
        ndc = np.stack([(ii / np.float32(W)) * 2 - 1, -((jj / np.float32(H)) * 2 - 1), np.full(ii.shape, W / H)], -1).astype(np.float32)
        _, idx = o.intersect(o.camera_rays(ndc.reshape(-1, 3)))
        c = np.full((H + 3, W + 3), -1, np.int32)          # corner (j, i) at c[j + 1, i + 1]
        c[1:H + 2, 1:W + 2] = idx.reshape(H + 1, W + 1)
        a, b, cc, d = c[0:H, 0:W], c[0:H, 3:W + 3], c[3:H + 3, 0:W], c[3:H + 3, 3:W + 3]
        m = np.where((a == b) & (a == cc) & (a == d), a, -1).astype(np.int32)
        m.setflags(write=False)
        _interior[v] = m
    return _interior[v]


def _bottom(d):
    """Surfaces of the lower chart: the ones a camera ray can hit."""
    return np.flatnonzero(d["cells"][:, 2] == 0)


def _err(got, ref):
    return np.abs(got - ref).max(-1) / np.maximum(np.abs(ref).max(-1), 1e-3)


BITWISE = [(None, False), (0.0, False), (0.0, True)]                   # (sun, blocker) at one bounce
TOLERANCE = [(sun, facing) for sun in (None, RADIUS, 0.5) for facing in (False, True)]


# ---------------------------------------------------------------------------- no GPU: the chart and what the oracle makes of it
@pytest.mark.parametrize("alpha", [True, False])
@pytest.mark.parametrize("sun,blocker,facing", [(None, False, False), (0.0, True, False), (0.5, False, True), (RADIUS, True, True)])
def test_chart_scene_shapes(ptx, sun, blocker, facing, alpha):
    p = _proc()
    d = p.chart_scene(sun=sun, blocker=blocker, facing=facing, alpha=alpha)
    rows = [r for r in p.CHART_REGIMES if alpha or (r[2] == 1.0 and not r[7])]
    assert len(p.CHART_REGIMES) == 29 and len(rows) == (29 if alpha else 22) and len({r[0] for r in p.CHART_REGIMES}) == 29
    n = len(rows) * (2 if facing else 1) + int(blocker)
    assert n <= 64                                                  # the queue pipeline's limit
    assert d["vertices"].shape == (4 * n, 11) and d["vertices"].dtype == np.float32
    assert d["triangles"].shape == (2 * n, 3) and d["triangles"].dtype == np.uint32 and d["triangles"].max() == 3
    assert d["materials"].shape == (n, 11) and d["surf_range"].shape == (n, 4) and d["model_surf"].tolist() == [[0, n]]
    assert len(d["names"]) == n and d["cells"].shape == (n, 3) and len(set(d["names"])) == n
    assert (d["sun"] is None) if sun is None else (d["sun"].shape == (13,) and d["sun"][12] == np.float32(sun))
    if sun is not None:
        assert d["sun"][7] >= 0.5                                   # at least 30 degrees above the plane
    if not alpha:
        assert (d["materials"][:, 3] == 1).all() and not d["materials"][:, 10].any()
    # coplanar patches with gaps; every patch faces up but `backface` (the upper chart: the other way round)
    for k in range(n - int(blocker)):
        v = d["vertices"][4 * k:4 * k + 4]
        level, flipped = d["cells"][k, 2], d["names"][k].startswith("backface")
        assert (v[:, 1] == (p.CHART_TOP if level else 0)).all() and (v[:, 6] == (1 if (level == 0) != flipped else -1)).all()
        t = d["triangles"][2 * k]
        assert np.sign(np.cross(v[t[1], :3] - v[t[0], :3], v[t[2], :3] - v[t[0], :3])[1]) == v[0, 6]      # the winding agrees with the normal
        assert np.allclose(v[:, 0].max() - v[:, 0].min(), 0.9) and np.allclose(v[:, 2].max() - v[:, 2].min(), 0.9)
    info = product_from_dict(ptx, None, d).info()
    assert info["n_surfaces"] == n and info["lds_resident"] == 1     # the GPU tests' default route: everything in LDS


def test_opacities_next_to_one_are_opaque_by_the_rule():
    """renderer.cpp:466: !is_approx(opacity, 1) with math::epsilon = 0.0001f. The three opacities next to 1 are all on the opaque side; a
    draw could not pass through the nearest one anyway (the largest draw is 1 - 2^-24 = that opacity)."""
    f = np.float32
    ops = {r[0]: f(r[2]) for r in _proc().CHART_REGIMES if r[0].startswith("opacity_")}
    approx = {k: bool(v == f(1) or abs(v - f(1)) < f(0.0001)) for k, v in ops.items()}
    assert approx == {"opacity_0": False, "opacity_0.5": False, "opacity_below1": True, "opacity_1m5e-7": True, "opacity_1m2e-6": True}
    assert len({v.tobytes() for v in ops.values()}) == 5 and all(v < 1 for v in ops.values())


@pytest.mark.parametrize("alpha", [True, False])
def test_every_patch_collects_its_samples_and_keeps_its_interior(ora, alpha):
    """From the oracle alone: every patch is the primary hit of >= 2000 samples (both integrators), the interior rule keeps >= 60 % of
    each patch's samples, and no interior pixel has a sample on another surface."""
    v = _variant(alpha=alpha)
    d, inner = _scene(v), _interior_of(ora, v)
    for ig in (0, 1):
        m = _member(ora, v, ig)
        count = np.bincount(m[m >= 0], minlength=len(d["names"]))
        assert count.min() >= 2000, count.tolist()
        kept = np.bincount(inner[inner >= 0], minlength=len(d["names"])) * SPP
        assert (kept >= 0.6 * count).all(), (kept / count).round(3).tolist()
        assert (m[inner >= 0] == inner[inner >= 0][:, None]).all()
    # the blocker and the upper chart change nothing the camera sees
    for other in (_variant(0.0, True, alpha=alpha), _variant(0.5, False, True, alpha=alpha)):
        np.testing.assert_array_equal(_interior_of(ora, other), inner)


def test_blocker_shadows_whole_patches(ora):
    """A sharp sun: the shadow rays from the corners of a patch agree, columns 3-5 are shadowed and 0-2 lit; the blocker is never a
    primary hit."""
    v = _variant(0.0, True)
    d, o = _scene(v), _oracle(ora, v)
    blocker = d["names"].index("blocker")
    assert not (_member(ora, v, 0) == blocker).any() and not (_member(ora, v, 1) == blocker).any()
    sun = d["sun"][6:9]
    for k in _bottom(d):
        p = d["vertices"][4 * k:4 * k + 4, :3] + np.float32([0, 1e-4, 0])
        _, idx = o.intersect(np.concatenate([p, np.tile(sun, (4, 1))], 1).astype(np.float32))
        assert ((idx == blocker) == (d["cells"][k, 0] >= 3)).all(), d["names"][k]


@pytest.mark.parametrize("ig", [0, 1])
def test_one_bounce_without_sun_has_three_values_per_patch(ora, ig):
    """No sun, one bounce: a sample is emissive x 10 (the surface), the environment factor (passed through) or 0 — and the worker adds the
    emissive before its opacity and back-face tests, so there a sample that passes through, or ends on the back face, keeps it. The regimes
    the bitwise GPU test rests on are there: the back face, emissive patches, both outcomes on the half-transparent patches."""
    v = _variant()
    d, ref, m = _scene(v), _ref(ora, v, ig, 1), _member(ora, v, ig)
    env = np.float32(ENV)
    for k, name in enumerate(d["names"]):
        e10 = d["materials"][k, 6:9] * np.float32(10)
        allowed = [np.float32([0, 0, 0])] * (name == "backface") + [e10, env] + ([e10 + env] if ig == 1 else [])
        got = np.unique(ref[m == k], axis=0)
        assert all(any((g == a).all() for a in allowed) for g in got), (name, got.tolist())
        through = (ref[m == k] == allowed[-1]).all(-1).mean()
        op = d["materials"][k, 3]
        if name == "opacity_0":
            assert through == 1
        elif op == np.float32(0.5):
            assert 0.4 < through < 0.6, (name, through)
        else:
            assert through == 0, (name, through)
    back = d["names"].index("backface")                      # emissive 0.1: black in trace(), which returns first; the worker has added it by then
    assert (ref[m == back] == (np.float32(1) if ig == 1 else 0)).all()
    assert (ref[m < 0] == env).all()


@pytest.mark.parametrize("ig", [0, 1])
def test_catchers_lit_and_shadowed_in_the_oracle(ora, ig):
    """A sharp sun, one bounce. LIB: a lit catcher passes the ray through (environment), a shadowed one is black. WORKER: the same, and
    black unless lit. The half-transparent catcher passes about half its samples through before the catcher rule is asked."""
    env = np.float32(ENV)
    for blocker in (False, True):
        v = _variant(0.0, blocker)
        d, ref, m = _scene(v), _ref(ora, v, ig, 1), _member(ora, v, ig)
        a, b = ref[m == d["names"].index("catcher")], ref[m == d["names"].index("catcher_opacity0.5")]
        if blocker:
            assert (a == 0).all() and 0.4 < (b == env).all(-1).mean() < 0.6 and ((b == env).all(-1) | (b == 0).all(-1)).all()
        else:
            assert (a == env).all() and (b == env).all()


# ---------------------------------------------------------------------------- GPU
PRODUCTS = Scenes(lambda ptx, ctx, v: product_from_dict(ptx, ctx, _scene(v)))


def _product(ptx, ctx, mp, v, force_global):
    return PRODUCTS.get(ptx, ctx, mp, v, force_global)


def _each_route(ptx, ctx, mp, v):
    """(route, scene, expected pipeline) over the default-choice routes, with the route's switches set and its residency asserted; the call
    sites assert the pipeline."""
    for r, s in each_route(PRODUCTS, ptx, ctx, mp, v):
        assert s.info()["n_surfaces"] == len(_scene(v)["names"]), r.name
        yield r.name, s, r.pipeline


def _gpu_samples(ctx, s, ig, bounces, pipeline, what):
    out = np.zeros((H, W, SPP, 3), np.float32)
    for k in range(SPP):
        a, _ = s.render(W, H, 1, bounces, env=ENV, sample0=k, integrator=ig)
        assert ctx.timing()["pipeline"] == pipeline, what
        assert (a[..., 3] == 1).all(), what
        out[:, :, k] = a[..., :3]
    return out


@pytest.mark.gpu
@pytest.mark.parametrize("alpha", [True, False], ids=["alpha", "opaque"])
@pytest.mark.parametrize("sun,blocker", BITWISE, ids=["nosun", "sun0", "sun0-blocker"])
def test_one_bounce_is_bitwise_the_oracle(ptx, ctx, ora, clean_env, sun, blocker, alpha):
    """Check 1 and 2 at one bounce. Pins per regime, without a tolerance: the opacity rule, the back face, the roughness clamp,
    fresnel_schlick -> spec_prob, eval_brdf on the sun's direction, the direct clamp, the shadow answer, the catcher lit / shadowed, the
    worker's `catcher black unless lit` and its emissive-before-opacity order."""
    v = _variant(sun, blocker, False, alpha)
    d, inner = _scene(v), _interior_of(ora, v)
    seen = np.unique(inner[inner >= 0])
    assert len(seen) == len(_bottom(d))                                   # every regime appears under the mask
    for ig in (0, 1):
        ref, first = _ref(ora, v, ig, 1), None
        for route, s, pipeline in _each_route(ptx, ctx, clean_env, v):
            what = f"sun {sun} blocker {blocker} alpha {alpha} integrator {ig} / {route}"
            got = _gpu_samples(ctx, s, ig, 1, pipeline, what)
            for k in seen:                                                # per patch, so a failure names its regime
                sel = inner == k
                np.testing.assert_array_equal(_bits(got[sel]), _bits(ref[sel]), err_msg=f"{what}: {d['names'][k]}")
            np.testing.assert_array_equal(_bits(got[inner < 0]), _bits(ref[inner < 0]), err_msg=f"{what}: edges and gaps")
            if first is None:
                first = got
            else:
                np.testing.assert_array_equal(_bits(got), _bits(first), err_msg=what)


def _patch_report(d, member, got, ref, what):
    """Per patch of the lower chart: (name, samples, share within 1e-3, share within 1e-5, largest error), printed; -> list of failures."""
    bad, err = [], _err(got, ref)
    if not (np.isfinite(got).all() and (got >= 0).all()):
        bad.append(f"{what}: a sample is negative or not finite")
    for k in _bottom(d):
        sel = member == k
        n = int(sel.sum())
        if n == 0:
            bad.append(f"{what}: {d['names'][k]}: no samples")
            continue
        e = err[sel]
        s3, s5, mx = (e < 1e-3).mean(), (e < 1e-5).mean(), e.max()
        hist = np.histogram(e, [0, 1e-7, 1e-6, 1e-5, 1e-4, 1e-3, 1e-2, np.inf])[0]
        print(f"{what} | {d['names'][k]:20s} n {n:5d}  <1e-3 {s3:.4%}  <1e-5 {s5:.4%}  max {mx:.3e}  hist {hist.tolist()}")
        if s3 < 0.995 or s5 < 0.98:
            bad.append(f"{what}: {d['names'][k]}: {s3:.4%} within 1e-3, {s5:.4%} within 1e-5, max {mx:.3e}")
    return bad


@pytest.mark.gpu
@pytest.mark.parametrize("alpha", [True, False], ids=["alpha", "opaque"])
@pytest.mark.parametrize("sun,facing", TOLERANCE, ids=[f"{'nosun' if s is None else 'sun' + str(s)}{'-facing' if f else ''}" for s, f in TOLERANCE])
def test_throughput_and_multi_vertex_paths_per_patch(ptx, ctx, ora, clean_env, sun, facing, alpha):
    """Check 3 (and 2). On the flat chart at two bounces a continued path always escapes: the sample is direct + T x env, a direct reading
    of clamp(brdf / pdf) of one BSDF sample under the non-grey environment (0.5, 0.25, 1). Four bounces between the facing charts are
    multi-vertex paths through other regimes. Bars per patch and configuration: finite and >= 0, >= 99.5 % within 1e-3 relative (floor
    1e-3), >= 98 % within 1e-5 — the project's own (test_gpu_parity), for every regime alike; none needed a bar of its own.

    Measured on an MI355X (the routes are bitwise equal), over all 48 configurations: every patch has 100 % of its samples within 1e-3; the
    lowest share within 1e-5 is 99.73 % (rough0.3_metal0.5; 99.82 % rough0.3_metal0 and _metal1, >= 99.97 % everywhere else). Largest
    error of a patch over all configurations:
      rough0_metal0 2.2e-6, _metal0.5 4.2e-6, _metal1 1.3e-7; rough0.01_metal0 2.8e-6, _metal0.5 1.2e-5, _metal1 2.0e-6;
      rough0.05_metal0 8.0e-6, _metal0.5 1.4e-5, _metal1 6.6e-7; rough0.3_metal0 2.3e-5, _metal0.5 3.1e-5, _metal1 1.8e-5;
      rough1_metal0 9.0e-6, _metal0.5 7.6e-6, _metal1 1.7e-6; opacity_0 0, opacity_0.5 7.9e-7, opacity_below1 5.4e-6,
      opacity_1m5e-7 1.1e-5, opacity_1m2e-6 7.0e-6; emissive_dielectric 1.6e-6, emissive_metal 5.9e-6; albedo0 7.0e-6, albedo1 1.8e-6;
      ior1 1.5e-5, ior2.5 2.4e-5; backface 0; catcher 3.4e-6, catcher_opacity0.5 1.6e-6.
    The sharp regimes (roughness <= 0.05, metallic 1) are among the closest: brdf / pdf cancels the peaked specular pdf."""
    v = _variant(sun, False, facing, alpha)
    d, bad = _scene(v), []
    for ig in (0, 1):
        member = _member(ora, v, ig)
        for bounces in (2, 4):
            ref, first = _ref(ora, v, ig, bounces), None
            for route, s, pipeline in _each_route(ptx, ctx, clean_env, v):
                what = f"sun {sun} facing {facing} alpha {alpha} integrator {ig} bounces {bounces} / {route}"
                got = _gpu_samples(ctx, s, ig, bounces, pipeline, what)
                if first is None:
                    first = got
                    bad += _patch_report(d, member, got, ref, what)
                else:
                    np.testing.assert_array_equal(_bits(got), _bits(first), err_msg=what)
    assert not bad, "\n".join(bad)


@pytest.mark.gpu
@pytest.mark.parametrize("blocker", [False, True], ids=["lit", "blocker"])
def test_transparent_render_and_guide_buffers_on_the_chart(ptx, ctx, ora, clean_env, blocker):
    """Check 5, a sharp sun, one bounce, LIB, default route: ptx_render_transparent is bitwise the blend restatement
    (tests/_transparent_restatement.py) fed with the oracle's samples and alphas (opacity 0, the opacities next to 1, the catchers lit without
    the blocker and shadowed under it), ptx_render_aov bitwise tests/_aov_restatement.py's; interior pixels."""
    v = _variant(0.0, blocker)
    d, o, inner = _scene(v), _oracle(ora, v), _interior_of(ora, v)
    one, zero = _ref(ora, v, 0, 1, env=(1.0, 1.0, 1.0)), _ref(ora, v, 0, 1, env=(0.0, 0.0, 0.0))
    alpha = _alpha_of(one - zero)
    m = _member(ora, v, 0)
    name = d["names"].index
    assert (alpha[m == name("opacity_0")] == 0).all() and (alpha[m < 0] == 0).all()
    assert (alpha[m == name("catcher")] == (1 if blocker else 0)).all()
    for k in ("opacity_below1", "opacity_1m5e-7", "opacity_1m2e-6", "backface", "rough0_metal1"):
        assert (alpha[m == name(k)] == 1).all(), k
    half = alpha[m == name("opacity_0.5")]
    assert 0.4 < half.mean() < 0.6
    want = blend_restatement(one, alpha)
    s = _product(ptx, ctx, clean_env, v, False)
    assert s.info()["lds_resident"] == 1
    pix, cl, _ = s.render_transparent(W, H, SPP, 1)
    assert ctx.timing()["pipeline"] == 0
    sel = inner >= 0
    assert sel.mean() > 0.4
    np.testing.assert_array_equal(_bits(pix[..., :3][sel]), _bits(want[0][sel]), err_msg="colour")
    np.testing.assert_array_equal(_bits(pix[..., 3][sel]), _bits(want[1][sel]), err_msg="alpha")
    np.testing.assert_array_equal(cl[sel], want[2][sel].astype(np.uint8), err_msg="claimed")
    want_a, want_n, counts = aov_restatement(ora, o, W_=W, H_=H, tile=(0, 0, W, H), sample0=0, spp=SPP, seed=0x5EED)
    assert counts["through"] >= 2000 and counts["miss"] >= counts["through"]
    alb, nd, _ = s.render_aov(W, H, SPP, seed=0x5EED)
    np.testing.assert_array_equal(_bits(alb[sel]), _bits(want_a[sel]), err_msg="albedo_cov")
    np.testing.assert_array_equal(_bits(nd[sel]), _bits(want_n[sel]), err_msg="normal_depth")
