"""The last vertex of a path: the vertex at depth == bounces - 1 of the library estimator.

renderer::trace(bounce, ..) of the reference returns black at bounce 0, so whatever the vertex before it samples, evaluates and
multiplies into the throughput is never read: the sample's value is final once that vertex has added its emission (and, under a
sun, queued its shadow request). shade_vertex therefore ends such a vertex right after the emission term. With bounces = 1 EVERY
vertex is a last vertex, with bounces = 2 every second one: the shapes here are chosen so that the early end is the common case and
meets every branch that stays in front of it — miss, opacity pass-through (same depth, the vertex behind it is again a last vertex),
back face, lit and shadowed shadow catcher at depth 0, the sun request of a dying path (REQ_ADD with no stream entry to land in: a
"zombie" entry in the queue pipeline), emissive and non-emissive, textured and untextured surfaces.

Bars are those of the tests these shapes come from (test_gpu_parity, test_transparent_background): > 99.5 % of samples within 1e-3
relative of the oracle, > 98 % within 1e-5 on Cornell, ray counts within 1e-4, the two pipelines bitwise equal, alpha exact.

Cornell at bounces = 1: LAST_VERTEX_EXACT below states what was measured on the commit before the early end existed and which
assertion follows from it.

The second step of the same change (no hit record for a last vertex that cannot emit, with a full-path fallback for a non-finite T)
measured as a loss and is not in the tree (profiles/EXPERIMENTS.md, Round 8), so nothing here aims at its branches; a non-finite T
cannot be produced through the C ABI anyway (T starts at 1 and is multiplied by factors clamped to [0, 1]).

The non-GPU tests at the top check, by the oracle alone, that the chosen shapes really contain the cases named above, so that a later
change of scene or seed cannot hollow the GPU tests out.
"""
import os

import numpy as np
import pytest

from _common import _bits, _proc
from _routes import Scenes, clean_env, ctx, each_route, forced_routes, resident_by_creation  # noqa: F401  (clean_env and ctx are fixtures)
from _transparent_restatement import _alpha_of, _oracle, _product_of
from conftest import CORNELL, JACK, oracle_from_dict, product_from_dict, ulp_diff

# Cornell, bounces = 1: a sample is `emissive * 10` of the first hit (no sun, no textures, closed box), a product of two stored
# floats, and no libm function lies on the path. Measured on the parent commit (96 x 54, 4 samples): every one of the 20 736 samples
# equals the oracle's bit for bit. So the test asserts exact equality there, and the project's bars at bounces 2 and 3.
LAST_VERTEX_EXACT = True


def _rel_err(got, ref):
    return np.abs(got - ref).max(-1) / np.maximum(np.abs(ref).max(-1), 1e-3)


def _gpu_samples(scene, W, H, spp, bounces, **kw):
    out = np.zeros((H, W, spp, 3), np.float32)
    for k in range(spp):
        a, _ = scene.render(W, H, 1, bounces, sample0=k, **kw)
        out[:, :, k] = a[..., :3]
    return out


def _ray_slack(n):
    """The project's bar on ray counts is 1e-4 relative. On frames of a few thousand samples that is less than one ray, while one sun
    sample whose `dot(normal, c) > 0` lands on the other side by a last-place difference between ocml and glibc cosf moves the count
    by one: at such sizes the bar is the two rays that smoke() allows on its 64 x 64 frame."""
    return max(2, 1e-4 * n)


_cache = {}


def _plaza(level, alpha):
    return _proc().plaza_scene(level=level, sun=True, alpha=alpha)


def _plaza_oracle(ora, level, alpha):
    if ("plaza", level, alpha) not in _cache:
        _cache[("plaza", level, alpha)] = oracle_from_dict(ora, _plaza(level, alpha))
    return _cache[("plaza", level, alpha)]


def _ref_samples(ora, o, key, W, H, spp, b, **kw):
    if (key, W, H, spp, b, tuple(sorted(kw.items()))) not in _cache:
        _cache[(key, W, H, spp, b, tuple(sorted(kw.items())))] = o.render_samples(ora.make_cfg(W, H, spp, b, **kw), threads=0)
    return _cache[(key, W, H, spp, b, tuple(sorted(kw.items())))]


PW, PH, PS = 64, 36, 4          # plaza
JW, JH, JS = 64, 36, 2          # jack-of-blades
TW, TH, TS = 96, 54, 4          # transparent background: the frame of test_transparent_background, one tile of it
TILE = (23, 11, 50, 31)


# ---------------------------------------------------------------------------- no GPU: the shapes contain the cases
@pytest.mark.parametrize("level", [2, 3])
def test_plaza_shapes_reach_the_last_vertex_cases(ora, level):
    """By the oracle alone, at bounces = 1 on the 64 x 36 x 4 plaza under the sun: the sun request of a last vertex changes samples
    (sun on against sun off), the alpha variant has pass-throughs at the last depth that end in a miss (alpha 0 behind a first hit)
    and samples that differ from the opaque variant's, and the two-bounce frame differs from the one-bounce frame."""
    for alpha in (True, False):
        o = _plaza_oracle(ora, level, alpha)
        one = _ref_samples(ora, o, ("plaza", level, alpha), PW, PH, PS, 1)
        two = _ref_samples(ora, o, ("plaza", level, alpha), PW, PH, PS, 2)
        assert np.isfinite(one).all() and np.isfinite(two).all()
        dark = oracle_from_dict(ora, _proc().plaza_scene(level=level, sun=False, alpha=alpha))
        unlit = dark.render_samples(ora.make_cfg(PW, PH, PS, 1), threads=0)
        lit = (one != unlit).any(-1).sum()
        deeper = (one != two).any(-1).sum()
        print(f"plaza level {level} alpha {alpha}: {lit} samples changed by the last vertex's sun request, {deeper} by the second bounce")
        assert lit >= 200 and deeper >= 200
    o = _plaza_oracle(ora, level, True)
    env1 = o.render_samples(ora.make_cfg(PW, PH, PS, 1, env=(1.0, 1.0, 1.0)), threads=0)
    env0 = o.render_samples(ora.make_cfg(PW, PH, PS, 1, env=(0.0, 0.0, 0.0)), threads=0)
    transparent = _alpha_of(env1 - env0) == 0
    first_hit = np.stack([o.intersect(o.primary_rays(ora.make_cfg(PW, PH, PS, 1), k).reshape(-1, 6))[1].reshape(PH, PW) >= 0 for k in range(PS)], -1)
    through = (transparent & first_hit).sum()          # hit something, passed through it (opacity or lit catcher), then missed
    stopped = (~transparent & first_hit).sum()
    a_on = _ref_samples(ora, o, ("plaza", level, True), PW, PH, PS, 1)
    a_off = _ref_samples(ora, _plaza_oracle(ora, level, False), ("plaza", level, False), PW, PH, PS, 1)
    print(f"plaza level {level}: {through} pass-throughs into a miss, {stopped} opaque first hits, {(a_on != a_off).any(-1).sum()} samples differ between the variants")
    assert through >= 50 and stopped >= 200 and (a_on != a_off).any(-1).sum() >= 50


def test_jack_shape_reaches_emitting_and_dark_first_hits(ora, jack_oracle, jack_arrays):
    """By the oracle alone, on the 64 x 36 x 2 jack-of-blades frame: camera rays land both on surfaces whose material emits and on
    surfaces whose material emits nothing, and on textured ones; bounces 1 and 2 give different frames."""
    emits = (np.asarray(jack_arrays.materials)[:, 6:9] != 0).any(1)
    assert emits.any() and not emits.all()
    idx = np.concatenate([jack_oracle.intersect(jack_oracle.primary_rays(ora.make_cfg(JW, JH, JS, 1), k).reshape(-1, 6))[1] for k in range(JS)])
    hit = idx[idx >= 0]
    print(f"jack: {emits[hit].sum()} camera rays on emitters, {(~emits[hit]).sum()} on dark surfaces, {(idx < 0).sum()} misses")
    assert emits[hit].sum() >= 20 and (~emits[hit]).sum() >= 200 and (idx < 0).sum() >= 20
    one = _ref_samples(ora, jack_oracle, "jack", JW, JH, JS, 1)
    two = _ref_samples(ora, jack_oracle, "jack", JW, JH, JS, 2)
    assert np.isfinite(one).all() and np.isfinite(two).all() and (one != two).any(-1).sum() >= 200


# ---------------------------------------------------------------------------- GPU
@pytest.fixture(scope="module")
def cornell(ptx, ctx):
    return ptx.Scene.load_gltf(ctx, CORNELL)


@pytest.fixture(scope="module")
def jack(ptx, ctx):
    return ptx.Scene.load_gltf(ctx, JACK)


@pytest.mark.gpu
@pytest.mark.parametrize("bounces", [1, 2, 3])
def test_cornell_per_sample_radiance_at_few_bounces(cornell, cornell_oracle, ora, bounces):
    W, H, spp = 96, 54, 4
    ref = _ref_samples(ora, cornell_oracle, "cornell", W, H, spp, bounces)
    got = _gpu_samples(cornell, W, H, spp, bounces)
    assert np.isfinite(got).all()
    err = _rel_err(got, ref)
    print(f"cornell bounces {bounces}: {(err < 1e-3).mean():.4%} within 1e-3, {(err < 1e-5).mean():.4%} within 1e-5, "
          f"{(_bits(got) == _bits(ref)).all(-1).mean():.4%} bitwise, max {int(ulp_diff(got, ref).max())} ulp")
    _, ost = cornell_oracle.render(ora.make_cfg(W, H, spp, bounces), threads=0)
    _, st = cornell.render(W, H, spp, bounces)
    assert abs(st["rays"] - int(ost[0])) <= _ray_slack(int(ost[0])), (st["rays"], int(ost[0]))
    if bounces == 1 and LAST_VERTEX_EXACT:
        np.testing.assert_array_equal(_bits(got), _bits(ref))
        assert st["rays"] == int(ost[0]) == W * H * spp      # one ray per sample, every one traced and counted
    assert (err < 1e-3).mean() > 0.995, f"only {(err < 1e-3).mean():.4%} of samples agree"
    assert (err < 1e-5).mean() > 0.98


@pytest.mark.gpu
@pytest.mark.parametrize("bounces", [1, 2])
@pytest.mark.parametrize("level", [2, 3])          # LDS kernels / global-memory kernels, as in test_plaza_sun_and_alpha_variants
@pytest.mark.parametrize("alpha", [True, False])
def test_plaza_sun_and_alpha_at_the_last_vertex(ptx, ctx, ora, alpha, level, bounces):
    """Sun request of a last vertex, pass-through behind a translucent surface at the last depth, lit and shadowed shadow catcher at
    depth 0 with bounces = 1."""
    s = product_from_dict(ptx, ctx, _plaza(level, alpha))
    o = _plaza_oracle(ora, level, alpha)
    ref = _ref_samples(ora, o, ("plaza", level, alpha), PW, PH, PS, bounces)
    got = _gpu_samples(s, PW, PH, PS, bounces)
    assert np.isfinite(got).all()
    err = _rel_err(got, ref)
    print(f"plaza level {level} alpha {alpha} bounces {bounces}: {(err < 1e-3).mean():.4%} within 1e-3")
    assert (err < 1e-3).mean() > 0.995, f"{(err < 1e-3).mean():.4%} of samples agree"
    _, ost = o.render(ora.make_cfg(PW, PH, PS, bounces), threads=0)
    _, st = s.render(PW, PH, PS, bounces)
    assert abs(st["rays"] - int(ost[0])) <= _ray_slack(int(ost[0])), (st["rays"], int(ost[0]))


class _Pipeline:
    """PTX_WAVEFRONT=0/1 for the calls inside: 0 = the fused kernel, 1 = the queue pipeline."""
    def __init__(self, on):
        self.on = on

    def __enter__(self):
        self.old = os.environ.get("PTX_WAVEFRONT")
        os.environ["PTX_WAVEFRONT"] = "1" if self.on else "0"

    def __exit__(self, *a):
        if self.old is None:
            os.environ.pop("PTX_WAVEFRONT", None)
        else:
            os.environ["PTX_WAVEFRONT"] = self.old


@pytest.mark.gpu
@pytest.mark.parametrize("bounces", [1, 2])
def test_queue_pipeline_bitwise_equals_fused_kernel_at_the_last_vertex(ptx, ctx, clean_env, bounces):
    """Library estimator. The many-surface atrium under the sun (the queue pipeline's default case: every dying path with a sun request
    becomes a zombie entry), whole frame, odd tile with a sample offset, and two samples per pass; then the sun + alpha plaza (pending
    catcher entries, pass-throughs at the last depth)."""
    atr = product_from_dict(ptx, ctx, _proc().atrium_scene(2))
    assert atr.info()["lds_resident"] != 1
    scenes = [(atr, kw) for kw in (dict(W=160, H=90, spp=3), dict(W=97, H=61, spp=2, tile=(13, 7, 70, 41), sample0=5), dict(W=64, H=48, spp=4, spp_per_pass=2))]
    plaza = product_from_dict(ptx, ctx, _plaza(3, True))
    if plaza.info()["lds_resident"] != 1:
        scenes.append((plaza, dict(W=160, H=90, spp=4)))
    for s, kw in scenes:
        out = []
        for on in (False, True):
            with _Pipeline(on):
                out.append(s.render(bounces=bounces, integrator=ptx.INTEGRATOR_LIB, **kw))
                assert ctx.timing()["pipeline"] == (1 if on else 0), kw
        (a0, s0), (a1, s1) = out
        assert np.isfinite(a0).all()
        np.testing.assert_array_equal(_bits(a1), _bits(a0), err_msg=str(kw))
        assert s1["rays"] == s0["rays"] and s1["samples"] == s0["samples"], kw


PRODUCTS = Scenes(_product_of)


def _each_route(ptx, ctx, mp, name):
    """(route name, scene, expected pipeline) over the forced routes, with the route's switches set."""
    n_surf = PRODUCTS.get(ptx, ctx, mp, name).info()["n_surfaces"]
    for r, s in each_route(PRODUCTS, ptx, ctx, mp, name, forced_routes(n_surf), resident_by_creation):
        yield r.name, s, r.pipeline


@pytest.mark.gpu
@pytest.mark.parametrize("name", ["plaza", "jack"])
def test_transparent_background_at_one_bounce(ptx, ctx, ora, clean_env, name):
    """ptx_render_transparent at bounces = 1 on one tile of the 96 x 54 frame, on every route. Alpha is decided at depth 0, which is
    now also the last depth: it must equal the oracle's (env-1 minus env-0 differences) exactly on these two scenes, where everything
    the decision reads is pinned bit-exact (the catcher scene's own bar in test_transparent_background is not exactness, so it is not
    used here); colour of the opaque samples at that file's bar."""
    o = _oracle(ora, name)
    one = _ref_samples(ora, o, ("tb", name), TW, TH, TS, 1, env=(1.0, 1.0, 1.0))
    zero = _ref_samples(ora, o, ("tb", name), TW, TH, TS, 1, env=(0.0, 0.0, 0.0))
    ref = _ref_samples(ora, o, ("tb", name), TW, TH, TS, 1)
    x0, y0, w, h = TILE
    want = _alpha_of(one - zero)[y0:y0 + h, x0:x0 + w]
    ref = ref[y0:y0 + h, x0:x0 + w]
    assert (want == 0).sum() >= 50 and (want == 1).sum() >= 50
    for route, s, pipeline in _each_route(ptx, ctx, clean_env, name):
        rgb, alpha = np.zeros((h, w, TS, 3), np.float32), np.zeros((h, w, TS), np.float32)
        for k in range(TS):
            pix, cl, _ = s.render_transparent(TW, TH, 1, 1, sample0=k, tile=TILE)
            assert ctx.timing()["pipeline"] == pipeline, route
            assert pix.shape == (h, w, 4) and np.isfinite(pix).all() and not pix[cl == 0].any()
            rgb[:, :, k], alpha[:, :, k] = pix[..., :3], cl
        np.testing.assert_array_equal(alpha, want, err_msg=route)
        err = _rel_err(rgb, ref)[want == 1]
        print(f"{name} / {route}: {(err < 1e-3).mean():.4%} of opaque samples within 1e-3 relative")
        assert (err < 1e-3).mean() >= 0.995, f"{route}: {(err < 1e-3).mean():.4%}"


@pytest.mark.gpu
@pytest.mark.parametrize("bounces", [1, 2])
def test_jack_every_shading_variant_at_the_last_vertex(jack, jack_oracle, ora, bounces):
    """Textures, normal maps, textured opacity, sun, an emitting and many dark materials (see the non-GPU test above), at
    test_jack_render_matches_oracle's bars."""
    ref = _ref_samples(ora, jack_oracle, "jack", JW, JH, JS, bounces)
    got = _gpu_samples(jack, JW, JH, JS, bounces)
    assert np.isfinite(got).all()
    err = _rel_err(got, ref)
    print(f"jack bounces {bounces}: {(err < 1e-3).mean():.4%} within 1e-3")
    assert (err < 1e-3).mean() > 0.995, f"{(err < 1e-3).mean():.4%}"
    _, ost = jack_oracle.render(ora.make_cfg(JW, JH, JS, bounces), threads=0)
    _, st = jack.render(JW, JH, JS, bounces)
    assert abs(st["rays"] - int(ost[0])) <= _ray_slack(int(ost[0])), (st["rays"], int(ost[0]))
