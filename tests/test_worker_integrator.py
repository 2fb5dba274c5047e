"""PTX_INTEGRATOR_WORKER: the estimator of the HOST worker's stage pipeline (src/processors/worker/intersection_worker.cpp,
shading_worker.cpp, worker.cpp:114-149) for one worker.

The oracle's restatement (oracle/pt_oracle.cpp, trace_worker) is PINNED in tests/test_worker_pin.py: it replays the random streams
of the compiled, unmodified worker stages (oracle/host_harness.cpp) and returns their colours bit for bit. Not replicated, because not
a function of the input: entity visit order on exact distance ties between models, thread timing, bounce_count = 0 (uint8_t wrap).
Below: properties of that estimator that follow from the reference's text and from the LIB estimator it shares every building block
with, and the GPU tests that compare the product with the oracle on the same Philox keys, as for the LIB estimator."""
import numpy as np
import pytest

from _common import _proc
from _routes import ctx  # noqa: F401  (a fixture)


def _samples(o, ora, W, H, spp, b, integrator, **kw):
    return o.render_samples(ora.make_cfg(W, H, spp, b, integrator=integrator, **kw), threads=0)


# ------------------------------------------------------------------------------------------------ oracle (CPU)
def test_first_sample_is_not_jittered(cornell_oracle, ora):
    """worker.cpp:125-129: aa_offset = 0 for sample 0; every other sample is jittered exactly like renderer.cpp:363."""
    W, H = 64, 36
    lib0 = cornell_oracle.primary_rays(ora.make_cfg(W, H, 1, 4), 0)
    w0 = cornell_oracle.primary_rays(ora.make_cfg(W, H, 1, 4, integrator=1), 0)
    w1 = cornell_oracle.primary_rays(ora.make_cfg(W, H, 1, 4, integrator=1), 1)
    lib1 = cornell_oracle.primary_rays(ora.make_cfg(W, H, 1, 4), 1)
    np.testing.assert_array_equal(w1, lib1)
    assert not np.array_equal(w0, lib0)
    # worker.cpp:131-135 with aa_offset = 0, through the camera function pinned by the reference's golden vectors
    x, y = np.meshgrid(np.arange(W, dtype=np.float32), np.arange(H, dtype=np.float32))
    ndc_x = (x / np.float32(W)) * np.float32(2) - np.float32(1)
    ndc_y = -((y / np.float32(H)) * np.float32(2) - np.float32(1))
    ratio = np.full_like(ndc_x, np.float32(W) / np.float32(H))
    want = cornell_oracle.camera_rays(np.stack([ndc_x, ndc_y, ratio], -1).reshape(-1, 3))
    np.testing.assert_array_equal(w0.reshape(-1, 6).view(np.uint32), want.view(np.uint32))


def test_one_bounce_equals_lib_estimator(cornell_oracle, ora):
    """bounce_count = 1: both estimators return emissive*10 of the first opaque hit (or the environment): bit-identical."""
    W, H, spp = 48, 27, 3
    a = _samples(cornell_oracle, ora, W, H, spp, 1, 0)
    b = _samples(cornell_oracle, ora, W, H, spp, 1, 1)
    np.testing.assert_array_equal(a[:, :, 1:], b[:, :, 1:])
    assert (a > 0).any()


def test_two_bounces_differ_only_by_the_clamp(cornell_oracle, ora):
    """bounce_count = 2, no sun, opaque: LIB = E0 + min(f,1)*E1 (renderer.cpp:617-620), WORKER = E0 + min(f,10)*E1
    (shading_worker.cpp:173-175) on the same path."""
    W, H, spp = 64, 36, 4
    a = _samples(cornell_oracle, ora, W, H, spp, 2, 0)[:, :, 1:]
    b = _samples(cornell_oracle, ora, W, H, spp, 2, 1)[:, :, 1:]
    assert (b >= a * (1 - 1e-6) - 1e-7).all()
    same = np.abs(a - b).max(-1) <= 1e-5 * np.maximum(a.max(-1), 1e-3)
    assert 0.5 < same.mean() < 1.0


def test_russian_roulette_is_unbiased_and_active(cornell_oracle, ora):
    """shading_worker.cpp:182-190: survivors are divided by p. With bounce_count = 4 no vertex has bounce < 2, so the same
    paths run without roulette; deeper budgets only add light. The converged means must therefore be ordered and close."""
    W, H, spp = 24, 24, 256
    m4, st4 = cornell_oracle.render(ora.make_cfg(W, H, spp, 4, integrator=1), threads=0)
    m8, st8 = cornell_oracle.render(ora.make_cfg(W, H, spp, 8, integrator=1), threads=0)
    lib8, stl = cornell_oracle.render(ora.make_cfg(W, H, spp, 8), threads=0)
    assert np.isfinite(m8).all()
    l4, l8 = m4[..., :3].mean(), m8[..., :3].mean()
    assert l4 * 0.98 < l8 < l4 * 1.6
    # roulette terminates paths: fewer rays than the LIB estimator at the same budget
    assert int(st8[0]) < int(stl[0])
    # [0,10] throughput clamp instead of [0,1]: at least as bright as LIB, same order of magnitude
    assert lib8[..., :3].mean() * 0.98 < l8 < lib8[..., :3].mean() * 2.0


def test_shadow_catcher_without_sun_is_black(ora):
    """shading_worker.cpp:74-95: in_shadow stays true when there is no sun -> ray.color = 0."""
    d = _proc().plaza_scene(level=1, sun=False, alpha=True)
    from conftest import oracle_from_dict
    o = oracle_from_dict(ora, d)
    W, H = 48, 27
    rays = o.primary_rays(ora.make_cfg(W, H, 1, 4, integrator=1), 0).reshape(-1, 6)
    _, idx = o.intersect(rays)
    ground = (idx == 0).reshape(H, W)
    img = _samples(o, ora, W, H, 1, 4, 1)[:, :, 0]
    assert ground.sum() > 100
    assert (img[ground] == 0).all()
    assert (img[~ground] > 0).any()


def test_lit_shadow_catcher_passes_through(ora):
    """shading_worker.cpp:95-104: a catcher whose sun sample is unoccluded is transparent: the ray continues below the ground
    into the environment (1,1,1); catcher pixels are therefore exactly 0 (shadowed) or exactly the environment."""
    d = _proc().plaza_scene(level=1, sun=True, alpha=True)
    from conftest import oracle_from_dict
    o = oracle_from_dict(ora, d)
    W, H = 64, 36
    rays = o.primary_rays(ora.make_cfg(W, H, 1, 4, integrator=1), 0).reshape(-1, 6)
    _, idx = o.intersect(rays)
    ground = (idx == 0).reshape(H, W)
    img = _samples(o, ora, W, H, 1, 4, 1)[:, :, 0]
    g = img[ground]
    black = (g == 0).all(-1)
    env = (g == 1).all(-1)
    assert (black | env).all() and black.any() and env.any()


# ------------------------------------------------------------------------------------------------ product (GPU)
@pytest.fixture(scope="module")
def scene(ptx, ctx):
    from conftest import CORNELL
    return ptx.Scene.load_gltf(ctx, CORNELL)


def _gpu_samples(scene, W, H, spp, b):
    out = np.zeros((H, W, spp, 3), np.float32)
    for k in range(spp):
        a, _ = scene.render(W, H, 1, b, sample0=k, integrator=1)
        out[:, :, k] = a[..., :3]
    return out


def _agree(got, ref):
    assert np.isfinite(got).all()
    err = np.abs(got - ref).max(-1) / np.maximum(np.abs(ref).max(-1), 1e-3)
    return (err < 1e-3).mean()


@pytest.mark.gpu
def test_gpu_worker_cornell_matches_oracle(scene, ctx, cornell_oracle, ora):
    W, H, spp, b = 96, 54, 6, 8            # bounce < 6 from the fourth vertex on: roulette active
    ref = _samples(cornell_oracle, ora, W, H, spp, b, 1)
    got = _gpu_samples(scene, W, H, spp, b)
    assert _agree(got, ref) > 0.995
    W, H, spp, b = 256, 256, 16, 10        # the worker's own default bounce_count (worker.hpp:24)
    mean, st = cornell_oracle.render(ora.make_cfg(W, H, spp, b, integrator=1), threads=0)
    accum, gst = scene.render(W, H, spp, b, integrator=1)
    assert abs(gst["rays"] - int(st[0])) <= 1e-3 * int(st[0])
    psnr = ora.psnr8(ctx.tonemap_encode(accum, W, H, spp), ora.tonemap_write(mean))
    assert psnr >= 40.0, f"PSNR {psnr:.1f} dB"


@pytest.mark.gpu
@pytest.mark.parametrize("level", [2, 3])          # LDS-resident and global-memory kernels
@pytest.mark.parametrize("sun,alpha", [(True, True), (False, True), (True, False)])
def test_gpu_worker_plaza_matches_oracle(ptx, ctx, ora, sun, alpha, level):
    from conftest import oracle_from_dict, product_from_dict
    d = _proc().plaza_scene(level=level, sun=sun, alpha=alpha)
    o, s = oracle_from_dict(ora, d), product_from_dict(ptx, ctx, d)
    W, H, spp, b = 80, 45, 4, 6
    ref = _samples(o, ora, W, H, spp, b, 1)
    got = _gpu_samples(s, W, H, spp, b)
    assert _agree(got, ref) > 0.995
    assert s.info()["lds_resident"] == (1 if level == 2 else 2)


@pytest.mark.gpu
def test_gpu_worker_jack_matches_oracle(ptx, ctx, jack_oracle, ora):
    from conftest import JACK
    s = ptx.Scene.load_gltf(ctx, JACK)
    W, H, spp, b = 96, 54, 4, 6
    ref = _samples(jack_oracle, ora, W, H, spp, b, 1)
    got = _gpu_samples(s, W, H, spp, b)
    assert _agree(got, ref) > 0.995
    W, H, spp, b = 192, 108, 8, 6
    mean, _ = jack_oracle.render(ora.make_cfg(W, H, spp, b, integrator=1), threads=0)
    accum, _ = s.render(W, H, spp, b, integrator=1)
    assert ora.psnr8(ctx.tonemap_encode(accum, W, H, spp), ora.tonemap_write(mean)) >= 40.0
