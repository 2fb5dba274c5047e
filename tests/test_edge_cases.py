"""Edge cases of the hot path through the C ABI, each against the oracle: degenerate budgets (0 samples, 0 bounces), the
smallest and ragged image sizes, tiles on the image border, rays that all miss, an empty scene, zero-area triangles,
and a 4K frame (path ids close to the 32-bit pass limit)."""
import numpy as np
import pytest

from _checks import _glass_stack
from _common import _proc
from _routes import ctx, under_force_global  # noqa: F401  (ctx is a fixture)

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def scene(ptx, ctx):
    from conftest import CORNELL
    return ptx.Scene.load_gltf(ctx, CORNELL)


def test_zero_samples_and_zero_bounces(scene, cornell_oracle, ora):
    acc = np.full((9, 16, 4), 3.5, np.float32)
    out, st = scene.render(16, 9, 0, 4, accum=acc)
    assert (out == 3.5).all() and st["samples"] == 0 and st["rays"] == 0          # sample_count = 0: nothing traced, nothing added
    out, st = scene.render(16, 9, 5, 0)
    np.testing.assert_array_equal(out[..., :3], 0)                                # trace(0, ..) = (0,0,0,1), renderer.cpp:438-439
    np.testing.assert_array_equal(out[..., 3], 5)
    assert st["rays"] == 0
    mean, _ = cornell_oracle.render(ora.make_cfg(16, 9, 5, 0), threads=1)
    np.testing.assert_array_equal(mean[..., :3], 0)
    for integ in (0, 1):
        out, _ = scene.render(16, 9, 2, 0, integrator=integ)
        np.testing.assert_array_equal(out[..., :3], 0)


@pytest.mark.parametrize("W,H,spp", [(1, 1, 7), (7, 5, 3), (65, 3, 2), (3, 129, 1)])
def test_tiny_and_ragged_images(scene, cornell_oracle, ora, W, H, spp):
    """Sizes that are not multiples of the wave (64), the chunk (1024) or anything else."""
    ref = cornell_oracle.render_samples(ora.make_cfg(W, H, spp, 4), threads=2)
    got = np.zeros_like(ref)
    for k in range(spp):
        a, _ = scene.render(W, H, 1, 4, sample0=k)
        got[:, :, k] = a[..., :3]
    err = np.abs(got - ref).max(-1) / np.maximum(np.abs(ref).max(-1), 1e-3)
    assert (err < 1e-3).mean() >= 0.99
    a, st = scene.render(W, H, spp, 4)
    assert st["samples"] == W * H * spp
    np.testing.assert_allclose(a[..., :3], got.sum(2), rtol=1e-6, atol=1e-7)     # sums of the same per-sample values


def test_border_tiles_and_bad_tiles(scene, ptx):
    W, H, spp = 50, 30, 2
    full, _ = scene.render(W, H, spp, 4)
    for tile in [(49, 29, 1, 1), (0, 29, 50, 1), (49, 0, 1, 30), (17, 11, 33, 19)]:
        x0, y0, w, h = tile
        t, _ = scene.render(W, H, spp, 4, tile=tile)
        np.testing.assert_array_equal(t, full[y0:y0 + h, x0:x0 + w])
    for tile in [(49, 29, 2, 1), (50, 0, 1, 1), (0, 0, 51, 30)]:
        with pytest.raises(ptx.PtxError) as e:
            scene.render(W, H, spp, 4, tile=tile)
        assert e.value.code == ptx.ERR_INVALID
    with pytest.raises(ptx.PtxError) as e:
        scene.render(W, H, spp, 4, integrator=7)
    assert e.value.code == ptx.ERR_INVALID


def _from(ptx, ctx, d):
    from conftest import product_from_dict
    return product_from_dict(ptx, ctx, d)


def test_all_rays_miss_gives_the_environment(ptx, ctx, ora):
    """Camera turned away from everything: every sample is exactly environment_factor (renderer.cpp:443-451)."""
    d = _proc().plaza_scene(level=1, sun=True, alpha=True)
    cam = d["camera"].copy()
    cam[3:12] = np.array([1, 0, 0, 0, 0, 1, 0, -1, 0], np.float32)      # -z axis of the basis points straight up (+y)
    d["camera"] = cam
    s = _from(ptx, ctx, d)
    env = (0.25, 0.5, 2.0)
    for integ in (0, 1):
        a, st = s.render(33, 17, 3, 5, env=env, integrator=integ)
        np.testing.assert_array_equal(a[..., :3], np.broadcast_to(np.float32(3) * np.array(env, np.float32), (17, 33, 3)))
        assert st["rays"] == 33 * 17 * 3


def test_empty_scene(ptx, ctx, ora):
    """No models at all (a glTF with only a camera): renderer::intersect finds nothing, every pixel is the environment."""
    d = _proc().plaza_scene(level=0, sun=False, alpha=False)
    e = dict(model_xform=np.zeros((0, 12), np.float32), model_surf=np.zeros((0, 2), np.int32), surf_range=np.zeros((0, 4), np.int32),
             vertices=np.zeros((0, 11), np.float32), triangles=np.zeros((0, 3), np.uint32), materials=np.zeros((0, 11), np.float32),
             camera=d["camera"], sun=None)
    s = _from(ptx, ctx, e)
    info = s.info()
    assert info["n_models"] == 0 and info["n_triangles"] == 0
    a, st = s.render(20, 10, 2, 4)
    np.testing.assert_array_equal(a[..., :3], 2.0)
    h = s.intersect(np.zeros((5, 3), np.float32), np.tile(np.array([[0, 0, -1]], np.float32), (5, 1)))
    assert (h["surface"] == -1).all() and (h["distance"] == -1).all()


def test_zero_area_and_sliver_triangles(ptx, ctx, ora):
    """Degenerate triangles (two equal corners, three collinear corners) have a zero determinant: the reference's division
    yields inf / NaN and the +-epsilon tests reject them (triangle.cpp:160-183). They must not produce hits or NaNs here."""
    from conftest import oracle_from_dict
    d = _proc().plaza_scene(level=1, sun=True, alpha=False)
    tris = d["triangles"].copy()
    sr = d["surf_range"]
    t0 = sr[1][2]
    tris[t0 + 0] = [tris[t0][0], tris[t0][0], tris[t0][2]]          # two equal corners
    tris[t0 + 1] = [tris[t0 + 1][0], tris[t0 + 1][1], tris[t0 + 1][1]]
    verts = d["vertices"].copy()
    v0 = sr[1][0]
    a, b = verts[v0 + tris[t0 + 2][0], :3], verts[v0 + tris[t0 + 2][1], :3]
    verts[v0 + tris[t0 + 2][2], :3] = a + (b - a) * np.float32(0.5)  # collinear
    d = dict(d, triangles=tris, vertices=verts)
    o, s = oracle_from_dict(ora, d), _from(ptx, ctx, d)
    W, H, spp, b = 64, 36, 3, 5
    ref = o.render_samples(ora.make_cfg(W, H, spp, b), threads=0)
    got = np.zeros_like(ref)
    for k in range(spp):
        acc, _ = s.render(W, H, 1, b, sample0=k)
        got[:, :, k] = acc[..., :3]
    assert np.isfinite(got).all() and np.isfinite(ref).all()
    err = np.abs(got - ref).max(-1) / np.maximum(np.abs(ref).max(-1), 1e-3)
    assert (err < 1e-3).mean() > 0.995
    rays = o.primary_rays(ora.make_cfg(W, H, 1, b), 0).reshape(-1, 6)
    out, idx = o.intersect(rays)
    hits = s.intersect(rays[:, :3], rays[:, 3:])
    np.testing.assert_array_equal(hits["surface"], idx)
    m = idx >= 0
    pos = np.stack([hits["px"], hits["py"], hits["pz"]], 1)
    nrm = np.stack([hits["nx"], hits["ny"], hits["nz"]], 1)
    np.testing.assert_array_equal(pos[m].view(np.uint32), out[m, 0:3].view(np.uint32))
    np.testing.assert_array_equal(nrm[m].view(np.uint32), out[m, 11:14].view(np.uint32))


def test_4k_frame_one_sample(scene, cornell_oracle, ora):
    """BASELINE config 5's resolution: 8.3 M pixels in one pass; a tile of it against the oracle, and the whole frame's checksum
    against the sum of its four quadrants rendered separately."""
    W, H = 3840, 2160
    full, st = scene.render(W, H, 1, 4)
    assert st["samples"] == W * H and np.isfinite(full).all()
    tile = (1900, 1000, 96, 64)
    mean, _ = cornell_oracle.render(ora.make_cfg(W, H, 1, 4, tile=tile), threads=0)
    sub = full[tile[1]:tile[1] + tile[3], tile[0]:tile[0] + tile[2], :3]
    rel = np.abs(sub - mean[..., :3]).max(-1) / np.maximum(mean[..., :3].max(-1), 1e-3)
    assert (rel < 1e-3).mean() > 0.99
    q, _ = scene.render(W, H, 1, 4, tile=(W // 2, H // 2, W // 2, H // 2))
    np.testing.assert_array_equal(q, full[H // 2:, W // 2:])


def test_context_destroyed_before_its_scene(ptx):
    """Destruction order is free: a scene keeps its context alive (garbage collectors finalise cycles in arbitrary order)."""
    from conftest import CORNELL
    c = ptx.Context(0)
    s = ptx.Scene.load_gltf(c, CORNELL)
    c.close()                                   # ptx_ctx_destroy first
    a, st = s.render(32, 18, 2, 3)              # the scene still renders on the context it holds
    assert st["samples"] == 32 * 18 * 2 and np.isfinite(a).all()
    s.close()                                   # the last reference frees the context


def test_non_finite_rays_and_scene_churn(scene, ptx, ctx):
    """NaN / inf ray components are misses (every box comparison is false), never a hang; scenes can be created and destroyed
    repeatedly on one context."""
    from conftest import CORNELL
    bad = np.array([[np.nan, 0, 0], [0, np.inf, 0], [0, 2, 11], [0, 2, 11], [0, 2, 11], [-np.inf, np.nan, 0]], np.float32)
    dirs = np.array([[0, 0, -1], [0, 0, -1], [np.nan, 0, -1], [0, np.inf, 0], [0, 0, 0], [0, 0, -1]], np.float32)
    h = scene.intersect(bad, dirs)
    assert (h["surface"] == -1).all()
    good = scene.intersect(np.array([[0, 2, 11]], np.float32), np.array([[0, 0, -1]], np.float32))
    assert good["surface"][0] >= 0
    ref, _ = scene.render(24, 16, 2, 3)
    for _ in range(12):
        s = ptx.Scene.load_gltf(ctx, CORNELL)
        a, _ = s.render(24, 16, 2, 3)
        np.testing.assert_array_equal(a, ref)
        s.close()


def test_concurrent_callers(scene, ptx):
    """SURVEY §8b threading contract: ptx_render is safe to call from several host threads — on one context (serialised by the
    context's lock) and on two contexts of the same device (own streams and workspaces) — and returns what a serial caller gets."""
    import threading
    from conftest import CORNELL
    W, H, spp, b = 64, 48, 3, 4
    full, _ = scene.render(W, H, spp, b)
    tiles = [(0, 0, 32, 24), (32, 0, 32, 24), (0, 24, 32, 24), (32, 24, 32, 24)]
    out, errs = {}, []

    def work(sc, k, tile):
        try:
            for _ in range(5):
                out[k], _ = sc.render(W, H, spp, b, tile=tile)
        except Exception as e:        # pragma: no cover
            errs.append(e)

    c2 = ptx.Context(0)
    s2 = ptx.Scene.load_gltf(c2, CORNELL)
    th = [threading.Thread(target=work, args=(scene if k < 4 else s2, k, tiles[k % 4])) for k in range(8)]
    for t in th:
        t.start()
    for t in th:
        t.join()
    assert not errs, errs
    for k in range(8):
        x0, y0, w, h = tiles[k % 4]
        np.testing.assert_array_equal(out[k], full[y0:y0 + h, x0:x0 + w])


def test_many_pass_throughs_without_consuming_bounces(ptx, ctx, ora):
    """Opacity pass-through (renderer.cpp:466-472) re-traces from behind the surface WITHOUT consuming a bounce: 40 half-transparent
    layers, 2 bounces — paths cross up to 40 layers at depth 0 (pass counter 0..40 in the RNG key). Per-sample parity with the oracle."""
    from conftest import oracle_from_dict
    d = _glass_stack(40, 0.5)
    s, o = _from(ptx, ctx, d), oracle_from_dict(ora, d)
    W, H, spp, b = 24, 16, 6, 2
    ref = o.render_samples(ora.make_cfg(W, H, spp, b), threads=0)
    got = np.zeros_like(ref)
    rays = 0
    for k in range(spp):
        a, st = s.render(W, H, 1, b, sample0=k)
        got[:, :, k] = a[..., :3]
        rays += st["rays"]
    assert rays > 2.5 * W * H * spp                         # pass-throughs are extra renderer::intersect calls
    err = np.abs(got - ref).max(-1) / np.maximum(np.abs(ref).max(-1), 1e-3)
    assert (err < 1e-3).mean() > 0.995


def test_pass_through_cap_is_a_documented_safety_bound(ptx, ctx):
    """A path that would pass through more than 4096 surfaces at one depth ends there (kernels.hip shade_vertex; the reference would
    recurse until its stack overflows, renderer.cpp:466-472 has no bound): 4200 fully transparent layers (opacity 0) — the render
    terminates, every sample is finite, black (nothing was ever added) and costs exactly 4097 closest-hit queries."""
    d = _glass_stack(4200, 0.0)
    s = _from(ptx, ctx, d)
    a, st = s.render(4, 3, 2, 3)
    assert np.isfinite(a).all() and (a[..., :3] == 0).all() and (a[..., 3] == 2).all()
    assert st["rays"] == 4 * 3 * 2 * 4097


def test_pass_throughs_on_the_queue_based_pipeline(ptx, ctx, monkeypatch):
    """The same two pass-through cases through wavefront.hip (a scene made to keep its trees in global memory, PTX_FORCE_GLOBAL at
    creation; PTX_WAVEFRONT per call): one stream entry per pass-through and step — 40 half-transparent layers bitwise equal to the
    fused kernel; 4200 fully transparent ones stop at the same bound after exactly 4097 closest-hit queries per sample, 4097 steps."""
    s40, s4200 = under_force_global(monkeypatch, True, lambda: (_from(ptx, ctx, _glass_stack(40, 0.5)), _from(ptx, ctx, _glass_stack(4200, 0.0))))
    assert s40.info()["lds_resident"] == 0
    out = []
    for on in ("0", "1"):
        monkeypatch.setenv("PTX_WAVEFRONT", on)
        out.append(s40.render(24, 16, 6, 2))
    (a0, st0), (a1, st1) = out
    np.testing.assert_array_equal(a1.view(np.uint32), a0.view(np.uint32))
    assert st1["rays"] == st0["rays"] > 2.5 * 24 * 16 * 6
    monkeypatch.setenv("PTX_WAVEFRONT", "1")
    a, st = s4200.render(4, 3, 2, 3)
    assert np.isfinite(a).all() and (a[..., :3] == 0).all() and (a[..., 3] == 2).all()
    assert st["rays"] == 4 * 3 * 2 * 4097
