"""The 64-wide limits of both integrators, against the oracle.

Both integrators keep per-surface and per-model state in 64-wide words: the queue-based pipeline (wavefront.hip) a 64-bit mask
of entered surfaces per ray, one lane per surface in k_wf_classify and `range` masks built from `first_surface`; the fused
kernel (kernels.hip) the lengths of its deferral lists in the 64 lanes of one VGPR (surface units up to 64 surfaces, model
units from 2 up to 64 models, the non-deferred path above). procedural.cloud_scene builds scenes at and just past those
limits:
  * "overlap": every surface box contains the camera, so every camera ray enters every box (64 pairs per ray, full masks,
    results read past the four-pair prefetch);
  * "scattered": a ray enters a few boxes, so single surfaces / models are rarely entered and go to the deferral lists, up
    to lane 63.
Every route that can run a shape is checked: the fused kernel on LDS-resident geometry (the default at 16 triangles per
surface), the fused kernel on global memory (PTX_FORCE_GLOBAL at creation) and the queue-based pipeline (PTX_WAVEFRONT=1,
at most 64 surfaces), each with surface and model units (PTX_SURFACE_UNITS) where the scene allows them. Each route is
asserted from the scene's residency and the pipeline the render reports, so a silent fallback cannot pass.
Bars as in test_gpu_parity: hit records bit-exact, >= 99.5 % of samples within 1e-3 relative, ray counts within 2e-4, and
the routes bitwise equal to each other.
"""
import numpy as np
import pytest

from _checks import _check_records, _same_hits, _scene_parity
from _common import _bits, _proc
from _routes import clean_env, ctx, forced_routes, under_force_global  # noqa: F401  (clean_env and ctx are fixtures)
from conftest import oracle_from_dict, product_from_dict

W, H, SPP, B = 64, 36, 2, 5                 # per-sample radiance against the oracle
FW, FH, FSPP = 128, 72, 4                   # frames for the ray counts and the route agreement


# ---------------------------------------------------------------------------- the generator and the oracle (no GPU)
def _local_boxes(d):
    """Per surface: the box of its vertices in its model's local space, and the model's (basis, origin), world = basis @ local + origin."""
    out = []
    for m, (f, n) in enumerate(np.asarray(d["model_surf"])):
        x = np.asarray(d["model_xform"][m], np.float64)
        basis, origin = x[3:].reshape(3, 3).T, x[:3]
        for u in range(f, f + n):
            v0, nv = d["surf_range"][u][:2]
            p = np.asarray(d["vertices"][v0:v0 + nv, :3], np.float64)
            out.append((p.min(0), p.max(0), basis, origin))
    return out


@pytest.mark.parametrize("n_models,spm,spaces", [(1, 64, None), (1, 65, None), (64, 1, None), (2, 32, 1), (3, 21, None), (8, 8, 2)])
@pytest.mark.parametrize("layout", ["overlap", "scattered"])
def test_cloud_scene_shapes(n_models, spm, spaces, layout):
    d = _proc().cloud_scene(n_models, spm, 16, layout=layout, spaces=spaces)
    n_surf = n_models * spm
    assert d["vertices"].shape == (n_surf * 16 * 3, 11) and d["vertices"].dtype == np.float32
    assert d["triangles"].shape == (n_surf * 16, 3) and d["triangles"].max() < len(d["vertices"])
    assert np.isfinite(d["vertices"]).all()
    assert d["model_xform"].shape == (n_models, 12) and d["materials"].shape == (n_surf, 11)
    assert d["model_surf"].tolist() == [[m * spm, spm] for m in range(n_models)]
    sr = d["surf_range"]
    assert sr.shape == (n_surf, 4) and (sr[1:, 0] == sr[:-1, 0] + sr[:-1, 1]).all() and (sr[:, 3] == 16).all()
    assert d["camera"].shape == (13,) and d["sun"].shape == (13,)
    nrm = np.linalg.norm(d["vertices"][:, 5:8], axis=1)
    assert np.allclose(nrm, 1, atol=1e-5) and np.allclose(np.linalg.norm(d["vertices"][:, 8:11], axis=1), 1, atol=1e-5)
    # transforms: rotation x non-uniform scale; with `spaces` = k, model m repeats model m - k bitwise and differs from m - 1
    basis = d["model_xform"][:, 3:].reshape(-1, 3, 3)
    assert (np.abs(np.linalg.det(basis.astype(np.float64))) > 0.05).all()
    if spaces is not None and n_models > spaces:
        xb = d["model_xform"].view(np.uint32)
        assert (xb[spaces:] == xb[:-spaces]).all()
        if spaces > 1:
            assert (xb[1:] != xb[:-1]).any(1).all()
    elif n_models > 1:
        assert len(np.unique(d["model_xform"], axis=0)) == n_models
    if layout == "overlap":
        # every surface box, in its model's space, contains the camera and the inner cube [-0.5, 0.5]^3
        pts = np.concatenate([d["camera"][None, :3].astype(np.float64),
                              np.array([[sx, sy, sz] for sx in (-.5, .5) for sy in (-.5, .5) for sz in (-.5, .5)])])
        for lo, hi, basis, origin in _local_boxes(d):
            loc = (pts - origin) @ np.linalg.inv(basis).T
            assert (loc > lo).all() and (loc < hi).all()


def test_cloud_scene_is_deterministic_and_checks_its_arguments():
    a, b = _proc().cloud_scene(2, 5, 9, seed=3), _proc().cloud_scene(2, 5, 9, seed=3)
    for k in a:
        np.testing.assert_array_equal(a[k], b[k])
    with pytest.raises(ValueError):
        _proc().cloud_scene(1, 4, 8, layout="grid")
    with pytest.raises(ValueError):
        _proc().cloud_scene(1, 4, 7, layout="overlap")


@pytest.mark.parametrize("n_models,spm,spaces", [(1, 64, None), (1, 65, None), (8, 8, 2), (5, 13, None)])
def test_overlap_every_ray_tests_every_surface_in_the_oracle(ora, n_models, spm, spaces):
    """The oracle's own count: camera rays and rays from the inner cube test every surface's tree (model.cpp:37-60 — every
    model box is entered, then every surface box), and surfaces past index 32 win a real share of the closest hits."""
    d = _proc().cloud_scene(n_models, spm, 16, layout="overlap", spaces=spaces)
    o = oracle_from_dict(ora, d)
    rays = _inside_rays(o, 30_000, np.random.default_rng(1))
    out, idx, st = o.intersect(rays, stats=True)
    n_surf = n_models * spm
    assert int(st[1]) == n_surf * len(rays) and int(st[0]) == n_models * len(rays)
    assert 0.05 < (idx >= 0).mean() < 0.9
    hi = idx[idx >= 32]
    assert len(hi) > 0.1 * (idx >= 0).sum() and len(np.unique(hi)) >= 16
    if n_surf > 63:
        assert (idx == 63).any()


def test_scattered_rays_enter_few_surfaces(ora):
    d = _proc().cloud_scene(1, 64, 16, layout="scattered")
    o = oracle_from_dict(ora, d)
    prim = o.primary_rays(ora.make_cfg(W, H, 1, B), 0).reshape(-1, 6)
    out, idx = o.intersect(prim)
    win = np.unique(idx[idx >= 0])
    assert len(win) >= 48 and win.max() == 63
    # each surface box holds a cluster of a 0.5-spaced grid: a camera ray's entries stay few (the oracle reports tests,
    # so count entries from the boxes here)
    boxes = _local_boxes(d)
    lo = np.array([b[0] for b in boxes]); hi = np.array([b[1] for b in boxes])
    basis, origin = boxes[0][2], boxes[0][3]
    inv = np.linalg.inv(basis)
    ol = (prim[:, :3] - origin) @ inv.T
    dl = prim[:, 3:] @ inv.T
    with np.errstate(divide="ignore", invalid="ignore"):
        t0 = (lo[None] - ol[:, None]) / dl[:, None]
        t1 = (hi[None] - ol[:, None]) / dl[:, None]
    tn = np.minimum(t0, t1).max(-1)
    tf = np.maximum(t0, t1).min(-1)
    entered = ((tf >= tn) & (tf >= 0)).sum(1)
    assert entered.max() <= 4 and 0.05 < (entered > 0).mean() < 0.8


@pytest.mark.parametrize("n_surf", [64, 65])
def test_host_scene_reports_surface_counts(ptx, n_surf):
    d = _proc().cloud_scene(1, n_surf, 16)
    s = product_from_dict(ptx, None, d)
    info = s.info()
    assert info["n_surfaces"] == n_surf and info["n_models"] == 1 and info["n_triangles"] == 16 * n_surf
    assert info["lds_resident"] == 1                      # the GPU tests' default route: everything in LDS
    big = product_from_dict(ptx, None, _proc().cloud_scene(1, n_surf, 24))
    assert big.info()["lds_resident"] == 2                # 24 triangles per surface: hybrid residency without switches
    d2 = _proc().cloud_scene(n_surf, 1, 16, layout="scattered")
    assert product_from_dict(ptx, None, d2).info()["n_models"] == n_surf


# ---------------------------------------------------------------------------- GPU: every route against the oracle
def _inside_rays(o, n, rng):
    """Rays whose origins lie inside every "overlap" surface box: camera rays, then random points of the inner cube with finite unit
    directions."""
    from oracle import pt_oracle as ora
    cam = o.primary_rays(ora.make_cfg(160, 90, 1, B), 0).reshape(-1, 6)[:n]
    k = n - len(cam)
    org = rng.uniform(-0.5, 0.5, (k, 3)).astype(np.float32)
    d = rng.standard_normal((k, 3)).astype(np.float32)
    d /= np.linalg.norm(d, axis=1, keepdims=True).astype(np.float32)
    return np.concatenate([cam, np.concatenate([org, d.astype(np.float32)], 1)]).astype(np.float32)


def _hit_rays(o, ora, rng, n_bounce=20_000):
    """Camera rays plus bounce rays off their hit points (as _scene_parity builds them)."""
    prim = o.primary_rays(ora.make_cfg(160, 90, 1, B), 0).reshape(-1, 6)
    out, idx = o.intersect(prim)
    sel = rng.choice(np.flatnonzero(idx >= 0), n_bounce, replace=True)
    dd = rng.standard_normal((n_bounce, 3)).astype(np.float32)
    dd /= np.linalg.norm(dd, axis=1, keepdims=True).astype(np.float32)
    dd = np.where((dd * out[sel, 11:14]).sum(1, keepdims=True) < 0, -dd, dd).astype(np.float32)
    sec = np.concatenate([out[sel, :3] + out[sel, 11:14] * np.float32(1e-4), dd], 1).astype(np.float32)
    return np.concatenate([prim, sec]).astype(np.float32)


SHAPES = [(1, 63, None), (1, 64, None), (1, 65, None), (64, 1, None), (65, 1, None), (2, 32, 1), (3, 21, None), (8, 8, 2), (5, 13, None)]


@pytest.mark.gpu
@pytest.mark.parametrize("layout", ["overlap", "scattered"])
@pytest.mark.parametrize("n_models,spm,spaces", SHAPES, ids=[f"{a}x{b}" + (f"-spaces{c}" if c else "") for a, b, c in SHAPES])
def test_unit_limits_every_route_against_oracle(ptx, ctx, ora, clean_env, n_models, spm, spaces, layout):
    mp = clean_env
    n_surf = n_models * spm
    d = _proc().cloud_scene(n_models, spm, 16, layout=layout, spaces=spaces)
    mp.setenv("PTX_WAVEFRONT", "0")
    s_lds, o = _scene_parity(ptx, ctx, ora, d, W, H, SPP, B, n_rays=20_000)     # hit records + per-sample radiance, default route
    rays = _hit_rays(o, ora, np.random.default_rng(n_surf))
    out, idx = o.intersect(rays)
    if layout == "overlap" and n_surf > 32:
        assert (idx >= 32).mean() > 0.02                 # the upper half of the mask words wins closest hits
    ref = {ig: o.render_samples(ora.make_cfg(W, H, SPP, B, integrator=ig), threads=0) for ig in (0, 1)}
    oray = {ig: int(o.render(ora.make_cfg(FW, FH, FSPP, B, integrator=ig), threads=0)[1][0]) for ig in (0, 1)}
    units = ["0", "1"] if n_surf <= 64 else ["0"]        # surface units only where the 64-lane lists can hold every surface
    hits0, frames0, rays0 = None, {}, {}
    for name, force_global, env, mode, pipeline in forced_routes(n_surf):
        mp.setenv("PTX_WAVEFRONT", env["PTX_WAVEFRONT"])       # the other switches stay as the route before left them
        s = under_force_global(mp, True, lambda: product_from_dict(ptx, ctx, d)) if force_global else s_lds
        info = s.info()
        assert info["lds_resident"] == mode and info["n_surfaces"] == n_surf and info["n_models"] == n_models, name
        hits = s.intersect(rays[:, :3], rays[:, 3:])
        _check_records(hits, o, rays, out, idx)
        if hits0 is None:
            hits0 = hits
        else:
            _same_hits(hits, hits0, name)
        for un in (units if pipeline == 0 else [None]):
            if un is None:
                mp.delenv("PTX_SURFACE_UNITS", raising=False)
            else:
                mp.setenv("PTX_SURFACE_UNITS", un)
            what = f"{name} units={un}"
            for ig in (0, 1):
                got = np.zeros_like(ref[ig])
                for k in range(SPP):
                    a, _ = s.render(W, H, 1, B, sample0=k, integrator=ig)
                    assert ctx.timing()["pipeline"] == pipeline, what
                    got[:, :, k] = a[..., :3]
                assert np.isfinite(got).all()
                err = np.abs(got - ref[ig]).max(-1) / np.maximum(np.abs(ref[ig]).max(-1), 1e-3)
                assert (err < 1e-3).mean() > 0.995, f"{what} integrator {ig}: {(err < 1e-3).mean():.4%} of samples agree"
                frame, st = s.render(FW, FH, FSPP, B, integrator=ig)
                assert ctx.timing()["pipeline"] == pipeline, what
                assert abs(st["rays"] - oray[ig]) <= 2e-4 * oray[ig], (what, ig, st["rays"], oray[ig])
                if ig not in frames0:
                    frames0[ig], rays0[ig] = frame, st["rays"]
                else:
                    np.testing.assert_array_equal(_bits(frame), _bits(frames0[ig]), err_msg=f"{what} integrator {ig}")
                    assert st["rays"] == rays0[ig], what


# ---------------------------------------------------------------------------- GPU: the pair pool's overflow and exact fit
def _overflow_scene(ptx, ctx, ora, n, seed):
    """A FRESH 1 x 64 "overlap" scene at 24 triangles per surface (hybrid residency: the queue pipeline is its default route) and n rays
    that each enter exactly 64 surface boxes — proved from the oracle's count — with the oracle's records."""
    d = _proc().cloud_scene(1, 64, 24, layout="overlap")
    o = oracle_from_dict(ora, d)
    rays = _inside_rays(o, n, np.random.default_rng(seed))
    out, idx, st = o.intersect(rays, stats=True)
    assert int(st[1]) == 64 * n
    s = product_from_dict(ptx, ctx, d)
    assert s.info()["lds_resident"] == 2
    return s, o, rays, out, idx


def _assert_queue_route(s, ctx):
    """ptx_intersect_batch and ptx_render choose their pipeline with the same rule: a render of the scene under the same environment
    reports the route the batch took."""
    s.render(32, 18, 1, 2)
    assert ctx.timing()["pipeline"] == 1


@pytest.mark.gpu
def test_batch_overflowing_its_first_slice(ptx, ctx, ora, clean_env):
    """No switches: the first slice of a fresh scene is sized for min(surfaces, 4) = 4 pairs per ray in a 16 Mi-pair pool, but these
    320 000 rays need 64 each (20.5 M pairs): the slice overflows, k_wf_merge_batch must leave its outputs alone, and the host repeats
    the batch in smaller slices. Every output group is requested; the records are the oracle's and the fused kernel's, bit for bit."""
    n = 320_000
    s, o, rays, out, idx = _overflow_scene(ptx, ctx, ora, n, 3)
    assert 64 * n > 1 << 24
    hits = s.intersect(rays[:, :3], rays[:, 3:])
    _check_records(hits, o, rays, out, idx)
    _assert_queue_route(s, ctx)
    clean_env.setenv("PTX_WAVEFRONT", "0")
    _same_hits(s.intersect(rays[:, :3], rays[:, 3:]), hits, "fused kernel")


@pytest.mark.gpu
def test_batch_slice_that_fills_the_pool_exactly(ptx, ctx, ora, clean_env):
    """A 1 Mi-pair pool (PTX_WF_PAIRS_M=1): after the first slice (100 000 rays at the guess of 4 pairs per ray) overflows, the learnt 64
    pairs per ray give the 16 384-ray minimum slice, whose 16 x 65 536 pairs fill the pool to its last pair. That slice must fit:
    `base + block_total > pool_cap` in k_wf_classify (with `>=` the library gives up: "cannot hold a 16384-ray slice")."""
    clean_env.setenv("PTX_WF_PAIRS_M", "1")
    n = 100_000
    s, o, rays, out, idx = _overflow_scene(ptx, ctx, ora, n, 4)
    hits = s.intersect(rays[:, :3], rays[:, 3:])
    _check_records(hits, o, rays, out, idx)
    _assert_queue_route(s, ctx)
    assert ctx.timing()["pool_pairs"] == 1 << 20
    clean_env.setenv("PTX_WAVEFRONT", "0")
    _same_hits(s.intersect(rays[:, :3], rays[:, 3:]), hits, "fused kernel")


@pytest.mark.gpu
def test_render_overflowing_a_small_pool(ptx, ctx, ora, clean_env):
    """A render of a fresh 1 x 64 "overlap" scene in a 1 Mi-pair pool: its first step asks for 64 pairs per camera ray and overflows;
    the slabs are repeated smaller. Per-sample radiance against the oracle, and the frame and the ray count bitwise those of the fused
    kernel."""
    clean_env.setenv("PTX_WF_PAIRS_M", "1")
    d = _proc().cloud_scene(1, 64, 24, layout="overlap")
    o = oracle_from_dict(ora, d)
    rW, rH, spp = 192, 108, 2
    prim = o.primary_rays(ora.make_cfg(rW, rH, 1, B), 0).reshape(-1, 6)
    _, _, st = o.intersect(prim, stats=True)
    assert int(st[1]) == 64 * len(prim) and 64 * len(prim) > 1 << 20
    s = product_from_dict(ptx, ctx, d)
    assert s.info()["lds_resident"] == 2
    ref = o.render_samples(ora.make_cfg(rW, rH, spp, B), threads=0)
    got = np.zeros_like(ref)
    for k in range(spp):
        a, _ = s.render(rW, rH, 1, B, sample0=k)
        tm = ctx.timing()
        assert tm["pipeline"] == 1 and tm["pool_pairs"] == 1 << 20
        if k == 0:
            assert tm["pool_overflows"] >= 1
        got[:, :, k] = a[..., :3]
    err = np.abs(got - ref).max(-1) / np.maximum(np.abs(ref).max(-1), 1e-3)
    assert (err < 1e-3).mean() > 0.995, f"{(err < 1e-3).mean():.4%} of samples agree"
    frame, fst = s.render(rW, rH, spp, B)
    assert ctx.timing()["pipeline"] == 1
    mean, ost = o.render(ora.make_cfg(rW, rH, spp, B), threads=0)
    assert abs(fst["rays"] - int(ost[0])) <= 2e-4 * int(ost[0])
    clean_env.setenv("PTX_WAVEFRONT", "0")
    fused, fust = s.render(rW, rH, spp, B)
    assert ctx.timing()["pipeline"] == 0
    np.testing.assert_array_equal(_bits(frame), _bits(fused))
    assert fst["rays"] == fust["rays"]
