"""Moving a loaded scene, on the GPU: the lens in every caller of camera_ray against tests/_camera_restatement.py (the batch call, the guide
buffers bit for bit, per-sample radiance of ptx_render and ptx_render_nee through the proxy oracle), the product against itself with a lens
(fused against unfused, sample ranges, the adaptive loop), nothing moving without a lens, a moved pinhole camera and ptx_scene_set_model_xforms
against scenes created fresh, depth of field doing what it says, and the mirrors.

The worker estimator (PTX_INTEGRATOR_WORKER) takes its camera ray from the same device function; the oracle's worker frame does not take its
rays from primary_rays, so the proxy cannot serve it: its lens rays are covered by the restated primary_rays of the CPU file and the batch call.

Measured on the MI355X: every per-sample case has 100 % of its samples within 1e-3 of the restatement (worst: Cornell 3.6e-05, plaza 4.5e-07,
lit.gltf 4.5e-04, atrium 4.9e-06; moved Cornell 3.9e-07); depth of field: predicted circle of confusion 5.68 px, coverage reaches 0 px outside
the silhouette in focus and 5.0 px focused behind.
"""
import contextlib
import json
import os
import subprocess

import numpy as np
import pytest

import _adaptive_restatement as AR
from _aov_restatement import restate
from _camera_restatement import Camera, LensOracle, moved_xforms
from _common import _bits, _proc, _same
from _nee_common import SEED, _err
from _nee_estimator import render_samples
from _nee_lit_scenes import LIT
from _routes import (DEFAULT_ROUTES, ROUTE_VARS, Scenes, assert_route, clean_env, ctx, forced_routes, on_route, route_named,  # noqa: F401
                     under_force_global, use_route)
from conftest import CORNELL, ROOT, oracle_from_dict, product_from_dict

f32 = np.float32
pytestmark = pytest.mark.gpu

# ---------------------------------------------------------------------------- scenes and lenses
_dicts, _oracles = {}, {}
_MAKERS = {"plaza": lambda p: p.plaza_scene(level=1, sun=True, alpha=True), "atrium": lambda p: p.atrium_scene(0),
           "cloud": lambda p: p.emitter_cloud_scene(sun=False, alpha=False)}


def _dict(name):
    if name not in _dicts:
        _dicts[name] = _MAKERS[name](_proc())
    return _dicts[name]


def _oracle(ora, name):
    """(oracle scene, its arrays)"""
    if name not in _oracles:
        if name in ("cornell", "lit"):
            a = ora.load_gltf(CORNELL if name == "cornell" else LIT)
            _oracles[name] = (ora.OracleScene(a), a)
        else:
            o = oracle_from_dict(ora, _dict(name))
            _oracles[name] = (o, o.a)
    return _oracles[name]


def _make(ptx, ctx, name):
    if name in ("cornell", "lit"):
        return ptx.Scene.load_gltf(ctx, CORNELL if name == "cornell" else LIT)
    return product_from_dict(ptx, ctx, _dict(name))


SCENES = Scenes(_make)
_depths = {}


def _centre_depth(ora, name, cam14):
    """distance of what the central camera ray sees: the depth of the scene's centre"""
    if name not in _depths:
        ray = Camera(cam14).pinhole(np.zeros(1, f32), np.zeros(1, f32), np.full(1, f32(1.5)))
        out, idx = _oracle(ora, name)[0].intersect(ray)
        _depths[name] = float(np.linalg.norm(out[0, :3].astype(np.float64) - ray[0, :3])) if idx[0] >= 0 else 5.0
    return _depths[name]


def _lens(ora, name, cam14, which):
    """the two lenses: (R, F, blades, rotation) = (0.05, depth of the scene's centre, 6, 0) and (0.5, half that, 16, rotated)"""
    dc = _centre_depth(ora, name, cam14)
    return (0.05, dc, 6, 0.0) if which == 0 else (0.5, 0.5 * dc, 16, 0.4)


@contextlib.contextmanager
def lens_on(s, lens):
    """the scene with the lens on its camera; the pinhole again afterwards (the scenes are shared between the tests)"""
    c = s.camera()
    s.set_camera(c["origin"], c["basis"], c["yfov"], *lens)
    try:
        yield s
    finally:
        s.set_camera(c["origin"], c["basis"], c["yfov"])


def _proxy(ptx, ora, name, s, lens):
    o, a = _oracle(ora, name)
    return LensOracle(ora, o, Camera(s.array(ptx.ARR_CAMERA), *lens)), a


# ---------------------------------------------------------------------------- 5. the batch call
@pytest.mark.parametrize("which", [0, 1])
def test_lens_rays_batch_is_the_restatement(ptx, ctx, ora, clean_env, which):
    import torch
    s = SCENES.get(ptx, ctx, clean_env, "plaza")
    cam14 = s.array(ptx.ARR_CAMERA)
    rng = np.random.default_rng(5 + which)
    n = 5000
    in5 = np.concatenate([rng.uniform(-1, 1, (n, 2)), rng.uniform(0.5, 2.5, (n, 1)), rng.random((n, 2))], 1).astype(f32)
    in5[:700, 3] = 0.0                                  # u = 0
    in5[700:1400, 3] = f32(1) - f32(2.0 ** -24)         # the clamp of k
    in5[1400:2100:2, 4] = 0.0                           # v = 0
    in5[300:500, 4] = 0.0
    lens = _lens(ora, "plaza", cam14, which)
    pin = s.camera_rays(in5[:, :3])
    _same(s.lens_rays(in5), pin, "without a lens the batch gives the pinhole rays")
    with lens_on(s, lens):
        want = Camera(cam14, *lens).rays(in5[:, 0], in5[:, 1], in5[:, 2], in5[:, 3], in5[:, 4])
        got = s.lens_rays(in5)
        _same(got, want, "host pointers")
        assert (_bits(got) != _bits(pin)).any()
        _same(s.camera_rays(in5[:, :3]), pin, "ptx_camera_rays_batch stays the pinhole function")
        d_in, d_out = torch.from_numpy(in5).cuda(), torch.zeros((n, 6), dtype=torch.float32, device="cuda")
        assert ptx.lib().ptx_camera_lens_rays_batch(s.h, d_in.data_ptr(), n, d_out.data_ptr()) == 0
        ctx.synchronize()
        _same(d_out.cpu().numpy(), want, "device pointers")
        L = ptx.lib()
        assert L.ptx_camera_lens_rays_batch(None, in5.ctypes.data, n, got.ctypes.data) == ptx.ERR_INVALID
        assert L.ptx_camera_lens_rays_batch(s.h, None, n, got.ctypes.data) == ptx.ERR_INVALID
        assert L.ptx_camera_lens_rays_batch(s.h, in5.ctypes.data, n, d_out.data_ptr()) == ptx.ERR_INVALID   # mixed kinds
        assert L.ptx_camera_lens_rays_batch(s.h, None, 0, None) == 0
    host = _make(ptx, None, "plaza")
    assert ptx.lib().ptx_camera_lens_rays_batch(host.h, in5.ctypes.data, n, got.ctypes.data) == ptx.ERR_NO_DEVICE


# ---------------------------------------------------------------------------- 6. the guide buffers, depth included
AW, AH, ATILE, AS0, ASPP = 40, 24, (5, 3, 31, 19), 2, 3
AOV_ROUTES = [("plaza", r, w) for r, w in zip(DEFAULT_ROUTES, (0, 1, 1))] + [("cornell", DEFAULT_ROUTES[0], 1)]
_aov_refs = {}


def _aov_ref(ptx, ora, name, s, which):
    if (name, which) not in _aov_refs:
        lens = _lens(ora, name, s.array(ptx.ARR_CAMERA), which)
        _aov_refs[(name, which)] = restate(ora, _proxy(ptx, ora, name, s, lens)[0], W_=AW, H_=AH, tile=ATILE, sample0=AS0, spp=ASPP)[:2]
    return _aov_refs[(name, which)]


@pytest.mark.parametrize("name,route,which", AOV_ROUTES, ids=[f"{n}-{r.name.replace(' ', '_')}-lens{w}" for n, r, w in AOV_ROUTES])
def test_aov_with_a_lens_is_the_restatement(ptx, ctx, ora, clean_env, name, route, which):
    s = on_route(SCENES, ptx, ctx, clean_env, name, route)
    assert_route(ctx, s, route, f"{name} {route.name}")
    want_a, want_n = _aov_ref(ptx, ora, name, s, which)
    pin_a, pin_n, _ = s.render_aov(AW, AH, ASPP, tile=ATILE, sample0=AS0, seed=SEED)
    with lens_on(s, _lens(ora, name, s.array(ptx.ARR_CAMERA), which)):
        alb, nd, _ = s.render_aov(AW, AH, ASPP, tile=ATILE, sample0=AS0, seed=SEED)
        _same(alb, want_a, "albedo_cov")
        _same(nd, want_n, "normal_depth")
        assert (_bits(nd[..., 3]) != _bits(pin_n[..., 3])).any(), "the depth is measured from the lens point"
        if route.name != "lds fused":
            return
        x0, y0, w, h = ATILE
        a2, n2 = np.zeros_like(alb), np.zeros_like(nd)
        for (tx, tw) in ((x0, 13), (x0 + 13, w - 13)):     # two tiles, each in two adjacent sample ranges
            a, n, _ = s.render_aov(AW, AH, 1, tile=(tx, y0, tw, h), sample0=AS0, seed=SEED)
            a, n, _ = s.render_aov(AW, AH, ASPP - 1, tile=(tx, y0, tw, h), sample0=AS0 + 1, seed=SEED, albedo=a, normal_depth=n)
            a2[:, tx - x0:tx - x0 + tw], n2[:, tx - x0:tx - x0 + tw] = a, n
        _same(a2, alb, "tiles and sample ranges: albedo_cov"), _same(n2, nd, "tiles and sample ranges: normal_depth")
        parts = [s.render_aov(AW, AH, ASPP, tile=ATILE, sample0=AS0, seed=SEED, shard=(k, 3, 8))[:2] for k in range(3)]
        _same(parts[0][0] + parts[1][0] + parts[2][0], alb, "shards: albedo_cov")
        _same(parts[0][1] + parts[1][1] + parts[2][1], nd, "shards: normal_depth")


# ---------------------------------------------------------------------------- 7. per-sample radiance through the proxy
RW, RH, RSPP, RB = 24, 16, 2, 4
_rad_refs = {}


def _rad_ref(ptx, ora, name, s, which, lights):
    key = (name, which, lights)
    if key not in _rad_refs:
        proxy, a = _proxy(ptx, ora, name, s, _lens(ora, name, s.array(ptx.ARR_CAMERA), which))
        _rad_refs[key] = render_samples(ora, proxy, a, RW, RH, RSPP, RB, seed=SEED, lights=lights)["rad"]
    return _rad_refs[key]


def _samples(call):
    out = np.zeros((RH, RW, RSPP, 3), f32)
    for k in range(RSPP):
        out[:, :, k] = call(k)[0][..., :3]
    return out


def _cornell_routes():
    return [("cornell", r, 0) for r in forced_routes(12)]


RAD_CASES = _cornell_routes() + [("plaza", DEFAULT_ROUTES[0], 1), ("lit", route_named(forced_routes(10), "lds fused"), 1), ("atrium", DEFAULT_ROUTES[1], 0)]


@pytest.mark.parametrize("name,route,which", RAD_CASES, ids=[f"{n}-{r.name.replace(' ', '_')}-lens{w}" for n, r, w in RAD_CASES])
def test_per_sample_radiance_with_a_lens(ptx, ctx, ora, clean_env, name, route, which):
    """test_gpu_parity's bar: every sample finite and >= 0, >= 99.5 % within 1e-3 relative (floor 1e-3), for ptx_render (the restatement
    without light samples) and the unfused ptx_render_nee."""
    s = on_route(SCENES, ptx, ctx, clean_env, name, route, resident_ok=lambda r, res: (res == 0) == r.force_global)
    with lens_on(s, _lens(ora, name, s.array(ptx.ARR_CAMERA), which)):
        for what, lights, call in (("ptx_render", False, lambda k: s.render(RW, RH, 1, RB, seed=SEED, sample0=k)),
                                   ("ptx_render_nee", True, lambda k: s.render_nee(RW, RH, 1, RB, seed=SEED, sample0=k))):
            got = _samples(call)
            assert ctx.timing()["pipeline"] == route.pipeline, (name, route.name, what)
            ref = _rad_ref(ptx, ora, name, s, which, lights)
            assert np.isfinite(got).all() and (got >= 0).all()
            e = _err(got, ref)
            share = (e <= 1e-3).mean()
            print(f"{name} / {route.name} / {what}: {share * 100:.3f} % of samples within 1e-3, worst {e.max():.3g}")
            assert share >= 0.995, (name, route.name, what, share)


# ---------------------------------------------------------------------------- 8. the product against itself, with a lens
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
    return budget


def _routed(ptx, ctx, mp, name, route, make=_make):
    """a scene of its own for the route ("lds fused", "hybrid", "global fused", "queue"), the route's switches set -> (scene, pipeline)"""
    for k in ROUTE_VARS:
        mp.delenv(k, raising=False)
    if route == "hybrid":
        _hybrid(ptx, ctx, mp, name)
        s = make(ptx, ctx, name)
        mp.delenv("PTX_LDS_BUDGET")
        mp.setenv("PTX_WAVEFRONT", "0")
        assert s.info()["lds_resident"] == 2, s.info()
        return s, 0
    r = route_named(forced_routes(1), route)
    s = under_force_global(mp, r.force_global, lambda: make(ptx, ctx, name))
    use_route(mp, r)
    assert (s.info()["lds_resident"] == 0) == r.force_global, s.info()
    return s, r.pipeline


@pytest.mark.parametrize("name,route,which,flags", [("cornell", "lds fused", 0, 0), ("cloud", "hybrid", 1, 0), ("plaza", "global fused", 1, 0), ("cornell", "lds fused", 1, -1)])
def test_fused_nee_with_a_lens_is_the_unflagged_call(ptx, ctx, ora, clean_env, name, route, which, flags):
    if flags < 0:
        flags = ptx.NEE_CANDIDATES(4) | ptx.NEE_SAMPLER_PDF
    s, _ = _routed(ptx, ctx, clean_env, name, route)
    with lens_on(s, _lens(ora, name, s.array(ptx.ARR_CAMERA), which)):
        want, st0 = s.render_nee(40, 28, 4, 4, seed=SEED, flags=flags)
        assert ctx.timing()["fused_launches"] == 0
        got, st = s.render_nee(40, 28, 4, 4, seed=SEED, flags=flags | ptx.NEE_FUSED)
        tm = ctx.timing()
        assert tm["pipeline"] == 0 and tm["fused_launches"] == st["passes"] > 0, tm
        _same(got, want, f"{name} / {route}")
        assert st["rays"] == st0["rays"] and st["light_samples"] == st0["light_samples"]
    pin, _ = s.render_nee(40, 28, 4, 4, seed=SEED, flags=flags)
    assert (_bits(pin) != _bits(want)).any()
    s.close()


def test_transparent_and_adaptive_compose_with_a_lens(ptx, ctx, ora, clean_env):
    s = SCENES.get(ptx, ctx, clean_env, "plaza")
    W, H, b = 40, 28, 3
    with lens_on(s, _lens(ora, "plaza", s.array(ptx.ARR_CAMERA), 1)):
        whole, claimed, _ = s.render_transparent(W, H, 4, b, seed=SEED)
        px, cl, _ = s.render_transparent(W, H, 1, b, seed=SEED)
        px, cl, _ = s.render_transparent(W, H, 3, b, seed=SEED, sample0=1, pixels=px, claimed=cl)
        _same(px, whole, "ptx_render_transparent over two ascending sample ranges")
        np.testing.assert_array_equal(cl, claimed)
    c = SCENES.get(ptx, ctx, clean_env, "cornell")
    with lens_on(c, _lens(ora, "cornell", c.array(ptx.ARR_CAMERA), 0)):
        # the product's own ptx_render_nee of the rounds' half ranges, snapshotted per round, and the restated decision replayed on them
        cap, mn, step, thr = 16, 8, 8, 0.1
        a, bb, st = c.render_adaptive_nee(W, H, cap, b, mn, step, thr, seed=SEED)
        sa, sb, snaps, given = np.zeros_like(a), np.zeros_like(bb), [], 0
        for k in AR.round_sizes(cap, mn, step):
            c.render_nee(W, H, k // 2, b, accum=sa, seed=SEED, sample0=given, want_stats=False)
            c.render_nee(W, H, k // 2, b, accum=sb, seed=SEED, sample0=given + k // 2, want_stats=False)
            given += k
            snaps.append((sa.copy(), sb.copy()))
        wa, wb, rounds, _ = AR.replay(snaps, thr)
        _same(a, wa, "ptx_render_adaptive_nee: first halves"), _same(bb, wb, "ptx_render_adaptive_nee: second halves")
        assert st["rounds"] == rounds


# ---------------------------------------------------------------------------- 9. nothing moves without a lens
@pytest.mark.parametrize("name", ["cornell", "plaza"])
def test_nothing_moves_without_a_lens(ptx, ctx, clean_env, name):
    W, H = 40, 28

    def frames(s):
        return (s.render(W, H, 3, 4, seed=SEED)[0], *s.render_aov(W, H, 3, seed=SEED)[:2], s.render_nee(W, H, 3, 4, seed=SEED, flags=ptx.NEE_FUSED)[0])
    want = frames(SCENES.get(ptx, ctx, clean_env, name))      # a scene on which no test sets anything but through lens_on
    fresh = _make(ptx, ctx, name)
    for got, ref in zip(frames(fresh), want):
        _same(got, ref, "a scene never touched")
    c = fresh.camera()
    fresh.set_camera(c["origin"], c["basis"], c["yfov"], c["lens_radius"], c["focus_distance"], c["blades"], c["blade_rotation"])
    for got, ref in zip(frames(fresh), want):
        _same(got, ref, "after set_camera(get_camera())")
    fresh.set_camera(c["origin"], c["basis"], c["yfov"], 0.0, 123.0, 7, 1.5)
    for got, ref in zip(frames(fresh), want):
        _same(got, ref, "after set_camera with lens_radius 0 and other lens fields arbitrary")
    with lens_on(fresh, (0.3, 4.0, 5, 0.2)):
        assert (_bits(frames(fresh)[0]) != _bits(want[0])).any()
    for got, ref in zip(frames(fresh), want):
        _same(got, ref, "after the lens was taken off again")
    fresh.close()


# ---------------------------------------------------------------------------- 10. a moved pinhole camera
def test_a_moved_pinhole_camera_is_a_scene_created_with_that_pose(ptx, ctx, clean_env):
    d = _dict("plaza")
    pose = np.concatenate([_proc()._look_at([-3.0, 2.0, 7.0], [0.2, 0.8, 0.0]), [f32(0.9)]]).astype(f32)
    a = product_from_dict(ptx, ctx, d)
    a.render(32, 20, 1, 2, seed=SEED)
    a.set_camera(pose[:3], pose[3:12], pose[12])
    b = product_from_dict(ptx, ctx, dict(d, camera=pose))
    _same(a.array(ptx.ARR_CAMERA), b.array(ptx.ARR_CAMERA), "ARR_CAMERA")
    _same(a.render(40, 28, 3, 4, seed=SEED)[0], b.render(40, 28, 3, 4, seed=SEED)[0], "ptx_render")
    for x, y in zip(a.render_aov(40, 28, 3, seed=SEED)[:2], b.render_aov(40, 28, 3, seed=SEED)[:2]):
        _same(x, y, "ptx_render_aov")
    a.close(), b.close()


# ---------------------------------------------------------------------------- 11. depth of field does what it says
def _two_quads(d1, d2, half1, fov):
    v = np.zeros((8, 11), f32)
    for q, (z, hs) in enumerate(((-d1, half1), (-d2, 40.0))):
        v[4 * q:4 * q + 4, :3] = [[-hs, -hs, z], [hs, -hs, z], [hs, hs, z], [-hs, hs, z]]     # counter-clockwise seen from +z, where the camera is
        v[4 * q:4 * q + 4, 3:5] = [[0, 0], [1, 0], [1, 1], [0, 1]]
        v[4 * q:4 * q + 4, 7] = 1.0
        v[4 * q:4 * q + 4, 8] = 1.0
    mats = np.array([[1, 0, 0, 1, 0.5, 0, 0, 0, 0, 1.33, 0], [0, 0, 1, 1, 0.5, 0, 0, 0, 0, 1.33, 0]], f32)
    return dict(model_xform=np.array([[0, 0, 0, 1, 0, 0, 0, 1, 0, 0, 0, 1]], f32), model_surf=np.array([[0, 2]], np.int32),
                surf_range=np.array([[0, 4, 0, 2], [4, 4, 2, 2]], np.int32), vertices=v, triangles=np.array([[0, 1, 2], [0, 2, 3]] * 2, np.uint32),
                materials=mats, camera=np.array([0, 0, 0, 1, 0, 0, 0, 1, 0, 0, 0, 1, fov], f32), sun=None)


def _outside_distance(sil):
    """per pixel: Euclidean distance in pixels to the nearest pixel of the silhouette"""
    ys, xs = np.nonzero(sil)
    yy, xx = np.mgrid[:sil.shape[0], :sil.shape[1]]
    return np.sqrt(((yy[..., None] - ys) ** 2 + (xx[..., None] - xs) ** 2).min(-1))


def test_depth_of_field_does_what_it_says(ptx, ctx, clean_env):
    W, H, spp, d1, d2, fov, Rl = 64, 48, 32, 2.0, 6.0, 0.8, 0.3
    s = product_from_dict(ptx, ctx, _two_quads(d1, d2, 0.25, fov))
    tan = float(s.array(ptx.ARR_CAMERA)[13])
    radius = Rl * abs(d1 - d2) / d1 * (H / 2) / (tan * d2)          # of the circle of confusion of the first quad with F = d2, in pixels
    assert radius >= 4, radius

    def coverage():
        alb = s.render_aov(W, H, spp, seed=SEED)[0]
        assert (alb[..., 3] == spp).all()                              # every sample ends on one of the quads
        return alb[..., 0] / spp                                       # the first quad is the red one
    sil = coverage() > 0
    dist = _outside_distance(sil)
    assert 100 < sil.sum() < 400, sil.sum()
    c = s.camera()
    s.set_camera(c["origin"], c["basis"], c["yfov"], Rl, d1, 16, 0.0)
    sharp = coverage()
    s.set_camera(c["origin"], c["basis"], c["yfov"], Rl, d2, 16, 0.0)
    blurred = coverage()
    reach = dist[blurred > 0].max()
    print(f"circle of confusion {radius:.2f} px; in focus: coverage reaches {dist[sharp > 0].max():.2f} px outside the silhouette; focused behind: {reach:.2f} px")
    assert (sharp[dist > 1] == 0).all(), "in focus, the quad stays inside its pinhole silhouette"
    assert reach >= 0.5 * radius, (reach, radius)
    assert (blurred[dist > radius + 1.5] == 0).all(), "and no further than the circle of confusion"
    assert blurred[sil].min() < 1, "its edge is blurred inwards as well"
    s.close()


# ---------------------------------------------------------------------------- 12. model transforms on the device
XW, XH, XSPP, XB = 40, 28, 3, 4


def _frames(ptx, s, fused):
    out = {"ptx_render": s.render(XW, XH, XSPP, XB, seed=SEED)[0], "ptx_render_nee": s.render_nee(XW, XH, XSPP, XB, seed=SEED)[0]}
    out["aov albedo"], out["aov normal_depth"] = s.render_aov(XW, XH, XSPP, seed=SEED)[:2]
    if fused:
        out["ptx_render_nee fused"] = s.render_nee(XW, XH, XSPP, XB, seed=SEED, flags=ptx.NEE_FUSED)[0]
    return out


@pytest.mark.parametrize("route", ["lds fused", "hybrid", "global fused", "queue"])
def test_set_model_xforms_renders_as_a_fresh_scene(ptx, ctx, clean_env, route):
    """The emitter cloud: four models of sixteen surfaces, emitters among them, so the light list moves with the models."""
    d = _dict("cloud")
    moved = moved_xforms(d["model_xform"])
    a, pipeline = _routed(ptx, ctx, clean_env, "cloud", route)
    before = _frames(ptx, a, pipeline == 0)
    geom_before = a.array(ptx.ARR_LIGHT_GEOM)
    assert len(geom_before) > 0
    if route == "global fused" or route == "queue":
        clean_env.setenv("PTX_FORCE_GLOBAL", "1")      # the residency choice is made again at every upload
    a.set_model_xforms(moved)
    clean_env.delenv("PTX_FORCE_GLOBAL", raising=False)
    env_now = {k: os.environ.get(k) for k in ROUTE_VARS}
    b, _ = _routed(ptx, ctx, clean_env, "cloud", route, make=lambda ptx_, ctx_, name: product_from_dict(ptx_, ctx_, dict(d, model_xform=moved)))
    assert {k: os.environ.get(k) for k in ROUTE_VARS} == env_now
    assert a.info() == b.info()
    _same(a.array(ptx.ARR_LIGHT_GEOM), b.array(ptx.ARR_LIGHT_GEOM), "ARR_LIGHT_GEOM after the move")
    assert (_bits(a.array(ptx.ARR_LIGHT_GEOM)) != _bits(geom_before)).any()
    got, want = _frames(ptx, a, pipeline == 0), _frames(ptx, b, pipeline == 0)
    assert ctx.timing()["pipeline"] == pipeline
    for k in want:
        _same(got[k], want[k], f"{route}: {k}")
        assert (_bits(got[k]) != _bits(before[k])).any(), k
    a.close(), b.close()


def test_a_render_before_and_after_set_model_xforms_with_stats(ptx, ctx, clean_env):
    d = _dict("plaza")
    moved = moved_xforms(d["model_xform"], share=False)
    a = product_from_dict(ptx, ctx, d)
    first, st0 = a.render(XW, XH, XSPP, XB, seed=SEED, want_stats=True)
    a.set_model_xforms(moved)
    second, st1 = a.render(XW, XH, XSPP, XB, seed=SEED, want_stats=True)
    b = product_from_dict(ptx, ctx, dict(d, model_xform=moved))
    want, st = b.render(XW, XH, XSPP, XB, seed=SEED, want_stats=True)
    _same(second, want, "the render after the call")
    assert st1["rays"] == st["rays"] and st1["samples"] == st["samples"] and st0["samples"] == st["samples"]
    assert (_bits(first) != _bits(second)).any()
    a.set_model_xforms(d["model_xform"])
    _same(a.render(XW, XH, XSPP, XB, seed=SEED)[0], first, "and moved back")
    a.close(), b.close()


def test_cornell_from_gltf_with_its_models_moved(ptx, ctx, ora, clean_env):
    import copy
    arrays = ora.load_gltf(CORNELL)
    x = np.asarray(arrays.model_xform, f32).copy()
    x[-1, 0:3] += f32(0.25) * np.array([1, 0.5, -1], f32)        # the sphere moves, the tall box turns and stretches
    x[-2] = moved_xforms(x[-2:-1], share=False)[0]
    a2 = copy.copy(arrays)
    a2.model_xform = x
    ref = ora.OracleScene(a2).render_samples(ora.make_cfg(RW, RH, RSPP, RB, seed=SEED), threads=0)
    s = ptx.Scene.load_gltf(ctx, CORNELL)
    s.set_model_xforms(x)
    got = _samples(lambda k: s.render(RW, RH, 1, RB, seed=SEED, sample0=k))
    untouched = ora.OracleScene(arrays).render_samples(ora.make_cfg(RW, RH, RSPP, RB, seed=SEED), threads=0)
    e = _err(got, ref)
    share = (e <= 1e-3).mean()
    print(f"moved Cornell: {share * 100:.3f} % of samples within 1e-3, worst {e.max():.3g}; {(_err(untouched, ref) > 1e-3).mean() * 100:.1f} % of the untouched scene's differ")
    assert np.isfinite(got).all() and share >= 0.995
    assert (_err(untouched, ref) > 1e-3).mean() > 0.02
    s.close()


# ---------------------------------------------------------------------------- 13. mirrors and CLI
def test_mirrors_and_cli_give_the_c_calls_frame(ptx, ctx, ora, clean_env, tmp_path):
    from PIL import Image
    W, H, spp, b = 48, 27, 8, 3
    lens = (0.05, 3.5, 6, 0.3)
    s = SCENES.get(ptx, ctx, clean_env, "cornell")
    with lens_on(s, lens):
        want, _ = s.render(W, H, spp, b, seed=SEED)
        want_nee, _ = s.render_nee(W, H, spp, b, seed=SEED)
    r = ptx.Renderer(0)
    r.resolution, r.sample_count, r.bounce_count, r.seed = (W, H), spp, b, SEED
    r.load_gltf(CORNELL)
    pin = r.render_accum()
    r.lens_radius, r.focus_distance, r.blades, r.blade_rotation = lens
    _same(r.render_accum(), want, "Renderer fields: render_accum")
    _same(r.render_nee(), want_nee, "Renderer fields: render_nee")
    r.lens_radius = 0.0
    _same(r.render_accum(), pin, "Renderer: the lens taken off")
    cli = os.path.join(ROOT, "distributed-path-tracer_amd", "ptx_render_cli")
    size = [str(W), str(H), str(spp), str(b)]
    out = subprocess.run([cli, "--lens", "0.05:3.5:6:0.3", CORNELL, str(tmp_path / "f.png"), *size], capture_output=True, text=True, timeout=120)
    assert out.returncode == 0, out.stderr
    np.testing.assert_array_equal(np.array(Image.open(tmp_path / "f.png")), ctx.tonemap_encode(want, W, H, spp))
    out = subprocess.run([cli, "--lens", "0.05:3.5", "--nee-fused", "--adaptive", "0.1:4:4", "--denoise", CORNELL, str(tmp_path / "g.png"), *size],
                         capture_output=True, text=True, timeout=120)
    assert out.returncode == 0, out.stderr
    js = json.loads(out.stdout)
    assert js["W"] == W and js["adaptive_rounds"] >= 1
    img = np.array(Image.open(tmp_path / "g.png"))
    assert img.shape == (H, W, 4) and img[..., :3].any() and (img[..., 3] == 255).all()
    for bad in ("0.05", "0:3", "0.05:-1", "0.05:3:2", "0.05:3:40", "x", "0.05:3:6:0.1:9"):
        out = subprocess.run([cli, "--lens", bad, CORNELL, str(tmp_path / "h.png"), *size], capture_output=True, text=True, timeout=120)
        assert out.returncode != 0 and "--lens" in out.stderr, bad
    assert not (tmp_path / "h.png").exists()
