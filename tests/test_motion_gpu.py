"""ptx_render_motion on the GPU, bit for bit against its restatement from the oracle (tests/_motion_restatement.py; tests/test_temporal.py
shows on the CPU that the restatement means what it says): every intersect route, a static scene, a moved camera, moved models with one
left in place, a lens, opacity pass-throughs (the plaza's half-transparent sphere, Jack's alpha textures), and the compositions the guide
buffers have — tiles, adjacent sample ranges, spp_per_pass, shards, host and device buffers.
"""
import numpy as np
import pytest

from _aov_restatement import H, S0, SEED, SPP, TILE, W
from _camera_restatement import Camera, LensOracle
from _common import _bits, _proc, _same
from _motion_restatement import Pose, restate
from _routes import DEFAULT_ROUTES, Route, Scenes, assert_route, clean_env, ctx, on_route, use_route  # noqa: F401  (clean_env and ctx are fixtures)
from conftest import JACK, oracle_from_dict, product_from_dict

f32 = np.float32
pytestmark = pytest.mark.gpu
ORBIT = 0.02
LENS = (0.05, 9.0, 6, 0.0)


def orbit(cam13, angle, centre=(0.0, 0.0, 0.0)):
    cam = np.asarray(cam13, np.float64).reshape(-1)[:13].copy()
    c, R = np.asarray(centre, np.float64), np.array([[np.cos(angle), 0, np.sin(angle)], [0, 1, 0], [-np.sin(angle), 0, np.cos(angle)]])
    cam[0:3] = c + R @ (cam[0:3] - c)
    cam[3:12] = (R @ cam[3:12].reshape(3, 3).T).T.reshape(-1)
    return cam.astype(f32)


def _plaza():
    return _proc().plaza_scene(level=2)


def _make(ptx, ctx, name):
    return ptx.Scene.load_gltf(ctx, JACK) if name == "jack" else product_from_dict(ptx, ctx, _plaza())


SCENES = Scenes(_make)
_kept = {}


def _cam_dict(cam13):
    return dict(origin=cam13[0:3], basis=cam13[3:12], yfov=cam13[12])


def _pose(ptx, cam13):
    """a camera with the host's tan_half_fov: what a host-only scene created with it stores"""
    key = ("pose", tuple(np.asarray(cam13, f32)[:13].tolist()))
    if key not in _kept:
        d = dict(_plaza(), camera=np.asarray(cam13, f32)[:13])
        _kept[key] = Pose.of(product_from_dict(ptx, None, d).array(ptx.ARR_CAMERA))
    return _kept[key]


def _prev_xform(xf):
    """every model but model 0 was elsewhere one frame ago"""
    out = np.asarray(xf, f32).reshape(-1, 12).copy()
    for m in range(1, len(out)):
        out[m, 0:3] += np.array([0.04 * m, 0.01, -0.03], f32)
        out[m, 3:12] *= f32(1.0 + 0.01 * m)
    return out


def _case(ptx, ora, case, **shape):
    """-> (kwargs of Scene.render_motion, lens or None, the restatement), computed once per case and shape"""
    key = (case, tuple(sorted(shape.items())))
    if key not in _kept:
        d = _plaza()
        o = oracle_from_dict(ora, d)
        cam = np.asarray(d["camera"], f32)[:13]
        cur = _pose(ptx, cam)
        kw, lens, rkw = {}, None, {}
        if case in ("camera", "both", "lens"):
            prev_cam = orbit(cam, ORBIT)
            kw["prev_camera"], rkw["prev_pose"] = _cam_dict(prev_cam), _pose(ptx, prev_cam)
        if case in ("models", "both"):
            kw["prev_model_xform"] = rkw["prev_xform"] = _prev_xform(d["model_xform"])
        if case == "lens":
            lens = LENS
            cam14 = np.concatenate([cam, [cur.tan]]).astype(f32)
            o = LensOracle(ora, o, Camera(cam14, *lens))
        mot, counts = restate(ora, o, cur_pose=cur, **rkw, **shape)
        mot.setflags(write=False)
        _kept[key] = (kw, lens, mot, counts)
    return _kept[key]


def _motion(s, kw, **over):
    args = dict(tile=TILE, sample0=S0, seed=SEED)
    args.update(kw)
    args.update(over)
    return s.render_motion(W, H, args.pop("spp", SPP), **args)


@pytest.mark.parametrize("case", ["static", "camera", "models", "both", "lens"])
@pytest.mark.parametrize("route", DEFAULT_ROUTES, ids=[r.name.replace(" ", "_") for r in DEFAULT_ROUTES])
def test_plaza_bitwise_on_every_route(ptx, ctx, ora, clean_env, route, case):
    kw, lens, want, counts = _case(ptx, ora, case)
    s = on_route(SCENES, ptx, ctx, clean_env, "plaza", route)
    assert_route(ctx, s, route, f"plaza {route.name}")
    c = s.camera()
    if lens:
        s.set_camera(c["origin"], c["basis"], c["yfov"], *lens)
    try:
        mot, st = _motion(s, kw)
    finally:
        if lens:
            s.set_camera(c["origin"], c["basis"], c["yfov"])
    _same(mot, want, f"{case} on {route.name}")
    assert counts["surface"] > 5000 and st["samples"] == SPP * TILE[2] * TILE[3] and st["rays"] > st["samples"]   # pass-throughs add rays
    if case == "static":
        assert (mot[..., :2] == 0).all()
    else:
        assert (mot[..., :2] != 0).any()
    if case in ("models", "both"):
        assert 0 < counts["moved"] < counts["surface"]
    if case == "models":   # a static camera: the pixels of the model left in place do not move
        assert ((mot[..., :2] == 0).all(-1) & (mot[..., 3] > 0)).sum() > 1000
    alb, _, _ = s.render_aov(W, H, SPP, tile=TILE, sample0=S0, seed=SEED)
    if not lens:
        np.testing.assert_array_equal(mot[..., 3], alb[..., 3])   # every surface sample is in front of both cameras


HYBRID = [Route("jack", False, {}, 2, 1), Route("jack", False, {"PTX_WAVEFRONT": "0"}, 2, 0)]


@pytest.mark.parametrize("route", HYBRID, ids=["queue", "fused"])
def test_jack_hybrid_routes_bitwise(ptx, ctx, ora, jack_oracle, clean_env, route):
    """Textures, alpha textures and the hybrid residency, on both of its routes; the camera turned about Jack."""
    shape = dict(W_=48, H_=27, tile=(6, 4, 33, 17), sample0=S0, spp=2)
    s = SCENES.get(ptx, ctx, clean_env, "jack")
    use_route(clean_env, route)
    assert_route(ctx, s, route, f"jack {route.name}")
    cam14 = s.array(ptx.ARR_CAMERA).reshape(-1)
    if "jack" not in _kept:
        prev_cam = orbit(cam14, ORBIT)
        host = ptx.Scene.load_gltf(None, JACK)
        host.set_camera(prev_cam[0:3], prev_cam[3:12], prev_cam[12])
        _kept["jack"] = (prev_cam, restate(ora, jack_oracle, prev_pose=Pose.of(host.array(ptx.ARR_CAMERA)), cur_pose=Pose.of(cam14), **shape))
    prev_cam, (want, counts) = _kept["jack"]
    mot, _ = s.render_motion(48, 27, 2, prev_camera=_cam_dict(prev_cam), tile=shape["tile"], sample0=S0, seed=SEED)
    _same(mot, want, f"jack {route.name}")
    assert counts["surface"] > 100 and (mot[..., :2] != 0).any()


def test_tiles_sample_ranges_passes_shards_and_buffer_kinds_compose(ptx, ctx, ora, clean_env):
    import torch
    kw, _, want, _ = _case(ptx, ora, "both")
    s = on_route(SCENES, ptx, ctx, clean_env, "plaza", DEFAULT_ROUTES[0])
    x0, y0, w, h = TILE
    whole, st = _motion(s, kw, spp_per_pass=2)
    _same(whole, want, "spp_per_pass = 2")
    assert st["passes"] == 3
    built = np.zeros_like(whole)
    for (tx, tw) in ((x0, 29), (x0 + 29, w - 29)):     # two tiles, each in two adjacent sample ranges
        m, _ = _motion(s, kw, tile=(tx, y0, tw, h), spp=2)
        m, _ = _motion(s, kw, tile=(tx, y0, tw, h), spp=SPP - 2, sample0=S0 + 2, motion=m)
        built[:, tx - x0:tx - x0 + tw] = m
    _same(built, want, "tiles and adjacent sample ranges")
    for n in (2, 3):
        parts = [_motion(s, kw, shard=(k, n, 8))[0] for k in range(n)]
        assert all(p.any() for p in parts)
        _same(sum(parts[1:], parts[0]), want, f"{n} shards")
    dev = torch.zeros((h, w, 4), dtype=torch.float32, device="cuda:0")
    out, _ = _motion(s, kw, motion=dev, want_stats=False)
    ctx.synchronize()
    assert out is dev
    _same(dev.cpu().numpy(), want, "device buffer")
    base = np.full((h, w, 4), 0.5, f32)
    added, _ = _motion(s, kw, motion=base.copy())
    assert (added[..., 3] == f32(0.5) + want[..., 3]).all()   # sums, added to what the caller passes in


def test_a_scene_moved_by_the_setters_is_a_scene_created_moved(ptx, ctx, ora, clean_env):
    """Frame t reached by ptx_scene_set_camera and ptx_scene_set_model_xforms from frame t - 1, against a scene created from frame t's
    arrays: the same motion against frame t - 1, bit for bit, and the restatement's."""
    d = _plaza()
    cam_prev = np.asarray(d["camera"], f32)[:13]
    xf_prev = np.ascontiguousarray(d["model_xform"], f32)
    cam_now, xf_now = orbit(cam_prev, -ORBIT), _prev_xform(xf_prev)
    d_now = dict(d, camera=cam_now, model_xform=xf_now)
    fresh = product_from_dict(ptx, ctx, d_now)
    moved = product_from_dict(ptx, ctx, d)
    moved.set_camera(cam_now[0:3], cam_now[3:12], cam_now[12])
    moved.set_model_xforms(xf_now)
    kw = dict(prev_camera=_cam_dict(cam_prev), prev_model_xform=xf_prev)
    a, _ = _motion(fresh, kw)
    b, _ = _motion(moved, kw)
    _same(b, a, "setters against a fresh scene")
    want, counts = restate(ora, oracle_from_dict(ora, d_now), prev_pose=_pose(ptx, cam_prev), prev_xform=xf_prev, cur_pose=_pose(ptx, cam_now))
    _same(a, want, "the restatement of the moved scene")
    assert counts["moved"] > 0 and (_bits(a[..., :2]) != 0).any()
