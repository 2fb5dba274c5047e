"""Moving a loaded scene, host side (no GPU): the restated camera against the oracle, the lens restatement's own properties, the camera
setter and the aperture table, and ptx_scene_set_model_xforms against a scene created from the moved arrays. Host-only scenes throughout."""
import numpy as np
import pytest

from _camera_restatement import Camera, aperture_table, moved_xforms
from _common import _proc, _same
from conftest import CORNELL, oracle_from_dict, product_from_dict

f32 = np.float32
N_ARRAYS = 31   # ptx_array values 0 .. 30


def _dict_of(ptx, s):
    return {k: s.array(getattr(ptx, "ARR_" + k.upper())) for k in ("model_xform", "model_surf", "surf_range", "vertices", "triangles", "materials", "camera")}


# ---------------------------------------------------------------------------- 1. the pinhole restatement is the oracle's camera
@pytest.mark.parametrize("name", ["cornell", "plaza"])
def test_restated_pinhole_is_the_oracles_primary_rays(ptx, ora, cornell_oracle, name):
    """Full 32 x 18 frame, samples 0 and 1, bit for bit; tan_half_fov comes from ARR_CAMERA [13], and numpy's tan of the float32 fov is
    printed against it (the pitfall the restatement avoids)."""
    if name == "cornell":
        o, s = cornell_oracle, ptx.Scene.load_gltf(None, CORNELL)
    else:
        d = _proc().plaza_scene(level=1)
        o, s = oracle_from_dict(ora, d), product_from_dict(ptx, None, d)
    cam14 = s.array(ptx.ARR_CAMERA)
    print(f"{name}: tan_half_fov {cam14[13]!r}, numpy float32 tan {np.tan(f32(cam14[12]) * f32(0.5))!r}")
    cam = Camera(cam14)
    for sample in (0, 1):
        cfg = ora.make_cfg(32, 18, 1, 1)
        _same(cam.primary_rays(ora, cfg, sample), o.primary_rays(cfg, sample), f"{name} sample {sample}")
    for ig in (0, 1):   # the worker's un-jittered sample 0
        cfg = ora.make_cfg(32, 18, 1, 1, integrator=ig)
        _same(cam.primary_rays(ora, cfg, 0), o.primary_rays(cfg, 0), f"{name} integrator {ig}")


# ---------------------------------------------------------------------------- 2. properties of the lens restatement
@pytest.mark.parametrize("n", [3, 6, 16])
@pytest.mark.parametrize("R,F,tan", [(0.05, 3.0, 0.4), (0.5, 1.0, 1.0), (2.0, 0.5, 1.2)])
def test_lens_restatement_properties(R, F, tan, n):
    rng = np.random.default_rng(1000 * n + int(100 * R))
    N = 100000
    cam14 = np.array([0, 0, 0, 1, 0, 0, 0, 1, 0, 0, 0, 1, 0, tan], f32)
    cam = Camera(cam14, R, F, n, 0.3)
    ndc = rng.uniform(-1, 1, (N, 2)).astype(f32)
    ratio = rng.uniform(0.5, 2.5, N).astype(f32)
    uv = rng.random((N, 2), dtype=f32)
    pf, lp, dl = cam.lens_parts(ndc[:, 0], ndc[:, 1], ratio, uv[:, 0], uv[:, 1])
    # every ray passes pf: distance of pf from the line lp + s dl, in float64 on the float32 results
    P, Lp, D = pf.astype(np.float64), lp.astype(np.float64), dl.astype(np.float64)
    w = P - Lp
    dist = np.linalg.norm(w - (w * D).sum(-1, keepdims=True) * D / (D * D).sum(-1, keepdims=True), axis=-1)
    rel = dist / np.linalg.norm(w, axis=-1)
    dlen = np.abs(np.linalg.norm(D, axis=-1) - 1)
    r2 = (Lp * Lp).sum(-1) / float(f32(R)) ** 2
    want = (2 + np.cos(2 * np.pi / n)) / 6
    print(f"R {R} F {F} tan {tan} n {n}: miss of pf {rel.max():.3g} of |pf - lp|, | |d| - 1 | {dlen.max():.3g}, mean |lp|^2 / R^2 {r2.mean():.5f} (want {want:.5f}), max |lp| / R {np.sqrt(r2.max()):.7f}")
    assert rel.max() <= 1e-6
    assert dlen.max() <= 4e-7
    assert abs(r2.mean() / want - 1) <= 0.01
    assert np.all(np.linalg.norm(lp.astype(np.float64), axis=-1) <= float(f32(R)))
    assert np.all(lp[:, 2] == 0)


# ---------------------------------------------------------------------------- 3. the setter, the getter, the table
def _cam_state(ptx, s):
    c = s.camera()
    return (s.array(ptx.ARR_CAMERA).tobytes(), s.array(ptx.ARR_LENS).tobytes(), c["origin"].tobytes(), c["basis"].tobytes(),
            c["yfov"].tobytes(), c["lens_radius"].tobytes(), c["focus_distance"].tobytes(), c["blades"], c["blade_rotation"].tobytes())


def test_set_camera_round_trip_and_table(ptx, ora):
    s = ptx.Scene.load_gltf(None, CORNELL)
    cam14 = s.array(ptx.ARR_CAMERA)
    c = s.camera()
    _same(np.concatenate([c["origin"], c["basis"], [c["yfov"]]]), cam14[:13], "get_camera of a loaded scene")
    assert c["lens_radius"] == 0 and c["focus_distance"] == 0 and c["blades"] == 0 and c["blade_rotation"] == 0
    assert s.array(ptx.ARR_LENS).shape == (0, 2)
    pose = _proc()._look_at([1.0, 2.0, 5.0], [0.0, 1.0, 0.0])
    for blades, rot in ((3, 0.0), (16, 0.0), (32, 0.0), (6, 0.7), (0, -1.1)):
        s.set_camera(pose[:3], pose[3:12], 0.9, 0.25, 3.5, blades, rot)
        c = s.camera()
        _same(c["origin"], pose[:3], "origin"); _same(c["basis"], pose[3:12], "basis")
        assert c["yfov"] == f32(0.9) and c["lens_radius"] == f32(0.25) and c["focus_distance"] == f32(3.5) and c["blade_rotation"] == f32(rot)
        n = blades or 16
        assert c["blades"] == n
        got14 = s.array(ptx.ARR_CAMERA)
        _same(got14[:13], np.concatenate([pose, [f32(0.9)]]), "ARR_CAMERA")
        assert got14[13] == f32(ora.lib().ora_tan_half_fov(ora.C.c_float(0.9)))   # std::tan(yfov * 0.5F), as at creation
        t = s.array(ptx.ARR_LENS)
        assert t.shape == (n + 1, 2)
        _same(t, aperture_table(0.25, n, rot), f"aperture table n {n} rot {rot}")
        _same(t[n], t[0], "the last entry is the first")
    # radius 0: the table is empty and the lens fields are stored as zeros, whatever they held
    s.set_camera(pose[:3], pose[3:12], 0.9, 0.0, -7.0, 5, 2.0)
    c = s.camera()
    assert s.array(ptx.ARR_LENS).shape == (0, 2)
    assert c["lens_radius"] == 0 and c["focus_distance"] == 0 and c["blades"] == 0 and c["blade_rotation"] == 0


def test_set_camera_refusals_leave_the_camera(ptx):
    s = ptx.Scene.load_gltf(None, CORNELL)
    pose = _proc()._look_at([1.0, 2.0, 5.0], [0.0, 1.0, 0.0])
    s.set_camera(pose[:3], pose[3:12], 0.9, 0.25, 3.5, 6, 0.7)
    before = _cam_state(ptx, s)
    o, b = pose[:3], pose[3:12]
    nan_o, inf_b = o.copy(), b.copy()
    nan_o[1], inf_b[4] = np.nan, np.inf
    bad = [dict(origin=nan_o), dict(basis=inf_b), dict(yfov=np.nan), dict(yfov=0.0), dict(yfov=-0.5), dict(yfov=float(np.pi)), dict(yfov=4.0),
           dict(lens_radius=-0.1), dict(lens_radius=np.inf), dict(lens_radius=0.1, focus_distance=0.0), dict(lens_radius=0.1, focus_distance=-1.0),
           dict(focus_distance=np.nan), dict(blades=1), dict(blades=2), dict(blades=33), dict(blade_rotation=np.nan), dict(blade_rotation=np.inf)]
    for kw in bad:
        args = dict(origin=o, basis=b, yfov=0.9, lens_radius=0.25, focus_distance=3.5, blades=6, blade_rotation=0.7)
        args.update(kw)
        with pytest.raises(ptx.PtxError) as e:
            s.set_camera(**args)
        assert e.value.code == ptx.ERR_INVALID, kw
        assert _cam_state(ptx, s) == before, kw
    L = ptx.lib()
    cam = ptx.Camera()
    assert L.ptx_scene_set_camera(None, ptx.C.byref(cam)) == ptx.ERR_INVALID
    assert L.ptx_scene_set_camera(s.h, None) == ptx.ERR_INVALID
    assert L.ptx_scene_get_camera(None, ptx.C.byref(cam)) == ptx.ERR_INVALID
    assert L.ptx_scene_get_camera(s.h, None) == ptx.ERR_INVALID
    assert _cam_state(ptx, s) == before


# ---------------------------------------------------------------------------- 4. model transforms without a rebuild
def _scene_dicts(ptx):
    p = _proc()
    c = _dict_of(ptx, ptx.Scene.load_gltf(None, CORNELL))
    return {"emitter_cloud": p.emitter_cloud_scene(), "plaza": p.plaza_scene(level=2), "cornell_mesh": p.cornell_with_mesh(c, level=2)}


def _everything(ptx, s):
    return [np.asarray(s.array(a)).tobytes() if a != ptx.ARR_MODEL_NAMES else s.array(a) for a in range(N_ARRAYS)], s.info()


@pytest.mark.parametrize("name", ["emitter_cloud", "plaza", "cornell_mesh"])
def test_set_model_xforms_equals_a_fresh_scene(ptx, name):
    d = _scene_dicts(ptx)[name]
    a = product_from_dict(ptx, None, d)
    n_spaces_before = len({bytes(r) for r in np.asarray(d["model_xform"], f32)})
    a.array(ptx.ARR_LIGHT_GEOM)   # the list is built before the move: it must be dropped, not kept
    moved = moved_xforms(d["model_xform"])
    a.set_model_xforms(moved)
    b = product_from_dict(ptx, None, dict(d, model_xform=moved))
    arr_a, info_a = _everything(ptx, a)
    arr_b, info_b = _everything(ptx, b)
    for k in range(N_ARRAYS):
        assert arr_a[k] == arr_b[k], f"{name}: ptx_array {k} differs"
    assert info_a == info_b
    _same(a.array(ptx.ARR_MODEL_XFORM), moved, "the transforms as set")
    assert len({bytes(r) for r in moved}) != n_spaces_before or len(moved) == 1, "the move changes the count of distinct transforms"
    # refusals leave the scene unchanged
    L = ptx.lib()
    bad = moved.copy(); bad[0, 4] = np.nan
    for call in (lambda: a.set_model_xforms(moved[:-1]), lambda: a.set_model_xforms(np.concatenate([moved, moved[:1]])), lambda: a.set_model_xforms(bad)):
        with pytest.raises(ptx.PtxError) as e:
            call()
        assert e.value.code == ptx.ERR_INVALID
    assert L.ptx_scene_set_model_xforms(None, moved.ctypes.data, len(moved)) == ptx.ERR_INVALID
    assert L.ptx_scene_set_model_xforms(a.h, None, len(moved)) == ptx.ERR_INVALID
    again, info_again = _everything(ptx, a)
    assert again == arr_a and info_again == info_a
    # and back: the scene equals the one it was created as
    a.set_model_xforms(d["model_xform"])
    first, _ = _everything(ptx, product_from_dict(ptx, None, d))
    back, _ = _everything(ptx, a)
    assert back == first


def test_set_model_xforms_keeps_camera_and_punctual_lights(ptx):
    d = _proc().plaza_scene(level=1)
    s = product_from_dict(ptx, None, d)
    pose = _proc()._look_at([1.0, 2.0, 5.0], [0.0, 1.0, 0.0])
    s.set_camera(pose[:3], pose[3:12], 0.9, 0.25, 3.5, 6, 0.7)
    lamp = np.array([[0, 3, 0, 0, 0, -1, 0, 0, 5, 5, 5, 0, 0, 0, 0, 0]], f32)
    s.set_punctual_lights(lamp)
    before = _cam_state(ptx, s)
    s.set_model_xforms(moved_xforms(d["model_xform"]))
    assert _cam_state(ptx, s) == before
    _same(s.array(ptx.ARR_PUNCTUAL), lamp, "the punctual lights stay where they are")
