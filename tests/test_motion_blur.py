"""Motion blur without a GPU (include/ptx.h: MOTION): ptx_scene_set_motion on host-only scenes. The state at a time against the formula in
numpy float32, the three inspection arrays through a set, a clear and the two setters that end a motion, every refusal, the light list with
a moving emitter, the restated time of a sample, the mirror's signatures, and the procedural scene the GPU tests use."""
import inspect

import numpy as np
import pytest

from _common import _bits, _same
from _motion_common import BLOCK_TIME, begin_camera, movers, sample_time
from conftest import product_from_dict

f32 = np.float32
STATIC = [0, 1]               # movers_scene: the floor and the emissive quad
MOVING = [2, 3, 4, 5, 6, 7, 8]


def _scene(ptx, emissive=False):
    d = movers(emissive)
    return d, product_from_dict(ptx, None, d)


def _cam12(s):
    c = s.camera()
    return np.concatenate([c["origin"], c["basis"]]).astype(f32)


def test_movers_scene_is_what_the_tests_need():
    d = movers(True, True, True)
    assert len(d["surf_range"]) <= 64 and 200 <= len(d["triangles"]) <= 600
    a, b = d["begin_model_xform"], d["model_xform"]
    moved = (_bits(a) != _bits(b)).any(1)
    assert list(np.nonzero(~moved)[0]) == STATIC and moved.sum() == 8
    _same(b[5], b[6], "the pair that meets at u = 1")
    assert (_bits(a[5]) != _bits(a[6])).any()
    _same(a[7], a[8], "the pair equal in both keys")
    _same(b[7], b[8], "the pair equal in both keys")
    assert d["model_surf"][4, 1] == 2                                   # the two-surface model
    assert (_bits(b[1]) == 0x80000000).any()                            # -0.0 entries in a static transform
    assert d["materials"][-1, 6:9].max() > 0 and d["materials"][1, 6:9].max() > 0   # the moving and the static emitter
    assert d["materials"][5, 3] == f32(0.5) and d["sun"] is not None
    assert (_bits(d["begin_camera"][:12]) != _bits(d["camera"][:12])).any()
    assert movers()["sun"] is None and len(movers()["model_xform"]) == 9


def test_state_is_the_formula_in_float32(ptx):
    d, s = _scene(ptx)
    s.set_motion(d["begin_model_xform"], begin_camera(d), (0.0, 1.0))
    a, b = d["begin_model_xform"], d["model_xform"]
    ca, cb = d["begin_camera"][:12], d["camera"][:12]
    us = [0.0, 0.3, 0.75, 1.0] + list(np.random.default_rng(3).uniform(0, 1, 16))
    for u in us:
        x, cam = s.motion_state(u)
        uf = f32(u)
        want = (a + (b - a) * uf).astype(f32)
        _same(x[MOVING], want[MOVING], f"moving models at u = {u}")
        _same(x[STATIC], b[STATIC], f"static models at u = {u}: bitwise current, -0.0 kept")
        _same(cam, (ca + (cb - ca) * uf).astype(f32), f"camera at u = {u}")
    assert (_bits(s.motion_state(0.5)[0][MOVING]) != _bits(b[MOVING])).any()
    # a static camera comes back as stored; without motion everything does
    s.set_motion(d["begin_model_xform"])
    _same(s.motion_state(0.3)[1], _cam12(s), "static camera")
    s.clear_motion()
    x, cam = s.motion_state(0.3)
    _same(x, b, "no motion: the current transforms")
    _same(cam, _cam12(s), "no motion: the current camera")


def test_inspection_arrays_through_set_clear_and_the_setters(ptx):
    d, s = _scene(ptx)

    def arrays():
        return [s.array(k) for k in (ptx.ARR_MOTION_XFORM, ptx.ARR_MOTION_MOVED, ptx.ARR_MOTION_CAMERA)]

    def empty():
        return all(a.size == 0 for a in arrays())

    assert empty()
    s.set_motion(d["begin_model_xform"], begin_camera(d), (0.25, 0.75))
    x, moved, cam = arrays()
    _same(x, d["begin_model_xform"], "ARR_MOTION_XFORM")
    assert x.shape == (9, 12) and moved.dtype == np.uint32
    np.testing.assert_array_equal(moved, [0, 0, 1, 1, 1, 1, 1, 1, 1])
    _same(cam, np.concatenate([d["begin_camera"][:12], f32([1, 0.25, 0.75])]), "ARR_MOTION_CAMERA")
    # a refused call leaves them unchanged
    with pytest.raises(ptx.PtxError):
        s.set_motion(d["begin_model_xform"], begin_camera(d), (0.8, 0.2))
    for got, want in zip(arrays(), (x, moved, cam)):
        np.testing.assert_array_equal(got.view(np.uint32), want.view(np.uint32))
    s.clear_motion()
    assert empty()
    # the two setters end a motion
    s.set_motion(d["begin_model_xform"])
    assert s.array(ptx.ARR_MOTION_MOVED).sum() == 7 and s.array(ptx.ARR_MOTION_CAMERA)[12] == 0
    s.set_model_xforms(d["model_xform"])
    assert empty()
    s.set_motion(None, begin_camera(d))
    assert not s.array(ptx.ARR_MOTION_MOVED).any() and s.array(ptx.ARR_MOTION_CAMERA)[12] == 1
    c = s.camera()
    s.set_camera(c["origin"], c["basis"], c["yfov"])
    assert empty()
    # inactive motion: all keys equal; the arrays are there and nothing has moved
    s.set_motion(d["model_xform"], (d["camera"][:3], d["camera"][3:12], 0.3), (0.1, 0.2))
    x, moved, cam = arrays()
    assert not moved.any() and cam[12] == 0
    _same(x, d["model_xform"], "inactive: the begin keys are the current ones")
    _same(cam[:12], d["camera"][:12], "inactive: the begin camera is the current one (its yfov is ignored)")


def test_refusals(ptx):
    d, s = _scene(ptx)
    L = ptx.lib()
    assert L.ptx_scene_set_motion(None, None) == ptx.ERR_INVALID
    assert L.ptx_scene_motion_state(None, 0.5, None, None) == ptx.ERR_INVALID
    good = d["begin_model_xform"]
    cam = begin_camera(d)

    def refused(*a, **k):
        with pytest.raises(ptx.PtxError) as e:
            s.set_motion(*a, **k)
        assert e.value.code == ptx.ERR_INVALID
        assert s.array(ptx.ARR_MOTION_XFORM).size == 0, "a refused call touched the scene"

    refused(good[:5])
    for bad in (np.nan, np.inf, -np.inf):
        x = good.copy()
        x[3, 7] = bad
        refused(x)
        o = np.array(cam[0], f32)
        o[1] = bad
        refused(None, (o, cam[1], cam[2]))
        b = np.array(cam[1], f32)
        b[4] = bad
        refused(None, (cam[0], b, cam[2]))
        refused(None, (cam[0], cam[1], bad))
    for yfov in (0.0, -0.3, 3.2):
        refused(None, (cam[0], cam[1], yfov))
    for shutter in ((np.nan, 1.0), (0.0, np.nan), (-0.1, 0.5), (0.5, 1.1), (0.6, 0.4)):
        refused(good, cam, shutter)
    with pytest.raises(ptx.PtxError):
        s.motion_state(np.nan)
    s.set_motion(good, cam, (0.5, 0.5))   # open == close is a shutter
    s.set_motion(good, cam, (0.0, 0.0))
    s.set_motion(good, cam, (1.0, 1.0))


def test_mirror_signatures(ptx):
    S = ptx.Scene
    assert list(inspect.signature(S.set_motion).parameters) == ["self", "begin_model_xform", "begin_camera", "shutter"]
    assert inspect.signature(S.set_motion).parameters["shutter"].default == (0.0, 1.0)
    assert list(inspect.signature(S.clear_motion).parameters) == ["self"]
    assert list(inspect.signature(S.motion_state).parameters) == ["self", "u"]
    assert list(inspect.signature(S.intersect_motion).parameters)[:4] == ["self", "origins", "dirs", "time"]
    assert (ptx.ARR_MOTION_XFORM, ptx.ARR_MOTION_MOVED, ptx.ARR_MOTION_CAMERA) == (33, 34, 35)
    for sym in ("ptx_scene_set_motion", "ptx_scene_motion_state", "ptx_intersect_batch_motion"):
        assert sym in ptx.declared_symbols() and hasattr(ptx.lib(), sym)


def test_host_only_scene_has_no_timed_batch(ptx):
    d, s = _scene(ptx)
    s.set_motion(d["begin_model_xform"])
    with pytest.raises(ptx.PtxError) as e:
        s.intersect_motion(np.zeros((4, 3), f32), np.tile(f32([0, 0, 1]), (4, 1)), np.zeros(4, f32))
    assert e.value.code == ptx.ERR_NO_DEVICE


def test_light_list_leaves_out_a_moving_emitter(ptx):
    d, s = _scene(ptx, emissive=True)
    lights = (ptx.ARR_LIGHT_TRIS, ptx.ARR_LIGHT_CDF, ptx.ARR_LIGHT_GEOM)
    before = [s.array(k).copy() for k in lights]
    mover_surface = len(d["surf_range"]) - 1
    assert set(before[0][:, 0]) == {1, mover_surface} and len(before[0]) == 2 + 12
    s.set_motion(d["begin_model_xform"])
    tris, cdf, geom = [s.array(k) for k in lights]
    assert set(tris[:, 0]) == {1} and len(tris) == 2 and len(geom) == 2
    assert cdf[-1] == 1.0 and len(cdf) == 2
    s.clear_motion()
    for k, want in zip(lights, before):
        np.testing.assert_array_equal(s.array(k).view(np.uint32), want.view(np.uint32), err_msg="the light list after clear_motion")
    # motion of the camera alone, and inactive motion, leave the list as it is
    s.set_motion(None, begin_camera(d))
    assert len(s.array(ptx.ARR_LIGHT_TRIS)) == 14
    s.set_motion(d["model_xform"])
    assert len(s.array(ptx.ARR_LIGHT_TRIS)) == 14
    # ... and set_model_xforms after a motion lists the mover again, where it now is
    s.set_motion(d["begin_model_xform"])
    s.set_model_xforms(d["begin_model_xform"])
    assert len(s.array(ptx.ARR_LIGHT_TRIS)) == 14


def test_time_restatement(ora):
    """the time of a sample as the GPU tests restate it: within the shutter, and exactly `open` when the shutter is degenerate"""
    seed = 0x5EED
    rs = np.array([ora.draws(p, s, seed, 0, 0, BLOCK_TIME)[0] for p in range(40) for s in range(4)], f32)
    assert (rs >= 0).all() and (rs < 1).all() and 0.3 < rs.mean() < 0.7 and len(set(rs.tolist())) > 150
    for shutter in ((0.0, 1.0), (0.2, 0.9), (0.999, 1.0), (0.0, 1e-6)):
        us = np.array([sample_time(ora, p, s, seed, shutter) for p in range(40) for s in range(4)], f32)
        assert (us >= f32(shutter[0])).all() and (us <= f32(shutter[1])).all(), shutter
    for u in (0.0, 0.3, 0.75, 1.0):
        for p in range(8):
            assert _bits(sample_time(ora, p, 1, seed, (u, u))) == _bits(f32(u))
    # the time does not depend on the jitter's block: block 2 gives other numbers
    assert f32(ora.draws(5, 1, seed, 0, 0, 2)[0]) != f32(ora.draws(5, 1, seed, 0, 0, BLOCK_TIME)[0])
