"""What the two motion-blur test files share: the movers scene, the begin camera as Scene.set_motion takes it, and the restated time of a
sample (include/ptx.h: MOTION). Not collected (underscore prefix); import by name."""
import numpy as np

from _common import _proc

f32 = np.float32
BLOCK_TIME = 0x300   # the Philox block of a sample's time
_dicts = {}


def movers(emissive=False, sun=False, alpha=False):
    key = (emissive, sun, alpha)
    if key not in _dicts:
        _dicts[key] = _proc().movers_scene(emissive, sun, alpha)
    return _dicts[key]


def begin_camera(d):
    return d["begin_camera"][:3], d["begin_camera"][3:12], d["begin_camera"][12]


def sample_time(ora, pixel, sample, seed, shutter):
    """u = open + (close - open) * r in float32, each operation rounded on its own, r = draws(pixel, sample, 0, 0, BLOCK_TIME).x"""
    r = f32(ora.draws(pixel, sample, seed, 0, 0, BLOCK_TIME)[0])
    o, c = f32(shutter[0]), f32(shutter[1])
    return f32(o + f32(f32(c - o) * r))
