"""What the five render entry points refuse, and with which code: one table, every row one C call through ctypes.

The entry points share one cfg check (render_rect, csrc/api_internal.hpp) but differ in where it sits among their other refusals, so the
code a caller sees for a cfg with several faults depends on the order: ptx_render_adaptive looks at the rectangle before the missing
context, the others after; ptx_render_aov refuses the worker integrator before anything about the image and ignores `bounces`. The
expected code of every row is a recording: the library as it was before the entry points were split over three files, run once on this
table (without a device for the first half, on the MI355X for the second). Every refusal is decided before any kernel launch.
"""
import ctypes as C

import numpy as np
import pytest

from conftest import CORNELL

OK, INVALID, NO_DEVICE, UNSUPPORTED = 0, 1, 5, 7
ENTRIES = ("ptx_render", "ptx_render_transparent", "ptx_render_aov", "ptx_render_nee", "ptx_render_adaptive")

# faults of a cfg, as overrides of the valid one (8 x 8, the whole frame given as a tile, LIB integrator, no sharding)
FAULTS = {
    "valid": {},
    "W=0": dict(W=0),
    "tile outside": dict(x0=4, w=8),
    "w=0,h!=0": dict(w=0, h=4),
    "bounces=65536": dict(bounces=65536),
    "worker": dict(integrator=1),
    "integrator=7": dict(integrator=7),
    "shard_index>=count": dict(shard_index=2, shard_count=2),
    "w*h>2^31-1": dict(W=65536, H=65536, w=65536, h=32768),
    "tile outside + worker": dict(x0=4, w=8, integrator=1),
    "W=0 + integrator=7": dict(W=0, integrator=7),
    "bounces=65536 + worker": dict(bounces=65536, integrator=1),
    "worker + shard_index>=count": dict(integrator=1, shard_index=2, shard_count=2),
    "bounces=65536 + tile outside": dict(bounces=65536, x0=4, w=8),
}
# arguments passed as NULL, per entry point ("both buffers": a ptx_aov_buffers with two NULL members)
NULLS = {"ptx_render": ("sc", "cfg", "accum"), "ptx_render_transparent": ("sc", "cfg", "pixel_rgba", "claimed"),
         "ptx_render_aov": ("sc", "cfg", "out", "both buffers"), "ptx_render_nee": ("sc", "cfg", "accum"),
         "ptx_render_adaptive": ("sc", "cfg", "acfg", "accum_a", "accum_b")}

# (entry point, fault, NULL argument or None, adaptive cfg overrides) -> code, on a scene WITHOUT a context: every row that is not
# refused for its arguments ends on PTX_ERR_NO_DEVICE
HOST_ROWS = [
    ('ptx_render', 'valid', None, {}, 5),
    ('ptx_render', 'W=0', None, {}, 5),
    ('ptx_render', 'tile outside', None, {}, 5),
    ('ptx_render', 'w=0,h!=0', None, {}, 5),
    ('ptx_render', 'bounces=65536', None, {}, 5),
    ('ptx_render', 'worker', None, {}, 5),
    ('ptx_render', 'integrator=7', None, {}, 5),
    ('ptx_render', 'shard_index>=count', None, {}, 5),
    ('ptx_render', 'w*h>2^31-1', None, {}, 5),
    ('ptx_render', 'tile outside + worker', None, {}, 5),
    ('ptx_render', 'W=0 + integrator=7', None, {}, 5),
    ('ptx_render', 'bounces=65536 + worker', None, {}, 5),
    ('ptx_render', 'worker + shard_index>=count', None, {}, 5),
    ('ptx_render', 'bounces=65536 + tile outside', None, {}, 5),
    ('ptx_render', 'valid', 'sc', {}, 1),
    ('ptx_render', 'valid', 'cfg', {}, 1),
    ('ptx_render', 'valid', 'accum', {}, 1),
    ('ptx_render', 'tile outside', 'sc', {}, 1),
    ('ptx_render_transparent', 'valid', None, {}, 5),
    ('ptx_render_transparent', 'W=0', None, {}, 5),
    ('ptx_render_transparent', 'tile outside', None, {}, 5),
    ('ptx_render_transparent', 'w=0,h!=0', None, {}, 5),
    ('ptx_render_transparent', 'bounces=65536', None, {}, 5),
    ('ptx_render_transparent', 'worker', None, {}, 7),
    ('ptx_render_transparent', 'integrator=7', None, {}, 5),
    ('ptx_render_transparent', 'shard_index>=count', None, {}, 5),
    ('ptx_render_transparent', 'w*h>2^31-1', None, {}, 5),
    ('ptx_render_transparent', 'tile outside + worker', None, {}, 7),
    ('ptx_render_transparent', 'W=0 + integrator=7', None, {}, 5),
    ('ptx_render_transparent', 'bounces=65536 + worker', None, {}, 7),
    ('ptx_render_transparent', 'worker + shard_index>=count', None, {}, 7),
    ('ptx_render_transparent', 'bounces=65536 + tile outside', None, {}, 5),
    ('ptx_render_transparent', 'valid', 'sc', {}, 1),
    ('ptx_render_transparent', 'valid', 'cfg', {}, 1),
    ('ptx_render_transparent', 'valid', 'pixel_rgba', {}, 1),
    ('ptx_render_transparent', 'valid', 'claimed', {}, 1),
    ('ptx_render_transparent', 'tile outside', 'sc', {}, 1),
    ('ptx_render_aov', 'valid', None, {}, 5),
    ('ptx_render_aov', 'W=0', None, {}, 5),
    ('ptx_render_aov', 'tile outside', None, {}, 5),
    ('ptx_render_aov', 'w=0,h!=0', None, {}, 5),
    ('ptx_render_aov', 'bounces=65536', None, {}, 5),
    ('ptx_render_aov', 'worker', None, {}, 7),
    ('ptx_render_aov', 'integrator=7', None, {}, 1),
    ('ptx_render_aov', 'shard_index>=count', None, {}, 5),
    ('ptx_render_aov', 'w*h>2^31-1', None, {}, 5),
    ('ptx_render_aov', 'tile outside + worker', None, {}, 7),
    ('ptx_render_aov', 'W=0 + integrator=7', None, {}, 1),
    ('ptx_render_aov', 'bounces=65536 + worker', None, {}, 7),
    ('ptx_render_aov', 'worker + shard_index>=count', None, {}, 7),
    ('ptx_render_aov', 'bounces=65536 + tile outside', None, {}, 5),
    ('ptx_render_aov', 'valid', 'sc', {}, 1),
    ('ptx_render_aov', 'valid', 'cfg', {}, 1),
    ('ptx_render_aov', 'valid', 'out', {}, 1),
    ('ptx_render_aov', 'valid', 'both buffers', {}, 1),
    ('ptx_render_aov', 'tile outside', 'sc', {}, 1),
    ('ptx_render_nee', 'valid', None, {}, 5),
    ('ptx_render_nee', 'W=0', None, {}, 5),
    ('ptx_render_nee', 'tile outside', None, {}, 5),
    ('ptx_render_nee', 'w=0,h!=0', None, {}, 5),
    ('ptx_render_nee', 'bounces=65536', None, {}, 5),
    ('ptx_render_nee', 'worker', None, {}, 7),
    ('ptx_render_nee', 'integrator=7', None, {}, 5),
    ('ptx_render_nee', 'shard_index>=count', None, {}, 5),
    ('ptx_render_nee', 'w*h>2^31-1', None, {}, 5),
    ('ptx_render_nee', 'tile outside + worker', None, {}, 7),
    ('ptx_render_nee', 'W=0 + integrator=7', None, {}, 5),
    ('ptx_render_nee', 'bounces=65536 + worker', None, {}, 7),
    ('ptx_render_nee', 'worker + shard_index>=count', None, {}, 7),
    ('ptx_render_nee', 'bounces=65536 + tile outside', None, {}, 5),
    ('ptx_render_nee', 'valid', 'sc', {}, 1),
    ('ptx_render_nee', 'valid', 'cfg', {}, 1),
    ('ptx_render_nee', 'valid', 'accum', {}, 1),
    ('ptx_render_nee', 'tile outside', 'sc', {}, 1),
    ('ptx_render_adaptive', 'valid', None, {}, 5),
    ('ptx_render_adaptive', 'W=0', None, {}, 1),
    ('ptx_render_adaptive', 'tile outside', None, {}, 1),
    ('ptx_render_adaptive', 'w=0,h!=0', None, {}, 1),
    ('ptx_render_adaptive', 'bounces=65536', None, {}, 1),
    ('ptx_render_adaptive', 'worker', None, {}, 5),
    ('ptx_render_adaptive', 'integrator=7', None, {}, 1),
    ('ptx_render_adaptive', 'shard_index>=count', None, {}, 1),
    ('ptx_render_adaptive', 'w*h>2^31-1', None, {}, 1),
    ('ptx_render_adaptive', 'tile outside + worker', None, {}, 1),
    ('ptx_render_adaptive', 'W=0 + integrator=7', None, {}, 1),
    ('ptx_render_adaptive', 'bounces=65536 + worker', None, {}, 1),
    ('ptx_render_adaptive', 'worker + shard_index>=count', None, {}, 1),
    ('ptx_render_adaptive', 'bounces=65536 + tile outside', None, {}, 1),
    ('ptx_render_adaptive', 'valid', 'sc', {}, 1),
    ('ptx_render_adaptive', 'valid', 'cfg', {}, 1),
    ('ptx_render_adaptive', 'valid', 'acfg', {}, 1),
    ('ptx_render_adaptive', 'valid', 'accum_a', {}, 1),
    ('ptx_render_adaptive', 'valid', 'accum_b', {}, 1),
    ('ptx_render_adaptive', 'tile outside', 'sc', {}, 1),
    ('ptx_render_adaptive', 'valid', None, {'min_spp': 3}, 1),
    ('ptx_render_adaptive', 'shard_count=2', None, {}, 7),
    ('ptx_render_adaptive', 'tile outside', None, {'min_spp': 3}, 1),
    ('ptx_render_adaptive', 'shard_count=2 + tile outside', None, {}, 1),
]

# the refusals behind the context check, on a device scene (Cornell, 8 x 8, spp = 1): (entry point, fault, which buffer is device memory)
DEVICE_ROWS = [
    ('ptx_render_aov', 'W=0', None, 1),
    ('ptx_render_aov', 'tile outside', None, 1),
    ('ptx_render_aov', 'valid', 'albedo_cov', 1),
    ('ptx_render_aov', 'valid', 'normal_depth', 1),
    ('ptx_render_transparent', 'valid', 'pixel_rgba', 1),
    ('ptx_render_transparent', 'valid', 'claimed', 1),
    ('ptx_render_adaptive', 'valid', 'accum_a', 1),
    ('ptx_render_adaptive', 'valid', 'accum_b', 1),
]


def host_cases():
    """The table's rows without their codes (the recording fills them in)."""
    rows = []
    for e in ENTRIES:
        rows += [(e, f, None, {}) for f in FAULTS]
        rows += [(e, "valid", n, {}) for n in NULLS[e]]
        rows += [(e, "tile outside", "sc", {})]   # a NULL argument and a bad cfg at once
    rows += [("ptx_render_adaptive", "valid", None, dict(min_spp=3)), ("ptx_render_adaptive", "shard_count=2", None, {}),
             ("ptx_render_adaptive", "tile outside", None, dict(min_spp=3)), ("ptx_render_adaptive", "shard_count=2 + tile outside", None, {})]
    return rows


ADAPTIVE_FAULTS = {"shard_count=2": dict(shard_index=0, shard_count=2), "shard_count=2 + tile outside": dict(shard_index=0, shard_count=2, x0=4, w=8)}
device_cases = [("ptx_render_aov", "W=0", None), ("ptx_render_aov", "tile outside", None), ("ptx_render_aov", "valid", "albedo_cov"),
                ("ptx_render_aov", "valid", "normal_depth"), ("ptx_render_transparent", "valid", "pixel_rgba"), ("ptx_render_transparent", "valid", "claimed"),
                ("ptx_render_adaptive", "valid", "accum_a"), ("ptx_render_adaptive", "valid", "accum_b")]


def call(ptx, scene, entry, fault, null=None, acfg_over=None, device=None):
    """One call of `entry`; -> (code, message). device: the name of the one buffer given as device memory (the others are host memory)."""
    L = ptx.lib()
    fields = dict(W=8, H=8, spp=2 if entry == "ptx_render_adaptive" else 1, bounces=2, x0=0, y0=0, w=8, h=8)
    fields.update(FAULTS.get(fault, ADAPTIVE_FAULTS.get(fault)))
    cfg = ptx.RenderCfg(env=(C.c_float * 3)(1, 1, 1), seed_lo=0x5EED, **fields)
    keep = []

    def buf(name, shape=(8, 8, 4), dtype=np.float32):
        if name == null:
            return None
        if name == device:
            import torch
            t = torch.zeros(shape, dtype=torch.float32 if dtype == np.float32 else torch.uint8, device="cuda")
            keep.append(t)
            return t.data_ptr()
        a = np.zeros(shape, dtype)
        keep.append(a)
        return a.ctypes.data

    sc = None if null == "sc" else scene.h
    pcfg = None if null == "cfg" else C.byref(cfg)
    if entry == "ptx_render":
        rc = L.ptx_render(sc, pcfg, buf("accum"), None)
    elif entry == "ptx_render_transparent":
        rc = L.ptx_render_transparent(sc, pcfg, buf("pixel_rgba"), buf("claimed", (8, 8), np.uint8), None)
    elif entry == "ptx_render_aov":
        out = ptx.AovBuffers(None, None) if null == "both buffers" else ptx.AovBuffers(buf("albedo_cov"), buf("normal_depth"))
        rc = L.ptx_render_aov(sc, pcfg, None if null == "out" else C.byref(out), None)
    elif entry == "ptx_render_nee":
        rc = L.ptx_render_nee(sc, pcfg, None, buf("accum"), None)
    else:
        acfg = ptx.AdaptiveCfg(**dict(dict(min_spp=2, step_spp=0, threshold=0.0), **(acfg_over or {})))
        rc = L.ptx_render_adaptive(sc, pcfg, None if null == "acfg" else C.byref(acfg), buf("accum_a"), buf("accum_b"), None)
    msg = L.ptx_last_error().decode(errors="replace") if rc != OK else ""
    assert rc == OK or all(not isinstance(k, np.ndarray) or not k.any() for k in keep), "a refused call wrote into a buffer"
    return rc, msg


@pytest.fixture(scope="module")
def host_scene(ptx):
    return ptx.Scene.load_gltf(None, CORNELL)


def test_the_table_is_complete():
    assert [r[:4] for r in HOST_ROWS] == host_cases() and [r[:3] for r in DEVICE_ROWS] == device_cases


@pytest.mark.parametrize("entry,fault,null,acfg_over,code", HOST_ROWS, ids=lambda v: str(v).replace(" ", "") if not isinstance(v, dict) else "+".join(v) or "-")
def test_refusals_without_a_device(ptx, host_scene, entry, fault, null, acfg_over, code):
    rc, msg = call(ptx, host_scene, entry, fault, null, acfg_over)
    assert rc == code, msg
    assert msg.startswith(entry + ":"), msg


@pytest.mark.gpu
def test_refusals_behind_the_context_check(ptx):
    ctx = ptx.Context(0)
    scene = ptx.Scene.load_gltf(ctx, CORNELL)
    for entry, fault, device, code in DEVICE_ROWS:
        rc, msg = call(ptx, scene, entry, fault, device=device)
        assert rc == code, (entry, fault, device, msg)
        assert msg.startswith(entry + ":"), msg
    for entry in ENTRIES:   # and the valid call is taken
        assert call(ptx, scene, entry, "valid")[0] == OK, entry
