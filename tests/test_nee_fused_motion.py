"""PTX_NEE_FUSED_MOTION without a GPU (include/ptx.h): the mirror's constant, and which flag words ptx_render_nee and
ptx_render_adaptive_nee know. A known word on a host-only scene ends at PTX_ERR_NO_DEVICE, an unknown one at PTX_ERR_INVALID with
"unknown flag", both decided before any device work. Fails on the parent, which refuses 8192 as unknown.
"""
import ctypes as C

import numpy as np

from _motion_common import begin_camera, movers
from conftest import product_from_dict


def test_constant_and_known_flags_without_a_device(ptx):
    assert ptx.NEE_FUSED_MOTION == 8192
    FM = ptx.NEE_FUSED | ptx.NEE_FUSED_MOTION
    d = movers()
    s = product_from_dict(ptx, None, d)
    s.set_motion(d["begin_model_xform"], begin_camera(d), (0.2, 0.9))   # works on host-only scenes; the refusals below do not depend on it
    cfg = ptx.RenderCfg(8, 8, 8, 2, (C.c_float * 3)(1, 1, 1), 1, 0, 0, 0, 8, 8, 0, 0, 0, 0, 0, 0)
    acc, acc_b = np.zeros((8, 8, 4), np.float32), np.zeros((8, 8, 4), np.float32)
    ad = ptx.AdaptiveCfg(8, 0, 0.1)

    def nee(flags):
        return ptx.lib().ptx_render_nee(s.h, C.byref(cfg), C.byref(ptx.NeeCfg(flags)), acc.ctypes.data, None)

    def adaptive(flags):
        return ptx.lib().ptx_render_adaptive_nee(s.h, C.byref(cfg), C.byref(ad), C.byref(ptx.NeeCfg(flags)), acc.ctypes.data, acc_b.ctypes.data, None)

    every = ptx.NEE_NO_LIGHT_SAMPLES | ptx.NEE_ENV_SAMPLES | ptx.NEE_SAMPLER_PDF | ptx.NEE_CANDIDATES(16)
    for call in (nee, adaptive):
        for extra in (0, ptx.NEE_NO_LIGHT_SAMPLES, ptx.NEE_ENV_SAMPLES, ptx.NEE_SAMPLER_PDF, ptx.NEE_CANDIDATES(4), every):
            assert call(FM | extra) == ptx.ERR_NO_DEVICE, (call.__name__, extra)
        assert call(ptx.NEE_FUSED_MOTION) == ptx.ERR_NO_DEVICE, call.__name__   # without NEE_FUSED the bit is accepted
        for bad in (16384, 4096, FM | 2, FM | 16384, 1 << 31):
            assert call(bad) == ptx.ERR_INVALID and "unknown flag" in ptx.lib().ptx_last_error().decode(), (call.__name__, bad)
    assert (acc == 0).all() and (acc_b == 0).all()
    s.close()
