"""The scenes of tests/test_nee_lights.py — the loads of lit.gltf, the emitter clouds, the chart under an environment map, the glass stacks
before a listed wall — with their oracles, and the LDS budget that makes one of them a hybrid scene (tests/test_nee_env.py uses the loads
and the budget too). Not collected (underscore prefix). Oracles and flat arrays are kept here once; product scenes are kept per test module.
"""
import os

import numpy as np

from _checks import _glass_stack
from _common import _proc
from conftest import GOLD, oracle_from_dict, product_from_dict

f32 = np.float32
LIT = os.path.join(GOLD, "textures", "lit.gltf")
SKY = os.path.join(GOLD, "hdr", "sky_rle.hdr")
NO_SUN = 0xFFFFFFFF
LIT_PRIMS = ["emit_palette_normal", "emit_hdr_srgb", "emit_factor", "emit_black_region", "recv_base_mr", "recv_normal_mr_hdr", "recv_plain",
             "occluder", "blend_emissive_alpha_tex", "blend_factor"]          # primitives of mesh "lit", in file order
LIT_OPAQUE = list(range(8))                                                      # the last two can pass a ray through
# name -> (sun_light_index, work): the four loads, and D's (no float sRGB emitter: its powf differs between ocml and glibc; no unlisted emitter)
LIT_LOADS = {"lit": (0, None), "lit_nosun": (NO_SUN, None), "lit_opaque": (0, {"lit": LIT_OPAQUE}), "lit_opaque_nosun": (NO_SUN, {"lit": LIT_OPAQUE}),
             "lit_first": (NO_SUN, {"lit": [0, 2, 3, 4, 5, 6, 7]})}
CLOUDS = {"cloud": (True, True), "cloud_nosun": (False, True), "cloud_opaque": (True, False), "cloud_opaque_nosun": (False, False)}   # name -> (sun, alpha)


def _glass_wall(n_layers, opacity):
    """_checks._glass_stack plus a listed emissive wall behind the camera, facing the stack: a vertex on layer k samples the wall
    through the layers in front of it (only layer 0 sees it), and a path that leaves a layer towards the wall passes the layers in front
    (pass > 0 when it arrives: the emission's weight is 1 there)."""
    d = _glass_stack(n_layers, opacity)
    q = np.zeros((4, 11), f32)
    q[:, :3] = [[-5, -5, 1.0], [-5, 5, 1.0], [5, 5, 1.0], [5, -5, 1.0]]     # counter-clockwise seen from -z
    q[:, 7] = -1.0
    q[:, 8] = 1.0
    nv, nt = len(d["vertices"]), len(d["triangles"])
    d["vertices"] = np.concatenate([d["vertices"], q])
    d["triangles"] = np.concatenate([d["triangles"], np.array([[0, 1, 2], [0, 2, 3]], np.uint32)])
    d["surf_range"] = np.concatenate([d["surf_range"], np.array([[nv, 4, nt, 2]], np.int32)])
    d["model_surf"] = np.array([[0, 2]], np.int32)
    d["materials"] = np.concatenate([d["materials"], np.array([[0.7, 0.7, 0.7, 1.0, 0.6, 0.0, 0.3, 0.25, 0.2, 1.33, 0]], f32)])
    return d


# ---------------------------------------------------------------------------- scenes, built once
_dicts, _oracles = {}, {}


def _dict(name):
    if name not in _dicts:
        if name in CLOUDS:
            sun, alpha = CLOUDS[name]
            _dicts[name] = _proc().emitter_cloud_scene(sun=sun, alpha=alpha)
        elif name == "chart_env":
            _dicts[name] = _proc().chart_scene(facing=True, alpha=False)
        elif name == "glass40":
            _dicts[name] = _glass_wall(40, 0.5)
        elif name == "glass4200":
            _dicts[name] = _glass_wall(4200, 0.0)
    return _dicts[name]


def _oracle(ora, name):
    """(oracle scene, its arrays)"""
    if name not in _oracles:
        if name in LIT_LOADS:
            sun, work = LIT_LOADS[name]
            a = ora.load_gltf(LIT, sun_light_index=sun, work=work)
            _oracles[name] = (ora.OracleScene(a), a)
        else:
            o = oracle_from_dict(ora, _dict(name))
            if name == "chart_env":
                o.set_environment(SKY)
            _oracles[name] = (o, o.a)
    return _oracles[name]


def _host_scene(ptx, name, ctx=None):
    if name in LIT_LOADS:
        sun, work = LIT_LOADS[name]
        return ptx.Scene.load_gltf(ctx, LIT, sun_light_index=sun, work=work)
    s = product_from_dict(ptx, ctx, _dict(name))
    if name == "chart_env":
        s.set_environment(SKY)
    return s


def _hybrid_budget(ptx, mp, name):
    """One byte short of ARR_RES_PLAN[0], as test_nee_fused.test_hybrid_scene_bitwise takes it. Where leaf-ordered copies have made the
    resident arrays larger than what the residency choice counts (one record per triangle: plan_residency), that budget still holds every
    surface; then one byte short of the arrays without leaf order, which is never more than the choice counts."""
    budget = int(_host_scene(ptx, name).array(ptx.ARR_RES_PLAN)[0]) - 1
    mp.setenv("PTX_LDS_BUDGET", str(budget))
    fits = _host_scene(ptx, name).info()["lds_resident"] == 1
    mp.delenv("PTX_LDS_BUDGET")
    if fits:
        mp.setenv("PTX_LDS_LEAF_ORDER", "0")
        budget = int(_host_scene(ptx, name).array(ptx.ARR_RES_PLAN)[0]) - 1
        mp.delenv("PTX_LDS_LEAF_ORDER")
    return budget
