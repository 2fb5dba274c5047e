"""The scenes of tests/test_nee_lights.py — the loads of lit.gltf, the emitter clouds, the chart under an environment map, the glass stacks
before a listed wall — with their oracles, and the LDS budget that makes one of them a hybrid scene (tests/test_nee_env.py uses the loads
and the budget too). Not collected (underscore prefix). Oracles and flat arrays are kept here once; product scenes are kept per test module.

Below them, what the modules that set maps on their scenes share (test_nee_env.py, test_nee_sampler_pdf.py, test_nee_ris.py,
test_nee_punctual_gpu.py, test_nee_restatement_bits.py): the flag values, the `maps` fixture, fresh oracle and product scenes under a map, the
product's environment table, the variance ratio.
"""
import os

import numpy as np
import pytest

import _nee_common
import _nee_env_restatement as E
from _checks import _glass_stack
from _common import _proc
from conftest import CORNELL, GOLD, oracle_from_dict, product_from_dict

f32 = np.float32
NO_LIGHTS, FUSED, ENV, SPDF = 1, 4, 16, 64   # PTX_NEE_NO_LIGHT_SAMPLES, PTX_NEE_FUSED, PTX_NEE_ENV_SAMPLES, PTX_NEE_SAMPLER_PDF


def CAND(m):
    return (m - 1) << 8


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


# ---------------------------------------------------------------------------- scenes under a map: fresh ones, since a map is set on them
@pytest.fixture(scope="module")
def maps(tmp_path_factory):
    """name -> (path, srgb). .hdr maps are read linearly: a float sRGB texel goes through powf, ocml's on the device and glibc's in the oracle.
    Small uncompressed Radiance files written into tmp (a 16 x 8 grey map with one hot texel in the top-left corner, the same with a black
    background, a uniform map of value 1, a black map), and tests/golden's."""
    d = tmp_path_factory.mktemp("env_maps")
    tex = os.path.join(GOLD, "textures")
    return {"hot": (E.write_hdr(d / "hot.hdr", E.hot_texel()), False), "hot_only": (E.write_hdr(d / "hot_only.hdr", E.hot_texel(base=0.0)), False),
            "uniform": (E.write_hdr(d / "uniform.hdr", np.full((8, 16, 3), 1.0)), False), "black": (E.write_hdr(d / "black.hdr", np.zeros((4, 8, 3))), False),
            "sky": (SKY, False), "emit_6x5": (os.path.join(tex, "emit_6x5.hdr"), False), "l1_37x53": (os.path.join(tex, "l1_37x53.png"), True),
            "pt_1x1": (os.path.join(tex, "pt_1x1.png"), True)}


def _any_dict(name):
    return _dict(name) if name in CLOUDS or name.startswith("glass") else _nee_common._dict(name)


def _new_oracle(ora, name, env_map=None):
    if name == "cornell":
        o = ora.OracleScene(ora.load_gltf(CORNELL))
    elif name in LIT_LOADS:
        sun, work = LIT_LOADS[name]
        o = ora.OracleScene(ora.load_gltf(LIT, sun_light_index=sun, work=work))
    else:
        o = oracle_from_dict(ora, _any_dict(name))
    if env_map:
        o.set_environment(env_map[0], srgb=env_map[1])
    return o


def _new_scene(ptx, name, ctx=None, env_map=None):
    if name == "cornell":
        s = ptx.Scene.load_gltf(ctx, CORNELL)
    elif name in LIT_LOADS:
        sun, work = LIT_LOADS[name]
        s = ptx.Scene.load_gltf(ctx, LIT, sun_light_index=sun, work=work)
    else:
        s = product_from_dict(ptx, ctx, _any_dict(name))
    if env_map:
        s.set_environment(env_map[0], srgb=env_map[1])
    return s


def _tables(ptx, s):
    return s.array(ptx.ARR_ENV_ROW_CDF), s.array(ptx.ARR_ENV_CELL_CDF)


def _table(ptx, s):
    return E.table(*_tables(ptx, s))


_under_maps = {}


def _oracle_and_table(ptx, ora, maps, name, map_name, flags):
    """(oracle scene under the map, the environment table if the flags ask for one), kept"""
    key = (name, map_name, bool(flags & ENV))
    if key not in _under_maps:
        o = _new_oracle(ora, name, maps[map_name] if map_name else None)
        tab = _table(ptx, _new_scene(ptx, name, env_map=maps[map_name])) if flags & ENV else None
        _under_maps[key] = (o, tab)
    return _under_maps[key]


def _variance_ratio(flagged, unflagged):
    """mean over pixels and channels of the per-pixel sample variance, flagged / unflagged; rad [h, w, spp, 3]"""
    return float(flagged.var(2, ddof=1, dtype=np.float64).mean() / unflagged.var(2, ddof=1, dtype=np.float64).mean())
