"""Point and spot lights as a third light-sampling strategy of ptx_render_nee (include/ptx.h: ptx_scene_set_punctual_lights,
ptx_gltf_read_punctual_lights, PUNCTUAL LIGHTS), without a GPU: the symbols and the setter's refusals on a host-only scene, the stored arrays,
the glTF reader on tests/golden/lights/lamps.gltf, and the estimator on tests/_nee_estimator.py.

The expectation is pinned to a stand-in: the point light replaced by a small emissive triangle at the light's position that faces the test
region, with Le * area = the light's intensity, rendered by the restatement of the existing estimator (no punctual lights). The test region is
the patch of floor straight below the lamp, seen through a narrow camera, so that the triangle's cosine is 1 there; 2 bounces, so that only
vertex 0 takes a light sample (a Lambertian triangle and an isotropic point light differ in every other direction). GPU tests:
tests/test_nee_punctual_gpu.py.
"""
import ctypes as C
import json
import os

import numpy as np
import pytest

import _nee_punctual_restatement as PU
from _common import _bits, _proc
from _nee_common import K_BATCH, SEED, _batch_stat, _oracle, _same_expectation
from _nee_estimator import render_samples
from _nee_lit_scenes import SKY, _table
from conftest import GOLD, oracle_from_dict, product_from_dict

f32 = np.float32
LAMPS = os.path.join(GOLD, "lights", "lamps.gltf")


def _lamp(pos=(0, 1, 0), rng=0.0, direction=(0, 0, -1), kind=0, intensity=(1, 1, 1), ci=1.0, co=0.70710677):
    return np.array([*pos, rng, *direction, kind, *intensity, ci, co, 0, 0, 0], f32)


def _floor(ptx):
    d, _ = _proc().lamp_scene(1)
    return product_from_dict(ptx, None, d)


# ---------------------------------------------------------------------------- symbols, refusals, stored arrays
def test_symbols_and_constants(ptx):
    """fails on the parent: neither the functions nor the array ids exist there"""
    assert {"ptx_scene_set_punctual_lights", "ptx_gltf_read_punctual_lights"} <= set(ptx.declared_symbols())
    assert hasattr(ptx.lib(), "ptx_scene_set_punctual_lights") and hasattr(ptx.lib(), "ptx_gltf_read_punctual_lights")
    assert (ptx.ARR_PUNCTUAL, ptx.ARR_PUNCTUAL_CDF) == (28, 29)
    assert callable(ptx.read_punctual_lights) and callable(ptx.Scene.set_punctual_lights) and callable(ptx.Renderer.set_punctual_lights)


BAD = {"nan position": _lamp(pos=(np.nan, 1, 0)), "inf range": _lamp(rng=np.inf), "inf in the padding": np.concatenate([_lamp()[:15], [f32(np.inf)]]).astype(f32),
       "kind 2": _lamp(kind=2), "kind 0.5": _lamp(kind=0.5), "negative green": _lamp(intensity=(1, -0.1, 1)), "negative range": _lamp(rng=-1.0),
       "spot of length 1.01": _lamp(kind=1, direction=(0, -1.01, 0)), "spot of length 0": _lamp(kind=1, direction=(0, 0, 0)),
       "cos_inner below cos_outer": _lamp(kind=1, direction=(0, -1, 0), ci=0.5, co=0.6)}


@pytest.mark.parametrize("what", sorted(BAD))
def test_setter_refuses_on_a_host_only_scene(ptx, what):
    """every refusal is PTX_ERR_INVALID and leaves the lights that were set before"""
    s = _floor(ptx)
    good = np.stack([_lamp(), _lamp(pos=(1, 2, 0), kind=1, direction=(0, -1, 0), intensity=(2, 2, 2), ci=0.9, co=0.8)])
    s.set_punctual_lights(good)
    with pytest.raises(ptx.PtxError) as e:
        s.set_punctual_lights(np.stack([good[0], BAD[what]]))
    assert e.value.args[0] == ptx.ERR_INVALID or getattr(e.value, "code", None) == ptx.ERR_INVALID, e.value
    np.testing.assert_array_equal(_bits(s.array(ptx.ARR_PUNCTUAL)), _bits(good))


def test_setter_refuses_null_arguments_and_too_many(ptx):
    s = _floor(ptx)
    L = ptx.lib()
    one = _lamp()
    assert L.ptx_scene_set_punctual_lights(None, one.ctypes.data, 1) == ptx.ERR_INVALID
    assert L.ptx_scene_set_punctual_lights(s.h, None, 1) == ptx.ERR_INVALID
    many = np.tile(_lamp(), (65537, 1))
    assert L.ptx_scene_set_punctual_lights(s.h, many.ctypes.data, 65537) == ptx.ERR_INVALID
    assert L.ptx_scene_set_punctual_lights(s.h, many.ctypes.data, 65536) == ptx.OK and len(s.array(ptx.ARR_PUNCTUAL_CDF)) == 65536
    assert L.ptx_scene_set_punctual_lights(s.h, None, 0) == ptx.OK and len(s.array(ptx.ARR_PUNCTUAL)) == 0
    # a point light's direction and cones are not looked at; a spot within 1e-3 of unit length passes
    s.set_punctual_lights(np.stack([_lamp(direction=(0, 0, 0), ci=0.1, co=0.9), _lamp(kind=1, direction=(0, -1.0009, 0))]))
    assert len(s.array(ptx.ARR_PUNCTUAL_CDF)) == 2


def test_stored_arrays_and_the_cdf(ptx):
    """the records as given; the CDF against a float64 rebuild (the restatement's cdf_of), a black light with probability 0, n = 0 and
    all-black lights both leave no lights"""
    s = _floor(ptx)
    assert len(s.array(ptx.ARR_PUNCTUAL)) == 0 and len(s.array(ptx.ARR_PUNCTUAL_CDF)) == 0
    _, lights = _proc().lamp_scene(37, spots=True, lamp_range=3.0)
    lights[5, 8:11] = 0
    s.set_punctual_lights(lights)
    np.testing.assert_array_equal(_bits(s.array(ptx.ARR_PUNCTUAL)), _bits(lights))
    cdf = s.array(ptx.ARR_PUNCTUAL_CDF)
    lum = lights[:, 8:11].astype(np.float64) @ [0.2126, 0.7152, 0.0722]
    want = (np.cumsum(lum) / lum.sum()).astype(f32)
    want[-1] = 1
    np.testing.assert_allclose(cdf, want, rtol=0, atol=2 ** -23)
    np.testing.assert_array_equal(_bits(cdf), _bits(PU.cdf_of(lights)))
    assert cdf[-1] == 1 and (np.diff(cdf) >= 0).all() and cdf[5] == cdf[4]
    s.set_punctual_lights(None)
    assert len(s.array(ptx.ARR_PUNCTUAL)) == 0 and len(s.array(ptx.ARR_PUNCTUAL_CDF)) == 0
    s.set_punctual_lights(lights)
    black = lights.copy()
    black[:, 8:11] = 0
    s.set_punctual_lights(black)
    assert len(s.array(ptx.ARR_PUNCTUAL)) == 0 and len(s.array(ptx.ARR_PUNCTUAL_CDF)) == 0 and PU.cdf_of(black) is None
    # a host-only scene refuses the render as before, lights or not
    s.set_punctual_lights(lights)
    cfg = ptx.RenderCfg(8, 8, 2, 2, (C.c_float * 3)(1, 1, 1), 1, 0, 0, 0, 8, 8, 0, 0, 0, 0, 0, 0)
    acc = np.zeros((8, 8, 4), f32)
    assert ptx.lib().ptx_render_nee(s.h, C.byref(cfg), None, acc.ctypes.data, None) == ptx.ERR_NO_DEVICE


# ---------------------------------------------------------------------------- the reader
def _world_matrices(g):
    """float64 world matrix per node of scenes[0], pre-order, from the file's TRS (the loader ignores `matrix`)"""
    out, order = {}, []

    def local(n):
        x, y, z, w = n.get("rotation", [0, 0, 0, 1])
        R = np.array([[1 - 2 * (y * y + z * z), 2 * (x * y - z * w), 2 * (x * z + y * w)],
                      [2 * (x * y + z * w), 1 - 2 * (x * x + z * z), 2 * (y * z - x * w)],
                      [2 * (x * z - y * w), 2 * (y * z + x * w), 1 - 2 * (x * x + y * y)]])
        M = np.eye(4)
        M[:3, :3] = R * np.asarray(n.get("scale", [1, 1, 1]), np.float64)[None, :]
        M[:3, 3] = n.get("translation", [0, 0, 0])
        return M

    def walk(i, parent):
        n = g["nodes"][i]
        out[i] = parent @ local(n)
        order.append(i)
        for c in n.get("children", []):
            walk(c, out[i])
    for i in g["scenes"][0]["nodes"]:
        walk(i, np.eye(4))
    return out, order


def test_reader_against_the_files_own_node_matrices(ptx):
    """positions, directions, intensities and cones of lamps.gltf from its JSON in float64. Tolerance: the loader composes float32 transforms,
    two levels deep here, so a position carries a few ulp of the scene's extent (|coordinate| <= 5): 8 * 2^-23 * 5 < 5e-6; a unit direction
    8 * 2^-23 < 1e-6; intensities and cosines are one float32 product or rounding: 2^-23 relative."""
    with open(LAMPS) as fh:
        g = json.load(fh)
    defs = g["extensions"]["KHR_lights_punctual"]["lights"]
    M, order = _world_matrices(g)
    want, kinds = [], []
    for i in order:
        ref = g["nodes"][i].get("extensions", {}).get("KHR_lights_punctual")
        if ref is None or defs[ref["light"]]["type"] == "directional":
            continue
        l = defs[ref["light"]]
        z = -M[i][:3, 2]
        spot = l.get("spot", {})
        want.append(dict(pos=M[i][:3, 3], dir=z / np.linalg.norm(z), kind=1.0 if l["type"] == "spot" else 0.0, range=l.get("range", 0.0),
                         I=np.asarray(l.get("color", [1, 1, 1]), np.float64) * l.get("intensity", 1.0),
                         ci=np.cos(spot.get("innerConeAngle", 0.0)), co=np.cos(spot.get("outerConeAngle", np.pi / 4))))
        kinds.append(l["name"])
    assert kinds == ["lamp_point", "lamp_spot", "lamp_default", "lamp_dark"]          # pre-order; the sun skipped
    assert [d["type"] for d in defs].count("directional") == 1
    rig = next(n for n in g["nodes"] if n["name"] == "rig")
    assert len(set(rig["scale"])) == 3 and rig["rotation"][3] != 1                  # rotated, non-uniformly scaled parent
    got = ptx.read_punctual_lights(LAMPS)
    assert got.shape == (4, 16) and got.dtype == f32
    for k, w in enumerate(want):
        np.testing.assert_allclose(got[k, 0:3], w["pos"], rtol=0, atol=5e-6)
        np.testing.assert_allclose(got[k, 4:7], w["dir"], rtol=0, atol=1e-6)
        assert abs(float(np.linalg.norm(got[k, 4:7].astype(np.float64))) - 1) < 1e-6
        assert got[k, 7] == w["kind"] and got[k, 3] == f32(w["range"])
        np.testing.assert_allclose(got[k, 8:11], w["I"], rtol=2 ** -22, atol=0)
        np.testing.assert_allclose(got[k, 11:13], [w["ci"], w["co"]], rtol=2 ** -23, atol=0)
        assert (got[k, 13:] == 0).all()
    # the defaults: colour 1, intensity 1, range 0, inner angle 0, outer angle pi / 4
    np.testing.assert_array_equal(got[2, [3, 8, 9, 10, 11]], f32([0, 1, 1, 1, 1]))
    assert got[2, 12] == f32(np.cos(np.pi / 4)) and got[2, 7] == 1
    assert (got[3, 8:11] == 0).all()                                               # the zero-intensity lamp is read; the setter gives it probability 0
    s = ptx.Scene.load_gltf(None, LAMPS)
    assert s.info()["has_sun"] == 1 and len(s.array(ptx.ARR_PUNCTUAL)) == 0          # the loader keeps the sun and picks no lamp up
    s.set_punctual_lights(got)
    cdf = s.array(ptx.ARR_PUNCTUAL_CDF)
    assert len(cdf) == 4 and cdf[3] == cdf[2] == 1


def test_reader_count_only_small_buffer_and_missing_file(ptx, tmp_path):
    L = ptx.lib()
    assert L.ptx_gltf_read_punctual_lights(os.fsencode(LAMPS), None, 0) == 4
    buf = np.full(70, 7, f32)
    assert L.ptx_gltf_read_punctual_lights(os.fsencode(LAMPS), buf.ctypes.data, 63) == -ptx.ERR_INVALID and (buf == 7).all()
    assert L.ptx_gltf_read_punctual_lights(os.fsencode(LAMPS), buf.ctypes.data, 64) == 4 and (buf[64:] == 7).all() and buf[7] == 0
    assert L.ptx_gltf_read_punctual_lights(os.fsencode(str(tmp_path / "none.gltf")), None, 0) == -ptx.ERR_IO
    assert L.ptx_gltf_read_punctual_lights(None, None, 0) == -ptx.ERR_INVALID
    (tmp_path / "broken.gltf").write_text("{ \"scenes\": [")
    assert L.ptx_gltf_read_punctual_lights(os.fsencode(str(tmp_path / "broken.gltf")), None, 0) == -ptx.ERR_PARSE
    with pytest.raises(ptx.PtxError):
        ptx.read_punctual_lights(str(tmp_path / "none.gltf"))
    (tmp_path / "plain.gltf").write_text(json.dumps({"asset": {"version": "2.0"}, "scenes": [{"nodes": []}], "nodes": []}))
    assert ptx.read_punctual_lights(str(tmp_path / "plain.gltf")).shape == (0, 16)     # a file without the extension has no lamps


# ---------------------------------------------------------------------------- the estimator on the restatement
def _same(a, b, what):
    np.testing.assert_array_equal(_bits(a), _bits(b), err_msg=what)


@pytest.mark.parametrize("name,M", [("cornell", 1), ("cornell", 4), ("chart", 2)])
def test_without_lights_the_restatement_is_the_one_it_extends(ora, name, M):
    """punctual=None, an empty array and all-black lights: the frame and counts without the argument bit for bit, on scenes of the existing tests"""
    o, a = _oracle(ora, name)
    W, H, spp, b = 16, 12, 2, 3
    want = render_samples(ora, o, a, W, H, spp, b, M=M, seed=SEED)
    black = np.stack([_lamp(intensity=(0, 0, 0))])
    for tag, lights in (("None", None), ("empty", np.zeros((0, 16), f32)), ("black", black)):
        got = render_samples(ora, o, a, W, H, spp, b, M=M, seed=SEED, punctual=lights)
        _same(got["rad"], want["rad"], f"{name} M = {M}: {tag}")
        assert all(got[k] == want[k] for k in ("light_samples", "light_visible", "rays")), (tag, got, want)
    assert want["light_samples"] > 0


# the narrow camera straight below lamp 0: 0.9 above the floor, a field of 0.05 rad, so the patch seen is +-0.023 wide 2 below the lamp:
# 1 - cos <= (0.033 / 2)^2 / 2 = 1.4e-4, the stand-in's cosine error there
STAND_IN_LEG = 0.04      # a right triangle with legs of 0.04 at distance 2: its solid-angle error against a point is of the order (0.04 / 2)^2 / 4 = 1e-4
EXP_W, EXP_H, EXP_B = 12, 8, 2


def _narrow(d, lamp):
    d = dict(d)
    x, _, z = (float(v) for v in lamp[0:3])
    d["camera"] = np.array([x, 0.9, z, 1, 0, 0, 0, 0, -1, 0, 1, 0, 0.05], f32)      # -z of the camera points down
    return d


def _with_stand_in(d, lamp, leg):
    """the scene plus a small emissive triangle centred on the lamp, facing down, with Le * area = the lamp's intensity"""
    d = dict(d)
    x, y, z = (float(v) for v in lamp[0:3])
    x0, z0 = x - leg / 3, z - leg / 3
    v = np.zeros((3, 11), f32)
    v[:, 0:3] = [[x0, y, z0], [x0 + leg, y, z0], [x0, y, z0 + leg]]
    v[:, 5:8] = [0, -1, 0]
    v[:, 8:11] = [1, 0, 0]
    area = 0.5 * leg * leg
    mat = np.array([0, 0, 0, 1.0, 1.0, 0.0, *(lamp[8:11].astype(np.float64) / (10.0 * area)), 1.33, 0], f32)   # Le = 10 * emissive
    nv, nt, ns = len(d["vertices"]), len(d["triangles"]), len(d["materials"])
    d["vertices"] = np.concatenate([d["vertices"], v])
    d["triangles"] = np.concatenate([d["triangles"], np.array([[0, 1, 2]], np.uint32)])
    d["surf_range"] = np.concatenate([d["surf_range"], np.array([[nv, 3, nt, 1]], np.int32)])
    d["materials"] = np.concatenate([d["materials"], mat[None]])
    d["model_surf"] = np.array([[0, ns + 1]], np.int32)
    return d


_cases = {}


def _case(ptx, ora, name):
    """name -> (oracle scene with the lamp's geometry only, oracle scene with the stand-in, its half-size twin, lights, table or None, flags)"""
    if name not in _cases:
        d, lights = _proc().lamp_scene(1, emitters=name == "emitter", blocker=False)
        d = _narrow(d, lights[0])
        scenes = [oracle_from_dict(ora, d), oracle_from_dict(ora, _with_stand_in(d, lights[0], STAND_IN_LEG)),
                  oracle_from_dict(ora, _with_stand_in(d, lights[0], STAND_IN_LEG / 2))]
        tab = None
        if name == "map":
            for o in scenes:
                o.set_environment(SKY, srgb=False)
            s = product_from_dict(ptx, None, d)
            s.set_environment(SKY, srgb=False)
            tab = _table(ptx, s)
        _cases[name] = (*scenes, lights, tab)
    return _cases[name]


def _batches(render, seed0, K=K_BATCH, spp=32):
    return _batch_stat(np.stack([render(seed0 + k, spp)["rad"].mean(2) for k in range(K)]))


_stand_in_batches = {}


def _stand_in(ptx, ora, name, half=False):
    """the batches of the stand-in scene on the existing estimator, computed once and left unchanged"""
    if (name, half) not in _stand_in_batches:
        _, full, small, _, tab = _case(ptx, ora, name)
        o = small if half else full
        ref = _batches(lambda seed, spp: render_samples(ora, o, o.a, EXP_W, EXP_H, spp, EXP_B, tab=tab, seed=seed), 0xB000)
        ref.setflags(write=False)
        _stand_in_batches[(name, half)] = ref
    return _stand_in_batches[(name, half)]


def _punctual_batches(ptx, ora, name, M=1, wrong=()):
    o, _, _, lights, tab = _case(ptx, ora, name)
    return _batches(lambda seed, spp: render_samples(ora, o, o.a, EXP_W, EXP_H, spp, EXP_B, tab=tab, M=M, seed=seed, punctual=lights, wrong=wrong), 0xA000)


@pytest.mark.parametrize("name", ["bare", "emitter", "map"])
def test_point_light_has_the_expectation_of_its_stand_in(ptx, ora, name):
    """16 batches of 32 spp of the point-light restatement against 16 of the stand-in on the existing restatement, _nee_common's statistic
    with its thresholds: the bare floor (c_p = 1), the floor with an emitter (c_p = 0.5), under the sky map with PTX_NEE_ENV_SAMPLES
    (c_p = 0.5, c_env = 1 against the stand-in's c_env = 0.5). The stand-in at half its size gives the same answer: its solid-angle error is
    below the statistic's resolution.
    Measured, worst z frame / quadrant at leg 0.04, then at 0.02: bare 0.75 / 1.51, 0.33 / 1.31; emitter 1.67 / 1.14, 0.40 / 0.83; map
    0.29 / 0.69 twice."""
    got = _punctual_batches(ptx, ora, name)
    assert got[:, 0].mean() > 0
    for half in (False, True):
        ok, zf, zq = _same_expectation(got, _stand_in(ptx, ora, name, half))
        print(f"{name}, stand-in leg {STAND_IN_LEG / (2 if half else 1)}: worst z frame {zf:.2f} quadrant {zq:.2f}; frame mean {got[:, 0].mean(0)}")
        assert ok, (name, half, zf, zq)


@pytest.mark.parametrize("wrong,name", [("forget_bsdf_side", "map"), ("forget_cp", "emitter"), ("forget_cp", "map")])
def test_the_statistic_can_tell(ptx, ora, wrong, name):
    """(1 - c_p) left out of the BSDF-side weights (the miss weight then takes too little of the map), and 1 / c_p left out of x (half the
    lamp): both fail the statistic the right form passes, on the scenes where c_p = 0.5.
    Measured, worst z frame / quadrant: forget_bsdf_side under the map 5.57 / 3.60; forget_cp with the emitter 14.96 / 8.42, under the map
    7.28 / 4.44 (the right form: 0.29 - 1.67 / 0.69 - 1.51)."""
    got = _punctual_batches(ptx, ora, name, wrong=(wrong,))
    ok, zf, zq = _same_expectation(got, _stand_in(ptx, ora, name))
    print(f"{wrong} on {name}: worst z frame {zf:.2f} quadrant {zq:.2f}")
    assert not ok, (zf, zq)


def test_candidates_same_expectation_and_no_more_variance_on_many_lamps(ora):
    """64 lamps of intensities spread over a decade, half of them spots, above the floor with its blocker (c_p = 1): M = 4 has the expectation
    of M = 1 (other seeds) and a per-pixel sample variance that is not larger.
    Measured: worst z 0.92 / 1.53; variance ratio 0.678; light samples 9296 against 5230."""
    d, lights = _proc().lamp_scene(64, spots=True)
    o = oracle_from_dict(ora, d)
    W, H, b = 24, 16, 3

    def render(M):
        return lambda seed, spp: render_samples(ora, o, o.a, W, H, spp, b, M=M, seed=seed, punctual=lights)
    ok, zf, zq = _same_expectation(_batches(render(4), 0xA000), _batches(render(1), 0xB000))
    print(f"64 lamps, M = 4 against M = 1: worst z frame {zf:.2f} quadrant {zq:.2f}")
    assert ok, (zf, zq)
    r = {M: render(M)(SEED, 32) for M in (1, 4)}
    ratio = float(r[4]["rad"].var(2, ddof=1, dtype=np.float64).mean() / r[1]["rad"].var(2, ddof=1, dtype=np.float64).mean())
    print(f"per-pixel sample variance M = 4 / M = 1: {ratio:.4f}; light samples {r[4]['light_samples']} against {r[1]['light_samples']}")
    assert ratio <= 1 and r[4]["light_samples"] >= r[1]["light_samples"] > 0
