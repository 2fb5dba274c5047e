"""ptx_render_nee on textured emitters and on long light lists, in both forms (nee.hip's rounds and PTX_NEE_FUSED's k_nee_fused).

Two scenes carry it:
  lit.gltf (tests/golden/textures/, oracle/make_golden.py --only-lit-textures): one mesh of textured quads instanced by two nodes that face
      each other, the second turned half round and scaled (1.3, 0.8, 1). Listed emitters: an 8-bit palette emissive with a normal map, the float
      sRGB .hdr emissive, a factor-only one, and an RGB emissive whose columns 0-5 are solid black (Le = 0: the light sample is rejected);
      a BLEND emitter whose opacity comes from a texture stays off the list. uvs run outside [0, 1]; an opaque quad and the BLEND quads stand
      between the instances; light 0 is a sun. Four loads (sun or NO_SUN_LIGHT, every primitive or the opaque ones through `work`) give the four
      (TEX, ALPHA, SUN) = (T, ., .) kernels.
  procedural.emitter_cloud_scene: 64 surfaces under four rotated, non-uniformly scaled models, 18 emissive surfaces spread over surface ids
      0 ... 62 (271 listed triangles, one collapsed triangle left out, one half-transparent emitter left out). Its four (sun, alpha)
      combinations give the four (F, ., .) kernels.
The yardstick is tests/_nee_estimator.py on tests/_nee_restatement.py (pinned here, on these scenes and under an environment map, to OracleScene.render_samples bit for
bit). Bars are the project's: test_gpu_parity's per-sample bar (_nee_common._err), bitwise equality between the two forms and between routes.

Without a GPU: the fixtures' light lists, kernel triples and sample statistics, the pin, the host-only light arrays.
On the GPU: A per-sample radiance against the restatement, B every variant of k_nee_fused against the unflagged form bit for bit, C the routes
against each other with a non-empty list, D the first light sample bit for bit, E pass-through layers and the 4096 bound.
"""
import json
import os

import numpy as np
import pytest

import _nee_restatement as R
from _common import _bits, _proc
from _nee_common import SAME_STATS, SEED, _check_list, _err, _pair
from _nee_estimator import render_samples
from _nee_lit_scenes import CLOUDS, LIT, LIT_LOADS, LIT_OPAQUE, LIT_PRIMS, SKY, _dict, _host_scene, _hybrid_budget, _oracle, f32
from _routes import clean_env, ctx  # noqa: F401  (fixtures)
from _routes import DEFAULT_ROUTES, ROUTE_VARS, Route, Scenes, on_route, route_named, under_force_global
from conftest import GOLD, oracle_from_dict

LIT_EMITTERS = LIT_PRIMS[:4]
SIZE = {**{n: (48, 32) for n in LIT_LOADS}, **{n: (64, 36) for n in CLOUDS}, "chart_env": (48, 40), "glass40": (24, 16), "glass4200": (4, 3)}
# what each scene's kernels are compiled with: (TEX, ALPHA, SUN)
TRIPLES = {"lit": (True, True, True), "lit_nosun": (True, True, False), "lit_opaque": (True, False, True), "lit_opaque_nosun": (True, False, False),
           "lit_first": (True, False, False), "cloud": (False, True, True), "cloud_nosun": (False, True, False), "cloud_opaque": (False, False, True),
           "cloud_opaque_nosun": (False, False, False), "chart_env": (True, False, False), "glass40": (False, True, False), "glass4200": (False, True, False)}


def _triple(ptx, s, env=False):
    """(TEX, ALPHA, SUN) of a scene from its arrays and scene_build.cpp's rule: a texture in any slot (or an environment map) sets TEX; an
    opacity that is not approximately 1, an opacity texture or a shadow catcher sets ALPHA; a sun sets SUN."""
    mats, tex, sun = s.array(ptx.ARR_MATERIALS).reshape(-1, 11), s.array(ptx.ARR_SURF_TEX).reshape(-1, 7), s.array(ptx.ARR_SUN)
    op = mats[:, 3]
    alpha = bool((~((op == f32(1)) | (np.abs(op - f32(1)) < f32(0.0001)))).any() or (mats[:, 10] != 0).any() or (tex[:, 2] >= 0).any())
    return bool((tex >= 0).any() or env), alpha, len(sun) > 0


def _lit_names(a, work):
    """per surface of a lit.gltf load: 'node/primitive'"""
    keep = LIT_PRIMS if work is None else [LIT_PRIMS[k] for k in work["lit"]]
    assert len(a.materials) == len(a.model_names) * len(keep)
    return [f"{m}/{p}" for m in a.model_names for p in keep]


def _world_tris(a, tris):
    """float64 world corners [n, 3, 3] of (surface, triangle) rows, from the arrays alone"""
    model_of = np.zeros(len(a.surf_range), np.int64)
    for m, (first, cnt) in enumerate(np.asarray(a.model_surf)):
        model_of[first:first + cnt] = m
    out = np.zeros((len(tris), 3, 3))
    for i, (s, t) in enumerate(np.asarray(tris, np.int64)):
        X = np.asarray(a.model_xform, np.float64)[model_of[s]]
        basis, origin = X[3:].reshape(3, 3).T, X[:3]
        v0, _, t0, _ = (int(x) for x in np.asarray(a.surf_range)[s][:4])
        out[i] = np.asarray(a.vertices, np.float64)[v0 + np.asarray(a.triangles[t0 + t], np.int64), :3] @ basis.T + origin
    return out


def _check_world_geometry(a, ll):
    """area and unit normal of every listed triangle against a float64 computation in world space"""
    P = _world_tris(a, ll["tris"])
    cr = np.cross(P[:, 1] - P[:, 0], P[:, 2] - P[:, 0])
    ln = np.linalg.norm(cr, axis=1)
    np.testing.assert_allclose(ll["geom"][:, 3], 0.5 * ln, rtol=1e-5)
    np.testing.assert_allclose(ll["geom"][:, :3], cr / ln[:, None], atol=1e-5)


# ---------------------------------------------------------------------------- no GPU: the fixtures deliver what they claim
def test_lit_fixture_is_what_the_generator_writes(tmp_path, monkeypatch):
    """oracle/make_golden.py --only-lit-textures rewrites lit.gltf and lit.bin byte for byte and black_8x8.png pixel for pixel, from the
    committed images alone."""
    from PIL import Image
    import oracle.make_golden as mg
    tex = os.path.join(GOLD, "textures")
    mine = ("lit.gltf", "lit.bin", mg.LIT_BLACK)
    for n in os.listdir(tex):
        if n not in mine:
            os.symlink(os.path.join(tex, n), tmp_path / n)
    monkeypatch.setattr(mg, "TEX_DIR", str(tmp_path))
    monkeypatch.setattr(mg, "LIT_GLTF", str(tmp_path / "lit.gltf"))
    mg.write_lit_texture_scene()
    for n in mine[:2]:
        assert (tmp_path / n).read_bytes() == open(os.path.join(tex, n), "rb").read(), n
    black = np.asarray(Image.open(os.path.join(tex, mg.LIT_BLACK)))
    np.testing.assert_array_equal(np.asarray(Image.open(tmp_path / mg.LIT_BLACK)), black)
    assert black.shape == (8, 8, 3) and (black[:, :6] == 0).all() and (black[:, 6:] > 0).all() and os.path.getsize(os.path.join(tex, mg.LIT_BLACK)) < 1024
    with open(LIT) as fh:
        g = json.load(fh)
    assert [g["materials"][p["material"]]["name"] for p in g["meshes"][0]["primitives"]] == LIT_PRIMS and mg.LIT_OPAQUE == LIT_OPAQUE
    assert g["extensions"]["KHR_lights_punctual"]["lights"][0]["type"] == "directional"


@pytest.mark.parametrize("name", ["lit", "lit_nosun", "lit_opaque", "lit_opaque_nosun", "lit_first"])
def test_lit_light_list(ora, name):
    _, a = _oracle(ora, name)
    names = _lit_names(a, LIT_LOADS[name][1])
    ll = R.light_list(a)
    _check_list(ll, len(names))
    _check_world_geometry(a, ll)
    listed = {names[k] for k in set(ll["tris"][:, 0].tolist())}
    want = {f"{m}/{p}" for m in ("lit_a", "lit_b") for p in LIT_EMITTERS if not (name == "lit_first" and p == "emit_hdr_srgb")}
    assert listed == want and len(ll["cdf"]) == 2 * len(want)
    assert sorted(a.model_names) == ["lit_a", "lit_b"]
    X = np.asarray(a.model_xform, np.float64)[a.model_names.index("lit_b")]
    basis = X[3:].reshape(3, 3).T
    np.testing.assert_allclose(basis, np.diag([-1.3, 0.8, -1.0]), atol=1e-6)   # half a turn about Y, scaled (1.3, 0.8, 1)
    for k, (s, _) in enumerate(ll["tris"]):                                     # world normals and world areas
        b = names[s].startswith("lit_b")
        np.testing.assert_allclose(ll["geom"][k], [0, 0, -1 if b else 1, 0.98 * (1.04 if b else 1.0)], atol=1e-5)
    mats, tex = np.asarray(a.materials, f32), np.asarray(a.surf_tex)
    for s, n in enumerate(names):
        p = n.split("/")[1]
        if p in LIT_EMITTERS:
            assert (tex[s, 6] >= 0) == (p != "emit_factor") and (tex[s, 0] >= 0) == (p == "emit_palette_normal")
            if tex[s, 6] >= 0:
                assert a.images[tex[s, 6]].dtype == (np.float32 if p == "emit_hdr_srgb" else np.uint8) and a.image_srgb[tex[s, 6]]
        if p == "blend_emissive_alpha_tex":      # emissive, opacity from a texture: must stay unlisted
            assert (mats[s, 6:9] > 0).all() and tex[s, 2] >= 0 and n not in listed
    if LIT_LOADS[name][1] is None:
        assert {"lit_a/blend_emissive_alpha_tex", "lit_b/blend_emissive_alpha_tex"} <= set(names)
    v = np.asarray(a.vertices, f32)
    assert v[:, 3:5].min() < -2 and v[:, 3:5].max() > 3                          # uvs outside [0, 1]


@pytest.mark.parametrize("name", sorted(CLOUDS))
def test_cloud_light_list(ora, name):
    d = _dict(name)
    _, a = _oracle(ora, name)
    ll = R.light_list(a)
    _check_list(ll, 64)
    _check_world_geometry(a, ll)
    assert len(d["materials"]) == 64 and len(d["model_xform"]) == 4
    emissive = set(np.flatnonzero((d["materials"][:, 6:9] > 0).any(1)).tolist())
    assert emissive == set(d["emissive"].tolist()) == {u for u in range(63) if u % 4 == 1} | {0, 62}
    assert (d["materials"][5, 6:9] > 0).sum() == 1
    unlisted = {9} if CLOUDS[name][1] else set()
    assert set(d["unlisted"].tolist()) == unlisted and d["materials"][9, 3] == (0.5 if unlisted else 1.0)
    assert set(ll["tris"][:, 0].tolist()) == emissive - unlisted
    rows = {tuple(r) for r in ll["tris"].tolist()}
    assert d["collapsed"] == (1, 5) and (1, 5) not in rows and {(1, 4), (1, 6)} <= rows     # the gap at the zero-area triangle
    assert len(ll["cdf"]) == 16 * len(emissive - unlisted) - 1
    assert (ll["surf_first"][sorted(emissive - unlisted)] >= 0).all() and (np.delete(ll["surf_first"], sorted(emissive - unlisted)) == -1).all()
    for X in np.asarray(d["model_xform"], np.float64):                              # every model rotated and non-uniformly scaled
        basis = X[3:].reshape(3, 3).T
        sc = np.linalg.norm(basis, axis=0)
        assert sc.max() / sc.min() > 1.05 and np.abs(basis / sc - np.eye(3)).max() > 0.1
    base = _proc().cloud_scene(3, 21, 16, layout="scattered", tri_size=0.15)       # the wrapped generator's surfaces, untouched but for one corner
    nv = len(base["vertices"])
    same = np.ones(nv, bool)
    same[d["surf_range"][1][0] + d["triangles"][d["surf_range"][1][2] + 5][2]] = False
    np.testing.assert_array_equal(_bits(d["vertices"][:nv][same]), _bits(base["vertices"][same]))
    np.testing.assert_array_equal(d["triangles"][:len(base["triangles"])], base["triangles"])
    if CLOUDS[name][0]:
        np.testing.assert_array_equal(_bits(d["sun"]), _bits(base["sun"]))
    else:
        assert d["sun"] is None


def test_four_loads_give_the_four_triples(ptx):
    got = {n: _triple(ptx, _host_scene(ptx, n), env=n == "chart_env") for n in TRIPLES}
    assert got == TRIPLES
    for family, tex in ((("lit", "lit_nosun", "lit_opaque", "lit_opaque_nosun"), True), (sorted(CLOUDS), False)):
        assert {got[n] for n in family} == {(tex, a, s) for a in (False, True) for s in (False, True)}
    assert _host_scene(ptx, "lit").info()["n_textures"] > 0 and _host_scene(ptx, "cloud").info()["n_textures"] == 0


A_SCENES = ["lit", "lit_opaque_nosun", "cloud_nosun", "cloud_opaque", "chart_env"]
_refs = {}


def _ref(ora, name, **kw):
    """the restatement at A's size (2 spp, 4 bounces), computed once"""
    key = (name, tuple(sorted(kw.items())))
    if key not in _refs:
        o, a = _oracle(ora, name)
        log = []
        _refs[key] = render_samples(ora, o, a, *SIZE[name], 2, 4, seed=SEED, light_draws=log, **kw)
        _refs[key]["draw_keys"] = np.concatenate(log) if log else np.zeros((0, 4), np.uint32)
    return _refs[key]


def _restated_draws(ora, name, keys):
    """draw -> triangle -> (beta, gamma) -> material, from the Philox keys of the vertices that drew: (surface per draw, Le per draw)"""
    o, a = _oracle(ora, name)
    ll = R.light_list(a)
    r = R.draws(ora, keys[:, 0], keys[:, 1], keys[:, 2].astype(np.int64), keys[:, 3].astype(np.int64), R.BLOCK_LIGHT, SEED)
    k = np.minimum(np.searchsorted(ll["cdf"], r[:, 0], side="right"), len(ll["cdf"]) - 1)
    su = np.sqrt(r[:, 1])
    beta, gamma = su * (f32(1) - r[:, 2]), su * r[:, 2]
    ls, lt = ll["tris"][k, 0].astype(np.int64), ll["tris"][k, 1].astype(np.int64)
    _, uv, _, _ = R._Attr(a).at(ls, lt, beta, gamma)
    return ls, R._material(o, ls, uv)[:, 9:12] * f32(10)


@pytest.mark.parametrize("name", A_SCENES[:4])
def test_the_restatement_exercises_the_lists_at_the_gpu_sizes(ora, name):
    ref = _ref(ora, name)
    o, a = _oracle(ora, name)
    surf, Le = _restated_draws(ora, name, ref["draw_keys"])
    listed = sorted(set(R.light_list(a)["tris"][:, 0].tolist()))
    per_surface = {s: int((surf == s).sum()) for s in listed}
    black = int((Le.max(1) == 0).sum())
    share = ref["light_visible"] / ref["light_samples"]
    off = (ref["rad"] != _ref(ora, name, lights=False)["rad"]).any(-1).mean()
    print(f"{name}: {len(surf)} light draws, {ref['light_samples']} light samples, visible share {share:.3f}, least chosen surface {min(per_surface.values())} times, "
          f"Le == 0 on {black} draws, {off * 100:.1f} % of samples differ from the empty-list run, vertex 1 listed on {ref['v1_listed'].mean() * 100:.1f} %")
    assert ref["light_samples"] >= 1000 and 0.2 <= share <= 0.9
    assert min(per_surface.values()) >= 20, per_surface
    if name.startswith("lit"):
        assert black >= 50
        names = _lit_names(a, LIT_LOADS[name][1])
        assert {names[s].split("/")[1] for s in surf[Le.max(1) == 0]} == {"emit_black_region"}
    else:
        assert black == 0


@pytest.mark.parametrize("name", ["lit", "cloud", "chart_env"])
def test_restatement_without_lights_is_the_pinned_oracle(ora, name):
    """on the new scenes and under an environment map (OracleScene.env_lookup on a miss): bit for bit"""
    o, a = _oracle(ora, name)
    W, H = SIZE[name]
    ref = o.render_samples(ora.make_cfg(W, H, 2, 4, seed=SEED), threads=0)
    got = render_samples(ora, o, a, W, H, 2, 4, seed=SEED, lights=False, fold="recursive")["rad"]
    np.testing.assert_array_equal(_bits(got), _bits(ref))
    if name == "chart_env":      # the map is in use: the frame is not the constant environment's, and a scaled factor scales the misses
        flat = render_samples(ora, oracle_from_dict(ora, _dict(name)), a, W, H, 2, 4, seed=SEED, lights=False)["rad"]
        assert (_bits(flat) != _bits(got)).any(-1).mean() > 0.05
        ref = o.render_samples(ora.make_cfg(W, H, 2, 4, env=(0.5, 1.25, 2.0), seed=SEED), threads=0)
        got = render_samples(ora, o, a, W, H, 2, 4, seed=SEED, env=(0.5, 1.25, 2.0), lights=False, fold="recursive")["rad"]
        np.testing.assert_array_equal(_bits(got), _bits(ref))


@pytest.mark.parametrize("name", ["lit", "lit_nosun", "lit_opaque", "lit_opaque_nosun", "lit_first"] + sorted(CLOUDS) + ["glass40"])
def test_host_only_light_arrays(ptx, ora, name):
    _, a = _oracle(ora, name)
    ll = R.light_list(a)
    s = _host_scene(ptx, name)
    np.testing.assert_array_equal(s.array(ptx.ARR_LIGHT_TRIS).reshape(-1, 2), ll["tris"])
    np.testing.assert_array_equal(_bits(s.array(ptx.ARR_LIGHT_CDF)), _bits(ll["cdf"]))
    np.testing.assert_array_equal(_bits(s.array(ptx.ARR_LIGHT_GEOM).reshape(-1, 4)), _bits(ll["geom"]))
    assert len(ll["cdf"]) > 0


@pytest.mark.parametrize("name", ["lit", "lit_nosun", "lit_opaque", "lit_opaque_nosun"] + sorted(CLOUDS))
def test_the_hybrid_budget_leaves_some_surface_in_global_memory(ptx, monkeypatch, name):
    full = _host_scene(ptx, name)
    assert full.info()["lds_resident"] == 1
    monkeypatch.setenv("PTX_LDS_BUDGET", str(_hybrid_budget(ptx, monkeypatch, name)))
    s = _host_scene(ptx, name)
    n_res, n_surf = int(s.array(ptx.ARR_RES_PLAN)[1]), s.info()["n_surfaces"]
    assert s.info()["lds_resident"] == 2 and 0 < n_res < n_surf
    assert ((s.array(ptx.ARR_LDS_ROOT) == 0xFFFFFFFF).sum()) == n_surf - n_res


# ---------------------------------------------------------------------------- GPU
HYBRID = Route("hybrid", None, {"PTX_WAVEFRONT": "0"}, 2, 0)   # created with PTX_LDS_BUDGET one byte short of the resident geometry; the fused kernel asked for at the call


def _make_hybrid(ptx, ctx, name):
    with pytest.MonkeyPatch.context() as mp:
        mp.setenv("PTX_LDS_BUDGET", str(_hybrid_budget(ptx, mp, name)))
        return _host_scene(ptx, name, ctx)


PRODUCTS, HYBRIDS = Scenes(lambda ptx, ctx, name: _host_scene(ptx, name, ctx)), Scenes(_make_hybrid)


def _route(ptx, ctx, mp, name, route):
    """the scene of `name` for one of the default-choice routes or HYBRID, with the route's switches set -> (scene, expected pipeline)"""
    r = HYBRID if route == "hybrid" else route_named(DEFAULT_ROUTES, route)
    for k in ROUTE_VARS:      # a scene of this module is created with no switch set but the one that makes it what it is
        mp.delenv(k, raising=False)
    s = on_route(HYBRIDS if r is HYBRID else PRODUCTS, ptx, ctx, mp, name, r)
    assert _triple(ptx, s, env=name == "chart_env") == TRIPLES[name]
    return s, r.pipeline


def _samples(ptx, ctx, s, name, spp, bounces, flags, pipeline, **kw):
    """per-sample radiance [H, W, spp, 3] from one call per sample, the route asserted on every call -> (radiance, summed stats)"""
    W, H = SIZE[name]
    out = np.zeros((H, W, spp, 3), f32)
    tot = dict(light_samples=0, light_visible=0, rays=0)
    for k in range(spp):
        acc, st = s.render_nee(W, H, 1, bounces, seed=SEED, sample0=k, flags=flags, **kw)
        tm = ctx.timing()
        assert tm["pipeline"] == pipeline and tm["fused_launches"] == (1 if flags & ptx.NEE_FUSED else 0), (name, tm)
        assert (acc[..., 3] == 1).all()
        out[:, :, k] = acc[..., :3]
        for key in tot:
            tot[key] += st[key]
    return out, tot


def _against_the_restatement(tag, got, tot, ref):
    """A's bar: every sample finite and >= 0, >= 99.5 % within 1e-3 relative (floor 1e-3), light_samples and rays within 0.5 % + 1"""
    assert np.isfinite(got).all() and (got >= 0).all()
    e = _err(got, ref["rad"])
    share = (e <= 1e-3).mean()
    print(f"{tag}: {share * 100:.3f} % of samples within 1e-3, worst {e.max():.3g}; light samples {tot['light_samples']} (restated {ref['light_samples']}), "
          f"visible {tot['light_visible']} (restated {ref['light_visible']}), rays {tot['rays']} (restated {ref['rays']})")
    assert ref["light_samples"] > 0 and share >= 0.995
    assert abs(tot["light_samples"] - ref["light_samples"]) <= 0.005 * ref["light_samples"] + 1
    assert abs(tot["rays"] - ref["rays"]) <= 0.005 * ref["rays"] + 1


@pytest.mark.gpu
@pytest.mark.parametrize("form", ["unflagged", "flagged"])
@pytest.mark.parametrize("name", A_SCENES)
def test_per_sample_radiance_against_the_restatement(ptx, ctx, ora, clean_env, name, form):
    """A. Unflagged on the route the scene gets by default (the fused kernel's for lit.gltf and the chart, which are LDS-resident), flagged on
    'lds fused': textured emitters with Le(uv), n_y of a normal-mapped emitter, the Le = 0 rejection, the unlisted BLEND emitter, a 271-entry
    list under rotated and scaled models, the environment lookup on a miss.
    Measured on the MI355X, the same in both forms: 100 % of samples within 1e-3 on all five; worst error lit 7.9e-04, lit_opaque_nosun
    5.4e-04, cloud_nosun 6.1e-06, cloud_opaque 1.9e-06, chart_env 1.8e-05; light samples, visible ones and rays equal to the restated counts
    (1240 / 845, 1232 / 851, 1755 / 672, 1745 / 670) except chart_env: 784 / 781 against 785 / 782 restated."""
    ref = _ref(ora, name)
    s, pipeline = _route(ptx, ctx, clean_env, name, "lds fused")     # no switch is set on this route: it is the default one
    flags = ptx.NEE_FUSED if form == "flagged" else 0
    got, tot = _samples(ptx, ctx, s, name, 2, 4, flags, pipeline)
    _against_the_restatement(f"{name}, {form}, lds_resident {s.info()['lds_resident']}, pipeline {pipeline}, (TEX, ALPHA, SUN) = {TRIPLES[name]}", got, tot, ref)


B_LOADS = ["lit", "lit_nosun", "lit_opaque", "lit_opaque_nosun"] + sorted(CLOUDS)


@pytest.mark.gpu
@pytest.mark.parametrize("route", ["lds fused", "global fused", "hybrid"])
@pytest.mark.parametrize("name", B_LOADS)
def test_every_variant_of_the_fused_form_bitwise(ptx, ctx, clean_env, name, route):
    """B. 8 loads x 3 routes = the 24 variants MODE x TEX x ALPHA x SUN of k_nee_fused, each against the unflagged call: bitwise equal frames,
    equal stats, one launch per pass (_nee_common._pair)."""
    s, pipeline = _route(ptx, ctx, clean_env, name, route)
    assert pipeline == 0
    _, st = _pair(ptx, ctx, s, *SIZE[name], 4, 4)
    print(f"{name} / {route}: (TEX, ALPHA, SUN) = {TRIPLES[name]}, lds_resident {s.info()['lds_resident']}, light samples {st['light_samples']}, visible {st['light_visible']}")
    assert st["light_samples"] > 0 and st["n_lights"] > 0


@pytest.mark.gpu
def test_an_environment_map_alone_selects_the_texture_variant_bitwise(ptx, ctx, clean_env):
    """B, the 25th pair: the chart has no material texture; the map makes any_texture true and the miss branch looks it up."""
    s, _ = _route(ptx, ctx, clean_env, "chart_env", "lds fused")
    assert not (s.array(ptx.ARR_SURF_TEX) >= 0).any()
    got, st = _pair(ptx, ctx, s, *SIZE["chart_env"], 4, 4)
    print(f"chart_env / lds fused: (TEX, ALPHA, SUN) = {TRIPLES['chart_env']}, light samples {st['light_samples']}, visible {st['light_visible']}")
    assert st["light_samples"] > 0
    s.set_environment(None)
    flat, _ = s.render_nee(*SIZE["chart_env"], 4, 4, seed=SEED, flags=ptx.NEE_FUSED)
    s.set_environment(SKY)
    assert (_bits(flat) != _bits(got)).any(-1).mean() > 0.05     # the map was in use


@pytest.mark.gpu
@pytest.mark.parametrize("name", ["lit", "cloud"])
def test_routes_against_each_other_with_a_list(ptx, ctx, clean_env, name):
    """C. The unflagged frames of 'lds fused', 'global fused' and 'queue' are bitwise equal and so are their stats: hit records are bit-equal
    across routes (tests/test_unit_limits.py) and the vertex is one function."""
    W, H = SIZE[name]
    frames = {}
    for route in (r.name for r in DEFAULT_ROUTES):
        s, pipeline = _route(ptx, ctx, clean_env, name, route)
        frames[route] = s.render_nee(W, H, 4, 4, seed=SEED)
        tm = ctx.timing()
        assert tm["pipeline"] == pipeline and tm["fused_launches"] == 0, (route, tm)
    want, st0 = frames["lds fused"]
    assert st0["light_samples"] > 0
    for route in ("global fused", "queue"):
        got, st = frames[route]
        np.testing.assert_array_equal(_bits(got), _bits(want), err_msg=f"{name}: {route} against lds fused")
        assert all(st[k] == st0[k] for k in SAME_STATS), (route, st, st0)


@pytest.mark.gpu
@pytest.mark.parametrize("name", ["lit", "cloud"])
def test_queue_route_with_a_forced_pool_overflow_against_the_other_routes(ptx, ctx, clean_env, name):
    """C, with test_nee's pool switches: a 1 Mi-pair pool and a guess of 0.25 pairs per ray. 800 x 600 x 4 camera rays enter more than
    2^20 (ray, surface) pairs, so the first slice overflows and is repeated smaller. The frame is the unforced queue frame and the
    'lds fused' frame, bit for bit."""
    W, H, spp, b = 800, 600, 4, 3
    s, _ = _route(ptx, ctx, clean_env, name, "lds fused")
    want, st0 = s.render_nee(W, H, spp, b, seed=SEED)
    assert ctx.timing()["pipeline"] == 0
    q, _ = _route(ptx, ctx, clean_env, name, "queue")
    unforced, st1 = q.render_nee(W, H, spp, b, seed=SEED)
    assert ctx.timing()["pipeline"] == 1 and ctx.timing()["pool_overflows"] == 0
    fresh = under_force_global(clean_env, True, lambda: _host_scene(ptx, name, ctx))   # no pairs-per-ray measurement yet: the guess below decides the first slice
    clean_env.setenv("PTX_WF_PAIRS_M", "1")
    clean_env.setenv("PTX_WF_RATIO_GUESS", "0.25")
    forced, st2 = fresh.render_nee(W, H, spp, b, seed=SEED)
    tm = ctx.timing()
    fresh.close()
    assert tm["pipeline"] == 1 and tm["pool_overflows"] >= 1, tm
    for tag, (got, st) in (("queue", (unforced, st1)), ("queue, forced overflow", (forced, st2))):
        np.testing.assert_array_equal(_bits(got), _bits(want), err_msg=f"{name}: {tag} against lds fused")
        assert all(st[k] == st0[k] for k in SAME_STATS), (tag, st, st0)
    assert st0["light_samples"] > 0


@pytest.mark.gpu
@pytest.mark.parametrize("name", ["cloud_opaque_nosun", "lit_first"])
def test_first_light_sample_bitwise(ptx, ctx, ora, clean_env, name):
    """D. test_nee.test_first_light_sample_bitwise's construction (2 bounces, black environment, no unlisted emitter, no sun) on the long list
    and on the textured emitters without the float sRGB one: of the samples whose vertex 1 is not on a listed triangle, <= 0.5 % differ.
    Measured on the MI355X: none differs (cloud 0 of 8819, 1269 of them not black; lit.gltf 0 of 5967, 945 not black)."""
    o, a = _oracle(ora, name)
    W, H = SIZE[name]
    ref = render_samples(ora, o, a, W, H, 4, 2, seed=SEED, env=(0.0, 0.0, 0.0))
    s, pipeline = _route(ptx, ctx, clean_env, name, "lds fused")
    got, tot = _samples(ptx, ctx, s, name, 4, 2, 0, pipeline, env=(0.0, 0.0, 0.0))
    sel = ~ref["v1_listed"]
    assert sel.mean() >= 0.5
    differ = (_bits(got) != _bits(ref["rad"])).any(-1) & sel
    lit = (ref["rad"] > 0).any(-1) & sel
    print(f"{name}: {differ.sum()} of {sel.sum()} comparable samples differ ({lit.sum()} of them not black); light samples {tot['light_samples']} "
          f"(restated {ref['light_samples']}), visible {tot['light_visible']} (restated {ref['light_visible']})")
    assert ref["light_visible"] > 0 and differ.sum() <= 0.005 * sel.sum()
    assert abs(tot["light_samples"] - ref["light_samples"]) <= 0.005 * ref["light_samples"] + 1
    assert tot["rays"] >= tot["light_samples"] and abs(tot["rays"] - ref["rays"]) <= 0.005 * ref["rays"] + 1


@pytest.mark.gpu
def test_forty_half_transparent_layers_before_a_listed_wall(ptx, ctx, ora, clean_env):
    """E. (TEX, ALPHA, SUN) = (F, T, F), one of the two 768-thread builds. Paths cross up to 40 layers at one depth; a light ray from layer
    k > 0 is stopped by the layer in front of it; a path that leaves a layer towards the wall arrives there with pass > 0 (w = 1)."""
    name = "glass40"
    ref = _ref(ora, name)
    assert 0 < ref["light_visible"] < ref["light_samples"]
    s, pipeline = _route(ptx, ctx, clean_env, name, "lds fused")
    for form, flags in (("unflagged", 0), ("flagged", ptx.NEE_FUSED)):
        got, tot = _samples(ptx, ctx, s, name, 2, 4, flags, pipeline)
        _against_the_restatement(f"{name}, {form}", got, tot, ref)
        assert tot["rays"] > 2.5 * got.shape[0] * got.shape[1] * 2      # pass-throughs are extra closest-hit queries
    _, st = _pair(ptx, ctx, s, *SIZE[name], 4, 4)
    assert st["light_samples"] > st["light_visible"] > 0


@pytest.mark.gpu
def test_pass_through_bound_under_nee(ptx, ctx, clean_env):
    """E. 4200 layers of opacity 0 and a listed wall no path reaches: every sample ends at the 4096 bound after exactly 4097 closest-hit
    queries, the frame is black with alpha = spp, in both forms and bit for bit (the stack does not fit LDS, the wall does: a hybrid scene. The
    unflagged call on the route it gets by default, then both forms under PTX_WAVEFRONT=0, where the flag is honoured)."""
    name = "glass4200"
    W, H = SIZE[name]
    s = PRODUCTS.get(ptx, ctx, clean_env, name)
    assert s.info()["lds_resident"] == 2 and _triple(ptx, s) == TRIPLES[name]

    def check(a, st):
        assert np.isfinite(a).all() and (a[..., :3] == 0).all() and (a[..., 3] == 2).all()
        assert st["rays"] == W * H * 2 * 4097 and st["n_lights"] == 2 and st["light_samples"] == 0
    a, st = s.render_nee(W, H, 2, 3, seed=SEED)
    assert ctx.timing()["fused_launches"] == 0
    check(a, st)
    clean_env.setenv("PTX_WAVEFRONT", "0")
    got, st = _pair(ptx, ctx, s, W, H, 2, 3)
    check(got, st)
    np.testing.assert_array_equal(_bits(got), _bits(a))
