"""The yardstick's own yardstick: tests/_nee_estimator.py against the recorded results of the five estimator restatements it replaced.

tests/golden/nee_restatement_bits.npz holds, for a matrix of cases, what _nee_restatement, _nee_env_restatement, _nee_pdf_restatement,
_nee_ris_restatement and _nee_punctual_restatement's render_samples returned at the commit named in its `provenance`: the radiance as uint32
bit patterns, the integer counts, v1_listed, the light_draws log and the first_env arrays, where the function had them. `cases` names each
case's arguments (JSON): scene, map, whether the map's table is given, the lamps, the keywords of _nee_estimator.render_samples, and `via`,
the function that was recorded. Every case is 16 x 12 pixels, 2 spp, 3 bounces. A case recorded via several functions is one on which they agreed.

The matrix reaches every keyword with a non-default value and every wrong form, on scenes with and without a sun, with lit shadow catchers
(plaza, chart_alpha_sun), pass-through (glass40, cloud), textures (lit), a map without a table, a map with a table with and without listed
triangles, lamps alone (c_p = 1) and lamps with emitters and a map (c_p = 0.5); where a strategy is possible its count is above zero.
"""
import json
import os

import numpy as np
import pytest

import _nee_estimator as NE
from _common import _bits, _proc
from _nee_lit_scenes import ENV, _oracle_and_table, _table
from _nee_lit_scenes import maps  # noqa: F401  (fixture)
from conftest import GOLD, oracle_from_dict, product_from_dict

f32 = np.float32
W, H, SPP, BOUNCES = 16, 12, 2, 3
FIXTURE = np.load(os.path.join(GOLD, "nee_restatement_bits.npz"))
CASES = [json.loads(s) for s in FIXTURE["cases"]]
COUNTS = ("rays", "light_samples", "light_visible", "env_samples", "env_rejected_box")
LAMP_SCENES = {"lamp1": dict(n_lamps=1), "lamp1_range": dict(n_lamps=1, lamp_range=2.6), "lamp64": dict(n_lamps=64, spots=True),
               "lamp8_emit": dict(n_lamps=8, emitters=True, spots=True)}   # procedural.lamp_scene's arguments
_lamp_scenes = {}


def _scene_of(ptx, ora, maps, c):
    """-> (oracle scene under the case's map, the map's table or None, the lamps or None)"""
    name, map_name = c["scene"], c["map"]
    if name in LAMP_SCENES:
        key = (name, map_name, c["tab"])
        if key not in _lamp_scenes:
            d, own = _proc().lamp_scene(**LAMP_SCENES[name])
            o, tab = oracle_from_dict(ora, d), None
            if map_name:
                o.set_environment(maps[map_name][0], srgb=maps[map_name][1])
            if c["tab"]:
                s = product_from_dict(ptx, None, d)
                s.set_environment(maps[map_name][0], srgb=maps[map_name][1])
                tab = _table(ptx, s)
            _lamp_scenes[key] = (o, tab, own)
        o, tab, own = _lamp_scenes[key]
    else:
        o, tab = _oracle_and_table(ptx, ora, maps, name, map_name, ENV if c["tab"] else 0)
        own = None
    lamps = {None: None, "empty": np.zeros((0, 16), f32), "black": np.zeros((1, 16), f32), "scene": own}[c["lamps"]]
    return o, tab, lamps


@pytest.mark.parametrize("i", range(len(CASES)), ids=[f"{c['scene']}-{c['map']}-{c['via']}-{k}" for k, c in enumerate(CASES)])
def test_the_estimator_gives_the_recorded_bits(ptx, ora, maps, i):
    """bit equality of the radiance, equality of every count and log that the recorded function returned"""
    c = CASES[i]
    o, tab, lamps = _scene_of(ptx, ora, maps, c)
    log, first = [] if c["log"] else None, {} if c["first"] else None
    got = NE.render_samples(ora, o, o.a, W, H, SPP, BOUNCES, tab=tab, punctual=lamps, light_draws=log, first_env=first, **c["kw"])
    np.testing.assert_array_equal(_bits(got["rad"]), FIXTURE[f"{i}/rad"], err_msg=str(c))
    for k in COUNTS:
        if f"{i}/{k}" in FIXTURE:
            assert got[k] == int(FIXTURE[f"{i}/{k}"]), (k, got[k], int(FIXTURE[f"{i}/{k}"]), c)
    if f"{i}/v1_listed" in FIXTURE:
        np.testing.assert_array_equal(got["v1_listed"], FIXTURE[f"{i}/v1_listed"])
    if c["log"]:
        assert [len(r) for r in log] == list(FIXTURE[f"{i}/light_draws_rounds"])
        np.testing.assert_array_equal(np.concatenate(log), FIXTURE[f"{i}/light_draws"])
    if c["first"]:
        assert len(first["ids"]) > 0
        np.testing.assert_array_equal(first["ids"], FIXTURE[f"{i}/first_ids"])
        np.testing.assert_array_equal(first["visible"], FIXTURE[f"{i}/first_visible"])
        for k in ("wdir", "x"):
            np.testing.assert_array_equal(_bits(first[k]), FIXTURE[f"{i}/first_{k}"])


def test_the_matrix_reaches_every_switch():
    """every keyword with a value that is not its default, every wrong form, every kind of lamps, every recorded function"""
    kws = [c["kw"] for c in CASES]
    for k in ("tile", "sample0", "env", "seed"):
        assert any(k in kw for kw in kws), k
    assert any(kw.get("lights") is False for kw in kws) and any(kw.get("fold") == "recursive" for kw in kws) and any(kw.get("spdf") for kw in kws)
    assert {2, 4, 16} <= {kw.get("M") for kw in kws}
    assert {w for kw in kws for w in kw.get("wrong", ())} == set(NE.WRONG)
    assert {c["lamps"] for c in CASES} == {None, "empty", "black", "scene"} and {c["scene"] for c in CASES} >= set(LAMP_SCENES)
    assert any(c["log"] for c in CASES) and any(c["first"] for c in CASES)
    assert any(c["map"] and not c["tab"] for c in CASES) and any(c["tab"] and c["kw"].get("lights") is False for c in CASES)
    assert {c["via"] for c in CASES} == {"R", "E", "P", "RIS", "PU"}
