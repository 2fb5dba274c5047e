"""The light tree over ptx_render_nee's light list (include/ptx.h: ptx_scene_set_light_pick, LIGHT PICK), without a GPU: the symbols, the
setter's refusals and the mode's lifetime on host-only scenes, the stored tree and path words against tests/_nee_light_tree_restatement.py
bit for bit, the restated pick's and directed pmf's own properties, the restated tree-mode vertex loop (pinned to tests/_nee_estimator.py
in CDF mode, its expectation against the CDF mode's, three wrong forms that must fail), and the variance ratio R0 that the GPU test's bar
is built on. Every test reaches the product: the tests of the restatement take their tree and path words from the library's host-only
scene (tree_of), so each fails on the parent for want of the symbols. GPU tests: tests/test_nee_light_tree_gpu.py.
"""
import ctypes as C
import inspect
import math

import numpy as np
import pytest

import _nee_light_tree_restatement as LT
from _common import _bits, _proc
from _nee_common import K_BATCH, SEED, _batch_stat, _same_expectation
from _nee_estimator import render_samples
from _nee_light_tree_scenes import TREE_CASES, host_scene, restated
from conftest import oracle_from_dict, product_from_dict

f32 = np.float32
_product_trees = {}


def tree_of(ptx, ora, name):
    """(oracle scene, arrays, light list, tree, path) of a case with the tree and the path words taken from the PRODUCT's host-only scene in
    tree mode (ARR_LIGHT_TREE, ARR_LIGHT_PATH), held equal to the numpy build and its list to the restated list: what the tests below walk,
    sample and render with is what the library stores. Read once per case and left unchanged."""
    if name not in _product_trees:
        o, a, ll, T, path = restated(ora, name)
        s = host_scene(ptx, name)
        got_T, got_path = s.array(ptx.ARR_LIGHT_TREE), s.array(ptx.ARR_LIGHT_PATH).reshape(-1)
        np.testing.assert_array_equal(got_T, T)
        np.testing.assert_array_equal(got_path, path)
        np.testing.assert_array_equal(s.array(ptx.ARR_LIGHT_TRIS).reshape(-1, 2), ll["tris"])
        np.testing.assert_array_equal(_bits(s.array(ptx.ARR_LIGHT_GEOM).reshape(-1, 4)), _bits(ll["geom"]))
        for v in (got_T, got_path):
            v.setflags(write=False)
        _product_trees[name] = (o, a, ll, got_T, got_path)
    return _product_trees[name]


# ---------------------------------------------------------------------------- constants, symbols, signatures
def test_symbols_constants_and_mirror_signatures(ptx):
    names = {"ptx_scene_set_light_pick", "ptx_scene_get_light_pick", "ptx_light_pick_batch", "ptx_light_pmf_batch"}
    assert names <= set(ptx.declared_symbols()) and all(hasattr(ptx.lib(), n) for n in names)
    assert (ptx.LIGHT_PICK_CDF, ptx.LIGHT_PICK_TREE, ptx.ARR_LIGHT_TREE, ptx.ARR_LIGHT_PATH) == (0, 1, 37, 38)
    assert list(inspect.signature(ptx.Scene.set_light_pick).parameters) == ["self", "pick"]
    assert list(inspect.signature(ptx.Scene.get_light_pick).parameters) == ["self"]
    assert list(inspect.signature(ptx.Scene.light_pick_batch).parameters) == ["self", "pos_u"]
    assert list(inspect.signature(ptx.Scene.light_pmf_batch).parameters) == ["self", "pos", "light"]
    assert callable(ptx.Renderer.set_light_pick)
    with open(ptx.HEADER_PATH) as fh:
        text = fh.read()
    assert "PTX_LIGHT_PICK_CDF = 0, PTX_LIGHT_PICK_TREE = 1" in text and "PTX_ARR_LIGHT_TREE = 37" in text and "PTX_ARR_LIGHT_PATH = 38" in text
    # no NEE flag was added: the flag words are the older tests'
    assert (ptx.NEE_NO_LIGHT_SAMPLES | ptx.NEE_FUSED | ptx.NEE_ENV_SAMPLES | ptx.NEE_SAMPLER_PDF) < 8192 and "PTX_NEE_FUSED_MOTION 8192u" in text
    assert ptx.PUNCTUAL_PICK_TREE == 1 and ptx.ARR_PUNCTUAL_TREE == 36


def test_refusals_and_the_round_trip(ptx):
    s = host_scene(ptx, "3 triangles", tree=False)
    L = ptx.lib()
    v = C.c_uint32(7)
    assert s.get_light_pick() == "cdf"
    assert L.ptx_scene_set_light_pick(None, 1) == ptx.ERR_INVALID
    assert L.ptx_scene_get_light_pick(None, C.byref(v)) == ptx.ERR_INVALID and L.ptx_scene_get_light_pick(s.h, None) == ptx.ERR_INVALID
    s.set_light_pick("tree")
    assert L.ptx_scene_get_light_pick(s.h, C.byref(v)) == 0 and v.value == ptx.LIGHT_PICK_TREE
    for bad in (2, 3, 0xFFFFFFFF, "bvh"):
        with pytest.raises(ptx.PtxError) as e:
            s.set_light_pick(bad)
        assert e.value.code == ptx.ERR_INVALID
        assert s.get_light_pick() == "tree"                      # a refused call leaves the mode
    # independent of the punctual mode
    assert s.punctual_pick == ptx.PUNCTUAL_PICK_CDF
    s.set_punctual_pick(ptx.PUNCTUAL_PICK_TREE)
    s.set_light_pick(ptx.LIGHT_PICK_CDF)
    assert s.get_light_pick() == "cdf" and s.punctual_pick == ptx.PUNCTUAL_PICK_TREE
    # the batches need a device: a host-only scene refuses them whatever else is wrong
    pu, x, k, p = np.zeros((2, 4), f32), np.zeros((2, 3), f32), np.zeros(2, np.int32), np.zeros(2, f32)
    assert L.ptx_light_pick_batch(s.h, pu.ctypes.data, 2, k.ctypes.data, p.ctypes.data) == ptx.ERR_NO_DEVICE
    assert L.ptx_light_pmf_batch(s.h, x.ctypes.data, k.ctypes.data, 2, p.ctypes.data) == ptx.ERR_NO_DEVICE
    assert L.ptx_light_pick_batch(None, pu.ctypes.data, 2, k.ctypes.data, p.ctypes.data) == ptx.ERR_INVALID
    assert L.ptx_light_pmf_batch(None, x.ctypes.data, k.ctypes.data, 2, p.ctypes.data) == ptx.ERR_INVALID


def test_the_modes_lifetime(ptx, ora):
    """the mode outlives the list; the tree is built with the list, dropped with it and rebuilt with it"""
    d = _proc().movers_scene(emissive_mover=True)
    s = product_from_dict(ptx, None, d)
    assert len(s.array(ptx.ARR_LIGHT_TREE)) == 0 and len(s.array(ptx.ARR_LIGHT_PATH)) == 0          # CDF mode: both empty
    n = len(s.array(ptx.ARR_LIGHT_CDF))
    assert n > 1
    cdf0 = s.array(ptx.ARR_LIGHT_CDF).copy()
    s.set_light_pick("tree")
    T0, P0 = s.array(ptx.ARR_LIGHT_TREE).copy(), s.array(ptx.ARR_LIGHT_PATH).copy()
    assert T0.shape == (2 * n - 1, 8) and P0.shape[0] == n
    np.testing.assert_array_equal(_bits(s.array(ptx.ARR_LIGHT_CDF)), _bits(cdf0))                   # the list is the same list
    # set_model_xforms drops the list and the tree; both come back for the moved models
    xf = s.array(ptx.ARR_MODEL_XFORM).copy()
    xf[:, 0:3] += f32(0.25)
    s.set_model_xforms(xf)
    assert s.get_light_pick() == "tree"
    T1 = s.array(ptx.ARR_LIGHT_TREE)
    assert T1.shape == T0.shape and (T1[:, 0:3].view(f32) != T0[:, 0:3].view(f32)).any()
    o1 = oracle_from_dict(ora, dict(d, model_xform=xf))
    want_T, want_P = LT.build(o1.a)
    np.testing.assert_array_equal(T1, want_T)                                                       # rebuilt from the moved corners
    np.testing.assert_array_equal(s.array(ptx.ARR_LIGHT_PATH).reshape(-1), want_P)
    # set_motion both ways: a moving model's emitter leaves the list, and the tree with it
    begin = xf.copy()
    begin[:, 0] -= f32(0.5)
    s.set_motion(begin_model_xform=begin, shutter=(0.0, 1.0))
    n_m = len(s.array(ptx.ARR_LIGHT_CDF))
    assert s.get_light_pick() == "tree" and len(s.array(ptx.ARR_LIGHT_PATH)) == n_m
    assert len(s.array(ptx.ARR_LIGHT_TREE)) == (2 * n_m - 1 if n_m else 0) and n_m < n
    s.set_motion()
    np.testing.assert_array_equal(s.array(ptx.ARR_LIGHT_TREE), T1)
    s.set_light_pick("cdf")                                                                         # CDF mode: no tree, the list stays
    assert len(s.array(ptx.ARR_LIGHT_TREE)) == 0 and len(s.array(ptx.ARR_LIGHT_PATH)) == 0 and len(s.array(ptx.ARR_LIGHT_CDF)) == n
    s.set_light_pick("tree")
    np.testing.assert_array_equal(s.array(ptx.ARR_LIGHT_TREE), T1)
    # an empty list: both arrays empty in tree mode
    e = product_from_dict(ptx, None, _proc().lamp_scene(1)[0])
    e.set_light_pick("tree")
    assert len(e.array(ptx.ARR_LIGHT_CDF)) == 0 and len(e.array(ptx.ARR_LIGHT_TREE)) == 0 and len(e.array(ptx.ARR_LIGHT_PATH)) == 0


# ---------------------------------------------------------------------------- the tree array
@pytest.mark.parametrize("case", sorted(TREE_CASES))
def test_the_tree_and_the_path_words_are_the_restatements_bit_for_bit(ptx, ora, case):
    s = host_scene(ptx, case)
    _, a, ll, T, path = restated(ora, case)
    got, gpath = s.array(ptx.ARR_LIGHT_TREE), s.array(ptx.ARR_LIGHT_PATH).reshape(-1)
    m = TREE_CASES[case]
    assert len(ll["cdf"]) == m == len(s.array(ptx.ARR_LIGHT_CDF))
    assert got.dtype == np.uint32 and got.shape == T.shape == (2 * m - 1, 8), (got.shape, T.shape)
    np.testing.assert_array_equal(got, T)
    np.testing.assert_array_equal(gpath, path)
    leaves = got[(got[:, 7] & LT.LEAF) != 0, 7] & ~LT.LEAF
    assert sorted(leaves.tolist()) == list(range(m))
    dep = LT.depths(got)
    assert max(dep) <= math.ceil(math.log2(m)) + 1 and max(dep) - min(dep) <= 1
    assert (got[:, 3].view(f32) > 0).all()                                  # every leaf's power is positive, so every node's
    lo, hi = got[:, 0:3].view(f32), got[:, 4:7].view(f32)
    for i in np.flatnonzero((got[:, 7] & LT.LEAF) == 0):
        l = int(got[i, 7])
        assert i < l < len(got) - 1
        assert (np.minimum(lo[l], lo[l + 1]) == lo[i]).all() and (np.maximum(hi[l], hi[l + 1]) == hi[i]).all()
        pw = got[:, 3].view(f32).astype(np.float64)
        assert abs(pw[l] + pw[l + 1] - pw[i]) <= 2 ** -22 * pw[i]
    # every path word leads to its own leaf
    for k in range(m):
        node, word = 0, int(gpath[k])
        while not got[node, 7] & LT.LEAF:
            node, word = int(got[node, 7]) + (word & 1), word >> 1
        assert int(got[node, 7] & ~LT.LEAF) == k and word == 0, (case, k)


# ---------------------------------------------------------------------------- the restated pick and directed pmf
def _points(T, rng, n):
    lo, hi = T[0, 0:3].view(f32), T[0, 4:7].view(f32)
    span = np.maximum(hi - lo, f32(1))
    return (lo - span + rng.random((n, 3)) * (hi - lo + 2 * span)).astype(f32)


@pytest.mark.parametrize("case", sorted(TREE_CASES))
def test_the_directed_pmf_is_the_picks_pmf_and_sums_to_one(ptx, ora, case):
    """Directed pmf == the stochastic pick's pmf bitwise for every (x, u) tried. At 256 random positions the directed pmfs of all leaves
    sum to 1 within 64 ulp x depth: a leaf's pmf is a product of at most depth - 1 rounded factors, each p or 1 - p with p + (1 - p) = 1
    up to one rounding, so each level of the tree loses at most a few ulp of 1 of the total mass (one for the product, one for 1 - p, one
    for the float64 sum's inputs being float32); 64 ulp a level leaves a wide margin and is still 1e-5 at depth 10."""
    _, _, ll, T, path = tree_of(ptx, ora, case)
    m = TREE_CASES[case]
    rng = np.random.default_rng(9)
    x = _points(T, rng, 256)
    table = LT.leaf_pmfs(T, x)
    tot = table.astype(np.float64).sum(1)
    depth = max(LT.depths(T))
    bound = 64 * 2.0 ** -23 * depth
    print(f"{case}: depth {depth}, worst |sum - 1| {np.abs(tot - 1).max():.3g} (bound {bound:.3g}); smallest pmf {table.min():.3g}")
    assert np.abs(tot - 1).max() <= bound and (table > 0).all()
    # the directed walk is the table's entry, and the pick's pmf is the directed one
    for k in (0, m // 2, m - 1):
        np.testing.assert_array_equal(_bits(LT.pmf(T, path, np.full(256, k), x)), _bits(table[:, k]))
    u = np.concatenate([rng.random(254).astype(f32), [f32(0), LT.ONE_BELOW]]).astype(f32)
    k, p = LT.pick(T, x, u)
    np.testing.assert_array_equal(_bits(p), _bits(LT.pmf(T, path, k, x)))
    if m == 1:
        assert (k == 0).all() and (p == f32(1)).all()                      # one triangle: (0, 1.0F)


@pytest.mark.parametrize("case", ["2 triangles", "3 triangles", "field32", "cloud", "coincident centroids", "centroids on one line"])
def test_the_pick_frequencies_follow_the_pmf(ptx, ora, case):
    """the frequencies of 20000 u match the pmf at three points (chi^2 over the entries with an expectation above 5: below its degrees of
    freedom + 5 sqrt(2 dof) + 10), as tests/test_nee_punctual_tree.py checks its pick"""
    _, _, ll, T, path = tree_of(ptx, ora, case)
    rng = np.random.default_rng(3)
    n_u = 20000
    us = np.concatenate([rng.random(n_u - 2).astype(f32), [f32(0), LT.ONE_BELOW]]).astype(f32)
    cen = LT.branch_centres(T)
    for x in (_points(T, rng, 1)[0], cen[0], cen[-1] + f32(0.01)):
        k, p = LT.pick(T, np.tile(x, (n_u, 1)), us)
        table = LT.leaf_pmfs(T, x[None])[0]
        np.testing.assert_array_equal(_bits(p), _bits(table[k]))
        exp = table.astype(np.float64) * n_u
        cnt = np.bincount(k, minlength=len(table))
        big = exp > 5
        chi, dof = float((((cnt - exp) ** 2) / np.maximum(exp, 1e-300))[big].sum()), int(big.sum()) - 1
        print(f"{case} at {x}: chi^2 {chi:.1f} over {dof} degrees of freedom; picks of entries with an expectation <= 5: {int(cnt[~big].sum())}")
        assert chi <= dof + 5 * math.sqrt(2 * max(dof, 1)) + 10 and cnt[~big].sum() <= 5 * (~big).sum() + 30


# ---------------------------------------------------------------------------- the restated vertex loop
PIN_CASES = [("field16", 16, 12, 2, 3, 1, False), ("field16", 12, 8, 2, 3, 4, True), ("cornell", 12, 12, 2, 3, 1, True), ("cornell", 8, 8, 1, 4, 16, False)]


@pytest.mark.parametrize("name,W,H,spp,b,M,spdf", PIN_CASES)
def test_the_loop_in_cdf_mode_is_the_estimator_bit_for_bit(ptx, ora, name, W, H, spp, b, M, spdf):
    """tests/_nee_estimator.py may not change here, so the tree-mode loop is pinned to it: with tree=None its per-sample radiance and its
    counts equal _nee_estimator.render_samples bit for bit on the scenes the tests below use"""
    o, a, *_ = tree_of(ptx, ora, name)      # the scene whose stored list and tree the other tests render with
    want = render_samples(ora, o, a, W, H, spp, b, M=M, spdf=spdf, seed=SEED)
    got = LT.render_samples(ora, o, a, W, H, spp, b, tree=None, M=M, spdf=spdf, seed=SEED)
    np.testing.assert_array_equal(_bits(got["rad"]), _bits(want["rad"]))
    assert all(got[k] == want[k] for k in ("rays", "light_samples", "light_visible")) and got["light_visible"] > 0


def test_one_triangle_in_tree_mode_is_the_cdf_mode_bitwise(ptx, ora):
    o, a, ll, T, path = tree_of(ptx, ora, "1 triangle")
    assert len(T) == 1 and path.tolist() == [0]
    cdf = LT.render_samples(ora, o, a, 16, 12, 2, 3, seed=SEED)
    tree = LT.render_samples(ora, o, a, 16, 12, 2, 3, tree=(T, path), seed=SEED)
    np.testing.assert_array_equal(_bits(tree["rad"]), _bits(cdf["rad"]))
    assert tree["light_visible"] == cdf["light_visible"] > 0


WHITE, BLACK = (1.0, 1.0, 1.0), (0.0, 0.0, 0.0)
EXPECT = {"field16": dict(W=16, H=12, spp=4, b=3, env=WHITE), "cornell": dict(W=12, H=12, spp=4, b=3, env=WHITE),
          "gloss4": dict(W=16, H=12, spp=16, b=3, env=BLACK)}
_batches = {}


def _restated_batches(ptx, ora, name, mode, wrong=()):
    """K_BATCH batch means of the restated loop; computed once per (scene, mode) and left unchanged"""
    key = (name, mode, tuple(wrong))
    if key not in _batches:
        o, a, ll, T, path = tree_of(ptx, ora, name)
        v = EXPECT[name]
        seed0 = 0xB000 if mode == "cdf" else 0xA000
        frames = [LT.render_samples(ora, o, a, v["W"], v["H"], v["spp"], v["b"], tree=(T, path) if mode == "tree" else None, seed=seed0 + k,
                                    wrong=wrong, env=v["env"])["rad"].mean(2) for k in range(K_BATCH)]
        _batches[key] = _batch_stat(np.stack(frames))
        _batches[key].setflags(write=False)
    return _batches[key]


@pytest.mark.parametrize("name", sorted(EXPECT))
def test_the_restated_tree_mode_has_the_cdf_modes_expectation(ptx, ora, name):
    """K_BATCH batches in tree mode against K_BATCH of other seeds in CDF mode, _nee_common's statistic with its own bars, on
    emitter_field_scene(16), the Cornell box and four large emitters over a glossy floor (where the emission weight carries the frame).
    Measured, worst z frame / quadrant: cornell 1.40 / 1.62 at 16 x 16 x 16; the wrong forms below give 4 to 140."""
    ok, zf, zq = _same_expectation(_restated_batches(ptx, ora, name, "tree"), _restated_batches(ptx, ora, name, "cdf"))
    print(f"{name}: restated tree against CDF mode, worst z frame {zf:.2f} quadrant {zq:.2f}")
    assert ok, (zf, zq)


@pytest.mark.parametrize("wrong", LT.WRONG)
def test_a_wrong_form_fails_the_expectation(ptx, ora, wrong):
    """the power of the check above: each wrong form of the tree-mode densities fails it on the scene that is meant to show it. A_total
    kept in p_l fails on every scene (z 35 to 140). The two wrong emission weights move a frame only where BSDF samples hit emitters with
    a large weight from points far from them, which is what the glossy scene is for: they must fail there (measured at 8 spp: z 8.7
    and 15.6 against the right form's 2.6)."""
    z = {}
    for name in sorted(EXPECT):
        ok, zf, zq = _same_expectation(_restated_batches(ptx, ora, name, "tree", (wrong,)), _restated_batches(ptx, ora, name, "cdf"))
        z[name] = (ok, round(zf, 2), round(zq, 2))
    print(f"{wrong}: {z}")
    assert not z["gloss4"][0], z
    if wrong == "area_total":
        assert not any(v[0] for v in z.values()), z


# ---------------------------------------------------------------------------- R0
def test_variance_ratio_r0(ptx, ora):
    """LT.VARIANCE_CASE (emitter_field_scene(64) at 32 x 24, 4 spp, 2 bounces, black environment) on the restatement: the sum over pixels and
    channels of the per-pixel sample variance in tree mode over the same in CDF mode, with the same seed. R0 is that figure, written
    down for the GPU test, whose bar is twice that."""
    v = LT.VARIANCE_CASE
    name = f"field{v['n']}"
    o, a, ll, T, path = tree_of(ptx, ora, name)
    rad = {m: LT.render_samples(ora, o, a, v["W"], v["H"], v["spp"], v["bounces"], tree=t, seed=SEED, env=(0.0, 0.0, 0.0))["rad"].astype(np.float64)
           for m, t in (("tree", (T, path)), ("cdf", None))}
    r0 = float(rad["tree"].var(2, ddof=1).sum() / rad["cdf"].var(2, ddof=1).sum())
    print(f"R0 = {r0:.4f} (recorded: {LT.R0})")
    assert r0 < 0.75                                          # the case counts only then
    assert abs(r0 / LT.R0 - 1) < 0.02                         # LT.R0 is this figure, written down for the GPU test
