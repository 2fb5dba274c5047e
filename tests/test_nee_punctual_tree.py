"""The light tree of ptx_render_nee's punctual lights (include/ptx.h: ptx_scene_set_punctual_pick, PUNCTUAL PICK), without a GPU: the symbols,
the setter's refusals and the mode's lifetime on host-only scenes, the stored tree against tests/_nee_punctual_tree_restatement.py bit for
bit, the restated pick's own properties, and the variance ratio R0 that the GPU test's bar is built on. Every test fails on the parent for
want of the symbols. GPU tests: tests/test_nee_punctual_tree_gpu.py.
"""
import ctypes as C
import math

import numpy as np
import pytest

import _nee_punctual_restatement as PU
import _nee_punctual_tree_restatement as PT
from _common import _bits, _proc
from _nee_common import SEED
from _nee_estimator import render_samples
from conftest import oracle_from_dict, product_from_dict

f32 = np.float32


def _floor(ptx):
    d, _ = _proc().lamp_scene(1)
    return product_from_dict(ptx, None, d)


def _lamps(n, **kw):
    return _proc().lamp_scene(n, **kw)[1]


def _special(name):
    base = _lamps(6, spots=True)
    if name == "coincident":
        base[:, 0:3] = [1, 2, 3]
    elif name == "coincident, one black":
        base = base[:4]
        base[:, 0:3] = [1, 2, 3]
        base[2, 8:11] = 0
    elif name == "on one line":
        base[:, 0] = [0.5, -1.0, 0.5, 2.0, -1.0, 0.25]      # ties along x, to be broken by the index
        base[:, 1], base[:, 2] = 2.0, 0.0
    elif name == "one black":
        base[3, 8:11] = 0
    elif name == "all black":
        base[:, 8:11] = 0
    elif name == "signed zeros":
        base[:, 0] = [0.0, -0.0, 0.0, -0.0, 1.0, -1.0]
    return base


TREE_CASES = {f"{n} lamps": (lambda n=n: _lamps(n, spots=True, lamp_range=3.0 if n == 64 else 0.0)) for n in (1, 2, 3, 5, 64, 257)}
TREE_CASES.update({k: (lambda k=k: _special(k)) for k in ("coincident", "coincident, one black", "on one line", "one black", "all black", "signed zeros")})


# ---------------------------------------------------------------------------- constants, symbols, signatures
def test_symbols_and_constants(ptx):
    names = {"ptx_scene_set_punctual_pick", "ptx_scene_get_punctual_pick", "ptx_punctual_pick_batch"}
    assert names <= set(ptx.declared_symbols()) and all(hasattr(ptx.lib(), n) for n in names)
    assert (ptx.PUNCTUAL_PICK_CDF, ptx.PUNCTUAL_PICK_TREE, ptx.ARR_PUNCTUAL_TREE) == (0, 1, 36)
    assert callable(ptx.Scene.set_punctual_pick) and callable(ptx.Scene.punctual_pick_batch) and isinstance(ptx.Scene.punctual_pick, property)
    assert callable(ptx.Renderer.set_punctual_pick)
    with open(ptx.HEADER_PATH) as fh:
        text = fh.read()
    assert "PTX_PUNCTUAL_PICK_CDF = 0, PTX_PUNCTUAL_PICK_TREE = 1" in text and "PTX_ARR_PUNCTUAL_TREE = 36" in text
    # no NEE flag was added: the known flag words are the older tests' (fused, env, sampler pdf, no lights, fused motion, candidates)
    assert (ptx.NEE_NO_LIGHT_SAMPLES | ptx.NEE_FUSED | ptx.NEE_ENV_SAMPLES | ptx.NEE_SAMPLER_PDF) < 8192 and "PTX_NEE_FUSED_MOTION 8192u" in text


def test_refusals_and_the_round_trip(ptx):
    s = _floor(ptx)
    L = ptx.lib()
    v = C.c_uint32(7)
    assert s.punctual_pick == ptx.PUNCTUAL_PICK_CDF
    assert L.ptx_scene_set_punctual_pick(None, 1) == ptx.ERR_INVALID
    assert L.ptx_scene_get_punctual_pick(None, C.byref(v)) == ptx.ERR_INVALID and L.ptx_scene_get_punctual_pick(s.h, None) == ptx.ERR_INVALID
    s.set_punctual_pick(ptx.PUNCTUAL_PICK_TREE)
    for bad in (2, 3, 0xFFFFFFFF):
        with pytest.raises(ptx.PtxError) as e:
            s.set_punctual_pick(bad)
        assert e.value.code == ptx.ERR_INVALID
        assert s.punctual_pick == ptx.PUNCTUAL_PICK_TREE          # a refused call leaves the mode
    s.set_punctual_pick(ptx.PUNCTUAL_PICK_CDF)
    assert s.punctual_pick == ptx.PUNCTUAL_PICK_CDF
    # the batch needs a device: a host-only scene refuses it whatever else is wrong
    s.set_punctual_lights(_lamps(3))
    pu, k, p = np.zeros((2, 4), f32), np.zeros(2, np.int32), np.zeros(2, f32)
    assert L.ptx_punctual_pick_batch(s.h, pu.ctypes.data, 2, k.ctypes.data, p.ctypes.data) == ptx.ERR_NO_DEVICE
    assert L.ptx_punctual_pick_batch(None, pu.ctypes.data, 2, k.ctypes.data, p.ctypes.data) == ptx.ERR_INVALID


def test_the_modes_lifetime(ptx):
    """the mode survives a new light set and a clear; the tree follows the lights; the three movers touch neither"""
    d, lights = _proc().lamp_scene(5, spots=True)
    s = product_from_dict(ptx, None, d)
    assert len(s.array(ptx.ARR_PUNCTUAL_TREE)) == 0
    s.set_punctual_pick(ptx.PUNCTUAL_PICK_TREE)                  # before any light: an empty tree
    assert len(s.array(ptx.ARR_PUNCTUAL_TREE)) == 0 and s.punctual_pick == 1
    s.set_punctual_lights(lights)
    tree5 = s.array(ptx.ARR_PUNCTUAL_TREE)
    np.testing.assert_array_equal(tree5, PT.build(lights))
    s.set_punctual_lights(None)                                   # a clear empties the array and keeps the mode
    assert len(s.array(ptx.ARR_PUNCTUAL_TREE)) == 0 and s.punctual_pick == 1
    other = _lamps(9)
    s.set_punctual_lights(other)
    np.testing.assert_array_equal(s.array(ptx.ARR_PUNCTUAL_TREE), PT.build(other))
    s.set_punctual_pick(ptx.PUNCTUAL_PICK_CDF)                   # CDF mode: no tree, the lights stay
    assert len(s.array(ptx.ARR_PUNCTUAL_TREE)) == 0 and len(s.array(ptx.ARR_PUNCTUAL)) == 9
    s.set_punctual_pick(ptx.PUNCTUAL_PICK_TREE)                  # and back: built from the stored lights
    want = s.array(ptx.ARR_PUNCTUAL_TREE)
    np.testing.assert_array_equal(want, PT.build(other))
    with pytest.raises(ptx.PtxError):                            # a refused light set leaves lights, tree and mode
        s.set_punctual_lights(np.full((1, 16), np.nan, f32))
    np.testing.assert_array_equal(s.array(ptx.ARR_PUNCTUAL_TREE), want)
    # the movers: lights are world-space state
    xf = s.array(ptx.ARR_MODEL_XFORM).copy()
    xf[:, 0:3] += f32(0.25)
    s.set_model_xforms(xf)
    cam = s.camera()
    s.set_camera(cam["origin"] + f32(0.5), cam["basis"], cam["yfov"])
    begin = xf.copy()
    begin[:, 0] -= f32(0.5)
    s.set_motion(begin_model_xform=begin, shutter=(0.0, 1.0))
    np.testing.assert_array_equal(s.array(ptx.ARR_PUNCTUAL_TREE), want)
    assert s.punctual_pick == 1 and len(s.array(ptx.ARR_PUNCTUAL)) == 9
    s.set_motion()
    np.testing.assert_array_equal(s.array(ptx.ARR_PUNCTUAL_TREE), want)


# ---------------------------------------------------------------------------- the tree array
@pytest.mark.parametrize("case", sorted(TREE_CASES))
def test_the_tree_is_the_restatements_bit_for_bit(ptx, case):
    lights = TREE_CASES[case]()
    s = _floor(ptx)
    s.set_punctual_pick(ptx.PUNCTUAL_PICK_TREE)
    s.set_punctual_lights(lights)
    got, want = s.array(ptx.ARR_PUNCTUAL_TREE), PT.build(lights)
    assert got.dtype == np.uint32 and got.shape == want.shape, (got.shape, want.shape)
    np.testing.assert_array_equal(got, want)
    m = int((PT.lum_of(lights) > 0).sum())
    if case == "all black":
        assert m == 0 and len(got) == 0 and len(s.array(ptx.ARR_PUNCTUAL)) == 0      # stores no lights, as today
        return
    assert len(got) == 2 * m - 1
    leaves = got[(got[:, 7] & PT.LEAF) != 0, 7] & ~PT.LEAF
    assert sorted(leaves.tolist()) == [k for k in range(len(lights)) if PT.lum_of(lights)[k] > 0]
    dep = PT.depths(got)
    assert max(dep) <= math.ceil(math.log2(m)) + 1 and max(dep) - min(dep) <= 1
    # a branch's children are the next free slots, left first, and its box and power hold theirs
    for i in np.flatnonzero((got[:, 7] & PT.LEAF) == 0):
        l = int(got[i, 7])
        assert i < l < len(got) - 1
        lo, hi = got[:, 0:3].view(f32), got[:, 4:7].view(f32)
        assert (np.minimum(lo[l], lo[l + 1]) == lo[i]).all() and (np.maximum(hi[l], hi[l + 1]) == hi[i]).all()
        pw = got[:, 3].view(f32).astype(np.float64)
        assert abs(pw[l] + pw[l + 1] - pw[i]) <= 2 ** -22 * pw[i]


# ---------------------------------------------------------------------------- the restated pick
PICK_CASES = ["1 lamps", "2 lamps", "3 lamps", "5 lamps", "64 lamps", "257 lamps", "coincident, one black", "on one line", "one black"]


def _points(lights, rng):
    """three points per case: on the floor, in the air among the lamps, and on a light"""
    return np.array([[rng.uniform(-4, 4), 0, rng.uniform(-4, 4)], [rng.uniform(-2, 2), rng.uniform(0.5, 2.5), rng.uniform(-2, 2)], lights[len(lights) // 2, 0:3]], f32)


@pytest.mark.parametrize("case", PICK_CASES)
def test_the_restated_pick(case):
    """the walked pmf is the product of the branch probabilities; the frequencies of 20000 u match the pmf at three points (chi^2 over the
    lights with an expectation above 5: below its degrees of freedom + 5 sqrt(2 dof) + 10); a leaf with I > 0 has pmf > 0; one light gives
    (0, 1.0f) for every u"""
    lights = TREE_CASES[case]()
    T = PT.build(lights)
    rng = np.random.default_rng(3)
    n_u = 20000
    us = np.concatenate([rng.random(n_u - 2).astype(f32), [f32(0), PT.ONE_BELOW]]).astype(f32)
    leaf_node = {int(T[i, 7] & ~PT.LEAF): i for i in range(len(T)) if T[i, 7] & PT.LEAF}
    for x in _points(lights, rng):
        X = np.tile(x, (n_u, 1))
        k, pmf = PT.pick(T, lights, X, us)
        table = PT.leaf_pmfs(T, lights, x[None])[0]
        assert abs(float(table.astype(np.float64).sum()) - 1) < 1e-5
        np.testing.assert_array_equal(_bits(pmf), _bits(table[k]))           # the walked pmf: the product, bit for bit
        assert (pmf > 0).all()                                                 # no pick of a light of pmf 0
        if len(T) == 1:
            assert (k == 0).all() and (pmf == f32(1)).all()
            continue
        for kk, node in leaf_node.items():
            if PT.importance(T, lights, np.array([node]), x[None])[0] > 0:
                assert table[kk] > 0, (case, kk)
        black = PT.lum_of(lights) <= 0
        assert (table[black] == 0).all() and not black[k].any()
        exp = table.astype(np.float64) * n_u
        cnt = np.bincount(k, minlength=len(lights))
        big = exp > 5
        chi, dof = float((((cnt - exp) ** 2) / np.maximum(exp, 1e-300))[big].sum()), int(big.sum()) - 1
        print(f"{case} at {x}: chi^2 {chi:.1f} over {dof} degrees of freedom; picks of lights with an expectation <= 5: {int(cnt[~big].sum())}")
        assert chi <= dof + 5 * math.sqrt(2 * max(dof, 1)) + 10 and cnt[~big].sum() <= 5 * (~big).sum() + 30


def test_cdf_pick_is_the_stored_cdf():
    lights = TREE_CASES["64 lamps"]()
    cdf = PU.cdf_of(lights)
    k, p = PT.cdf_pick(cdf, np.array([0, 0.5, PT.ONE_BELOW], f32))
    assert k[0] == 0 and k[2] == 63 and p[0] == cdf[0] and p[2] == f32(cdf[63] - cdf[62])


# ---------------------------------------------------------------------------- R0
def test_variance_ratio_r0(ora):
    """Construction D (2 bounces, black environment, no emitter: a sample's radiance is vertex 0's punctual sample alone) on
    lamp_scene(16, spots=True) at 32 x 24: with X_k the unchanged restatement's per-sample radiance of lamp k alone and p_k the pmf of a
    pick rule at the sample's vertex, the one-sample estimator X_k / p_k has the conditional variance sum_k lum(X_k)^2 / p_k -
    lum(sum_k X_k)^2. R0 is that sum over all samples with the tree's pmf over the same with the CDF's.
    Measured: R0 = 0.4402 (PT.R0; the GPU test's bar is twice that). The issue's simplified model gives 0.31 to 0.43 for 8 to 64 such lamps."""
    v = PT.VARIANCE_CASE
    d, lights = _proc().lamp_scene(**v["lamps"])
    o = oracle_from_dict(ora, d)
    W, H, spp = v["W"], v["H"], v["spp"]
    lum = lambda a: (0.2126 * a[..., 0].astype(np.float64) + 0.7152 * a[..., 1].astype(np.float64)) + 0.0722 * a[..., 2].astype(np.float64)
    X = np.stack([lum(render_samples(ora, o, o.a, W, H, spp, 2, seed=SEED, env=(0.0, 0.0, 0.0), punctual=lights[k:k + 1])["rad"]) for k in range(len(lights))], -1)
    pos = np.zeros((H, W, spp, 3), f32)
    hit = np.zeros((H, W, spp), bool)
    for s in range(spp):
        rays = o.primary_rays(ora.make_cfg(W, H, 1, 1, seed=SEED), s).reshape(-1, 6)
        out, surf = o.intersect(rays)
        pos[:, :, s], hit[:, :, s] = out[:, 0:3].reshape(H, W, 3), (surf >= 0).reshape(H, W)
    T = PT.build(lights)
    p_tree = PT.leaf_pmfs(T, lights, pos.reshape(-1, 3)).reshape(H, W, spp, -1).astype(np.float64)
    cdf = PU.cdf_of(lights)
    p_cdf = (cdf - np.concatenate([np.zeros(1, f32), cdf[:-1]])).astype(f32).astype(np.float64)
    assert (X[~hit] == 0).all() and ((X > 0) <= (p_tree > 0)).all()       # wherever a lamp contributes the tree can pick it
    tot2 = X.sum(-1) ** 2

    def cond_var(p):
        with np.errstate(all="ignore"):
            return float((np.where(X > 0, X * X / p, 0.0).sum(-1) - tot2).sum())
    r0 = cond_var(p_tree) / cond_var(np.broadcast_to(p_cdf, X.shape))
    print(f"R0 = {r0:.4f} (recorded: {PT.R0}); lit samples {(X.sum(-1) > 0).mean() * 100:.1f} %")
    assert r0 < 0.75                                          # the case counts only then
    assert abs(r0 / PT.R0 - 1) < 0.02                         # PT.R0 is this figure, written down for the GPU test
