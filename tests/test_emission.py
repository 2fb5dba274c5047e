"""ptx_render_emission, ptx_emission_split and ptx_emission_merge without a GPU: the numpy restatements (tests/_emission_restatement.py)
are shown to mean what include/ptx.h says, against the oracle's own integrator and against the four filter restatements; then the exported
symbols, the mirrors' signatures and every refusal of the C calls. All comparisons are bitwise: nothing here goes through libm.

The split and merge calls look at their context last, so their refusals are met with a NULL context; pointers of mixed kinds need a device
pointer: tests/test_emission_gpu.py.
"""
import ctypes as C
import inspect
import os

import numpy as np
import pytest

from _aov_restatement import H, S0, SEED, SPP, TILE, W
from _aov_restatement import restate as restate_aov
from _common import _bits, _proc, _same
from _denoise_counts_restatement import restate_counts, synthetic
from _denoise_restatement import restate as restate_denoise
from _emission_restatement import CORNELL_TILE, LIT_LOAD, LIT_TILE, checker_frame, merge, restate, split
from _temporal_counts_restatement import restate as restate_temporal_counts
from _temporal_restatement import motion_sums
from _temporal_restatement import restate as restate_temporal
from conftest import CORNELL, GOLD, oracle_from_dict, product_from_dict, ulp_diff

f32 = np.float32
LIT = os.path.join(GOLD, "textures", "lit.gltf")
_oracles, _refs = {}, {}


def _oracle(ora, name):
    if name not in _oracles:
        if name == "cloud":
            _oracles[name] = oracle_from_dict(ora, _proc().emitter_cloud_scene(sun=False))
        else:
            _oracles[name] = ora.OracleScene(ora.load_gltf(CORNELL) if name == "cornell" else ora.load_gltf(LIT, **LIT_LOAD))
    return _oracles[name]


def _tile(name):
    return {"cornell": CORNELL_TILE, "lit": LIT_TILE}.get(name, TILE)


def _ref(ora, name):
    """The restatement at the common AOV shape, computed once: (emission, counts, per-sample records). Never modified."""
    if name not in _refs:
        em, c, recs = restate(ora, _oracle(ora, name), tile=_tile(name), per_sample=True)
        em.setflags(write=False)
        _refs[name] = (em, c, recs)
    return _refs[name]


# ---------------------------------------------------------------------------- the restatement is not vacuous
def test_restatement_cornell_sees_its_light_and_no_back_face(ora):
    """At the common tile Cornell's light is out of sight (0 emissive samples): the tile is moved to the top row, see CORNELL_TILE."""
    em, c, _ = _ref(ora, "cornell")
    assert c["emissive"] >= 1 and c["back"] == 0 and c["miss"] == 0 and c["through"] == 0   # 224 emissive samples
    assert (em[..., 3] == SPP).all() and (em[..., :3] >= 0).all() and np.isfinite(em).all()
    lit = em[..., :3].any(-1)
    assert 0 < lit.sum() < lit.size   # the light's pixels and nothing else
    assert restate(ora, _oracle(ora, "cornell"))[1]["emissive"] == 0


def test_restatement_lit_gltf_has_a_textured_emitter(ora):
    _, c, recs = _ref(ora, "lit")
    vals = np.concatenate([r[r[:, :3].any(1), :3] for r in recs])
    assert c["emissive"] == len(vals) >= 100 and len(np.unique(_bits(vals), axis=0)) >= 2   # 676 samples; the emission follows the texture
    assert c["through"] >= 100 and c["back"] >= 1 and c["miss"] >= 1000                       # 265, 50, 4418


def test_restatement_jack_emits_but_never_behind_a_pass_through(ora, jack_oracle):
    """What the asset has at the common shape: its glow is seen directly by a few samples, never through the alpha-textured geometry. The
    emitter cloud below has an emissive sample behind a pass-through."""
    em, c = restate(ora, jack_oracle)
    assert c["through"] >= 200 and c["emissive"] >= 1    # 356 samples pass through; 25 record a non-zero emission
    assert c["emissive_through"] == 0                     # none of them behind a pass-through
    assert c["back"] >= 1                                 # 110 samples end on a back face
    assert np.isfinite(em).all()


def test_restatement_cloud_has_back_facing_first_hits_and_emission_behind_a_pass_through(ora):
    """The emitter cloud's triangles face every way: a back-facing one is a sample's surface for ptx_render_aov and records nothing here."""
    em, c, _ = _ref(ora, "cloud")
    alb, _, _ = restate_aov(ora, _oracle(ora, "cloud"))
    assert c["back"] >= 1 and c["emissive"] >= 1 and c["emissive_through"] >= 1   # 1610, 465, 1
    assert (em[..., 3] <= alb[..., 3]).all() and (em[..., 3] < alb[..., 3]).sum() >= 1
    assert c["surface"] - c["back"] == int(em[..., 3].sum()) and c["surface"] == int(alb[..., 3].sum())


# ---------------------------------------------------------------------------- against the oracle's own integrator
@pytest.mark.parametrize("name", ["cornell", "lit"])
def test_the_restatement_is_the_oracles_one_bounce_frame_without_environment(ora, name):
    o = _oracle(ora, name)
    assert o.a.sun is None, "the tie holds on a scene without a sun"
    em, _, _ = _ref(ora, name)
    smp = o.render_samples(ora.make_cfg(W, H, SPP, 1, env=(0.0, 0.0, 0.0), seed=SEED, tile=_tile(name), sample0=S0), threads=0)   # [h,w,spp,3]
    acc = np.zeros(smp.shape[:2] + (3,), f32)
    for s in range(SPP):
        acc += smp[:, :, s]
    _same(em[..., :3], acc, name)
    assert acc.any()


# ---------------------------------------------------------------------------- sample ranges
def test_two_ranges_into_one_buffer_are_one_call_and_separate_sums_differ_by_a_rounding(ora):
    o = _oracle(ora, "lit")
    em, _, recs = _ref(ora, "lit")
    built = np.zeros((TILE[3] * TILE[2], 4), f32)
    for r in recs[:2] + recs[2:]:      # the second range added to what the first left
        took = r[:, 3] > 0
        built[took] += r[took]
    _same(built.reshape(em.shape), em, "adjacent ranges into one buffer")
    e1, _ = restate(ora, o, tile=LIT_TILE, sample0=S0, spp=2)
    e2, _ = restate(ora, o, tile=LIT_TILE, sample0=S0 + 2, spp=SPP - 2)
    np.testing.assert_array_equal(e1[..., 3] + e2[..., 3], em[..., 3])
    err = np.abs((e1 + e2).astype(np.float64) - em) / np.maximum(np.abs(em), 1)
    assert err.max() <= SPP * 2.0 ** -23


# ---------------------------------------------------------------------------- split and merge: consequence (a)
def _awkward(shape, seed):
    rng = np.random.default_rng(seed)
    x = rng.normal(0, 3, shape + (4,)).astype(f32)
    x[..., 3] = rng.integers(1, 33, shape)
    flat = x.reshape(-1, 4)
    flat[0, 0], flat[-1, 1], flat[len(flat) // 2, 2] = f32(-0.0), f32(np.nan), f32(np.inf)
    return x


def test_a_zero_emission_buffer_changes_no_bit():
    a, b, out = _awkward((9, 13), 1), _awkward((9, 13), 2), _awkward((9, 13), 3)
    em = np.zeros((9, 13, 4), f32)
    em[..., 3] = 8        # the count of recording samples is not looked at
    em[0, 0, 0] = f32(-0.0)
    sa, sb = split(em, 8, a, b)
    _same(sa, a, "a"), _same(sb, b, "b"), _same(merge(em, 8, out), out, "out")
    assert split(em, 8, a)[1] is None


def test_a_channel_whose_mean_is_nan_or_negative_is_untouched():
    a, b, out = _awkward((4, 6), 4), _awkward((4, 6), 5), _awkward((4, 6), 6)
    em = np.full((4, 6, 4), 16, f32)
    em[1, 2, :3] = (np.nan, -3.0, 8.0)
    em[2, 3, :3] = (-np.inf, 0.0, np.inf)
    sa, sb = split(em, 8, a, b)
    mo = merge(em, 8, out)
    for got, was in ((sa, a), (sb, b), (mo, out)):
        _same(got[1, 2, :2], was[1, 2, :2], "NaN and negative")
        _same(got[2, 3, :2], was[2, 3, :2], "-inf and zero")
        _same(got[..., 3], was[..., 3], "counts")
    assert sa[1, 2, 2] == a[1, 2, 2] - a[1, 2, 3] * f32(1) and mo[1, 2, 2] == out[1, 2, 2] + f32(1)
    assert sa[0, 1, 0] == a[0, 1, 0] - a[0, 1, 3] * f32(2) and mo[0, 1, 0] == out[0, 1, 0] + f32(2)


def test_split_mean_merge_is_the_unsplit_mean_within_two_ulp_of_the_larger_operand():
    """col = (col - e) + e through the counts mean: a rounding in the product, one in the difference, one in the sum, each relative to the
    larger of the mean and e."""
    a, b, _, _, ng = synthetic(23, 31, 7)
    rng = np.random.default_rng(8)
    em = np.zeros(a.shape, f32)
    em[..., :3] = rng.uniform(0, 4, a.shape[:2] + (3,)) * (rng.random(a.shape[:2] + (1,)) < 0.5) * ng
    n = (a[..., 3] + b[..., 3])[..., None]
    mean = ((a[..., :3] + b[..., :3]) / n).astype(f32)
    sa, sb = split(em, ng, a, b)
    res = np.zeros(a.shape, f32)
    res[..., :3] = ((sa[..., :3] + sb[..., :3]) / n).astype(f32)
    back = merge(em, ng, res)[..., :3]
    e = (em[..., :3] / f32(ng)).astype(f32)
    larger = np.maximum(np.abs(mean), e).astype(np.float64)
    # per half: the product a.w * e and the difference round at the half's scale, n/2 * larger at most -> 2 * 2^-24 * larger each after / n
    assert (np.abs(back.astype(np.float64) - mean) <= 2 * np.spacing(larger.astype(f32)).astype(np.float64)).all()
    _same(back[e == 0], mean[e == 0], "pixels without emission")
    assert (e > 0).any() and (back != mean).any()


# ---------------------------------------------------------------------------- consequence (b): exactness on an emissive frame
def _zero_motion(A, N):
    return motion_sums(A, N, 0.0, 0.0)


FILTERS = {
    "denoise": lambda a, b, A, N, it, prev: (restate_denoise(a, b, A, N, 4, 4, iterations=it), None),
    "counts": lambda a, b, A, N, it, prev: (restate_counts(a, b, A, N, 8, iterations=it), None),
    "temporal": lambda a, b, A, N, it, prev: restate_temporal(a, b, A, N, _zero_motion(A, N), 4, 4, prev=prev, iterations=it)[:2],
    "temporal_counts": lambda a, b, A, N, it, prev: restate_temporal_counts(a, b, A, N, _zero_motion(A, N), 8, prev=prev, iterations=it)[:2],
}


@pytest.mark.parametrize("iterations", [1, 5])
@pytest.mark.parametrize("which", list(FILTERS))
def test_split_filter_merge_returns_the_emission_bit_for_bit(which, iterations):
    a, b, A, N, em, e = checker_frame()
    lit = e > 0
    plain, _ = FILTERS[which](a, b, A, N, iterations, None)
    assert np.abs(plain[..., :3] - e).max() > 0.5     # the filter alone blurs the checker: 0.98 at 1 iteration, 0.96 at 5
    sa, sb = split(em, 8, a, b)
    assert (sa[..., :3] + sb[..., :3] == 0).all() and sa[..., :3].any()
    prev = None
    for frame in range(3 if which.startswith("temporal") else 1):
        out, prev = FILTERS[which](sa, sb, A, N, iterations, prev)
        got = merge(em, 8, out)
        _same(got[..., :3][lit], e[lit], f"{which} frame {frame}")
        assert (got[..., :3][~lit] == 0).all()
        if prev is not None:
            assert (prev[0][..., :3] == 0).all(), "the history holds the residual"


# ---------------------------------------------------------------------------- the C calls
def test_symbols_are_declared_and_exported(ptx):
    L = ptx.lib()
    for name in ("ptx_render_emission", "ptx_emission_split", "ptx_emission_merge"):
        assert name in ptx.declared_symbols() and hasattr(L, name), name
    v, u32, sz = C.c_void_p, C.c_uint32, C.c_size_t
    assert L.ptx_render_emission.argtypes == [v, C.POINTER(ptx.RenderCfg), v, C.POINTER(ptx.RenderStats)]
    assert L.ptx_emission_split.argtypes == [v, v, u32, sz, v, v]
    assert L.ptx_emission_merge.argtypes == [v, v, u32, sz, v]
    assert C.sizeof(ptx.AovBuffers) == 2 * C.sizeof(v)   # the guide struct stays two pointers


def test_the_mirrors_signatures(ptx):
    em, mo = inspect.signature(ptx.Scene.render_emission).parameters, inspect.signature(ptx.Scene.render_motion).parameters
    assert list(em)[:5] == ["self", "W", "H", "spp", "emission"]
    for k in ("seed", "tile", "sample0", "spp_per_pass", "want_stats", "shard"):
        assert em[k].default == mo[k].default, k
    assert list(inspect.signature(ptx.Context.emission_split).parameters) == ["self", "emission", "guide_spp", "a", "b"]
    assert inspect.signature(ptx.Context.emission_split).parameters["b"].default is None
    assert list(inspect.signature(ptx.Context.emission_merge).parameters) == ["self", "emission", "guide_spp", "out"]
    for fn in (ptx.Renderer.render_denoised, ptx.Renderer.render_adaptive, ptx.Renderer.render_adaptive_nee, ptx.Renderer._denoise_counts):
        assert inspect.signature(fn).parameters["split_emission"].default is False, fn.__name__


def test_render_emission_refusals_before_any_device_work(ptx):
    """Host-only scene, so nothing here can reach a device. As in ptx_render_aov the missing device is refused before the cfg's rectangle is
    looked at: what ptx_render refuses in a cfg is met on the GPU (tests/test_emission_gpu.py)."""
    L = ptx.lib()
    s = product_from_dict(ptx, None, _proc().plaza_scene(1, sun=False, alpha=False))
    x0, y0, w, h = TILE
    em = np.zeros((h, w, 4), f32)

    def cfg(integrator=0, **over):
        f = dict(W=W, H=H, spp=SPP, bounces=0, env=(C.c_float * 3)(1, 1, 1), seed_lo=SEED, seed_hi=0, x0=x0, y0=y0, w=w, h=h, sample0=S0, spp_per_pass=2,
                 integrator=integrator, shard_index=0, shard_count=0, shard_tile=0)
        f.update(over)
        return ptx.RenderCfg(**f)

    def call(scene, c, buf):
        rc = L.ptx_render_emission(scene, C.byref(c) if c is not None else None, buf, None)
        return rc, L.ptx_last_error().decode()
    for args in ((None, cfg(), em.ctypes.data), (s.h, None, em.ctypes.data), (s.h, cfg(), None)):
        rc, msg = call(*args)
        assert rc == ptx.ERR_INVALID and "ptx_render_emission" in msg and "NULL" in msg
    rc, msg = call(s.h, cfg(ptx.INTEGRATOR_WORKER), em.ctypes.data)
    assert rc == ptx.ERR_UNSUPPORTED and "WORKER" in msg and "ptx_render_emission" in msg
    rc, msg = call(s.h, cfg(7), em.ctypes.data)
    assert rc == ptx.ERR_INVALID and "integrator" in msg
    rc, msg = call(s.h, cfg(bounces=0xFFFFFF), em.ctypes.data)    # bounces are ignored: the scene's missing device speaks
    assert rc == ptx.ERR_NO_DEVICE and "GPU context" in msg
    assert not em.any()
    with pytest.raises(ptx.PtxError) as e:
        s.render_emission(W, H, SPP)
    assert e.value.code == ptx.ERR_NO_DEVICE


def _buffers():
    return [np.full((3, 5, 4), 7, f32) for _ in range(3)]


@pytest.mark.parametrize("which", ["split", "merge"])
def test_split_and_merge_refusals_need_no_device(ptx, which):
    L = ptx.lib()
    em, x, y = _buffers()
    fn = L.ptx_emission_split if which == "split" else L.ptx_emission_merge

    def call(e=em.ctypes.data, spp=8, n=15, p=x.ctypes.data, q=y.ctypes.data):
        rc = fn(None, e, spp, n, p, q) if which == "split" else fn(None, e, spp, n, p)
        return rc, L.ptx_last_error().decode()
    cases = [(dict(e=None), "NULL argument"), (dict(p=None), "NULL argument"), (dict(spp=0), "guide_spp"), (dict(n=0), "n_pixels"), (dict(n=2 ** 31), "n_pixels"),
             (dict(p=em.ctypes.data), "shares"), (dict(spp=0, n=0), "guide_spp"), (dict(e=None, spp=0), "NULL argument")]
    if which == "split":
        cases += [(dict(q=em.ctypes.data), "shares"), (dict(q=x.ctypes.data), "shares")]
    for kw, word in cases:
        rc, msg = call(**kw)
        assert rc == ptx.ERR_INVALID and f"ptx_emission_{which}" in msg and word in msg, (kw, rc, msg)
    for kw in (dict(),) + ((dict(q=None),) if which == "split" else ()):     # nothing else wrong: refused for its context
        rc, msg = call(**kw)
        assert rc == ptx.ERR_INVALID and "NULL context" in msg, (kw, msg)
    assert all((b == 7).all() for b in (em, x, y))


def test_the_wrappers_refuse_mismatched_shapes(ptx):
    ctx = ptx.Context.__new__(ptx.Context)
    ctx.h = None
    em, x, y = _buffers()
    with pytest.raises(ValueError):
        ctx.emission_split(em, 8, x[:2], y)
    with pytest.raises(ValueError):
        ctx.emission_split(em[..., :3], 8, x[..., :3])
    with pytest.raises(ValueError):
        ctx.emission_merge(em, 8, x[:, :4])
    with pytest.raises(ptx.PtxError) as e:     # shapes in order: the library refuses the NULL context
        ctx.emission_split(em, 8, x, y)
    assert "NULL context" in str(e.value)
    with pytest.raises(ptx.PtxError) as e:
        ctx.emission_merge(em, 8, x)
    assert "NULL context" in str(e.value)
