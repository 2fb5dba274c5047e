"""The transparent-background blend of the reference restated in float32 numpy, the alpha of a sample derived from the oracle, and the
scenes tests/test_transparent_background.py pins them on (tests/test_last_vertex.py and tests/test_material_chart.py use them too).
Not collected (underscore prefix); every assert carries its own message, since pytest does not rewrite asserts here.
"""
import numpy as np

from _common import _proc
from conftest import CORNELL, JACK, oracle_from_dict, product_from_dict


def _source(name):
    """('dict', flat arrays) of a procedural scene or ('gltf', path)."""
    if name == "plaza":
        return "dict", _proc().plaza_scene(3, sun=False, alpha=False)
    if name == "plaza_sun_alpha":
        return "dict", _proc().plaza_scene(3, sun=True, alpha=True)
    return "gltf", {"jack": JACK, "cornell": CORNELL}[name]


_oracles = {}


def _oracle(ora, name):
    if name not in _oracles:
        kind, src = _source(name)
        _oracles[name] = oracle_from_dict(ora, src) if kind == "dict" else ora.OracleScene(ora.load_gltf(src))
    return _oracles[name]


def _product_of(ptx, ctx, name):
    kind, src = _source(name)
    return product_from_dict(ptx, ctx, src) if kind == "dict" else ptx.Scene.load_gltf(ctx, src)


def _alpha_of(diff):
    """data.w of every sample from the differences: 0 where the difference is (1,1,1), 1 where it is (0,0,0); anything else fails."""
    assert ((diff == 0) | (diff == 1)).all(), ("a difference that is neither 0 nor 1", np.unique(diff[(diff != 0) & (diff != 1)])[:8])
    assert (diff[..., 0] == diff[..., 1]).all() and (diff[..., 0] == diff[..., 2]).all(), "the channels of a difference disagree"
    return (np.float32(1) - diff[..., 0]).astype(np.float32)


def blend_restatement(rgb, alpha, state=None, s0=0):
    """RESTATEMENT of core/renderer.cpp:374-399 (`if (transparent_background) { ... }` and the blend after it) in np.float32, over all
    pixels at once, one operation per reference operation. rgb [H,W,n,3], alpha [H,W,n] = trace()'s data of samples s0 .. s0+n-1;
    state = (color [H,W,3], alpha [H,W], claimed [H,W] bool) or None for the reference's initial {fvec3::zero, 0, false} (:350).
    `sample` is a uint32_t that the arithmetic promotes to float (vec3.inl:180-200, common_type<float, uint32_t>), except in
    `1 / (sample + 1)` (:378), which is an INTEGER division. Returns (color, alpha, claimed, per-branch sample counts)."""
    rgb, alpha = np.asarray(rgb, np.float32), np.asarray(alpha, np.float32)
    if state is None:
        color, a, claimed = np.zeros(rgb.shape[:2] + (3,), np.float32), np.zeros(rgb.shape[:2], np.float32), np.zeros(rgb.shape[:2], bool)
    else:
        color, a, claimed = (np.array(x) for x in state)
    counts = np.zeros(4, np.int64)
    for k in range(rgb.shape[2]):
        sample = s0 + k
        fs, fs1 = np.float32(sample), np.float32(sample + 1)
        data, w = rgb[:, :, k], alpha[:, :, k]
        claims = (w > 0.5) & ~claimed                    # :375  data.w > 0.5 && !claimed
        only_alpha = (w < 0.5) & claimed & ~claims       # :382  data.w < 0.5 && claimed
        nothing = (w < 0.5) & ~claimed                   # :388  data.w < 0.5 (unclaimed)
        blends = ~(claims | only_alpha | nothing)        # :394-398 everything else
        color[claims] = data[claims]                     # :377
        a[claims] = np.float32(1 // (sample + 1))        # :378  integer division: 1 for sample 0, else 0
        t = a[only_alpha] * fs + w[only_alpha]           # :384
        a[only_alpha] = t / fs1                          # :385
        c = color[blends] * fs + data[blends]            # :395
        color[blends] = c / fs1                          # :396
        t = a[blends] * fs + w[blends]                   # :397
        a[blends] = t / fs1                              # :398
        claimed = claimed | claims                       # :379
        counts += [claims.sum(), only_alpha.sum(), nothing.sum(), blends.sum()]
    assert color.dtype == np.float32 and a.dtype == np.float32, (color.dtype, a.dtype)
    return color, a, claimed, counts
