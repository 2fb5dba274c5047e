"""ptx_denoise_counts: ptx_denoise for half-buffers that carry a per-pixel sample count in .w (include/ptx.h).

Only step 1 of the filter changes, so the restatement (tests/_denoise_counts_restatement.py) is pinned on the CPU against the existing one
(tests/_denoise_restatement.py) from both sides — uniform counts give its bits, and a per-pixel power-of-two rescaling of the halves, counts
included, changes nothing — and the product is then held to the restatement bit for bit: nothing on this path goes through libm.
"""
import ctypes as C

import numpy as np
import pytest

import _denoise_counts_restatement as DR
import _denoise_restatement as D0
from _common import _same
from _routes import ctx  # noqa: F401  (fixture)

f32 = np.float32


# ---------------------------------------------------------------------------- CPU: the restatement against the existing one
@pytest.mark.parametrize("spp_a,spp_b", [(4, 4), (3, 5)])
def test_uniform_counts_give_the_existing_restatement_bitwise(spp_a, spp_b):
    a, b, A, N, ng = DR.synthetic(23, 37, 1, uniform=(spp_a, spp_b))
    assert ng == spp_a + spp_b and (a[..., 3] == spp_a).all() and (b[..., 3] == spp_b).all()
    for it in (1, 3):
        _same(DR.restate_counts(a, b, A, N, ng, iterations=it), D0.restate(a, b, A, N, spp_a, spp_b, iterations=it), f"{it} iterations")


def test_per_pixel_power_of_two_scaling_changes_nothing():
    """a and b of pixel p times 2^k_p, counts included: every quotient of step 1 is unchanged exactly, so the output is, bit for bit. With
    uniform counts before the scaling this ties per-pixel counts to the existing restatement."""
    a, b, A, N, ng = DR.synthetic(23, 37, 2, uniform=(4, 4))
    want = D0.restate(a, b, A, N, 4, 4)
    rng = np.random.default_rng(3)
    sa, sb = (f32(2) ** rng.integers(-2, 5, (23, 37, 1))).astype(f32), (f32(2) ** rng.integers(-2, 5, (23, 37, 1))).astype(f32)
    assert len(np.unique(sa)) > 3
    # the two halves of a pixel must keep their ratio: (a + b) / (na + nb) is scale-free only under a common factor
    _same(DR.restate_counts(a * sa, b * sa, A, N, ng), want, "common per-pixel factor")
    # each half on its own factor changes the weights of the halves in the pixel's mean, and must change the output
    assert (DR.restate_counts(a * sa, b * sb, A, N, ng).view(np.uint32) != want.view(np.uint32)).any()
    # per-pixel counts proper: random counts against the same means
    a2, b2, A2, N2, ng2 = DR.synthetic(23, 37, 4)
    assert len(np.unique(a2[..., 3])) > 8 and ng2 == 8
    _same(DR.restate_counts(a2 * sa, b2 * sa, A2, N2, ng2), DR.restate_counts(a2, b2, A2, N2, ng2), "random counts, common per-pixel factor")


def test_zero_counts():
    """What step 1 as written gives. Both halves empty: n = 0, the colour is NaN, and the filter treats the pixel as it treats every
    non-finite one — it stays itself and no other pixel becomes non-finite. ONE half empty (b.w == 0 here): only the noise estimate is NaN
    (mb = 0 / 0), the colour (a + b) / n is finite, so the output is finite everywhere; the pixel is never filtered and keeps its own mean."""
    a, b, A, N, ng = DR.synthetic(23, 37, 5)
    a[5, 30], b[5, 30] = 0, 0
    b[11, 20] = 0
    out = DR.restate_counts(a, b, A, N, ng)
    bad = ~np.isfinite(out).all(-1)
    assert bad[5, 30] and bad.sum() == 1
    alb = np.fmax((A[11, 20, :3] + (f32(ng) - A[11, 20, 3])) / f32(ng), f32(0.001))
    own = ((a[11, 20, :3] / a[11, 20, 3]) / alb) * alb
    np.testing.assert_allclose(out[11, 20, :3], own, rtol=1e-5)   # centre tap only, iteration after iteration: (h * c) / h
    assert out[11, 20, 3] == 1


# ---------------------------------------------------------------------------- CPU: refusals
def _refusal_cases(ptx, ctx_h, a, b, A, N, out):
    ok = ptx.DenoiseCountsCfg(8, 4, 8, 0, 0, 0, 0)
    g = ptx.AovBuffers(A.ctypes.data, N.ctypes.data)
    pa, pb, po = a.ctypes.data, b.ctypes.data, out.ctypes.data
    nan = float("nan")
    cases = [((ctx_h, None, pa, pb, g, po), "NULL"), ((ctx_h, ok, None, pb, g, po), "NULL"), ((ctx_h, ok, pa, None, g, po), "NULL"), ((ctx_h, ok, pa, pb, None, po), "NULL"),
             ((ctx_h, ok, pa, pb, g, None), "NULL"), ((ctx_h, ok, pa, pb, ptx.AovBuffers(A.ctypes.data, None), po), "guide"),
             ((ctx_h, ptx.DenoiseCountsCfg(8, 4, 0, 0, 0, 0, 0), pa, pb, g, po), "guide_spp"), ((ctx_h, ptx.DenoiseCountsCfg(0, 4, 8, 0, 0, 0, 0), pa, pb, g, po), "W and H"),
             ((ctx_h, ptx.DenoiseCountsCfg(8, 16385, 8, 0, 0, 0, 0), pa, pb, g, po), "W and H"), ((ctx_h, ptx.DenoiseCountsCfg(8, 4, 8, 9, 0, 0, 0), pa, pb, g, po), "iterations"),
             ((ctx_h, ptx.DenoiseCountsCfg(8, 4, 8, 0, nan, 0, 0), pa, pb, g, po), "sigma"), ((ctx_h, ptx.DenoiseCountsCfg(8, 4, 8, 0, 0, -1.0, 0), pa, pb, g, po), "sigma"),
             ((ctx_h, ptx.DenoiseCountsCfg(8, 4, 8, 0, 0, 0, nan), pa, pb, g, po), "sigma")]
    return cases


def _call(ptx, args):
    c, cfg, pa, pb, g, po = args
    rc = ptx.lib().ptx_denoise_counts(c, C.byref(cfg) if cfg is not None else None, pa, pb, C.byref(g) if g is not None else None, po, None)
    return rc, ptx.lib().ptx_last_error().decode()


def test_refusals_without_a_context(ptx):
    a, b, A, N, out = (np.zeros((4, 8, 4), f32) for _ in range(5))
    rc, msg = _call(ptx, (None, ptx.DenoiseCountsCfg(8, 4, 8, 0, 0, 0, 0), a.ctypes.data, b.ctypes.data, ptx.AovBuffers(A.ctypes.data, N.ctypes.data), out.ctypes.data))
    assert rc == ptx.ERR_INVALID and "ptx_denoise_counts" in msg and "NULL" in msg, (rc, msg)
    # there is no context without a GPU: with a NULL one every faulty call is refused all the same, and nothing is touched
    for args, word in _refusal_cases(ptx, None, a, b, A, N, out):
        rc, msg = _call(ptx, args)
        assert rc == ptx.ERR_INVALID and "ptx_denoise_counts" in msg, (rc, msg, word)
    assert not out.any()


# ---------------------------------------------------------------------------- GPU
SIZES = [(1, 1), (7, 5), (70, 40), (130, 70)]   # w x h: one pixel, less than a tile, ragged tiles, more than one workgroup in both directions


@pytest.mark.gpu
@pytest.mark.parametrize("tiled", ["0", "0xff"])
@pytest.mark.parametrize("w,h", SIZES, ids=[f"{w}x{h}" for w, h in SIZES])
def test_bitwise_against_the_restatement(ptx, ctx, monkeypatch, w, h, tiled):
    import torch
    monkeypatch.setenv("PTX_DENOISE_TILED", tiled)
    a, b, A, N, ng = DR.synthetic(h, w, 100 + w)
    if w * h > 1:
        b[h // 2, w // 2] = 0   # a zero half count: a NaN noise estimate on a finite colour
        a[0, w - 1], b[0, w - 1] = 0, 0   # both: a non-finite pixel
    for it in (1, 3, 5, 8):
        want = DR.restate_counts(a, b, A, N, ng, iterations=it)
        got, st = ctx.denoise_counts(a, b, A, N, ng, iterations=it)
        _same(got, want, f"host, {it} iterations")
        assert st["iterations"] == it and st["kernel_ms"] > 0 and st["workspace_bytes"] == 8 * w * h * 16
    if w * h > 1:
        assert not np.isfinite(want[0, w - 1]).all() and (~np.isfinite(want).all(-1)).sum() == 1
    want = DR.restate_counts(a, b, A, N, ng)
    dev = [torch.from_numpy(x).to("cuda:0") for x in (a, b, A, N)]
    torch.cuda.synchronize()
    out, st = ctx.denoise_counts(*dev, ng)
    _same(out.cpu().numpy(), want, "device")
    assert st["iterations"] == 5 and st["workspace_bytes"] == 4 * w * h * 16
    out, none = ctx.denoise_counts(*dev, ng, out=dev[0], want_stats=False)   # out aliasing accum_a, no stats
    ctx.synchronize()
    assert out is dev[0] and none is None
    _same(out.cpu().numpy(), want, "device, out = accum_a")
    mine = a.copy()
    assert ctx.denoise_counts(mine, b, A, N, ng, out=mine)[0] is mine
    _same(mine, want, "host, out = accum_a")
    _same(ctx.denoise_counts(a, b, A, N, ng, sigma_l=2.0, sigma_n=0.25, sigma_z=0.5)[0], DR.restate_counts(a, b, A, N, ng, 5, 2.0, 0.25, 0.5), "sigmas of its own")


@pytest.mark.gpu
def test_uniform_counts_are_ptx_denoise_bitwise(ptx, ctx):
    a, b, A, N, ng = DR.synthetic(40, 70, 9, uniform=(3, 5))
    for it in (1, 5):
        _same(ctx.denoise_counts(a, b, A, N, ng, iterations=it)[0], ctx.denoise(a, b, A, N, 3, 5, iterations=it)[0], f"{it} iterations")


@pytest.mark.gpu
def test_refusals_with_a_live_context(ptx, ctx):
    import torch
    a, b, A, N, out = (np.zeros((4, 8, 4), f32) for _ in range(5))
    for args, word in _refusal_cases(ptx, ctx.h, a, b, A, N, out):
        rc, msg = _call(ptx, args)
        assert rc == ptx.ERR_INVALID and "ptx_denoise_counts" in msg and word in msg, (rc, msg, word)
    d = torch.zeros((4, 8, 4), device="cuda:0")
    torch.cuda.synchronize()
    with pytest.raises(ptx.PtxError) as e:
        ctx.denoise_counts(a, b, A, d, 8)
    assert e.value.code == ptx.ERR_INVALID and "all" in str(e.value)
    assert not out.any()
