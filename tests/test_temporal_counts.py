"""ptx_denoise_temporal_counts without a GPU: what its specification promises, shown on the float32 numpy restatement
(tests/_temporal_counts_restatement.py), the exported symbol, the mirror's signature and every refusal of the C call.

The refusals are decided before any device work and the context is the last argument looked at, so each of them is met here with a NULL
context; a call with nothing else wrong is refused for that context. Pointers of mixed kinds need a device pointer:
tests/test_temporal_counts_gpu.py.
"""
import ctypes as C
import inspect

import numpy as np
import pytest

from _common import _same
from _denoise_counts_restatement import restate_counts
from _denoise_restatement import f32
from _temporal_counts_restatement import SEARCH_3X3, UNIT_NORMALS, accumulate, motion_sums, restate, synthetic
from _temporal_restatement import accumulate as accumulate_frames

SA, SB, NG = 3, 5, 8


def _frame(W=40, H=28, seed=1, mv=(0.0, 0.0)):
    a, b, A, N = synthetic(W, H, SA, SB, seed)
    return a, b, A, N, motion_sums(A, N, *mv)


# ---------------------------------------------------------------------------- consequence (a): uniform power-of-two counts
@pytest.mark.parametrize("mv", [(0, 0), (0.375, -1.25), (3, 2), (-2.5, 0.5)], ids=str)
@pytest.mark.parametrize("shape", [(1, 1), (7, 5), (65, 9), (130, 70)], ids=lambda s: f"{s[0]}x{s[1]}")
def test_uniform_power_of_two_counts_are_the_frame_counted_call_scaled(shape, mv):
    """Six frames, 3 + 5 samples each: the history counted in frames with max_history 4 and the one counted in samples with max_history 32
    agree bit for bit in everything but N, which is 8 times as large."""
    W, H = shape
    old = new = None
    shares = []
    for f in range(6):
        fr = _frame(W, H, f + 1, mv)
        so = accumulate_frames(*fr, SA, SB, prev=old, max_history=4)
        sn = accumulate(*fr, NG, prev=new, max_history=32)
        for k in ("col", "var", "g", "alb", "alpha"):
            _same(sn[k], so[k], f"frame {f}: {k}")
        _same(sn["next"][1], so["next"][1], f"frame {f}: moments")
        _same(sn["next"][2], so["next"][2], f"frame {f}: geometry")
        _same(sn["next"][0][..., :3], so["next"][0][..., :3], f"frame {f}: colour")
        _same(sn["next"][0][..., 3], so["next"][0][..., 3] * f32(8), f"frame {f}: N")
        np.testing.assert_array_equal(sn["took"], so["took"])
        old, new = so["next"], sn["next"]
        shares.append(float(sn["took"].mean()))
    assert shares[0] == 0
    if shape == (130, 70):
        print(f"motion {mv}: share of pixels that took history per frame {[round(s, 3) for s in shares]}")
        assert all(85 <= round(100 * s) <= 95 for s in shares[1:]), shares   # in whole per cent (95.08 at zero motion): the chain is exercised
        assert (new[0][..., 3] == 32).any() and (new[0][..., 3] == 8).any()   # the cap is met, and some pixels started over


def test_a_per_pixel_power_of_two_rescale_changes_only_the_counts():
    """Both half sums, counts included, times 2^((x + 2y) % 3) per pixel: col and var are the uniform frame's bit for bit, N' = 8 * 2^k; and
    again one frame later at zero motion, where each pixel reads its own history."""
    W, H = 40, 28
    yy, xx = np.mgrid[0:H, 0:W]
    k = ((xx + 2 * yy) % 3).astype(f32)
    scale = np.exp2(k)[..., None].astype(f32)
    prev_u = prev_s = None
    for f in range(2):
        a, b, A, N, M = _frame(W, H, f + 1)
        u = accumulate(a, b, A, N, M, NG, prev=prev_u)
        s = accumulate(a * scale, b * scale, A, N, M, NG, prev=prev_s)
        _same(s["col"], u["col"], f"frame {f}: col")
        _same(s["var"], u["var"], f"frame {f}: var")
        _same(s["next"][1], u["next"][1], f"frame {f}: moments")
        _same(s["next"][0][..., 3], u["next"][0][..., 3] * scale[..., 0], f"frame {f}: N'")
        np.testing.assert_array_equal(s["took"], u["took"])
        prev_u, prev_s = u["next"], s["next"]
    surface = A[..., 3] > 0
    np.testing.assert_array_equal(s["took"], surface)
    np.testing.assert_array_equal(s["next"][0][..., 3], np.where(surface, f32(16), f32(8)) * scale[..., 0])


# ---------------------------------------------------------------------------- consequences (b), (c)
def test_first_frame_is_ptx_denoise_counts_bit_for_bit():
    rng = np.random.default_rng(5)
    a, b, A, N, M = _frame()
    a, b = a.copy(), b.copy()
    ca, cb = (2 * rng.integers(1, 8, a.shape[:2])).astype(f32), (2 * rng.integers(1, 8, a.shape[:2])).astype(f32)
    a *= (ca / SA)[..., None]
    b *= (cb / SB)[..., None]
    assert (a[..., 3] == ca).all() and (b[..., 3] == cb).all()
    for it in (1, 5):
        for flags in (0, SEARCH_3X3 | UNIT_NORMALS):
            out, nxt, took = restate(a, b, A, N, M, NG, prev=None, iterations=it, sigma_l=3.0, sigma_n=0.7, sigma_z=0.25, flags=flags)
            _same(out, restate_counts(a, b, A, N, NG, iterations=it, sigma_l=3.0, sigma_n=0.7, sigma_z=0.25), f"first frame, {it} iterations")
            assert not took.any()
            np.testing.assert_array_equal(nxt[0][..., 3], ca + cb)


def test_the_history_is_the_pooled_mean_of_all_samples():
    """Three frames of 2 + 2, 8 + 8 and 3 + 3 samples over the same guides at zero motion: where history was taken the integrated colour is
    the mean of the 26 samples, to float32 rounding (measured: 1.7e-7 relative), and N' = 26."""
    W, H = 40, 28
    _, _, A, N, M = _frame(W, H)
    rng = np.random.default_rng(11)
    prev, total = None, np.zeros((H, W, 3), np.float64)
    for ca, cb in ((2, 2), (8, 8), (3, 3)):
        a = np.concatenate([rng.uniform(0.05, 2.0, (H, W, 3)) * ca, np.full((H, W, 1), ca)], -1).astype(f32)
        b = np.concatenate([rng.uniform(0.05, 2.0, (H, W, 3)) * cb, np.full((H, W, 1), cb)], -1).astype(f32)
        total += a[..., :3].astype(np.float64) + b[..., :3]
        s = accumulate(a, b, A, N, M, NG, prev=prev)
        prev = s["next"]
    took = s["took"]
    np.testing.assert_array_equal(took, A[..., 3] > 0)
    assert (s["next"][0][..., 3][took] == 26).all() and (s["next"][0][..., 3][~took] == 6).all()
    pooled = (total / 26) / s["alb"].astype(np.float64)
    err = float((np.abs(s["col"][took] - pooled[took]) / pooled[took]).max())
    print(f"pooled mean of 26 samples: worst relative error {err:.2e}")
    assert err < 1e-6


# ---------------------------------------------------------------------------- the two flags
def _holed_history(W, H, holes):
    fr = _frame(W, H)
    own = accumulate(*fr, NG)
    color = own["next"][0].copy()
    color[..., 3][holes] = 0
    return fr, own, (color, own["next"][1], own["next"][2])


def test_the_search_finds_history_the_four_taps_miss():
    """65 x 33, motion (1, 0): the one tap of weight 1 is a hole for a third of the pixels. Without the flag 61.5 % take history, with it
    95.5 %, 34 % through the search; a pixel whose four taps succeed is bitwise what it was."""
    W, H = 65, 33
    yy, xx = np.mgrid[0:H, 0:W]
    fr, own, prev = _holed_history(W, H, (xx // 2 + yy // 2) % 3 == 0)
    a, b, A, N, _ = fr
    M = motion_sums(A, N, 1, 0)
    s0 = accumulate(a, b, A, N, M, NG, prev=prev)
    s1 = accumulate(a, b, A, N, M, NG, prev=prev, flags=SEARCH_3X3)
    share0, share1, through = float(s0["took"].mean()), float(s1["took"].mean()), float(s1["searched"].mean())
    print(f"took history: {share0:.4f} without the search, {share1:.4f} with it, {through:.4f} through it")
    assert abs(share0 - 0.615) < 0.005 and abs(share1 - 0.955) < 0.005 and abs(through - 0.34) < 0.005
    assert not s0["searched"].any() and (s1["took"] >= s0["took"]).all()
    np.testing.assert_array_equal(s1["took"] & ~s1["searched"], s0["took"])
    keep = s0["took"]
    for k in ("col", "var"):
        _same(s1[k][keep], s0[k][keep], k)
    for i in range(2):
        _same(s1["next"][i][keep], s0["next"][i][keep], f"next[{i}]")
    # the searched pixels: whole taps, so sw is their number, and the mean of the taken texels' N (8 each) is 8
    sw = s1["sw"][s1["searched"]]
    assert (sw == np.round(sw)).all() and sw.min() >= 1 and sw.max() <= 9 and (sw > 1).any()
    assert (s1["next"][0][..., 3][s1["searched"]] == 16).all()
    # here every surface pixel finds a texel; the pixels without a surface sample have a zero normal and start over
    np.testing.assert_array_equal(s1["took"], A[..., 3] > 0)
    assert (s1["next"][0][..., 3][~s1["took"]] == 8).all()


@pytest.mark.parametrize("target,most", [((0, 0), 3), ((64, 0), 3), ((0, 32), 3), ((64, 32), 3), ((-1, -1), 1), ((65, -1), 1), ((-1, 33), 1), ((65, 33), 1),
                                         ((-2, 5), 0), ((66, 40), 0)], ids=str)
def test_the_search_at_and_beyond_the_image_corners(target, most):
    """Every pixel's motion leads to one position: a corner (made a hole, so that the four taps fail: three of the nine texels are inside), one
    step outside it (one texel inside, the corner), two steps outside (none). The taken texels are whole and inside the image."""
    W, H = 65, 33
    yy, xx = np.mgrid[0:H, 0:W]
    corners = ((xx == 0) | (xx == W - 1)) & ((yy == 0) | (yy == H - 1))
    fr, own, prev = _holed_history(W, H, corners & (most == 3))
    a, b, A, N, _ = fr
    cov = A[..., 3]
    M = np.stack([(f32(target[0]) - xx) * cov, (f32(target[1]) - yy) * cov, N[..., 3], cov], -1).astype(f32)
    M[..., 2] = np.where(cov > 0, prev[2][min(max(target[1], 1), H - 2), min(max(target[0], 1), W - 2), 3] * cov, 0)   # expect the depth found there
    s0 = accumulate(a, b, A, N, M, NG, prev=prev, tau_n=0.01)
    s1 = accumulate(a, b, A, N, M, NG, prev=prev, tau_n=0.01, flags=SEARCH_3X3)
    assert not s0["took"].any()
    assert s1["sw"].max() == most and (s1["sw"] == np.round(s1["sw"])).all()
    np.testing.assert_array_equal(s1["took"], s1["sw"] > 0)
    np.testing.assert_array_equal(s1["took"], s1["searched"])
    if most:        # the pixels that expect the depth found there take it, and only texels near the target were read: N' = 8 + 8
        assert s1["took"].sum() > 100 and (s1["next"][0][..., 3][s1["took"]] == 16).all()
    if most == 1:   # the one texel is the corner's: h is its history
        cy, cx = min(max(target[1], 0), H - 1), min(max(target[0], 0), W - 1)
        hcol = prev[0][cy, cx, :3]
        t = s1["took"]
        _same(s1["col"][t], (hcol + (own["col"][t] - hcol) * f32(0.5)).astype(f32), "blend with the corner texel")
    for x in s1["next"] + (s1["col"], s1["var"]):
        assert np.isfinite(x).all()


def test_unit_normals_let_a_short_mean_normal_match_itself():
    """The full-coverage pixels with x % 4 == 1 hold four samples of normal (0, 0, 1) and four of (0, 1, 0): |mean|^2 = 0.5 < tau_n. At zero
    motion against the frame's own history none of them takes history without the flag, all do with it; nothing else changes."""
    W, H = 65, 33
    a, b, A, N, M = _frame(W, H)
    yy, xx = np.mgrid[0:H, 0:W]
    bent = (A[..., 3] == NG) & (xx % 4 == 1)
    assert bent.sum() == 456
    N = N.copy()
    N[bent, :3] = (0, 4, 4)
    own = accumulate(a, b, A, N, M, NG)
    s0 = accumulate(a, b, A, N, M, NG, prev=own["next"])
    s1 = accumulate(a, b, A, N, M, NG, prev=own["next"], flags=UNIT_NORMALS)
    surface = A[..., 3] > 0
    np.testing.assert_array_equal(s0["took"], surface & ~bent)
    np.testing.assert_array_equal(s1["took"], surface)
    _same(s1["next"][2], own["next"][2], "the stored geometry stays the unnormalised mean")
    np.testing.assert_array_equal(s1["g"][bent][:, :3], np.broadcast_to(f32([0, 0.5, 0.5]), (456, 3)))
    for k in ("col", "var"):
        _same(s1[k][~bent], s0[k][~bent], k)
    # a cov == 0 pixel has a zero normal: NaN after the normalisation, and the test fails
    assert (~surface).any() and not s1["took"][~surface].any()


# ---------------------------------------------------------------------------- cap and resets
def test_max_history_below_the_frames_count_replaces_the_history():
    a, b, A, N, M = _frame()
    own = accumulate(a, b, A, N, M, NG)
    a2, b2, _, _, _ = _frame(seed=2)
    s = accumulate(a2, b2, A, N, M, NG, prev=own["next"], max_history=5)
    surface = A[..., 3] > 0
    np.testing.assert_array_equal(s["took"], surface)
    assert (s["next"][0][..., 3] == 8).all()          # N' = min(8 + 8, max(5, 8)) = n, a = 1
    first = accumulate(a2, b2, A, N, M, NG)
    np.testing.assert_allclose(s["col"], first["col"], rtol=2e-6)   # h + (col - h) * 1
    _same(s["var"], first["var"], "N' < 4 n: var = v0 * (n / n)")
    # the default: min(32 * guide_spp, 1048576) samples
    prev = own["next"]
    for _ in range(40):
        prev = accumulate(a, b, A, N, M, NG, prev=prev)["next"]
    assert prev[0][..., 3].max() == 256
    big = (own["next"][0].copy(), own["next"][1], own["next"][2])
    big[0][..., 3] = 2 ** 20
    assert accumulate(a, b, A, N, M, 40000, prev=big)["next"][0][..., 3].max() == 2 ** 20


def test_non_finite_motion_or_history_resets_the_pixel_and_the_next_frame_is_finite():
    a, b, A, N, M = _frame()
    own = accumulate(a, b, A, N, M, NG)
    color, moments, geometry = (x.copy() for x in own["next"])
    M = M.copy()
    pm_nan, pm_inf, pm_far, pm_w, ph_col, ph_mom, ph_n, ph_z = (1, 1), (2, 8), (3, 9), (4, 10), (5, 2), (12, 3), (15, 8), (22, 5)   # no two are neighbours
    M[pm_nan][0] = np.nan
    M[pm_inf][1] = np.inf
    M[pm_far][0] = f32(1e9) * M[pm_far][3]
    M[pm_w][3] = np.nan
    color[ph_col][1] = np.nan
    moments[ph_mom][1] = np.inf
    color[ph_n][3] = np.nan
    geometry[ph_z][3] = np.nan
    bad = (pm_nan, pm_inf, pm_far, pm_w, ph_col, ph_mom, ph_n, ph_z)
    surface = A[..., 3] > 0
    assert all(surface[p] for p in bad)
    for flags in (0, SEARCH_3X3, UNIT_NORMALS, SEARCH_3X3 | UNIT_NORMALS):
        s1 = accumulate(a, b, A, N, M, NG, prev=(color, moments, geometry), flags=flags)
        want = surface.copy()
        for p in bad:
            want[p] = False
        if flags & SEARCH_3X3:   # a damaged texel is the one tap of its own pixel: the search finds the neighbours' (the motion stays unusable)
            for p in (ph_n, ph_z):
                want[p] = True
            assert s1["searched"][ph_n] and s1["searched"][ph_z] and s1["searched"].sum() == 2
        np.testing.assert_array_equal(s1["took"], want)
        for x in s1["next"] + (s1["col"], s1["var"]):
            assert np.isfinite(x).all()
        np.testing.assert_array_equal(s1["next"][0][..., 3], np.where(want, f32(16), f32(8)))
    s2 = accumulate(a, b, A, N, motion_sums(A, N), NG, prev=s1["next"])
    np.testing.assert_array_equal(s2["took"], surface)
    assert np.isfinite(s2["col"]).all()


def test_a_pixel_without_samples_starts_over_and_is_never_a_tap():
    a, b, A, N, M = _frame()
    a, b = a.copy(), b.copy()
    empty = (9, 12)
    a[empty], b[empty] = 0, 0
    s1 = accumulate(a, b, A, N, M, NG)
    assert s1["next"][0][empty][3] == 0 and not np.isfinite(s1["col"][empty]).all()
    s2 = accumulate(a, b, A, N, motion_sums(A, N, 0.5, 0.5), NG, prev=s1["next"], flags=SEARCH_3X3)
    assert not s2["took"][empty] and s2["next"][0][empty][3] == 0
    others = np.ones(a.shape[:2], bool)
    others[empty] = False
    assert np.isfinite(s2["col"][others]).all() and np.isfinite(s2["next"][1][others]).all()


# ---------------------------------------------------------------------------- the C call
def test_symbol_is_declared_and_exported(ptx):
    assert "ptx_denoise_temporal_counts" in ptx.declared_symbols() and hasattr(ptx.lib(), "ptx_denoise_temporal_counts")
    assert (ptx.TEMPORAL_SEARCH_3X3, ptx.TEMPORAL_UNIT_NORMALS) == (1, 2)
    assert [n for n, _ in ptx.TemporalCountsCfg._fields_] == ["W", "H", "guide_spp", "iterations", "sigma_l", "sigma_n", "sigma_z", "max_history", "tau_z", "tau_n",
                                                               "flags"]
    assert C.sizeof(ptx.TemporalCountsCfg) == 44


def test_the_mirrors_signature(ptx):
    sig = inspect.signature(ptx.Context.denoise_temporal_counts)
    names = list(sig.parameters)
    assert names[:9] == ["self", "a", "b", "albedo_cov", "normal_depth", "motion", "guide_spp", "prev", "next"]
    assert sig.parameters["prev"].default is None and sig.parameters["next"].default is None and sig.parameters["flags"].default == 0
    old = inspect.signature(ptx.Context.denoise_temporal).parameters
    for k in ("iterations", "sigma_l", "sigma_n", "sigma_z", "max_history", "tau_z", "tau_n", "out", "want_out", "want_stats"):
        assert sig.parameters[k].default == old[k].default, k


def _call(ptx, null=(), share=None, prev_given=True, **cfg_over):
    """One C call on 5 x 3 host buffers with a NULL context -> (code, message, the buffers that must stay untouched)."""
    L = ptx.lib()
    a, b, A, N = synthetic(5, 3, SA, SB)
    M = motion_sums(A, N)
    mk = lambda c: np.full((3, 5, c), 7, f32)
    prev, nxt, out = [mk(4), mk(2), mk(4)], [mk(4), mk(2), mk(4)], mk(4)
    fields = dict(W=5, H=3, guide_spp=NG, iterations=0, sigma_l=0, sigma_n=0, sigma_z=0, max_history=0, tau_z=0, tau_n=0, flags=0)
    fields.update(cfg_over)
    c = ptx.TemporalCountsCfg(**fields)
    p = lambda name, x: None if name in null else x.ctypes.data
    guides = ptx.AovBuffers(p("albedo_cov", A), p("normal_depth", N))
    h_prev = ptx.TemporalHistory(p("prev.color", prev[0]), p("prev.moments", prev[1]), p("prev.geometry", prev[2]))
    h_next = ptx.TemporalHistory(p("next.color", nxt[0]), p("next.moments", nxt[1]), p("next.geometry", nxt[2]))
    if share:
        setattr(h_next, share[0], getattr(h_prev, share[1]))
    rc = L.ptx_denoise_temporal_counts(None, None if "cfg" in null else C.byref(c), p("accum_a", a), p("accum_b", b), None if "guides" in null else C.byref(guides),
                                       p("motion", M), C.byref(h_prev) if prev_given else None, None if "next" in null else C.byref(h_next), p("out", out), None)
    return rc, L.ptx_last_error().decode(), nxt + [out]


REFUSALS = [
    (dict(null=("cfg",)), "NULL argument"), (dict(null=("accum_a",)), "NULL argument"), (dict(null=("accum_b",)), "NULL argument"),
    (dict(null=("guides",)), "NULL argument"), (dict(null=("motion",)), "NULL argument"), (dict(null=("next",)), "NULL argument"),
    (dict(null=("albedo_cov",)), "guide"), (dict(null=("normal_depth",)), "guide"),
    (dict(null=("next.color",)), "member of next"), (dict(null=("next.moments",)), "member of next"), (dict(null=("next.geometry",)), "member of next"),
    (dict(null=("prev.color",)), "member of prev"), (dict(null=("prev.moments",)), "member of prev"), (dict(null=("prev.geometry",)), "member of prev"),
    (dict(share=("color", "color")), "shares"), (dict(share=("geometry", "geometry")), "shares"), (dict(share=("moments", "moments")), "shares"),
    (dict(share=("color", "geometry")), "shares"),
    (dict(W=0), "W and H"), (dict(H=16385), "W and H"), (dict(guide_spp=0), "guide_spp"), (dict(iterations=9), "iterations"),
    (dict(sigma_l=-1.0), "sigma"), (dict(sigma_n=float("nan")), "sigma"), (dict(sigma_z=-0.5), "sigma"),
    (dict(max_history=1048577), "max_history"), (dict(tau_z=-0.1), "tau"), (dict(tau_n=float("nan")), "tau"), (dict(tau_n=-1.0), "tau"),
    (dict(flags=4), "flags"), (dict(flags=0x80000001), "flags"), (dict(flags=7), "flags"),
]


@pytest.mark.parametrize("kw,msg", REFUSALS, ids=[f"{i}-{m.split()[0]}" for i, (_, m) in enumerate(REFUSALS)])
def test_refusals_are_decided_before_the_context_is_looked_at(ptx, kw, msg):
    rc, err, untouched = _call(ptx, **kw)
    assert rc == ptx.ERR_INVALID and "ptx_denoise_temporal_counts" in err and msg in err, (rc, err)
    assert all((x == 7).all() for x in untouched)


def test_the_order_of_the_refusals_is_the_frame_counted_calls(ptx):
    """Two things wrong at once: the earlier rule of ptx_denoise_temporal's order speaks."""
    for kw, msg in ((dict(W=0, guide_spp=0), "W and H"), (dict(guide_spp=0, iterations=9), "guide_spp"), (dict(iterations=9, sigma_l=-1.0), "iterations"),
                    (dict(sigma_l=-1.0, max_history=1048577), "sigma"), (dict(max_history=1048577, tau_z=-1.0), "max_history"), (dict(tau_z=-1.0, flags=4), "tau"),
                    (dict(null=("next.color",), flags=4), "member of next")):
        rc, err, _ = _call(ptx, **kw)
        assert rc == ptx.ERR_INVALID and msg in err, (kw, err)


def test_a_call_with_nothing_else_wrong_is_refused_for_its_context(ptx):
    for kw in (dict(), dict(prev_given=False), dict(null=("out",)), dict(max_history=1048576, iterations=8, tau_z=0.5, tau_n=0.5, flags=3), dict(flags=1), dict(flags=2),
               dict(max_history=1025)):
        rc, err, untouched = _call(ptx, **kw)
        assert rc == ptx.ERR_INVALID and "NULL context" in err and "ptx_denoise_temporal_counts" in err, (kw, rc, err)
        assert all((x == 7).all() for x in untouched)


def test_the_wrapper_refuses_mismatched_shapes(ptx):
    a, b, A, N = synthetic(5, 3, SA, SB)
    M = motion_sums(A, N)
    ctx = ptx.Context.__new__(ptx.Context)
    ctx.h = None
    hist = (np.zeros((3, 5, 4), f32), np.zeros((3, 5, 2), f32), np.zeros((3, 5, 4), f32))
    for bad in ((a[:, :4], b, A, N, M), (a, b, A, N, M[:2]), (a, b, A, N, M[..., :3])):
        with pytest.raises(ValueError):
            ctx.denoise_temporal_counts(*bad, NG)
    with pytest.raises(ValueError):
        ctx.denoise_temporal_counts(a, b, A, N, M, NG, prev=(hist[0], hist[0], hist[2]))
    with pytest.raises(ValueError):
        ctx.denoise_temporal_counts(a, b, A, N, M, NG, next=hist[:2])
    with pytest.raises(ptx.PtxError) as e:   # shapes in order: the library refuses the NULL context
        ctx.denoise_temporal_counts(a, b, A, N, M, NG, prev=hist, flags=3)
    assert "NULL context" in str(e.value)
