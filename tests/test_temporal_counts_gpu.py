"""ptx_denoise_temporal_counts on the GPU, bit for bit against the float32 numpy restatement of its specification
(tests/_temporal_counts_restatement.py; tests/test_temporal_counts.py shows on the CPU that the restatement does what the specification
promises), against the calls it generalises, and end to end on adaptive frames of an orbit.

Nothing on this path goes through libm but the correctly rounded square root and division, so the product is held to BITWISE equality:
the output, the three history buffers, NaN positions included, and the two counters.
"""
import numpy as np
import pytest

from _common import _same
from _denoise_restatement import f32
from _routes import ctx  # noqa: F401  (a fixture)
from _temporal_counts_restatement import SEARCH_3X3, UNIT_NORMALS, accumulate, filter_tail, motion_sums, synthetic

NG = 8
SHAPES = [(1, 1), (7, 5), (65, 9), (130, 70)]
KNOBS = dict(sigma_l=3.0, sigma_n=0.7, sigma_z=0.25, max_history=40, tau_z=0.2, tau_n=0.8)
TKNOBS = {k: KNOBS[k] for k in ("max_history", "tau_z", "tau_n")}
SIGMAS = {k: KNOBS[k] for k in ("sigma_l", "sigma_n", "sigma_z")}


def _counted(W, H, seed, rng):
    """synthetic()'s frame with per-pixel even counts 2 .. 14 in each half, drawn independently, and the normals of the full-coverage pixels
    with x % 4 == 1 bent to a mean of length sqrt(0.5)."""
    a, b, A, N = synthetic(W, H, 3, 5, seed=seed)
    ca, cb = (2 * rng.integers(1, 8, (H, W))).astype(f32), (2 * rng.integers(1, 8, (H, W))).astype(f32)
    a, b = (a * (ca / f32(3))[..., None]).astype(f32), (b * (cb / f32(5))[..., None]).astype(f32)
    a[..., 3], b[..., 3] = ca, cb
    N = N.copy()
    bent = (A[..., 3] == NG) & (np.arange(W)[None, :] % 4 == 1)
    N[bent, :3] = (0, 4, 4)
    return a, b, A, N


_CASES = {}


def case(W, H):
    """The current frame, a wild motion and a damaged history of another frame with the same geometry (the damage of
    tests/test_temporal_gpu.py, and blocks of holes for the search). Motion: fractional everywhere (up to +-3 pixels, so that pixels near the
    border look outside), and single pixels that leave the image by far, hold NaN, an infinity or 1e9 pixels, or have a zero or negative
    count. History: one frame old in one half of the image and two frames old in the other, with 2 x 2 blocks of N = 0, single holes, and NaN
    colour, moments and depth entries. Made once per shape; nothing modifies it."""
    if (W, H) in _CASES:
        return _CASES[(W, H)]
    rng = np.random.default_rng(7 + 1000 * W + H)
    a, b, A, N = _counted(W, H, 1, rng)
    cov = A[..., 3]
    reach = min(3.0, max(W, H) / 4)   # the smallest buffers keep a tap inside
    mv = rng.uniform(-reach, reach, (H, W, 2)).astype(f32)
    M = np.stack([mv[..., 0] * cov, mv[..., 1] * cov, N[..., 3] * rng.uniform(0.9, 1.1, (H, W)).astype(f32), cov], -1).astype(f32)
    pa, pb, pA, pN = _counted(W, H, 2, rng)
    h0 = accumulate(pa, pb, pA, pN, motion_sums(pA, pN), NG)["next"]
    h1 = accumulate(pa, pb, pA, pN, motion_sums(pA, pN), NG, prev=h0, max_history=KNOBS["max_history"])["next"]
    left = (np.arange(W) * 2 < W)[None, :, None]
    prev = [np.where(left, x0, x1).astype(f32) for x0, x1 in zip(h0, h1)]
    yy, xx = np.mgrid[0:H, 0:W]
    prev[0][..., 3][((xx // 2 + yy // 2) % 3 == 0) & (yy * 2 >= H)] = 0   # blocks of holes in the lower half
    n = W * H
    if n >= 6:
        pick = rng.permutation(n)
        at = lambda k: np.unravel_index(pick[k::12][:max(n // 40, 1)], (H, W))
        M[at(0) + (0,)] = f32(4 * W) * M[at(0) + (3,)]      # leaves the image
        M[at(1) + (1,)] = np.nan
        M[at(2) + (0,)] = np.inf
        M[at(3) + (1,)] = f32(-1e9) * M[at(3) + (3,)]
        M[at(4) + (3,)] = 0
        M[at(5) + (3,)] = -2
        M[at(6) + (2,)] = np.nan
        prev[0][at(7) + (3,)] = 0                            # holes
        prev[0][at(8) + (1,)] = np.nan
        prev[1][at(9) + (0,)] = np.nan
        prev[1][at(10) + (1,)] = np.inf
        prev[2][at(11) + (3,)] = np.nan
    for x in (a, b, A, N, M) + tuple(prev):
        x.setflags(write=False)
    _CASES[(W, H)] = (a, b, A, N, M), tuple(prev)
    return _CASES[(W, H)]


def _check(got_out, got_next, want_out, want_next, what):
    if want_out is not None:
        _same(got_out, want_out, f"{what}: out")
    for name, g, w in zip(("color", "moments", "geometry"), got_next, want_next):
        _same(g, w, f"{what}: next.{name}")


# ---------------------------------------------------------------------------- bitwise against the restatement
@pytest.mark.gpu
@pytest.mark.parametrize("flags", [0, SEARCH_3X3, UNIT_NORMALS, SEARCH_3X3 | UNIT_NORMALS], ids=["plain", "search", "unit", "search+unit"])
@pytest.mark.parametrize("shape", SHAPES, ids=lambda s: f"{s[0]}x{s[1]}")
def test_synthetic_buffers_bitwise(ptx, ctx, monkeypatch, shape, flags):
    """Each flag combination, at 1, 5 and 8 iterations, in the global, the LDS-tiled and the mixed a-trous form; the counters."""
    W, H = shape
    frame, prev = case(W, H)
    s = accumulate(*frame, NG, prev=prev, flags=flags, **TKNOBS)
    took = s["took"]
    if W * H >= 300:
        plain = accumulate(*frame, NG, prev=prev, flags=0, **TKNOBS)["took"]
        assert took.mean() > 0.2 and (~took).mean() > 0.05, took.mean()
        assert np.isfinite(s["next"][0]).all() and np.isfinite(s["next"][1]).all()
        assert len(np.unique(s["next"][0][..., 3])) > 20                      # many history lengths
        if flags & SEARCH_3X3:
            assert s["searched"].sum() > 0.02 * W * H, s["searched"].sum()    # the search is exercised ...
        if flags & UNIT_NORMALS:
            assert (took & ~plain).sum() > 0.02 * W * H                       # ... and so is the normalisation
    for iterations, tiled in ((1, None), (5, 0xFF), (8, 0x55)):
        if tiled is None:
            monkeypatch.delenv("PTX_DENOISE_TILED", raising=False)
        else:
            monkeypatch.setenv("PTX_DENOISE_TILED", hex(tiled))
        want_out = filter_tail(s["col"], s["var"], s["g"], s["alb"], s["alpha"], iterations, **SIGMAS)
        out, nxt, st = ctx.denoise_temporal_counts(*frame, NG, prev=prev, iterations=iterations, flags=flags, **KNOBS)
        _check(out, nxt, want_out, s["next"], f"{iterations} iterations, tiled mask {tiled}")
        assert st["iterations"] == iterations
        assert (st["reprojected"], st["reset"]) == (int(took.sum()), W * H - int(took.sum())), st


@pytest.mark.gpu
def test_default_knobs_and_a_second_frame(ptx, ctx):
    """max_history (32 * guide_spp samples), the taus, the sigmas and the iterations at their defaults; the history the call returned goes into
    the next call."""
    frame, prev = case(65, 9)
    s = accumulate(*frame, NG, prev=prev)
    out, nxt, st = ctx.denoise_temporal_counts(*frame, NG, prev=prev)
    _check(out, nxt, filter_tail(s["col"], s["var"], s["g"], s["alb"], s["alpha"]), s["next"], "defaults")
    a, b, A, N, _ = frame
    s2 = accumulate(a, b, A, N, motion_sums(A, N), NG, prev=s["next"], flags=3)
    out2, nxt2, st2 = ctx.denoise_temporal_counts(a, b, A, N, motion_sums(A, N), NG, prev=nxt, flags=3)
    _check(out2, nxt2, filter_tail(s2["col"], s2["var"], s2["g"], s2["alb"], s2["alpha"]), s2["next"], "second frame")
    assert st2["reprojected"] == int(s2["took"].sum()) == int((A[..., 3] > 0).sum())


@pytest.mark.gpu
def test_the_search_at_the_image_corners_and_far_outside(ptx, ctx):
    """Every pixel's motion leads to one position: on a corner whose texel is a hole (three of the nine texels inside), one step outside it (one
    inside, the corner's, here not a hole), and as far outside as a usable motion goes, where every fetch is clamped and nothing is taken.
    Bitwise the restatement."""
    W, H = 65, 33
    a, b, A, N = synthetic(W, H, 3, 5, seed=1)
    own = accumulate(a, b, A, N, motion_sums(A, N), NG)["next"]
    yy, xx = np.mgrid[0:H, 0:W]
    color = own[0].copy()
    color[..., 3][((xx == 0) | (xx == W - 1)) & ((yy == 0) | (yy == H - 1))] = 0
    holed = (color, own[1], own[2])
    cov = A[..., 3]
    searched = 0
    for tx, ty in ((0, 0), (W - 1, H - 1), (-1, -1), (W, -1), (-1, H), (W, H), (32767.5, -32767.5), (-32767.5, 32767.5), (40000, 3)):
        prev = holed if 0 <= tx < W else own   # on a corner the hole makes the four taps fail; outside, the corner's texel is the one to find
        M = np.stack([(f32(tx) - xx) * cov, (f32(ty) - yy) * cov, N[..., 3], cov], -1).astype(f32)
        s = accumulate(a, b, A, N, M, NG, prev=prev, tau_z=0.5, tau_n=0.01, flags=SEARCH_3X3)
        out, nxt, st = ctx.denoise_temporal_counts(a, b, A, N, M, NG, prev=prev, tau_z=0.5, tau_n=0.01, flags=SEARCH_3X3, iterations=1)
        _check(out, nxt, filter_tail(s["col"], s["var"], s["g"], s["alb"], s["alpha"], 1), s["next"], f"target ({tx}, {ty})")
        assert st["reprojected"] == int(s["took"].sum()) == int(s["searched"].sum())
        assert (st["reprojected"] > 0) == (max(abs(tx), abs(ty)) < 100), (tx, ty, st)
        searched += st["reprojected"]
    assert searched > 1000


# ---------------------------------------------------------------------------- bitwise against the product
@pytest.mark.gpu
def test_without_prev_the_output_is_ptx_denoise_counts(ptx, ctx):
    frame, _ = case(65, 9)
    a, b, A, N, M = frame
    for it, flags in ((0, 0), (1, 3), (8, 1)):
        out, nxt, st = ctx.denoise_temporal_counts(*frame, NG, prev=None, iterations=it, flags=flags, **KNOBS)
        ref, _ = ctx.denoise_counts(a, b, A, N, NG, iterations=it, **SIGMAS)
        _same(out, ref, f"prev = NULL, iterations {it}")
        assert (st["reprojected"], st["reset"]) == (0, 65 * 9)
        np.testing.assert_array_equal(nxt[0][..., 3], a[..., 3] + b[..., 3])
        _check(None, nxt, None, accumulate(*frame, NG, prev=None, **TKNOBS)["next"], "first frame's history")


@pytest.mark.gpu
def test_uniform_power_of_two_frames_are_ptx_denoise_temporal(ptx, ctx):
    """Three frames of 3 + 5 samples with fractional motion: max_history 4 frames there, 32 samples here. Everything but N agrees bit for
    bit, and N is 8 times as large."""
    W, H = 130, 70
    old = new = None
    for f in range(3):
        a, b, A, N = synthetic(W, H, 3, 5, seed=f + 1)
        M = motion_sums(A, N, 0.375, -1.25)
        out_o, old, st_o = ctx.denoise_temporal(a, b, A, N, M, 3, 5, prev=old, max_history=4)
        out_n, new, st_n = ctx.denoise_temporal_counts(a, b, A, N, M, NG, prev=new, max_history=32)
        _same(out_n, out_o, f"frame {f}: out")
        _same(new[0][..., :3], old[0][..., :3], f"frame {f}: colour")
        _same(new[0][..., 3], old[0][..., 3] * f32(8), f"frame {f}: N")
        _same(new[1], old[1], f"frame {f}: moments")
        _same(new[2], old[2], f"frame {f}: geometry")
        assert (st_n["reprojected"], st_n["reset"]) == (st_o["reprojected"], st_o["reset"])
    assert st_n["reprojected"] > 0.8 * W * H and (new[0][..., 3] == 24).any()


@pytest.mark.gpu
def test_advancing_the_history_only(ptx, ctx):
    """out_rgba = NULL: the history is what the full call leaves, and the filter does not run."""
    import torch
    frame, prev = case(65, 9)
    want_next, took = (lambda s: (s["next"], s["took"]))(accumulate(*frame, NG, prev=prev, flags=3, **TKNOBS))
    out, nxt, st = ctx.denoise_temporal_counts(*frame, NG, prev=prev, want_out=False, flags=3, **KNOBS)
    assert out is None and st["kernel_ms"] == 0 and st["iterations"] == 0 and st["reprojected"] == int(took.sum())
    _check(None, nxt, None, want_next, "host pointers")
    dev = [torch.from_numpy(x.copy()).to("cuda:0") for x in frame]
    dprev = [torch.from_numpy(x.copy()).to("cuda:0") for x in prev]
    dnext = [torch.full_like(x, 7) for x in dprev]
    out, nxt, _ = ctx.denoise_temporal_counts(*dev, NG, prev=dprev, next=dnext, want_out=False, want_stats=False, flags=3, **KNOBS)
    ctx.synchronize()
    assert out is None and all(x is y for x, y in zip(nxt, dnext))
    _check(None, [x.cpu().numpy() for x in nxt], None, want_next, "device pointers, caller's next")


@pytest.mark.gpu
def test_host_and_device_buffers_give_the_same_bits(ptx, ctx):
    import torch
    frame, prev = case(130, 70)
    out, nxt, st = ctx.denoise_temporal_counts(*frame, NG, prev=prev, flags=3, **KNOBS)
    dev = [torch.from_numpy(x.copy()).to("cuda:0") for x in frame]
    dprev = [torch.from_numpy(x.copy()).to("cuda:0") for x in prev]
    dout, dnxt, dst = ctx.denoise_temporal_counts(*dev, NG, prev=dprev, flags=3, **KNOBS)
    _check(dout.cpu().numpy(), [x.cpu().numpy() for x in dnxt], out, nxt, "device against host")
    assert (dst["reprojected"], dst["reset"]) == (st["reprojected"], st["reset"])
    dout, dnxt, dst = ctx.denoise_temporal_counts(*dev, NG, prev=dprev, flags=3, want_stats=False, **KNOBS)
    ctx.synchronize()
    assert dst is None
    _check(dout.cpu().numpy(), [x.cpu().numpy() for x in dnxt], out, nxt, "device, no stats")
    for x, src in zip(dev + dprev, frame + prev):
        _same(x.cpu().numpy(), src, "an input was modified")


@pytest.mark.gpu
def test_pointers_of_mixed_kinds_are_refused(ptx, ctx):
    import torch
    frame, prev = case(7, 5)
    for k in range(5):
        mixed = [torch.from_numpy(x.copy()).to("cuda:0") if i == k else x for i, x in enumerate(frame)]
        with pytest.raises(ptx.PtxError) as e:
            ctx.denoise_temporal_counts(*mixed, NG, prev=prev)
        assert e.value.code == ptx.ERR_INVALID and "device or all be host" in str(e.value) and "ptx_denoise_temporal_counts" in str(e.value)
    dprev = [torch.from_numpy(x.copy()).to("cuda:0") for x in prev]
    for bad in (dict(prev=dprev), dict(prev=prev, next=[torch.zeros_like(x) for x in dprev]), dict(prev=prev, out=torch.zeros(5, 7, 4, device="cuda:0"))):
        with pytest.raises(ptx.PtxError) as e:
            ctx.denoise_temporal_counts(*frame, NG, **bad)
        assert e.value.code == ptx.ERR_INVALID and "device or all be host" in str(e.value)
    # a flag the call does not know is refused with a real context as without one
    with pytest.raises(ptx.PtxError) as e:
        ctx.denoise_temporal_counts(*frame, NG, prev=prev, flags=8)
    assert e.value.code == ptx.ERR_INVALID and "flags" in str(e.value)


# ---------------------------------------------------------------------------- end to end: adaptive frames of an orbit
def _tm(x):
    x = np.asarray(x[..., :3], np.float64)
    return x / (1 + x)


def _mse(x, ref):
    return float(np.mean((_tm(x) - _tm(ref)) ** 2))


def _orbit_pose(c0, pivot, angle):
    o0, b0 = c0["origin"].astype(np.float64), c0["basis"].astype(np.float64).reshape(3, 3).T   # columns x, y, z
    R = np.array([[np.cos(angle), 0, np.sin(angle)], [0, 1, 0], [-np.sin(angle), 0, np.cos(angle)]])
    return dict(origin=(pivot + R @ (o0 - pivot)).astype(f32), basis=(R @ b0).T.reshape(-1).astype(f32), yfov=c0["yfov"])


@pytest.mark.gpu
def test_six_adaptive_frames_of_an_orbit_beat_the_single_frame_filter(ptx, ctx):
    """Cornell at 96 x 54, six frames of a 0.01 rad orbit about what the central ray sees, each rendered by render_adaptive_nee in the fused form
    with 4 samples at least, 16 at most and threshold 0.05, a seed of their own, guides and motion over the 4 samples every pixel has. The
    temporal frame of the last view is nearer to a 1024-spp frame of that view than ptx_denoise_counts' frame of the same halves.
    Measured on the MI355X: see DESIGN.md §5.10 (the ratio is recorded there, not asserted)."""
    from conftest import CORNELL
    W, H, B, FRAMES, STEP, MIN, CAP, THR = 96, 54, 8, 6, 0.01, 4, 16, 0.05
    s = ptx.Scene.load_gltf(ctx, CORNELL)
    c0 = s.camera()
    alb, nd, _ = s.render_aov(W, H, 1, seed=1)
    pivot = c0["origin"].astype(np.float64) - c0["basis"].astype(np.float64).reshape(3, 3).T[:, 2] * float(nd[H // 2, W // 2, 3] / max(alb[H // 2, W // 2, 3], 1))
    hist, prev_cam, reprojected, counts = None, None, [], []
    for k in range(FRAMES):
        cam, seed = _orbit_pose(c0, pivot, STEP * k), 0x5EED + k
        s.set_camera(cam["origin"], cam["basis"], cam["yfov"])
        a, b, _ = s.render_adaptive_nee(W, H, CAP, B, min_spp=MIN, threshold=THR, seed=seed, flags=ptx.NEE_FUSED, want_stats=False)
        A, N, _ = s.render_aov(W, H, MIN, seed=seed, want_stats=False)
        M, _ = s.render_motion(W, H, MIN, prev_camera=prev_cam, seed=seed, want_stats=False)
        out, hist, st = ctx.denoise_temporal_counts(a, b, A, N, M, MIN, prev=hist)
        assert st["reprojected"] + st["reset"] == W * H
        reprojected.append(st["reprojected"] / (W * H))
        counts.append(float((a[..., 3] + b[..., 3]).mean()))
        prev_cam = cam
    single, _ = ctx.denoise_counts(a, b, A, N, MIN)
    ref, _ = s.render_nee(W, H, 1024, B, seed=77, flags=ptx.NEE_FUSED, want_stats=False)
    ref = ref / f32(1024)
    noisy = (a + b) / (a[..., 3:] + b[..., 3:])
    e_noisy, e_single, e_temporal = _mse(noisy, ref), _mse(single, ref), _mse(out, ref)
    print(f"cornell {W}x{H}, frame 6 of an orbit, adaptive {MIN}:{CAP}:{THR} (mean counts {[round(c, 2) for c in counts]}): mse unfiltered {e_noisy:.3e}, "
          f"ptx_denoise_counts {e_single:.3e}, temporal-counts {e_temporal:.3e} (single / temporal = {e_single / e_temporal:.2f}); "
          f"reprojected share per frame {[round(r, 3) for r in reprojected]}")
    n = a[..., 3] + b[..., 3]
    assert n.min() >= MIN and n.max() <= CAP
    assert reprojected[0] == 0 and min(reprojected[1:]) > 0.8   # Cornell is closed: nearly every pixel finds its history
    assert float(hist[0][..., 3].max()) <= FRAMES * CAP + 1e-3 and float(hist[0][..., 3].max()) > 2 * CAP
    assert e_temporal < e_single


@pytest.mark.gpu
def test_the_cpp_mirror_gives_the_python_mirrors_adaptive_frames(ptx, ctx, tmp_path):
    """core::renderer::temporal_sequence after set_adaptive (host/ptx_renderer.hpp), driven by tools/temporal_sequence_check with its adaptive
    argument over four camera poses, against the same sequence made with Scene.render_adaptive_nee / render_aov / render_motion and
    Context.denoise_temporal_counts: every frame and the last history, bit for bit."""
    import os
    import subprocess
    from conftest import CORNELL, ROOT
    W, H, CAP, B, SEED0, MIN, THR, TFLAGS = 48, 27, 12, 4, 0x5EED, 4, 0.4, SEARCH_3X3 | UNIT_NORMALS   # at 0.4 the pixels stop at 4, 8 and 12 samples
    exe = os.path.join(ROOT, "tools", "bin", "temporal_sequence_check")
    assert os.path.exists(exe), "tools/bin/temporal_sequence_check is built by build()"
    s = ptx.Scene.load_gltf(ctx, CORNELL)
    c0 = s.camera()
    o0, b0 = c0["origin"].astype(np.float64), c0["basis"].astype(np.float64).reshape(3, 3).T
    poses = []
    for k in range(4):
        a = 0.015 * k
        R = np.array([[np.cos(a), 0, np.sin(a)], [0, 1, 0], [-np.sin(a), 0, np.cos(a)]])
        poses.append(np.concatenate([R @ o0, (R @ b0).T.reshape(-1), [c0["yfov"]]]).astype(f32))
    (tmp_path / "poses.bin").write_bytes(np.stack(poses).tobytes())
    r = subprocess.run([exe, CORNELL, str(W), str(H), str(CAP), str(B), str(tmp_path / "poses.bin"), str(tmp_path / "out.bin"),
                        f"{MIN}:0:{THR}:{ptx.NEE_FUSED}:{TFLAGS}"], capture_output=True, text=True, timeout=120)
    assert r.returncode == 0, r.stderr
    got = np.fromfile(tmp_path / "out.bin", f32).reshape(len(poses) + 2, H, W, 4)
    hist, prev_cam, xf = None, None, s.array(ptx.ARR_MODEL_XFORM)
    for k, p in enumerate(poses):
        s.set_camera(p[0:3], p[3:12], p[12])
        a, b, _ = s.render_adaptive_nee(W, H, CAP, B, min_spp=MIN, threshold=THR, seed=SEED0 + k, flags=ptx.NEE_FUSED, want_stats=False)
        A, N, _ = s.render_aov(W, H, MIN, seed=SEED0 + k, want_stats=False)
        M, _ = s.render_motion(W, H, MIN, prev_camera=prev_cam, prev_model_xform=xf if prev_cam else None, seed=SEED0 + k, want_stats=False)
        out, hist, st = ctx.denoise_temporal_counts(a, b, A, N, M, MIN, prev=hist, flags=TFLAGS)
        _same(got[k], out, f"frame {k}")
        assert f"frame {k}: " in r.stdout and f"reprojected {st['reprojected']}, reset {st['reset']}" in r.stdout.splitlines()[k]
        prev_cam = s.camera()
    assert st["reprojected"] > 0.8 * W * H
    assert len(np.unique(a[..., 3] + b[..., 3])) == 3    # the counts do differ from pixel to pixel
    _same(got[len(poses)], hist[0], "the last frame's integrated colour and sample counts")
