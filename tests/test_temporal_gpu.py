"""ptx_denoise_temporal on the GPU, bit for bit against the float32 numpy restatement of its specification
(tests/_temporal_restatement.py; tests/test_temporal.py shows on the CPU that the restatement does what the specification promises).

Nothing on this path goes through libm, so the product is held to BITWISE equality: the output, the three history buffers, NaN positions
included, and the two counters.
"""
import ctypes as C

import numpy as np
import pytest

from _common import _same
from _denoise_restatement import f32
from _routes import ctx  # noqa: F401  (a fixture)
from _temporal_restatement import accumulate, motion_sums, restate, synthetic

SA, SB = 3, 5
SHAPES = [(1, 1), (2, 3), (63, 5), (64, 64), (130, 70)]
KNOBS = dict(sigma_l=3.0, sigma_n=0.7, sigma_z=0.25, max_history=3, tau_z=0.2, tau_n=0.8)


def case(W, H):
    """The current frame, a wild motion and a damaged history of another frame with the same geometry.
    Motion: fractional everywhere (up to +-3 pixels, so that pixels near the border look outside), and single pixels that leave the image
    by far, hold NaN, an infinity or 1e9 pixels, or have a zero or negative count. History: one frame old in one half of the image and two
    frames old in the other, with holes of N = 0, NaN colour, moments and depth entries."""
    rng = np.random.default_rng(7 + 1000 * W + H)
    a, b, A, N = synthetic(W, H, SA, SB, seed=1)
    cov = A[..., 3]
    reach = min(3.0, max(W, H) / 4)   # the smallest buffers keep a tap inside
    mv = rng.uniform(-reach, reach, (H, W, 2)).astype(f32)
    M = np.stack([mv[..., 0] * cov, mv[..., 1] * cov, N[..., 3] * rng.uniform(0.9, 1.1, (H, W)).astype(f32), cov], -1).astype(f32)
    pa, pb, pA, pN = synthetic(W, H, SA, SB, seed=2)
    h0 = accumulate(pa, pb, pA, pN, motion_sums(pA, pN), SA, SB)["next"]
    h1 = accumulate(pa, pb, pA, pN, motion_sums(pA, pN), SA, SB, prev=h0, max_history=KNOBS["max_history"])["next"]
    left = (np.arange(W) * 2 < W)[None, :, None]
    prev = [np.where(left, x0, x1).astype(f32) for x0, x1 in zip(h0, h1)]
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
    return (a, b, A, N, M), tuple(prev)


def _check(got_out, got_next, want_out, want_next, what):
    if want_out is not None:
        _same(got_out, want_out, f"{what}: out")
    for name, g, w in zip(("color", "moments", "geometry"), got_next, want_next):
        _same(g, w, f"{what}: next.{name}")


@pytest.mark.gpu
@pytest.mark.parametrize("iterations", [0, 1], ids=["default", "one"])
@pytest.mark.parametrize("shape", SHAPES, ids=lambda s: f"{s[0]}x{s[1]}")
def test_synthetic_buffers_bitwise(ptx, ctx, shape, iterations):
    """Host and device pointers; the counters; the inputs and prev are not modified."""
    import torch
    W, H = shape
    frame, prev = case(W, H)
    want_out, want_next, took = restate(*frame, SA, SB, prev=prev, iterations=iterations or 5, **KNOBS)
    if W * H >= 300:
        assert took.mean() > 0.3 and (~took).mean() > 0.05, took.mean()
        assert (want_next[0][..., 3] == 2).any() and (want_next[0][..., 3] == 3).any() and (want_next[0][..., 3] == 1).any()
        assert np.isfinite(want_next[0]).all() and np.isfinite(want_next[1]).all()
    out, nxt, st = ctx.denoise_temporal(*frame, SA, SB, prev=prev, iterations=iterations, **KNOBS)
    _check(out, nxt, want_out, want_next, "host pointers")
    assert st["iterations"] == (iterations or 5)
    assert (st["reprojected"], st["reset"]) == (int(took.sum()), W * H - int(took.sum())), st
    dev = [torch.from_numpy(x).to("cuda:0") for x in frame]
    dprev = [torch.from_numpy(x).to("cuda:0") for x in prev]
    out, nxt, st = ctx.denoise_temporal(*dev, SA, SB, prev=dprev, iterations=iterations, **KNOBS)
    _check(out.cpu().numpy(), [x.cpu().numpy() for x in nxt], want_out, want_next, "device pointers")
    assert st["reprojected"] + st["reset"] == W * H and st["reprojected"] == int(took.sum())
    out, nxt, st = ctx.denoise_temporal(*dev, SA, SB, prev=dprev, iterations=iterations, want_stats=False, **KNOBS)
    ctx.synchronize()
    assert st is None
    _check(out.cpu().numpy(), [x.cpu().numpy() for x in nxt], want_out, want_next, "device pointers, no stats")
    for x, src in zip(dev + dprev, frame + prev):
        _same(x.cpu().numpy(), src, "an input was modified")


@pytest.mark.gpu
def test_default_knobs_and_a_second_frame(ptx, ctx):
    """max_history, the taus and the sigmas at their defaults; the history the call returned goes into the next call."""
    frame, prev = case(67, 35)
    want_out, want_next, took = restate(*frame, SA, SB, prev=prev)
    out, nxt, st = ctx.denoise_temporal(*frame, SA, SB, prev=prev)
    _check(out, nxt, want_out, want_next, "defaults")
    a, b, A, N, _ = frame
    want2 = restate(a, b, A, N, motion_sums(A, N), SA, SB, prev=want_next)
    out2, nxt2, st2 = ctx.denoise_temporal(a, b, A, N, motion_sums(A, N), SA, SB, prev=nxt)
    _check(out2, nxt2, want2[0], want2[1], "second frame")
    assert st2["reprojected"] == int(want2[2].sum()) == int((A[..., 3] > 0).sum())


@pytest.mark.gpu
@pytest.mark.parametrize("mask", [0xFF, 0x55])
def test_both_kernel_forms_give_the_same_bits(ptx, ctx, monkeypatch, mask):
    frame, prev = case(130, 70)
    want_out, want_next, _ = restate(*frame, SA, SB, prev=prev, **KNOBS)
    monkeypatch.setenv("PTX_DENOISE_TILED", hex(mask))
    out, nxt, _ = ctx.denoise_temporal(*frame, SA, SB, prev=prev, **KNOBS)
    _check(out, nxt, want_out, want_next, f"PTX_DENOISE_TILED={mask:#x}")


@pytest.mark.gpu
def test_without_prev_the_output_is_ptx_denoise(ptx, ctx):
    frame, _ = case(67, 35)
    a, b, A, N, M = frame
    sig = {k: v for k, v in KNOBS.items() if k.startswith("sigma")}
    for it in (0, 1, 8):
        out, nxt, st = ctx.denoise_temporal(*frame, SA, SB, prev=None, iterations=it, **KNOBS)
        ref, _ = ctx.denoise(a, b, A, N, SA, SB, iterations=it, **sig)
        _same(out, ref, f"prev = NULL, iterations {it}")
        assert (st["reprojected"], st["reset"]) == (0, 67 * 35)
        assert (nxt[0][..., 3] == 1).all()
        _check(None, nxt, None, restate(*frame, SA, SB, prev=None, **KNOBS)[1], "first frame's history")


@pytest.mark.gpu
def test_advancing_the_history_only(ptx, ctx):
    """out_rgba = NULL: the history is what the full call leaves, and the filter does not run."""
    import torch
    frame, prev = case(63, 5)
    _, want_next, took = restate(*frame, SA, SB, prev=prev, **KNOBS)
    out, nxt, st = ctx.denoise_temporal(*frame, SA, SB, prev=prev, want_out=False, **KNOBS)
    assert out is None and st["kernel_ms"] == 0 and st["iterations"] == 0 and st["reprojected"] == int(took.sum())
    _check(None, nxt, None, want_next, "host pointers")
    dev = [torch.from_numpy(x).to("cuda:0") for x in frame]
    dprev = [torch.from_numpy(x).to("cuda:0") for x in prev]
    dnext = [torch.full_like(x, 7) for x in dprev]
    out, nxt, _ = ctx.denoise_temporal(*dev, SA, SB, prev=dprev, next=dnext, want_out=False, want_stats=False, **KNOBS)
    ctx.synchronize()
    assert out is None and all(x is y for x, y in zip(nxt, dnext))
    _check(None, [x.cpu().numpy() for x in nxt], None, want_next, "device pointers, caller's next")


@pytest.mark.gpu
def test_pointers_of_mixed_kinds_are_refused(ptx, ctx):
    import torch
    frame, prev = case(5, 3)
    for k in range(5):
        mixed = [torch.from_numpy(x).to("cuda:0") if i == k else x for i, x in enumerate(frame)]
        with pytest.raises(ptx.PtxError) as e:
            ctx.denoise_temporal(*mixed, SA, SB, prev=prev)
        assert e.value.code == ptx.ERR_INVALID and "device or all be host" in str(e.value)
    dprev = [torch.from_numpy(x).to("cuda:0") for x in prev]
    for bad in (dict(prev=dprev), dict(prev=prev, next=[torch.zeros_like(x) for x in dprev]), dict(prev=prev, out=torch.zeros(3, 5, 4, device="cuda:0"))):
        with pytest.raises(ptx.PtxError) as e:
            ctx.denoise_temporal(*frame, SA, SB, **bad)
        assert e.value.code == ptx.ERR_INVALID and "device or all be host" in str(e.value)
    # next sharing a buffer with prev is refused on the device as on the host
    with pytest.raises(ptx.PtxError) as e:
        ctx.denoise_temporal(*frame, SA, SB, prev=prev, next=(np.zeros_like(prev[0]), np.zeros_like(prev[1]), prev[2]))
    assert "shares" in str(e.value)


# ---------------------------------------------------------------------------- end to end: ptx_render_motion feeding ptx_denoise_temporal
def _tm(x):
    x = np.asarray(x[..., :3], np.float64)
    return x / (1 + x)


def _mse(x, ref):
    return float(np.mean((_tm(x) - _tm(ref)) ** 2))


@pytest.mark.gpu
def test_six_frames_of_an_orbit_beat_the_single_frame_filter(ptx, ctx):
    """Cornell at 96 x 54, six frames of a small orbit about what the central ray sees, 8 spp each with a seed of their own. The temporal
    frame of the last view is nearer to a 1024-spp frame of that view than ptx_denoise's frame of the same samples.
    Measured on the MI355X: see DESIGN.md §5.9 (the ratio is recorded there, not asserted)."""
    from conftest import CORNELL
    W, H, B, FRAMES, STEP = 96, 54, 8, 6, 0.01
    s = ptx.Scene.load_gltf(ctx, CORNELL)
    c0 = s.camera()
    o0, b0 = c0["origin"].astype(np.float64), c0["basis"].astype(np.float64).reshape(3, 3).T   # columns x, y, z
    alb, nd, _ = s.render_aov(W, H, 1, seed=1)
    pivot = o0 - b0[:, 2] * float(nd[H // 2, W // 2, 3] / max(alb[H // 2, W // 2, 3], 1))

    def pose(k):
        a = STEP * k
        R = np.array([[np.cos(a), 0, np.sin(a)], [0, 1, 0], [-np.sin(a), 0, np.cos(a)]])
        return dict(origin=(pivot + R @ (o0 - pivot)).astype(f32), basis=(R @ b0).T.reshape(-1).astype(f32), yfov=c0["yfov"])
    hist, prev_cam, reprojected = None, None, []
    for k in range(FRAMES):
        cam, seed = pose(k), 0x5EED + k
        s.set_camera(cam["origin"], cam["basis"], cam["yfov"])
        a, _ = s.render(W, H, 4, B, seed=seed, sample0=0, want_stats=False)
        b, _ = s.render(W, H, 4, B, seed=seed, sample0=4, want_stats=False)
        A, N, _ = s.render_aov(W, H, 8, seed=seed, want_stats=False)
        M, _ = s.render_motion(W, H, 8, prev_camera=prev_cam, seed=seed, want_stats=False)
        out, hist, st = ctx.denoise_temporal(a, b, A, N, M, 4, 4, prev=hist)
        assert st["reprojected"] + st["reset"] == W * H
        reprojected.append(st["reprojected"] / (W * H))
        prev_cam = cam
    single, _ = ctx.denoise(a, b, A, N, 4, 4)
    ref, _ = s.render(W, H, 1024, B, seed=77, want_stats=False)
    ref = ref / f32(1024)
    noisy = (a + b) / f32(8)
    e_noisy, e_single, e_temporal = _mse(noisy, ref), _mse(single, ref), _mse(out, ref)
    print(f"cornell {W}x{H}, frame 6 of an orbit at 8 spp: mse unfiltered {e_noisy:.3e}, ptx_denoise {e_single:.3e}, temporal {e_temporal:.3e} "
          f"(single / temporal = {e_single / e_temporal:.2f}); reprojected share per frame {[round(r, 3) for r in reprojected]}")
    assert reprojected[0] == 0 and min(reprojected[1:]) > 0.8   # Cornell is closed: nearly every pixel finds its history
    assert abs(float(hist[0][..., 3].max()) - FRAMES) < 1e-3   # six frames long, up to the rounding of the bilinear mean of N
    assert e_temporal < e_single


@pytest.mark.gpu
def test_the_cpp_mirror_gives_the_python_mirrors_frames(ptx, ctx, tmp_path):
    """core::renderer::temporal_sequence and core::renderer::render_motion (host/ptx_renderer.hpp), driven by tools/temporal_sequence_check
    over four camera poses, against the same sequence made with Scene.render / render_aov / render_motion and Context.denoise_temporal:
    every frame, the last history and the motion, bit for bit."""
    import os
    import subprocess
    from conftest import CORNELL, ROOT
    W, H, SPP, B, SEED0 = 48, 27, 4, 4, 0x5EED   # core::renderer's default seed
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
    r = subprocess.run([exe, CORNELL, str(W), str(H), str(SPP), str(B), str(tmp_path / "poses.bin"), str(tmp_path / "out.bin")],
                       capture_output=True, text=True, timeout=120)
    assert r.returncode == 0, r.stderr
    got = np.fromfile(tmp_path / "out.bin", f32).reshape(len(poses) + 2, H, W, 4)
    hist, prev_cam, xf = None, None, s.array(ptx.ARR_MODEL_XFORM)
    for k, p in enumerate(poses):
        s.set_camera(p[0:3], p[3:12], p[12])
        a, _ = s.render(W, H, SPP // 2, B, seed=SEED0 + k, want_stats=False)
        b, _ = s.render(W, H, SPP - SPP // 2, B, seed=SEED0 + k, sample0=SPP // 2, want_stats=False)
        A, N, _ = s.render_aov(W, H, SPP, seed=SEED0 + k, want_stats=False)
        M, _ = s.render_motion(W, H, SPP, prev_camera=prev_cam, prev_model_xform=xf if prev_cam else None, seed=SEED0 + k, want_stats=False)
        out, hist, st = ctx.denoise_temporal(a, b, A, N, M, SPP // 2, SPP - SPP // 2, prev=hist)
        _same(got[k], out, f"frame {k}")
        assert f"frame {k}: " in r.stdout and f"reprojected {st['reprojected']}, reset {st['reset']}" in r.stdout.splitlines()[k]
        prev_cam = s.camera()
    assert st["reprojected"] > 0.8 * W * H
    _same(got[len(poses)], hist[0], "the last frame's integrated colour")
    first = dict(origin=poses[0][0:3], basis=poses[0][3:12], yfov=poses[0][12])
    M, _ = s.render_motion(W, H, SPP, prev_camera=first, prev_model_xform=xf, seed=SEED0, want_stats=False)
    _same(got[len(poses) + 1], M, "render_motion against the first camera")
    assert (M[..., :2] != 0).any()
