"""The N > 1 path with the real library: multi-process jobs whose ranks each initialise HIP, create a Context, build the scenes,
render their share through multigpu.* and hand the buffer to a collective (tests/_dist_product_worker.py).

Jobs: transport gloo0 (every rank on GPU 0, gloo) at world sizes 2 and 3, and transport rccl (rank r on GPU r, nccl, plus
ptx_reduce_framebuffer on a communicator of its own) at world size 2 where the machine has two GPUs. One job per world size runs
every mode, so that at most four processes have the GPU open: this one and three ranks.

What a job is compared with is the same library in THIS process: the single-process frame, which the rest of the suite pins to the
oracle. Tile shards (x + 0) must give its bits; two sample ranges must give the bits of A + B; three leave the order of the sum to
the transport.
"""
import importlib
import json
import os
import signal
import socket
import subprocess
import sys
import time

import numpy as np
import pytest

from conftest import ROOT

import _dist_product_worker as wk
from _common import _same
from _denoise_restatement import QB, QH, QSEED, QW, restate

f32 = np.float32
WORKER = os.path.join(ROOT, "tests", "_dist_product_worker.py")
JOBS = [("gloo0", 2), ("gloo0", 3), ("rccl", 2)]
# The two-rank gloo job of test_multigpu_gloo.py (tiles) takes 4.2 s on the MI355X machine, start to end; the first run of the new
# gloo0 job took 4.8 s at world size 2 and 5.0 s at world size 3 (profiles/EXPERIMENTS.md). The limit is ten times that.
JOB_LIMIT_S = 50
_broken = []     # why a job failed: nothing more is started on the GPU after that


def _mg():
    return importlib.import_module("distributed-path-tracer_amd.multigpu")


# ---------------------------------------------------------------------------- CPU
def test_chosen_frames_give_every_rank_tiles():
    """The worker's sharding arithmetic without a GPU: the tile masks of the ranks partition each frame, and at the two frames the
    jobs render no rank is idle (at 65 x 7 with 64-pixel tiles there are two tiles, so a third rank has none: the partition still holds)."""
    mg = _mg()
    assert (wk.W, wk.H, wk.TILE) == (96, 54, 16) and (wk.Q_W, wk.Q_H, wk.Q_TILE) == (48, 32, 8)
    for (W, H, tile) in ((96, 54, 16), (48, 32, 8), (65, 7, 64)):
        for world in (2, 3):
            masks = [mg.tile_mask(r, world, W, H, tile) for r in range(world)]
            assert all(m.shape == (H, W) for m in masks)
            assert (np.sum(masks, axis=0) == 1).all(), (W, H, tile, world)
            for r, m in enumerate(masks):
                ys, xs = np.nonzero(m)
                assert all(mg.tile_owner(int(x), int(y), W, world, tile) == r for x, y in zip(xs[::37], ys[::37]))
            if tile != 64:
                assert all(m.any() for m in masks), (W, H, tile, world)
    assert [_mg().split_samples(r, 3, wk.SPP_UNEVEN)[1] for r in range(3)] == [6, 5, 5]
    assert [_mg().split_samples(r, 3, wk.SPP)[1] for r in range(3)] == [2, 2, 2]


# ---------------------------------------------------------------------------- the single-process frames
@pytest.fixture(scope="module")
def single(ptx):
    """Everything the jobs are compared with, rendered once by this process on Context(0)."""
    assert (wk.D_W, wk.D_H, wk.D_B, wk.D_SEED) == (QW, QH, QB, QSEED)
    ctx = ptx.Context(0)
    sc = wk.build_scenes(ptx, ctx)
    W, H, B = wk.W, wk.H, wk.B
    e = {}
    cornell = sc["cornell"]
    for spp in sorted({wk.SPP, wk.SPP_UNEVEN, 2 * wk.WEAK_SPP, 3 * wk.WEAK_SPP}):
        e["frame", spp] = cornell.render(W, H, spp, B)
    for spp in (wk.SPP, wk.SPP_UNEVEN):           # the two sample ranges of a two-rank split, each into a zeroed buffer of its own
        half = spp // 2
        e["halves", spp] = (cornell.render(W, H, half, B, sample0=0)[0], cornell.render(W, H, spp - half, B, sample0=half)[0])
    e["transparent"] = sc["plaza"].render_transparent(W, H, wk.T_SPP, wk.T_B)
    with wk.small_pair_pool():
        e["queue"] = sc["atrium"].render(wk.Q_W, wk.Q_H, wk.Q_SPP, wk.Q_B)
        assert ctx.timing()["pipeline"] == 1
    for name in wk.AOV_SCENES:
        e["aov", name] = sc[name].render_aov(W, H, wk.AOV_SPP)
    a, _ = cornell.render(QW, QH, wk.D_HALF, QB, seed=QSEED, sample0=0)
    b, _ = cornell.render(QW, QH, wk.D_HALF, QB, seed=QSEED, sample0=wk.D_HALF)
    A, N, _ = cornell.render_aov(QW, QH, 2 * wk.D_HALF, seed=QSEED)
    e["denoise_in"] = dict(a=a, b=b, albedo=A, normal=N)
    e["denoise"] = restate(a, b, A, N, wk.D_HALF, wk.D_HALF)
    for s in sc.values():
        s.close()
    ctx.close()
    return e


# ---------------------------------------------------------------------------- the jobs
def _run_job(transport, world, tmp):
    out = str(tmp / f"{transport}_{world}.npz")
    with socket.socket() as s:
        s.bind(("127.0.0.1", 0))
        port = s.getsockname()[1]
    cmd = [sys.executable, "-m", "torch.distributed.run", "--nnodes=1", "--nproc-per-node", str(world), "--master-addr", "127.0.0.1",
           "--master-port", str(port), WORKER, out, transport]
    env = dict(os.environ, MASTER_ADDR="127.0.0.1")
    log = str(tmp / f"{transport}_{world}.log")
    t0 = time.perf_counter()
    with open(log, "w") as fh:
        p = subprocess.Popen(cmd, env=env, stdout=fh, stderr=subprocess.STDOUT, start_new_session=True)
        try:
            rc = p.wait(timeout=JOB_LIMIT_S)
        except subprocess.TimeoutExpired:
            os.killpg(p.pid, signal.SIGKILL)       # the launcher and every rank: they share the session started above
            p.wait()
            rc = None
    dt = time.perf_counter() - t0
    with open(log) as fh:
        text = fh.read()
    print(f"{transport} world {world}: {dt:.1f} s, exit status {rc}")
    print("\n".join(l for l in text.splitlines() if "workspace_bytes" in l))
    if rc != 0:
        _broken.append(f"the {transport} job at world size {world} " + (f"ended with status {rc}" if rc is not None else f"did not end within {JOB_LIMIT_S} s"))
        pytest.fail(_broken[-1] + "\n" + text[-4000:])
    with np.load(out) as z:
        res = {k: z[k] for k in z.files}
    stats = []
    for r in range(world):
        with open(f"{out}.rank{r}.json") as fh:
            stats.append(json.load(fh))
    return dict(transport=transport, world=world, kinds=("dev",) if transport == "rccl" else ("host", "dev"), res=res, stats=stats)


@pytest.fixture(scope="module", params=JOBS, ids=[f"{t}-world{n}" for t, n in JOBS])
def job(request, single, tmp_path_factory):
    transport, world = request.param
    if _broken:
        pytest.skip(f"nothing more is started on the GPU: {_broken[0]}")
    if transport == "rccl":
        import torch
        if torch.cuda.device_count() < 2:
            pytest.skip("torch.cuda.device_count() >= 2")
    return _run_job(transport, world, tmp_path_factory.mktemp(f"{transport}{world}"))


def _keys(job, mode):
    return [(kind, f"{mode}_{kind}") for kind in job["kinds"]]


def _check_stats(job, key, total_samples, total_rays, per_rank_samples):
    st = [s[key] for s in job["stats"]]
    assert [s["samples"] for s in st] == per_rank_samples, key
    assert sum(s["samples"] for s in st) == total_samples, key
    assert sum(s["rays"] for s in st) == total_rays, key


def _tile_counts(world, W, H, tile, spp):
    return [int(_mg().tile_mask(r, world, W, H, tile).sum()) * spp for r in range(world)]


def _content(frame, what, world=1, tile=None):
    """Finite, and not a frame of zeros: with `tile`, in the pixels of every rank (an all-black shard would make x + 0 trivial)."""
    assert np.isfinite(frame).all(), what
    H, W = frame.shape[:2]
    for r in range(world):
        m = _mg().tile_mask(r, world, W, H, tile) if tile else np.ones((H, W), bool)
        assert (frame[m][:, :3] > 0).any(), f"{what}: no light in the pixels of rank {r}"


@pytest.mark.gpu
def test_tiles(job, single):
    full, fst = single["frame", wk.SPP]
    _content(full, "single-process frame", job["world"], wk.TILE)
    for kind, key in _keys(job, "tiles"):
        got = job["res"][key]
        _content(got, key, job["world"], wk.TILE)
        assert (got[..., 3] == wk.SPP).all(), key
        _same(got, full, key)
        _same(job["res"][f"tiles_nostats_{kind}"], full, f"tiles_nostats_{kind}")      # want_stats=False: the render returns in flight
        _check_stats(job, key, wk.W * wk.H * wk.SPP, fst["rays"], _tile_counts(job["world"], wk.W, wk.H, wk.TILE, wk.SPP))


@pytest.mark.gpu
def test_queue_route_tiles(job, single):
    full, fst = single["queue"]
    _content(full, "single-process frame", job["world"], wk.Q_TILE)
    for kind, key in _keys(job, "queue_tiles"):
        got = job["res"][key]
        _content(got, key, job["world"], wk.Q_TILE)
        assert (got[..., 3] == wk.Q_SPP).all(), key
        _same(got, full, key)
        _check_stats(job, key, wk.Q_W * wk.Q_H * wk.Q_SPP, fst["rays"], _tile_counts(job["world"], wk.Q_W, wk.Q_H, wk.Q_TILE, wk.Q_SPP))


@pytest.mark.gpu
def test_transparent_tiles(job, single):
    pix, cl, fst = single["transparent"]
    _content(pix, "single-process frame", job["world"], wk.TILE)
    assert pix[..., 3].min() < pix[..., 3].max() and cl.any()      # the alpha plane is not constant
    mine = _mg().tile_mask(0, job["world"], wk.W, wk.H, wk.TILE)
    for kind, key in _keys(job, "transparent"):
        _same(job["res"][key], pix, key)                       # colour and alpha
        got_cl = job["res"][f"transparent_claimed_{kind}"]
        np.testing.assert_array_equal(got_cl[mine], cl[mine], err_msg=f"{key}: rank 0's claimed flags on its own pixels")
        assert not got_cl[~mine].any(), f"{key}: claimed is not reduced, the other ranks' pixels stay zero"
        _check_stats(job, key, wk.W * wk.H * wk.T_SPP, fst["rays"], _tile_counts(job["world"], wk.W, wk.H, wk.TILE, wk.T_SPP))


@pytest.mark.gpu
def test_aov_tiles(job, single):
    for name in wk.AOV_SCENES:
        A, N, fst = single["aov", name]
        _content(A, f"single-process albedo, {name}", job["world"], wk.TILE)
        assert np.isfinite(N).all() and N[..., :3].any() and (N[..., 3] > 0).any()
        for kind in job["kinds"]:
            key = f"aov_tiles_{name}_albedo_{kind}"
            _same(job["res"][key], A, key)
            _same(job["res"][f"aov_tiles_{name}_normal_{kind}"], N, f"aov_tiles_{name}_normal_{kind}")
            _check_stats(job, key, wk.W * wk.H * wk.AOV_SPP, fst["rays"], _tile_counts(job["world"], wk.W, wk.H, wk.TILE, wk.AOV_SPP))


@pytest.mark.gpu
@pytest.mark.parametrize("mode", ["samples", "samples16", "weak"])
def test_sample_ranges(job, single, mode):
    """Two ranks: a two-operand float sum has one order, so the reduced frame is bitwise A + B of the two ranges rendered here into
    zeroed buffers of their own. Three ranks: the order of the sum is the transport's; against the single-call frame at the tolerance
    test_multigpu_gloo.py uses for the same comparison. The alpha plane (small integers) is exact either way."""
    mg, world = _mg(), job["world"]
    spp = {"samples": wk.SPP, "samples16": wk.SPP_UNEVEN, "weak": world * wk.WEAK_SPP}[mode]
    full, fst = single["frame", spp]
    if mode == "weak":
        counts = [mg.sample_range(r, world, wk.WEAK_SPP)[1] for r in range(world)]
    else:
        counts = [mg.split_samples(r, world, spp)[1] for r in range(world)]
    if mode == "samples16" and world == 3:
        assert counts == [6, 5, 5]
    for kind, key in _keys(job, mode):
        got = job["res"][key]
        _content(got, key)
        assert (got[..., 3] == spp).all(), key
        if world == 2:
            a, b = single["halves", spp]
            assert not np.array_equal(a + b, a + a)      # two different sample ranges: twice the first would not pass for a + b
            _same(got, a + b, key)
        else:
            np.testing.assert_array_equal(got[..., 3], full[..., 3], err_msg=key)
            np.testing.assert_allclose(got[..., :3], full[..., :3], rtol=2e-6, atol=1e-6, err_msg=key)
        _check_stats(job, key, wk.W * wk.H * spp, fst["rays"], [wk.W * wk.H * n for n in counts])


@pytest.mark.gpu
def test_denoise_after_the_reduces(job, single):
    """Reduce the four buffers, then filter on the root: the reduced inputs are the single-process ones (x + 0), so the filter's output
    is the restatement of the single-process buffers, bit for bit."""
    want = single["denoise"]
    _content(want, "restatement of the single-process buffers")
    noisy = (single["denoise_in"]["a"] + single["denoise_in"]["b"]) / f32(2 * wk.D_HALF)
    assert (want[..., :3] != noisy[..., :3]).mean() > 0.5          # the comparison is of filtered values
    for kind in job["kinds"]:
        for what, ref in single["denoise_in"].items():
            _same(job["res"][f"denoise_in_{what}_{kind}"], ref, f"reduced denoise input {what} ({kind})")
        _same(job["res"][f"denoise_{kind}"], want, f"denoise_{kind}")


@pytest.mark.gpu
def test_reduce_through_the_c_abi(job, single):
    """ptx_reduce_framebuffer with more than one rank (the rccl job only: RCCL refuses two ranks on one device)."""
    if job["transport"] != "rccl":
        assert "reduce_c_abi_dev" not in job["res"]
        return
    full, fst = single["frame", wk.SPP]
    got = job["res"]["reduce_c_abi_dev"]
    _content(got, "reduce_c_abi")
    _same(got, full, "reduce_c_abi")
    _check_stats(job, "reduce_c_abi_dev", wk.W * wk.H * wk.SPP, fst["rays"], _tile_counts(2, wk.W, wk.H, wk.TILE, wk.SPP))
