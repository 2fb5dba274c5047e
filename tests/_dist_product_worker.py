"""Worker for tests/test_multigpu_product.py: one rank of a job started by `python -m torch.distributed.run`, on the GPU.

    _dist_product_worker.py OUT TRANSPORT

Unlike tests/_dist_worker.py (an oracle-backed stand-in, CPU) this is the product: every rank initialises HIP, creates its own
Context, builds the real Scenes, renders its share through the unchanged multigpu functions and hands the buffer to the collective.
TRANSPORT is
  gloo0  every rank on GPU 0 (Context(0)), process group gloo: what a single-GPU machine can run. Host and device buffers.
  rccl   rank r on GPU r (torch.cuda.set_device(r), Context(r)), process group nccl. Device buffers only: the nccl backend has no
         collective for a CPU tensor, and the host-staged path does not depend on the transport (gloo0 covers it).
All modes (tiles, samples, weak, transparent, queue_tiles, aov_tiles, denoise and, under rccl, reduce_c_abi) run one after the other in this process. Rank 0 saves its buffers after the reduces to OUT (.npz, keys
"<mode>_<host|dev>"); every rank saves the stats of its local renders to OUT.rank<r>.json. The test module imports the constants and
`build_scenes` from here, so that the single-process frames it compares with are rendered from the same arguments.
"""
import contextlib
import ctypes
import importlib
import json
import os
import sys

import numpy as np
import torch
import torch.distributed as dist

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)
PKG = "distributed-path-tracer_amd"
CORNELL = os.path.join(ROOT, "scenes", "cornell-box", "cornell.gltf")

W, H, SPP, B, TILE = 96, 54, 6, 4, 16      # 6 x 4 tiles of 16 x 16, the bottom row 6 pixels high
SPP_UNEVEN = 16                            # split_samples(r, 3, 16) = 6, 5, 5
WEAK_SPP = 3                               # per rank
T_SPP, T_B = 8, 4                          # transparent plaza: the samples and bounces of test_transparent_background
Q_W, Q_H, Q_SPP, Q_B, Q_TILE = 48, 32, 2, 5, 8
AOV_SPP = 16
D_W, D_H, D_B, D_SEED, D_HALF = 96, 54, 8, 0x5EED, 8   # test_denoise.QW, QH, QB, QSEED; halves of samples 0..7 and 8..15
AOV_SCENES = ("cornell", "plaza")


def build_scenes(ptx, ctx):
    """The three small scenes every rank (and the comparing process) holds. The atrium is created under PTX_FORCE_GLOBAL=1 (its trees
    stay in global memory); with the variable unset again its 24-surface model renders through the queue pipeline."""
    proc = importlib.import_module(PKG + ".procedural")

    def from_dict(d):
        return ptx.Scene.from_arrays(ctx, d["model_xform"], d["model_surf"], d["surf_range"], d["vertices"], d["triangles"],
                                     d["materials"], d["camera"], d.get("sun"))
    scenes = {"cornell": ptx.Scene.load_gltf(ctx, CORNELL), "plaza": from_dict(proc.plaza_scene(2, sun=True, alpha=True))}
    os.environ["PTX_FORCE_GLOBAL"] = "1"
    try:
        scenes["atrium"] = from_dict(proc.atrium_scene(1))
    finally:
        os.environ.pop("PTX_FORCE_GLOBAL", None)
    return scenes


@contextlib.contextmanager
def small_pair_pool():
    """PTX_WF_PAIRS_M=1 for the renders inside: a 1 Mi-pair pool, so that a rank's workspace stays small."""
    os.environ["PTX_WF_PAIRS_M"] = "1"
    try:
        yield
    finally:
        os.environ.pop("PTX_WF_PAIRS_M", None)


def _bits(a):
    return np.ascontiguousarray(a, np.float32).view(np.uint32)


class _UniqueId(ctypes.Structure):
    _fields_ = [("internal", ctypes.c_char * 128)]


def main():
    out, transport = sys.argv[1], sys.argv[2]
    rank, world = int(os.environ["RANK"]), int(os.environ["WORLD_SIZE"])
    if transport == "rccl":
        dev = int(os.environ["LOCAL_RANK"])
        torch.cuda.set_device(dev)
        dist.init_process_group("nccl", device_id=torch.device("cuda", dev))
        kinds = ("dev",)
    elif transport == "gloo0":
        dev = 0
        torch.cuda.set_device(0)
        dist.init_process_group("gloo")
        kinds = ("host", "dev")
    else:
        raise SystemExit(f"unknown transport {transport!r}")
    assert dist.get_rank() == rank and dist.get_world_size() == world
    ptx = importlib.import_module(PKG)
    mg = importlib.import_module(PKG + ".multigpu")
    ctx = ptx.Context(dev)
    sc = build_scenes(ptx, ctx)
    res, stats = {}, {}

    def zeros(kind, shape, dtype=torch.float32):
        return torch.zeros(shape, dtype=dtype, device=f"cuda:{dev}" if kind == "dev" else "cpu")

    def host(t):
        ctx.synchronize()
        return t.cpu().numpy()

    def keep(key, buf, st=None):
        res[key] = host(buf).copy()
        if st is not None:
            stats[key] = {k: st[k] for k in ("rays", "samples", "passes")}

    def shard_kept(buf, own, mask, what):
        """On a rank other than the root the collective may leave anything in the other ranks' pixels; in its own it can only have
        added zeros to what this rank rendered."""
        if rank != 0:
            np.testing.assert_array_equal(_bits(host(buf))[mask], _bits(own)[mask], err_msg=f"rank {rank}: {what}: own shard after the reduce")

    mask = mg.tile_mask(rank, world, W, H, TILE)
    qmask = mg.tile_mask(rank, world, Q_W, Q_H, Q_TILE)
    # this rank's shard alone, into buffers no collective sees
    own_tiles, _ = sc["cornell"].render(W, H, SPP, B, shard=(rank, world, TILE))
    own_pix, own_cl, _ = sc["plaza"].render_transparent(W, H, T_SPP, T_B, shard=(rank, world, TILE))
    with small_pair_pool():
        own_queue, _ = sc["atrium"].render(Q_W, Q_H, Q_SPP, Q_B, shard=(rank, world, Q_TILE))
    assert (own_tiles[..., 3][mask] == SPP).all() and not own_tiles[~mask].any()

    for kind in kinds:
        acc = zeros(kind, (H, W, 4))
        torch.cuda.synchronize()
        st = mg.render_tiles(sc["cornell"], W, H, SPP, B, acc, rank, world, tile=TILE)
        keep(f"tiles_{kind}", acc, st)
        shard_kept(acc, own_tiles, mask, f"tiles_{kind}")

        # without stats the library returns with the render in flight on its own stream: only multigpu's synchronise orders the collective
        acc = zeros(kind, (H, W, 4))
        torch.cuda.synchronize()
        mg.render_tiles(sc["cornell"], W, H, SPP, B, acc, rank, world, tile=TILE, want_stats=False)
        keep(f"tiles_nostats_{kind}", acc)
        shard_kept(acc, own_tiles, mask, f"tiles_nostats_{kind}")

        for key, spp in (("samples", SPP), ("samples16", SPP_UNEVEN)):
            acc = zeros(kind, (H, W, 4))
            torch.cuda.synchronize()
            st = mg.render_samples(sc["cornell"], W, H, spp, B, acc, rank, world)
            keep(f"{key}_{kind}", acc, st)

        acc = zeros(kind, (H, W, 4))
        torch.cuda.synchronize()
        st = mg.render_sharded(sc["cornell"], W, H, WEAK_SPP, B, acc, rank, world)
        keep(f"weak_{kind}", acc, st)

        pix, cl = zeros(kind, (H, W, 4)), zeros(kind, (H, W), torch.uint8)
        torch.cuda.synchronize()
        st = mg.render_tiles(sc["plaza"], W, H, T_SPP, T_B, pix, rank, world, tile=TILE, transparent=True, claimed=cl)
        keep(f"transparent_{kind}", pix, st)
        res[f"transparent_claimed_{kind}"] = host(cl).copy()
        shard_kept(pix, own_pix, mask, f"transparent_{kind}")
        np.testing.assert_array_equal(res[f"transparent_claimed_{kind}"], own_cl, err_msg=f"rank {rank}: claimed is local: only the own tiles are set")

        acc = zeros(kind, (Q_H, Q_W, 4))
        torch.cuda.synchronize()
        with small_pair_pool():
            st = mg.render_tiles(sc["atrium"], Q_W, Q_H, Q_SPP, Q_B, acc, rank, world, tile=Q_TILE)
        tm = ctx.timing()
        assert tm["pipeline"] == 1, tm
        keep(f"queue_tiles_{kind}", acc, st)
        shard_kept(acc, own_queue, qmask, f"queue_tiles_{kind}")
        print(f"rank {rank}/{world} {transport} {kind}: workspace_bytes after the queue-route mode = {tm['workspace_bytes']}", flush=True)

        for name in AOV_SCENES:
            own_A, own_N, _ = sc[name].render_aov(W, H, AOV_SPP, shard=(rank, world, TILE))
            A, N = zeros(kind, (H, W, 4)), zeros(kind, (H, W, 4))
            torch.cuda.synchronize()
            _, _, st = sc[name].render_aov(W, H, AOV_SPP, albedo=A, normal_depth=N, shard=(rank, world, TILE))
            ctx.synchronize()
            assert not host(A)[~mask].any() and not host(N)[~mask].any(), f"rank {rank}: {name}: guide pixels written outside the shard's tiles"
            mg.reduce_accum(A, 0)
            mg.reduce_accum(N, 0)
            keep(f"aov_tiles_{name}_albedo_{kind}", A, st)
            keep(f"aov_tiles_{name}_normal_{kind}", N)
            shard_kept(A, own_A, mask, f"aov_tiles {name} albedo {kind}")
            shard_kept(N, own_N, mask, f"aov_tiles {name} normal_depth {kind}")

        # denoise: "reduce the buffers first, then filter on the root" (include/ptx.h)
        a, b, A, N = (zeros(kind, (D_H, D_W, 4)) for _ in range(4))
        torch.cuda.synchronize()
        mg.render_tiles(sc["cornell"], D_W, D_H, D_HALF, D_B, a, rank, world, tile=TILE, seed=D_SEED, sample0=0)
        mg.render_tiles(sc["cornell"], D_W, D_H, D_HALF, D_B, b, rank, world, tile=TILE, seed=D_SEED, sample0=D_HALF)
        sc["cornell"].render_aov(D_W, D_H, 2 * D_HALF, albedo=A, normal_depth=N, seed=D_SEED, shard=(rank, world, TILE))
        ctx.synchronize()
        mg.reduce_accum(A, 0)
        mg.reduce_accum(N, 0)
        torch.cuda.synchronize()
        before = [host(x).copy() for x in (a, b, A, N)]
        # every rank filters what it holds (only the root's buffers are the frame, and only its result is kept)
        filtered, _ = ctx.denoise(a, b, A, N, D_HALF, D_HALF)
        for x, was, what in zip((a, b, A, N), before, ("a", "b", "albedo", "normal_depth")):
            np.testing.assert_array_equal(_bits(host(x)), _bits(was), err_msg=f"rank {rank}: ptx_denoise modified its input {what} ({kind})")
        keep(f"denoise_{kind}", filtered)
        for x, what in zip(before, ("a", "b", "albedo", "normal")):
            res[f"denoise_in_{what}_{kind}"] = x

    if transport == "rccl":
        # ptx_reduce_framebuffer on a communicator made the way a C++ host would: rank 0's ncclGetUniqueId reaches the others through
        # the process group, then ncclCommInitRank on every rank
        rccl = ctypes.CDLL(os.path.join(os.path.dirname(torch.__file__), "lib", "librccl.so"), mode=ctypes.RTLD_GLOBAL)
        uid = _UniqueId()
        if rank == 0:
            assert rccl.ncclGetUniqueId(ctypes.byref(uid)) == 0
        box = [bytes(uid)]
        dist.broadcast_object_list(box, src=0)
        uid = _UniqueId.from_buffer_copy(box[0])
        comm = ctypes.c_void_p()
        rccl.ncclCommInitRank.argtypes = [ctypes.POINTER(ctypes.c_void_p), ctypes.c_int, _UniqueId, ctypes.c_int]
        rccl.ncclCommDestroy.argtypes = [ctypes.c_void_p]
        assert rccl.ncclCommInitRank(ctypes.byref(comm), world, uid, rank) == 0
        try:
            acc = zeros("dev", (H, W, 4))
            torch.cuda.synchronize()
            _, st = sc["cornell"].render(W, H, SPP, B, accum=acc, shard=(rank, world, TILE))
            ctx.reduce_framebuffer(comm, acc, root=0)      # on the context's stream, behind the render
            keep("reduce_c_abi_dev", acc, st)
            shard_kept(acc, own_tiles, mask, "reduce_c_abi")
        finally:
            rccl.ncclCommDestroy(comm)

    with open(f"{out}.rank{rank}.json", "w") as fh:
        json.dump(stats, fh)
    if rank == 0:
        np.savez(out, **res)
    dist.barrier()
    dist.destroy_process_group()
    for s in sc.values():
        s.close()
    ctx.close()


if __name__ == "__main__":
    main()
