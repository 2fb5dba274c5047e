"""Multi-GPU host logic for the one exchange step the path has: the framebuffer sum.

One process per GPU (torch.distributed; backend "nccl" is RCCL over xGMI on ROCm, "gloo" on CPU in the tests).
The scene is replicated on every GPU (it is small next to 288 GB of HBM). ONE frame is sharded in one of two ways
(SURVEY.md section 8e), both ending in ONE sum-reduce of the float32 accumulation buffer (W*H*4 floats: 33.2 MB at 1080p,
132.7 MB at 4K) onto rank 0:

  * samples (`render_samples`, strong scaling, the default): rank r traces the r-th of `world` contiguous slices of the
    frame's sample indices, of every pixel — perfectly balanced whatever the image looks like. Random numbers are keyed by
    (pixel, GLOBAL sample index), so the union over ranks is exactly the sample set of a single-GPU render.
  * tiles (`render_tiles`, strong scaling; "image tiles shard across the GPUs" of BASELINE configs 4-5): the frame is cut into
    64 x 64 tiles, tile t (row-major) belongs to rank t % world — interleaved, so that expensive and cheap image regions are
    dealt out evenly; each rank renders all samples of its tiles in ONE launch sequence (ptx_render_cfg.shard_*: a pixel list
    inside the library) straight into a zeroed full-frame buffer; the sum (x + 0 = x) is bitwise the single-GPU frame.

`render_adaptive_tiles` is the tile split for frames of noise-driven per-pixel sample counts (Scene.render_adaptive*): besides the sum at
the end the ranks exchange one byte per pixel per round, and the result is bitwise the frame of one process.

`render_sharded` is the weak-scaling variant (every rank adds `spp` samples of its own: the frame gets world * spp).
This replaces the reference's planned (never implemented) SNS/SQS fan-in — path-tracer-core/src/models/work_info.hpp:22-23,
intersection_worker.cpp:78-110.
"""

TILE = 64   # interleaved 64 x 64 tiles


def sample_range(rank: int, world: int, spp_per_rank: int):
    """First sample index and count for `rank` (weak scaling: every rank traces spp_per_rank samples per pixel)."""
    if not (0 <= rank < world) or spp_per_rank < 0:
        raise ValueError("bad rank / world / spp")
    return rank * spp_per_rank, spp_per_rank


def split_samples(rank: int, world: int, spp_total: int):
    """Strong-scaling split of a fixed sample budget: contiguous, disjoint, complete, sizes differ by at most 1."""
    if not (0 <= rank < world) or spp_total < 0:
        raise ValueError("bad rank / world / spp")
    base, extra = divmod(spp_total, world)
    first = rank * base + min(rank, extra)
    return first, base + (1 if rank < extra else 0)


def tile_owner(x: int, y: int, W: int, world: int, tile: int = TILE):
    """Rank that renders pixel (x, y): the row-major index of its tile, modulo the number of ranks (ptx_render_cfg.shard_*)."""
    tiles_x = (W + tile - 1) // tile
    return ((y // tile) * tiles_x + (x // tile)) % world


def tile_mask(rank: int, world: int, W: int, H: int, tile: int = TILE):
    """Boolean [H, W] mask of the pixels `rank` renders under interleaved tile sharding."""
    import numpy as np
    if not (0 <= rank < world):
        raise ValueError("bad rank / world")
    tiles_x = (W + tile - 1) // tile
    ty, tx = np.meshgrid(np.arange(H) // tile, np.arange(W) // tile, indexing="ij")
    return (ty * tiles_x + tx) % world == rank


def _order_before_reduce(scene):
    """The library launches on its context's own non-blocking stream; the collective runs on torch's. Wait for the render
    before the buffer is handed to the collective (the host-side sync costs microseconds next to a frame)."""
    ctx = getattr(scene, "ctx", None)
    if ctx is not None:
        ctx.synchronize()


def reduce_accum(accum, dst: int = 0):
    """Sum-reduce the accumulation buffer (a torch tensor, on the GPU for nccl / on the CPU for gloo) onto rank dst."""
    import torch.distributed as dist
    if dist.is_available() and dist.is_initialized():
        dist.reduce(accum, dst=dst, op=dist.ReduceOp.SUM)
    return accum


_NO_SAMPLE_SPLIT = ("transparent_background blends the samples of a pixel in sample order (a recurrence, not a sum: renderer.cpp:374-399): "
                    "sample ranges rendered into separate buffers cannot be merged — shard the frame by tiles (render_tiles)")


def render_sharded(scene, W, H, spp_per_rank, bounces, accum, rank, world, transparent=False, **kw):
    """WEAK scaling: render this rank's own `spp_per_rank` samples (global indices [rank*spp, (rank+1)*spp)) into `accum` (sums)
    and reduce onto rank 0: the frame receives world * spp_per_rank samples. Returns the stats of the local render.
    `scene` is a distributed-path-tracer_amd.Scene (anything with the same .render signature). `accum` must be ready (zeroed)
    before the call as far as the library's stream is concerned: synchronise torch's stream after preparing it.
    transparent=True raises ValueError: the transparent-background blend does not compose over sample ranges."""
    if transparent:
        raise ValueError(_NO_SAMPLE_SPLIT)
    s0, n = sample_range(rank, world, spp_per_rank)
    _, stats = scene.render(W, H, n, bounces, accum=accum, sample0=s0, **kw)
    _order_before_reduce(scene)
    reduce_accum(accum, 0)
    return stats


def render_samples(scene, W, H, spp_total, bounces, accum, rank, world, transparent=False, **kw):
    """STRONG scaling by samples: ONE frame of `spp_total` samples per pixel; this rank traces its contiguous share of the
    sample indices of every pixel, then the buffers are sum-reduced onto rank 0.
    transparent=True raises ValueError: the transparent-background blend does not compose over sample ranges."""
    if transparent:
        raise ValueError(_NO_SAMPLE_SPLIT)
    s0, n = split_samples(rank, world, spp_total)
    stats = {"rays": 0, "samples": 0, "passes": 0, "kernel_ms": 0.0}
    if n > 0:
        _, stats = scene.render(W, H, n, bounces, accum=accum, sample0=s0, **kw)
    _order_before_reduce(scene)
    reduce_accum(accum, 0)
    return stats


def render_tiles(scene, W, H, spp, bounces, accum, rank, world, tile=TILE, transparent=False, claimed=None, **kw):
    """STRONG scaling by interleaved tiles: this rank renders ALL `spp` samples of the 64 x 64 image tiles t with
    t % world == rank into the full-frame `accum` ([H,W,4], zero elsewhere); the sum-reduce then assembles the frame on rank 0
    (x + 0 == x: bitwise the single-GPU frame). Returns the stats of the local render.
    transparent=True: renderer::transparent_background. `accum` is then the full-frame blend state of Scene.render_transparent
    (running colour and alpha: means, to be written with spp = 1) and `claimed` its [H,W] uint8 flags of the same kind (zeroed; this
    rank's part of them stays local — only `accum` is reduced). Every pixel belongs to one rank, which blends all of its samples in
    order, so the sum of the ranks' buffers is bitwise the single-GPU frame here too."""
    if transparent:
        if claimed is None:
            raise ValueError("render_tiles(transparent=True) needs a zeroed `claimed` buffer ([H,W] uint8) beside `accum`")
        _, _, stats = scene.render_transparent(W, H, spp, bounces, pixels=accum, claimed=claimed, shard=(rank, world, tile), **kw)
    else:
        _, stats = scene.render(W, H, spp, bounces, accum=accum, shard=(rank, world, tile), **kw)
    _order_before_reduce(scene)
    reduce_accum(accum, 0)
    return stats if stats is not None else {"rays": 0, "samples": 0, "passes": 0, "kernel_ms": 0.0}


def render_adaptive_tiles(scene, W, H, cap, bounces, a, b, rank, world, tile=TILE, min_spp=8, step_spp=0, threshold=0.1, nee_flags=None,
                          transparent=False, **kw):
    """Noise-driven per-pixel sample counts over interleaved tiles: this rank runs the adaptive loop on the `tile` x `tile` image tiles t
    with t % world == rank, into the zeroed full-frame half-buffers `a` and `b` ([H,W,4], both host memory — numpy, or CPU tensors for gloo — or both torch-on-GPU). After every
    round the ranks merge one byte per pixel — which pixels are still noisy — with an all-reduce (MAX), and each decides the whole frame
    from the merged mask, so all ranks run the same number of rounds; then `a` and `b` are sum-reduced onto rank 0. The result there is
    BITWISE Scene.render_adaptive (nee_flags=None) or Scene.render_adaptive_nee (nee_flags: an int, its flags) of one process with the
    same arguments: every pixel belongs to one rank, which gives it the samples the one-process loop gives it. Returns the stats of the
    local render: rays, samples, passes and the light-sample counts are this rank's own, `rounds` is the same on every rank, and
    `active_last` sums over the ranks to the one-process value.
    The mask lives in the same kind of memory as `a`: a device tensor is reduced in place by the process group (nccl = RCCL on ROCm), a
    numpy array through gloo. transparent=True raises ValueError: the adaptive decision takes radiance sums, which the transparent-background
    blend does not produce."""
    import numpy as np
    import torch
    import torch.distributed as dist
    if transparent:
        raise ValueError("render_adaptive_tiles: the adaptive decision takes radiance sums, which transparent_background's blend does not produce")
    ctx = scene.ctx
    x0, y0, w, h = kw.get("tile") or (0, 0, W, H)   # Scene.render_adaptive's rectangle (kw["tile"]), not the shard tile
    on_host = isinstance(a, np.ndarray) or a.device.type == "cpu"
    # the mask in the kind of memory `a` is in, and as the tensor the collective takes (torch.from_numpy shares the array's memory)
    mask = np.zeros(w * h, np.uint8) if isinstance(a, np.ndarray) else torch.zeros(w * h, dtype=torch.uint8, device=a.device)
    wire = torch.from_numpy(mask) if isinstance(mask, np.ndarray) else mask
    live = dist.is_available() and dist.is_initialized()

    def exchange(_mask, _n_bytes):
        if live:
            dist.all_reduce(wire, op=dist.ReduceOp.MAX)
            if not on_host:
                torch.cuda.synchronize(a.device)   # the collective ran on torch's stream: the library reads the mask on its own
        return 0

    if not on_host:
        torch.cuda.synchronize(a.device)   # the fill of `mask` ran on torch's stream
    ctx.set_mask_exchange(exchange, mask)
    try:
        if nee_flags is None:
            _, _, stats = scene.render_adaptive(W, H, cap, bounces, min_spp, step_spp, threshold, a=a, b=b, shard=(rank, world, tile), **kw)
        else:
            _, _, stats = scene.render_adaptive_nee(W, H, cap, bounces, min_spp, step_spp, threshold, a=a, b=b, shard=(rank, world, tile), flags=nee_flags, **kw)
    finally:
        ctx.set_mask_exchange(None)
    _order_before_reduce(scene)
    for buf in (a, b):
        reduce_accum(torch.from_numpy(buf) if isinstance(buf, np.ndarray) else buf, 0)
    return stats
