#!/usr/bin/env python3
"""ptx_render_adaptive on the MI355X: what a decision costs next to the round it follows, and what the per-pixel counts buy.

  tools/bench_adaptive.py cost [reps]        plaza (level 3), 8 samples first, 8 per round, cap 64, threshold 0.1, device buffers, at
                                             1920 x 1080 and 3840 x 2160: the decision kernels' HIP-event time per round (select_ms / rounds)
                                             next to the integrator kernels' time per round, the smallest of `reps` calls; and the wall
                                             time of one stand-alone ptx_adaptive_select on the finished buffers (it includes the sync).
  tools/bench_adaptive.py payoff [ref_spp]   plaza (level 3), atrium (detail 5) and Cornell at 1920 x 1080, thresholds 0.05, 0.1 and 0.2, cap 64:
                                             wall time and tonemapped mean squared error (the product's own image write, bytes / 255)
                                             against the product's ref_spp frame (4096, seed 77) of the adaptive render and of the uniform
                                             ptx_render at the next even count above the adaptive mean.
  tools/bench_adaptive.py --nee [out] [ref_spp]   ptx_render_adaptive_nee and ptx_denoise_counts on Cornell (threshold 0.2) and plaza (level 3,
                                             threshold 0.1) at 1920 x 1080, 8 samples first, 8 per round, cap 64, device buffers; wall times are the
                                             smallest of 3 synchronised calls after a warm-up, the variants alternated call by call:
                                             (a) the call with and without PTX_NEE_FUSED, against the same rounds rendered as one sequence of
                                                 passes per half (PTX_ADAPTIVE_NEE_HALVES=1: two ptx_render_nee pass sequences per round plus the
                                                 decision) — the difference over the rounds is the fixed price per round that the one-sequence
                                                 form saves;
                                             (b) error and wall time against the uniform ptx_render_nee frame at the next even count above the
                                                 adaptive mean (tonemapped mean squared error against the product's ref_spp frame, 1024, seed 77);
                                             (c) ptx_denoise_counts: kernel time, and the error after it.
                                             The JSON lines go to `out` (profiles/adaptive_nee_bench.txt) too.
  tools/bench_adaptive.py --sharded [out]    the sharded decision (ptx_ctx_set_mask_exchange) on ONE GPU: plaza (level 3), threshold 0.1, device
                                             buffers and a device mask, at 1920 x 1080 and 3840 x 2160. The rank is 0 of 2 with a shard tile of
                                             16384, so it owns every pixel and the exchange is the identity: the frame is the unsharded one, and
                                             what is timed is the sharded kernels and the callback's round trip. select_ms per round of the two
                                             forms, alternated call by call (the smallest of 3 after a warm-up), and the exchange's wall time per
                                             round. Then the balance figure: from the per-pixel counts of that 1080p frame and of a Cornell
                                             frame with light sampling, the per-rank sample share (max / mean) of 8 ranks under interleaved
                                             64 x 64 tiles and under 8 horizontal strips. The JSON lines go to `out`
                                             (profiles/adaptive_sharded_bench.txt) too.
Prints one JSON line per measurement.
"""
import importlib
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
ptx = importlib.import_module("distributed-path-tracer_amd")
proc = importlib.import_module("distributed-path-tracer_amd.procedural")
CORNELL = os.path.join(ROOT, "scenes", "cornell-box", "cornell.gltf")
BOUNCES, SEED, MIN, STEP, CAP = 4, 0x5EED, 8, 8, 64
KEYS = ("model_xform", "model_surf", "surf_range", "vertices", "triangles", "materials", "camera", "sun")


def zeros(W, H):
    import torch
    t = torch.zeros((H, W, 4), device="cuda:0")
    torch.cuda.synchronize()   # the fill runs on torch's stream, the library on its own
    return t


def cost(reps):
    ctx = ptx.Context(0)
    s = ptx.Scene.from_arrays(ctx, *[proc.plaza_scene()[k] for k in KEYS])
    for W, H in ((1920, 1080), (3840, 2160)):
        best = None
        for rep in range(reps + 1):   # the first call warms up
            a, b, st = s.render_adaptive(W, H, CAP, BOUNCES, MIN, STEP, 0.1, a=zeros(W, H), b=zeros(W, H), seed=SEED)
            if rep and (best is None or st["select_ms"] < best["select_ms"]):
                best = st
        alone = 1e9
        for rep in range(reps):
            t0 = time.perf_counter()
            ctx.adaptive_select(a, b, 0.1)
            alone = min(alone, (time.perf_counter() - t0) * 1e3)
        r = best["rounds"]
        print(json.dumps(dict(scene="plaza3", W=W, H=H, rounds=r, mean_spp=round(best["samples"] / (W * H), 2), select_ms_per_round=round(best["select_ms"] / r, 4),
                              render_kernel_ms_per_round=round(best["kernel_ms"] / r, 3), select_share=round(best["select_ms"] / (best["select_ms"] + best["kernel_ms"]), 5),
                              standalone_select_wall_ms=round(alone, 4))))


def payoff(ref_spp):
    ctx = ptx.Context(0)
    W, H = 1920, 1080
    scenes = {"plaza3": lambda: ptx.Scene.from_arrays(ctx, *[proc.plaza_scene()[k] for k in KEYS]),
              "atrium5": lambda: ptx.Scene.from_arrays(ctx, *[proc.atrium_scene()[k] for k in KEYS]),
              "cornell": lambda: ptx.Scene.load_gltf(ctx, CORNELL)}

    def image(mean):
        return ctx.tonemap_encode(mean, W, H, 1)[..., :3].astype(np.float64) / 255

    def mse(x, ref):
        return float(np.mean((x - ref) ** 2))
    for name, make in scenes.items():
        s = make()
        acc = zeros(W, H)
        s.render(W, H, ref_spp, BOUNCES, accum=acc, seed=77, want_stats=False)
        ref = image(ctx.accum_mean(acc))
        s.render_adaptive(W, H, CAP, BOUNCES, MIN, STEP, 0.2, a=zeros(W, H), b=zeros(W, H), seed=SEED, want_stats=False)   # warm-up
        for thr in (0.05, 0.1, 0.2):
            a, b = zeros(W, H), zeros(W, H)
            t0 = time.perf_counter()
            s.render_adaptive(W, H, CAP, BOUNCES, MIN, STEP, thr, a=a, b=b, seed=SEED, want_stats=False)   # always synchronises
            t_adaptive = time.perf_counter() - t0
            counts = (a[..., 3] + b[..., 3]).cpu().numpy()
            n = 2 * int(counts.mean() // 2) + 2
            u = zeros(W, H)
            t0 = time.perf_counter()
            s.render(W, H, n, BOUNCES, accum=u, seed=SEED, want_stats=False)
            ctx.synchronize()
            t_uniform = time.perf_counter() - t0
            print(json.dumps(dict(scene=name, W=W, H=H, threshold=thr, cap=CAP, mean_spp=round(float(counts.mean()), 2), at_min=round(float((counts == MIN).mean()), 4),
                                  at_cap=round(float((counts == CAP).mean()), 4), adaptive_s=round(t_adaptive, 4), adaptive_mse=mse(image(ctx.accum_mean(a, b)), ref),
                                  uniform_spp=n, uniform_s=round(t_uniform, 4), uniform_mse=mse(image(ctx.accum_mean(u)), ref), ref_spp=ref_spp)))
        s.close()


def nee(out_path, ref_spp):
    ctx = ptx.Context(0)
    W, H, reps = 1920, 1080, 3
    FUSED = ptx.NEE_FUSED
    scenes = {"cornell": (lambda: ptx.Scene.load_gltf(ctx, CORNELL), 0.2),
              "plaza3": (lambda: ptx.Scene.from_arrays(ctx, *[proc.plaza_scene()[k] for k in KEYS]), 0.1)}
    lines = []

    def emit(**kw):
        lines.append(json.dumps(kw))
        print(lines[-1], flush=True)

    def image(mean):
        return ctx.tonemap_encode(mean, W, H, 1)[..., :3].astype(np.float64) / 255

    def mse(x, ref):
        return float(np.mean((x - ref) ** 2))

    def timed(call):
        """wall seconds of one synchronised call on fresh device buffers"""
        a, b = zeros(W, H), zeros(W, H)
        t0 = time.perf_counter()
        out = call(a, b)
        ctx.synchronize()
        return time.perf_counter() - t0, a, b, out
    for name, (make, thr) in scenes.items():
        s = make()

        def adaptive(flags, halves):
            def call(a, b):
                if halves:
                    os.environ["PTX_ADAPTIVE_NEE_HALVES"] = "1"
                try:
                    return s.render_adaptive_nee(W, H, CAP, BOUNCES, MIN, STEP, thr, a=a, b=b, seed=SEED, want_stats=False, flags=flags)
                finally:
                    os.environ.pop("PTX_ADAPTIVE_NEE_HALVES", None)
            return call
        variants = {"fused": adaptive(FUSED, False), "fused_two_sequences": adaptive(FUSED, True), "unfused": adaptive(0, False), "unfused_two_sequences": adaptive(0, True)}
        # (a) alternated: a warm-up of every variant, then `reps` rounds over the variants
        best, keep = {k: 1e9 for k in variants}, None
        for rep_i in range(reps + 1):
            for k, call in variants.items():
                t, a, b, _ = timed(call)
                if rep_i:
                    best[k] = min(best[k], t)
                if k == "fused":
                    keep = (a, b)
        a, b = keep
        _, _, st = s.render_adaptive_nee(W, H, CAP, BOUNCES, MIN, STEP, thr, a=zeros(W, H), b=zeros(W, H), seed=SEED, flags=FUSED)
        rounds = st["rounds"]
        counts = (a[..., 3] + b[..., 3]).cpu().numpy()
        emit(part="a", scene=name, W=W, H=H, threshold=thr, cap=CAP, rounds=rounds, passes=st["passes"], mean_spp=round(float(counts.mean()), 2),
             at_min=round(float((counts == MIN).mean()), 4), at_cap=round(float((counts == CAP).mean()), 4), **{k + "_s": round(v, 4) for k, v in best.items()},
             fused_saved_ms_per_round=round((best["fused_two_sequences"] - best["fused"]) * 1e3 / rounds, 3),
             unfused_saved_ms_per_round=round((best["unfused_two_sequences"] - best["unfused"]) * 1e3 / rounds, 3), select_ms_per_round=round(st["select_ms"] / rounds, 4))
        # (b) against the uniform frame at the next even count above the mean
        acc = zeros(W, H)
        s.render_nee(W, H, ref_spp, BOUNCES, accum=acc, seed=77, want_stats=False, flags=FUSED)
        ref = image(ctx.accum_mean(acc))
        n = 2 * int(counts.mean() // 2) + 2
        t_uniform, u = 1e9, None
        for rep_i in range(reps + 1):
            u = zeros(W, H)
            t0 = time.perf_counter()
            s.render_nee(W, H, n, BOUNCES, accum=u, seed=SEED, want_stats=False, flags=FUSED)
            ctx.synchronize()
            if rep_i:
                t_uniform = min(t_uniform, time.perf_counter() - t0)
        mse_adaptive = mse(image(ctx.accum_mean(a, b)), ref)
        emit(part="b", scene=name, threshold=thr, mean_spp=round(float(counts.mean()), 2), adaptive_s=round(best["fused"], 4), adaptive_mse=mse_adaptive, uniform_spp=n,
             uniform_s=round(t_uniform, 4), uniform_mse=mse(image(ctx.accum_mean(u)), ref), ref_spp=ref_spp)
        # (c) the filter on the adaptive halves, guides over the first MIN samples
        alb, nd = zeros(W, H), zeros(W, H)
        t0 = time.perf_counter()
        s.render_aov(W, H, MIN, albedo=alb, normal_depth=nd, seed=SEED, want_stats=False)
        ctx.synchronize()
        t_guides = time.perf_counter() - t0
        out, filter_ms = zeros(W, H), 1e9
        for rep_i in range(reps + 1):
            _, dst = ctx.denoise_counts(a, b, alb, nd, MIN, out=out)
            if rep_i:
                filter_ms = min(filter_ms, dst["kernel_ms"])
        emit(part="c", scene=name, guides_s=round(t_guides, 4), denoise_counts_kernel_ms=round(filter_ms, 3), unfiltered_mse=mse_adaptive, filtered_mse=mse(image(out), ref))
        s.close()
    with open(out_path, "w") as fh:
        fh.write("# tools/bench_adaptive.py --nee: 1920 x 1080, 4 bounces, 8 + 8 per round, cap 64; wall seconds are the smallest of 3 synchronised calls\n")
        fh.write("\n".join(lines) + "\n")


def sharded(out_path):
    import torch
    mg = importlib.import_module("distributed-path-tracer_amd.multigpu")
    ctx = ptx.Context(0)
    s = ptx.Scene.from_arrays(ctx, *[proc.plaza_scene()[k] for k in KEYS])
    lines, reps = [], 3

    def emit(**kw):
        lines.append(json.dumps(kw))
        print(lines[-1], flush=True)

    def balance(name, counts):
        H, W = counts.shape
        total = float(counts.sum(dtype=np.float64))
        tiles = [float(counts[mg.tile_mask(r, 8, W, H, 64)].sum(dtype=np.float64)) for r in range(8)]
        strips = [float(c.sum(dtype=np.float64)) for c in np.array_split(counts, 8, axis=0)]
        emit(part="balance", scene=name, W=W, H=H, ranks=8, mean_spp=round(float(counts.mean()), 2), tiles64_max_over_mean=round(max(tiles) / (total / 8), 4),
             strips_max_over_mean=round(max(strips) / (total / 8), 4))
    for W, H in ((1920, 1080), (3840, 2160)):
        mask = torch.zeros(W * H, dtype=torch.uint8, device="cuda:0")
        torch.cuda.synchronize()
        best = {"unsharded": None, "sharded": None}
        wall, frames = 1e9, {}
        for rep_i in range(reps + 1):   # the first call of each form warms up
            for form in best:
                if form == "sharded":
                    ctx.set_mask_exchange(lambda m, n: 0, mask)
                try:
                    a, b, st = s.render_adaptive(W, H, CAP, BOUNCES, MIN, STEP, 0.1, a=zeros(W, H), b=zeros(W, H), seed=SEED, shard=(0, 2, 16384) if form == "sharded" else None)
                finally:
                    ctx.set_mask_exchange(None)
                frames[form] = (a, b)
                if rep_i and (best[form] is None or st["select_ms"] < best[form]["select_ms"]):
                    best[form] = st
                if rep_i and form == "sharded":
                    wall = min(wall, ctx.mask_exchange_stats()["wall_ms"] / st["rounds"])
        same = all(torch.equal(x.view(torch.int32), y.view(torch.int32)) for x, y in zip(frames["unsharded"], frames["sharded"]))
        u, sh = best["unsharded"], best["sharded"]
        emit(part="cost", scene="plaza3", W=W, H=H, rounds=u["rounds"], same_bits=same, unsharded_select_ms_per_round=round(u["select_ms"] / u["rounds"], 4),
             sharded_select_ms_per_round=round(sh["select_ms"] / sh["rounds"], 4), ratio=round(sh["select_ms"] / u["select_ms"], 3), exchange_wall_ms_per_round=round(wall, 4),
             render_kernel_ms_per_round=round(u["kernel_ms"] / u["rounds"], 3))
        if W == 1920:
            a, b = frames["unsharded"]
            balance("plaza3", (a[..., 3] + b[..., 3]).cpu().numpy())
    s.close()
    c = ptx.Scene.load_gltf(ctx, CORNELL)
    a, b, _ = c.render_adaptive_nee(1920, 1080, CAP, BOUNCES, MIN, STEP, 0.2, a=zeros(1920, 1080), b=zeros(1920, 1080), seed=SEED, want_stats=False, flags=ptx.NEE_FUSED)
    balance("cornell_nee", (a[..., 3] + b[..., 3]).cpu().numpy())
    with open(out_path, "w") as fh:
        fh.write("# tools/bench_adaptive.py --sharded: one GPU, 4 bounces, 8 + 8 per round, cap 64; select_ms is HIP-event time of the decision kernels, the smallest of 3 calls\n")
        fh.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    if len(sys.argv) > 1 and sys.argv[1] == "--sharded":
        sharded(sys.argv[2] if len(sys.argv) > 2 else os.path.join(ROOT, "profiles", "adaptive_sharded_bench.txt"))
    elif len(sys.argv) > 1 and sys.argv[1] == "--nee":
        nee(sys.argv[2] if len(sys.argv) > 2 else os.path.join(ROOT, "profiles", "adaptive_nee_bench.txt"), int(sys.argv[3]) if len(sys.argv) > 3 else 1024)
    elif len(sys.argv) > 1 and sys.argv[1] == "payoff":
        payoff(int(sys.argv[2]) if len(sys.argv) > 2 else 4096)
    else:
        cost(int(sys.argv[2]) if len(sys.argv) > 2 else 5)
