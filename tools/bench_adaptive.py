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


if __name__ == "__main__":
    if len(sys.argv) > 1 and sys.argv[1] == "payoff":
        payoff(int(sys.argv[2]) if len(sys.argv) > 2 else 4096)
    else:
        cost(int(sys.argv[2]) if len(sys.argv) > 2 else 5)
