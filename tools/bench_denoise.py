#!/usr/bin/env python3
"""ptx_denoise on the MI355X: kernel time of both a-trous kernel forms, and the quality the filter reaches on the product's renders.

  tools/bench_denoise.py time [W H reps]     Cornell, 8 + 8 spp, device buffers. Per form (PTX_DENOISE_TILED = 0 / 0xFF) and iteration
                                             count k = 1 .. 5: the smallest kernel_ms of `reps` alternated calls. t(k) - t(k-1) is the
                                             cost of the iteration at step 2^(k-1) (t(1) also holds the prepare and prefilter kernels).
  tools/bench_denoise.py quality             mean squared error after x / (1 + x) against the product's 512-spp frame (seed 77), noisy /
                                             denoised, on Cornell, plaza level 2 and jack-of-blades at 96 x 54 and 240 x 135, 2+2 and 8+8 spp.
  tools/bench_denoise.py emission [W H reps] k_em_split (two halves) and k_em_merge (ptx_emission_split, ptx_emission_merge) on device buffers
                                             next to one a-trous iteration, alternated in one process. The two calls take no stats, so a batch
                                             of 100 back-to-back calls is timed on the host and divided (the smallest of `reps` batches); the
                                             bytes are 16 per pixel and buffer, read and written: 80 for the split, 48 for the merge. The
                                             a-trous row is kernel_ms(iterations = 2) - kernel_ms(iterations = 1) of ptx_denoise.
Prints one JSON line per measurement.
"""
import importlib
import json
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
ptx = importlib.import_module("distributed-path-tracer_amd")
proc = importlib.import_module("distributed-path-tracer_amd.procedural")
CORNELL = os.path.join(ROOT, "scenes", "cornell-box", "cornell.gltf")
JACK = os.path.join(ROOT, "scenes", "jack-of-blades", "jack-of-blades.gltf")
BOUNCES, SEED = 8, 0x5EED


def frames(s, W, H, half, device=False):
    import torch
    def mk():
        if not device:
            return np.zeros((H, W, 4), np.float32)
        t = torch.zeros((H, W, 4), device="cuda:0")
        torch.cuda.synchronize()   # the fill runs on torch's stream, the library on its own
        return t
    a, _ = s.render(W, H, half, BOUNCES, accum=mk(), seed=SEED)
    b, _ = s.render(W, H, half, BOUNCES, accum=mk(), seed=SEED, sample0=half)
    A, N, _ = s.render_aov(W, H, 2 * half, albedo=mk(), normal_depth=mk(), seed=SEED)
    return a, b, A, N


def time_forms(W, H, reps):
    import torch
    ctx = ptx.Context(0)
    s = ptx.Scene.load_gltf(ctx, CORNELL)
    a, b, A, N = frames(s, W, H, 8, device=True)
    out = torch.empty_like(a)
    best = {}
    for rep in range(reps + 1):   # the first round warms up
        for k in range(1, 6):
            for mask in (0, 0xFF):
                os.environ["PTX_DENOISE_TILED"] = str(mask)
                _, st = ctx.denoise(a, b, A, N, 8, 8, iterations=k, out=out)
                if rep:
                    best[(mask, k)] = min(best.get((mask, k), 1e9), st["kernel_ms"])
    floor_ms = W * H * 48 / 6.29e12 * 1e3   # 48 B per pixel and iteration at the measured float4 copy bandwidth
    for mask in (0, 0xFF):
        t = [best[(mask, k)] for k in range(1, 6)]
        print(json.dumps(dict(form="tiled" if mask else "global", W=W, H=H, reps=reps, total_ms_k1_to_k5=[round(x, 4) for x in t],
                              step_ms=[round(t[k] - t[k - 1], 4) for k in range(1, 5)], hbm_floor_ms_per_iteration=round(floor_ms, 4))))


def time_emission(W, H, reps, batch=100):
    import time
    import torch
    ctx = ptx.Context(0)
    s = ptx.Scene.load_gltf(ctx, CORNELL)
    a, b, A, N = frames(s, W, H, 8, device=True)
    E, _ = s.render_emission(W, H, 16, emission=torch.zeros_like(a), seed=SEED)
    out = torch.empty_like(a)
    torch.cuda.synchronize()
    n = W * H
    best = dict(split=1e9, merge=1e9, atrous=1e9)

    def batch_ms(call):
        ctx.synchronize()
        t = time.perf_counter()
        for _ in range(batch):
            call()
        ctx.synchronize()
        return (time.perf_counter() - t) * 1e3 / batch
    for rep in range(reps + 1):   # the first round warms up; the halves drift by batch * a.w * e, which no timing depends on
        t_split = batch_ms(lambda: ctx.emission_split(E, 16, a, b))
        t_merge = batch_ms(lambda: ctx.emission_merge(E, 16, out))
        k = [ctx.denoise(a, b, A, N, 8, 8, iterations=i, out=out)[1]["kernel_ms"] for i in (1, 2)]
        if rep:
            best["split"], best["merge"], best["atrous"] = min(best["split"], t_split), min(best["merge"], t_merge), min(best["atrous"], k[1] - k[0])
    for name, nbytes in (("k_em_split", 80 * n), ("k_em_merge", 48 * n), ("atrous_iteration", None)):
        ms = best[name.replace("k_em_", "").replace("_iteration", "")]
        print(json.dumps(dict(kernel=name, W=W, H=H, reps=reps, ms=round(ms, 4), gbytes_per_s=round(nbytes / ms / 1e6, 1) if nbytes else None)))


def quality():
    ctx = ptx.Context(0)
    scenes = {"cornell": lambda: ptx.Scene.load_gltf(ctx, CORNELL),
              "plaza2": lambda: ptx.Scene.from_arrays(ctx, *[proc.plaza_scene(level=2)[k] for k in ("model_xform", "model_surf", "surf_range", "vertices", "triangles", "materials", "camera", "sun")]),
              "jack": lambda: ptx.Scene.load_gltf(ctx, JACK)}

    def tm(x):
        x = np.asarray(x[..., :3], np.float64)
        return x / (1 + x)
    for name, make in scenes.items():
        s = make()
        for W, H in ((96, 54), (240, 135)):
            ref = s.render(W, H, 512, BOUNCES, seed=77)[0] / np.float32(512)
            for half in (2, 8):
                a, b, A, N = frames(s, W, H, half)
                out, _ = ctx.denoise(a, b, A, N, half, half)
                noisy = (a + b) / np.float32(2 * half)
                ratio = np.mean((tm(noisy) - tm(ref)) ** 2) / np.mean((tm(out) - tm(ref)) ** 2)
                print(json.dumps(dict(scene=name, W=W, H=H, spp=2 * half, mse_noisy_over_denoised=round(float(ratio), 3))))
        s.close()


if __name__ == "__main__":
    if len(sys.argv) > 1 and sys.argv[1] == "quality":
        quality()
    elif len(sys.argv) > 1 and sys.argv[1] == "emission":
        argv = sys.argv[2:]
        time_emission(int(argv[0]) if argv else 1920, int(argv[1]) if len(argv) > 1 else 1080, int(argv[2]) if len(argv) > 2 else 10)
    else:
        argv = sys.argv[2:]
        time_forms(int(argv[0]) if argv else 1920, int(argv[1]) if len(argv) > 1 else 1080, int(argv[2]) if len(argv) > 2 else 20)
