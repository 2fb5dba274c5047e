#!/usr/bin/env python3
"""ptx_render_nee on the MI355X: what the light samples cost and what they buy.

  tools/bench_nee.py [ref_spp] [reps]   Cornell, atrium (detail 5) and plaza (level 3, no alpha) at 1920 x 1080, 8 bounces, device buffers:
                                        ptx_render_nee at 16 and 64 spp — wall time of the synchronised call (the smallest of `reps`, after
                                        a warm-up call), Msamples/s, and the mean squared error of the written bytes (the product's own
                                        image write, bytes / 255) against the product's ref_spp ptx_render frame (4096) of another seed;
                                        next to it ptx_render at equal spp, and ptx_render at the spp that takes the same time.
Prints one JSON line per measurement. A scene without listed emitters (atrium) shows the cost of the wavefront form alone.
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
W, H, BOUNCES, SEED, REF_SEED = 1920, 1080, 8, 0x5EED, 77
KEYS = ("model_xform", "model_surf", "surf_range", "vertices", "triangles", "materials", "camera", "sun")


def zeros():
    import torch
    t = torch.zeros((H, W, 4), device="cuda:0")
    torch.cuda.synchronize()   # the fill runs on torch's stream, the library on its own
    return t


def main(ref_spp, reps):
    ctx = ptx.Context(0)
    scenes = {"cornell": lambda: ptx.Scene.load_gltf(ctx, CORNELL),
              "atrium5": lambda: ptx.Scene.from_arrays(ctx, *[proc.atrium_scene()[k] for k in KEYS]),
              "plaza3_opaque": lambda: ptx.Scene.from_arrays(ctx, *[proc.plaza_scene(alpha=False)[k] for k in KEYS])}

    def image(acc, spp):
        return ctx.tonemap_encode(acc, W, H, spp)[..., :3].astype(np.float64) / 255

    def timed(call, spp):
        """-> (seconds: the smallest of `reps` synchronised calls after one warm-up, the last call's buffer and stats)"""
        best, acc, st = 1e30, None, None
        for rep in range(reps + 1):
            acc = zeros()
            t0 = time.perf_counter()
            _, st = call(spp, acc)
            ctx.synchronize()
            if rep:
                best = min(best, time.perf_counter() - t0)
        return best, acc, st

    for name, make in scenes.items():
        s = make()
        ref_acc = zeros()
        s.render(W, H, ref_spp, BOUNCES, accum=ref_acc, seed=REF_SEED, want_stats=False)
        ctx.synchronize()
        ref = image(ref_acc, ref_spp)
        del ref_acc

        def mse(acc, spp):
            return float(np.mean((image(acc, spp) - ref) ** 2))

        def nee(spp, acc):
            return s.render_nee(W, H, spp, BOUNCES, accum=acc, seed=SEED)

        def lib(spp, acc):
            return s.render(W, H, spp, BOUNCES, accum=acc, seed=SEED)
        for spp in (16, 64):
            t_nee, a_nee, st = timed(nee, spp)
            t_lib, a_lib, st_lib = timed(lib, spp)
            spp_eq = max(1, int(round(spp * t_nee / t_lib)))
            t_eq, a_eq, _ = timed(lib, spp_eq)
            print(json.dumps(dict(scene=name, W=W, H=H, bounces=BOUNCES, spp=spp, n_lights=st["n_lights"], nee_s=round(t_nee, 4),
                                  nee_msamples_s=round(W * H * spp / t_nee / 1e6, 1), nee_rays=st["rays"], nee_light_samples=st["light_samples"],
                                  nee_light_visible=st["light_visible"], nee_mse=mse(a_nee, spp), lib_s=round(t_lib, 4),
                                  lib_msamples_s=round(W * H * spp / t_lib / 1e6, 1), lib_rays=st_lib["rays"], lib_mse=mse(a_lib, spp),
                                  lib_equal_time_spp=spp_eq, lib_equal_time_s=round(t_eq, 4), lib_equal_time_mse=mse(a_eq, spp_eq), ref_spp=ref_spp)), flush=True)
        s.close()


if __name__ == "__main__":
    main(int(sys.argv[1]) if len(sys.argv) > 1 else 4096, int(sys.argv[2]) if len(sys.argv) > 2 else 3)
