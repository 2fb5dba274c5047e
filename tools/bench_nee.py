#!/usr/bin/env python3
"""ptx_render_nee on the MI355X: what the light samples cost and what they buy.

  tools/bench_nee.py [ref_spp] [reps]   Cornell, atrium (detail 5) and plaza (level 3, no alpha) at 1920 x 1080, 8 bounces, device buffers:
                                        ptx_render_nee at 16 and 64 spp — wall time of the synchronised call (the smallest of `reps`, after
                                        a warm-up call), Msamples/s, and the mean squared error of the written bytes (the product's own
                                        image write, bytes / 255) against the product's ref_spp ptx_render frame (4096) of another seed;
                                        next to it ptx_render at equal spp, and ptx_render at the spp that takes the same time.
                                        The same for ptx_render_nee with PTX_NEE_FUSED (fused_*): its calls alternate with the unflagged
                                        ones in the same process, each kept with the spread of its repeats (*_s_max), and with ptx_render at
                                        the spp that takes the flagged call's time; fused_launches tells which route ran (0: the scene is on
                                        the queue route, where the flag is ignored).
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

    def timed(calls, spp):
        """calls: {key: call}, run alternately -> {key: (seconds: the smallest of `reps` synchronised calls after one warm-up, the largest of
        them, the last call's buffer and stats)}"""
        out = {k: [1e30, 0.0, None, None] for k in calls}
        for rep in range(reps + 1):
            for k, call in calls.items():
                acc = zeros()
                t0 = time.perf_counter()
                _, st = call(spp, acc)
                ctx.synchronize()
                dt = time.perf_counter() - t0
                if rep:
                    out[k][0] = min(out[k][0], dt)
                    out[k][1] = max(out[k][1], dt)
                out[k][2:] = [acc, st]
        return out

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

        def fused(spp, acc):
            r = s.render_nee(W, H, spp, BOUNCES, accum=acc, seed=SEED, flags=ptx.NEE_FUSED)
            fused.launches = ctx.timing()["fused_launches"]
            return r

        def lib(spp, acc):
            return s.render(W, H, spp, BOUNCES, accum=acc, seed=SEED)
        for spp in (16, 64):
            t = timed({"nee": nee, "fused": fused, "lib": lib}, spp)
            (t_nee, t_nee_max, a_nee, st), (t_fus, t_fus_max, a_fus, st_fus), (t_lib, _, a_lib, st_lib) = t["nee"], t["fused"], t["lib"]
            same = bool((a_fus == a_nee).all()) and all(st_fus[k] == st[k] for k in ("rays", "light_samples", "light_visible"))
            spp_eq, spp_eq_f = max(1, int(round(spp * t_nee / t_lib))), max(1, int(round(spp * t_fus / t_lib)))
            t_eq, _, a_eq, _ = timed({"lib": lib}, spp_eq)["lib"]
            t_eq_f, _, a_eq_f, _ = timed({"lib": lib}, spp_eq_f)["lib"]
            print(json.dumps(dict(scene=name, W=W, H=H, bounces=BOUNCES, spp=spp, n_lights=st["n_lights"], nee_s=round(t_nee, 4), nee_s_max=round(t_nee_max, 4),
                                  nee_msamples_s=round(W * H * spp / t_nee / 1e6, 1), nee_rays=st["rays"], nee_light_samples=st["light_samples"],
                                  nee_light_visible=st["light_visible"], nee_mse=mse(a_nee, spp),
                                  fused_s=round(t_fus, 4), fused_s_max=round(t_fus_max, 4), fused_msamples_s=round(W * H * spp / t_fus / 1e6, 1),
                                  fused_launches=fused.launches, fused_mse=mse(a_fus, spp), fused_bitwise_nee=same, fused_speedup=round(t_nee / t_fus, 3),
                                  lib_s=round(t_lib, 4),
                                  lib_msamples_s=round(W * H * spp / t_lib / 1e6, 1), lib_rays=st_lib["rays"], lib_mse=mse(a_lib, spp),
                                  lib_equal_time_spp=spp_eq, lib_equal_time_s=round(t_eq, 4), lib_equal_time_mse=mse(a_eq, spp_eq),
                                  lib_equal_fused_time_spp=spp_eq_f, lib_equal_fused_time_s=round(t_eq_f, 4), lib_equal_fused_time_mse=mse(a_eq_f, spp_eq_f),
                                  ref_spp=ref_spp)), flush=True)
        s.close()


if __name__ == "__main__":
    main(int(sys.argv[1]) if len(sys.argv) > 1 else 4096, int(sys.argv[2]) if len(sys.argv) > 2 else 3)
