#!/usr/bin/env python3
"""Cost of the guide-buffer pass (ptx_render_aov) against the beauty frame (ptx_render, 8 bounces) of the same 1080p frame at equal spp,
on Cornell and on the atrium, same process, same order: per call the median kernel_ms (from stats) of 5 runs after a warm-up. The first-hit
emission pass (ptx_render_emission) walks the same samples and is timed next to it; `jack` (jack-of-blades: textures, alpha) is run when named.
   python tools/bench_aov.py [--spp 16] [--only cornell,atrium,jack]"""
import argparse, importlib, json, os, statistics, sys
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import torch

ap = argparse.ArgumentParser(); ap.add_argument("--spp", type=int, default=16); ap.add_argument("--runs", type=int, default=5)
ap.add_argument("--only", default="", help="comma list of: cornell, atrium, jack")
args = ap.parse_args()
ptx = importlib.import_module("distributed-path-tracer_amd")
proc = importlib.import_module("distributed-path-tracer_amd.procedural")
ctx = ptx.Context(0)
W, H, B = 1920, 1080, 8
accum, albedo, normal = (torch.zeros((H, W, 4), dtype=torch.float32, device="cuda:0") for _ in range(3))
only = set(filter(None, args.only.split(",")))


def median_ms(call):
    call()   # warm-up: same size, so that every workspace has its final size
    return statistics.median(call()["kernel_ms"] for _ in range(args.runs))


def run(name, scene):
    beauty = median_ms(lambda: scene.render(W, H, args.spp, B, accum=accum)[1])
    rays = scene.render(W, H, args.spp, B, accum=accum)[1]
    aov = median_ms(lambda: scene.render_aov(W, H, args.spp, albedo=albedo, normal_depth=normal)[2])
    st = scene.render_aov(W, H, args.spp, albedo=albedo, normal_depth=normal)[2]
    em = median_ms(lambda: scene.render_emission(W, H, args.spp, emission=albedo)[1])
    n = W * H * args.spp
    print(json.dumps({"scene": name, "spp": args.spp, "beauty_kernel_ms": round(beauty, 3), "beauty_rays_per_sample": round(rays["rays"] / n, 3),
                      "aov_kernel_ms": round(aov, 3), "aov_rays_per_sample": round(st["rays"] / n, 4), "aov_passes": st["passes"],
                      "aov_msamples_per_s": round(n / aov / 1e3, 1), "aov_over_beauty": round(aov / beauty, 4),
                      "emission_kernel_ms": round(em, 3), "emission_over_aov": round(em / aov, 4)}), flush=True)


if not only or "cornell" in only:
    run("cornell", ptx.Scene.load_gltf(ctx, os.path.join(ROOT, "scenes/cornell-box/cornell.gltf")))
if "jack" in only:
    run("jack-of-blades", ptx.Scene.load_gltf(ctx, os.path.join(ROOT, "scenes/jack-of-blades/jack-of-blades.gltf")))
if not only or "atrium" in only:
    d = proc.atrium_scene()
    run("atrium (24 surfaces, 262 176 triangles)",
        ptx.Scene.from_arrays(ctx, d["model_xform"], d["model_surf"], d["surf_range"], d["vertices"], d["triangles"], d["materials"], d["camera"], d["sun"]))
