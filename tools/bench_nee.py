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
  tools/bench_nee.py --env [ref_spp] [reps]
                                        PTX_NEE_ENV_SAMPLES on the open plaza (level 3, no alpha, no analytic sun) at 960 x 540, 8 bounces, under a
                                        512 x 256 sky map with a sun disc of 2.5 degrees radius written to a temporary .hdr: ptx_render_nee with
                                        and without the flag (both with PTX_NEE_FUSED) at 16 and 64 spp — time, mean squared error of the
                                        written bytes against the product's ref_spp ptx_render frame (1024) of another seed: at equal
                                        samples, and the unflagged call at the spp that takes the flagged call's time; and the flagged call
                                        fused against unfused (time, bitwise). Also writes the lines to profiles/nee_env_bench.txt.
  tools/bench_nee.py --sampler-pdf [ref_spp] [reps]
                                        PTX_NEE_SAMPLER_PDF against the same call without it, on Cornell at 1920 x 1080 (triangle list) and on the
                                        --env scene at 960 x 540 (both with PTX_NEE_ENV_SAMPLES), 8 bounces, 16 and 64 spp, in both forms (with and
                                        without PTX_NEE_FUSED): the four calls alternate in one process, each kept at the smallest of `reps`
                                        synchronised calls after a warm-up; the time ratio flagged / unflagged, the mean squared error of the
                                        written bytes of each against the product's ref_spp ptx_render frame of another seed, and the ratio of
                                        each frame's mean linear radiance (R, G, B) to that frame's. Also writes the lines to
                                        profiles/nee_sampler_pdf_bench.txt.
  tools/bench_nee.py --ris [ref_spp] [reps] [spp]
                                        PTX_NEE_CANDIDATES on Cornell and on procedural.emitter_cloud_scene (271 listed triangles) at 1920 x 1080,
                                        8 bounces, 16 spp, with and without PTX_NEE_FUSED: M = 1, 2, 4, 8 alternate in one process, each kept at
                                        the smallest of `reps` synchronised calls after a warm-up. Per row: the time, light rays traced per sample,
                                        the mean squared error of the written bytes against the product's ref_spp ptx_render frame (4096) of
                                        another seed, and the error of M = 1 in the same form at the spp that takes the row's time. Also writes the
                                        lines to profiles/nee_ris_bench.txt.
  tools/bench_nee.py --punctual [ref_spp] [reps] [spp]
                                        Point and spot lights (Scene.set_punctual_lights) on procedural.lamp_scene with an emitter, with 1 lamp and
                                        with 64 (half of them spots), at 1920 x 1080, 8 bounces, 16 spp, with and without PTX_NEE_FUSED: the light
                                        of a punctual sample picked from the light tree (Scene.set_punctual_pick) at M = 1, and from the CDF at
                                        M = 1 and M = 4. The six calls of a scene alternate in one process, each kept at the smallest of `reps`
                                        synchronised calls after a warm-up. Per row: the time, light rays traced per sample, and the mean squared
                                        error of the written bytes against a ref_spp (1024) frame of the SAME call (unfused, CDF, M = 1) of another
                                        seed: ptx_render cannot see the lamps; a tree row also has the error of the CDF call (M = 1, same form) at
                                        the spp that takes the tree call's time. The lines are the first part of
                                        profiles/nee_punctual_tree_bench.txt (profiles/nee_punctual_bench.txt: the CDF rows before the tree existed).
  tools/bench_nee.py --light-tree [ref_spp] [reps] [spp] [W H]
                                        The emissive triangle of a light sample picked from the light tree over the light list
                                        (Scene.set_light_pick("tree")) against the CDF over area, on procedural.emitter_field_scene with 16 and
                                        with 256 emitters and on procedural.emitter_cloud_scene (271 listed triangles), at 1920 x 1080 (or W H),
                                        8 bounces, 16 spp, with and without PTX_NEE_FUSED, at M = 1 and M = 4. The eight calls of a scene alternate
                                        in one process, each kept at the smallest of `reps` synchronised calls after a warm-up. Per row: the time,
                                        light rays traced per sample, and the mean squared error of the written bytes against a ref_spp (1024)
                                        frame of the SAME call (unfused, CDF, M = 1) of another seed; a tree row also has the error of the CDF call
                                        (same form, same M) at the spp that takes the tree call's time. Also writes the lines to
                                        profiles/nee_light_tree_bench.txt.
  tools/bench_nee.py --motion [reps] [spp]
                                        Motion blur (Scene.set_motion): the unfused ptx_render_nee with the motion active against the same call
                                        without motion, on Cornell with one box moving and on procedural.movers_scene (its camera moving too),
                                        at 1920 x 1080, 8 bounces, 16 spp, shutter (0, 1): the two calls alternate in one process, `reps` (5)
                                        synchronised calls each after a warm-up, kept with their smallest and largest; the time ratio, and the
                                        rays traced. Also the unflagged static call alone, as the control that is compared between commits.
                                        Alternated with them on the same scene: the call with PTX_NEE_FUSED | PTX_NEE_FUSED_MOTION under the
                                        motion (fused_motion_*: the fused kernel with a time per lane, one launch per pass) and the
                                        PTX_NEE_FUSED call without motion (fused_static_*); the fused motion frame is checked bitwise
                                        against the unfused one. Also writes the lines to profiles/nee_fused_motion_bench.txt
                                        (profiles/motion_blur_bench.txt holds the two unfused columns as measured before the kernel existed).
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


def sun_disc_map(path, w=512, h=256, radius_deg=2.5, elevation_deg=40.0, azimuth_deg=60.0, sky=(0.25, 0.35, 0.55), sun=(6000.0, 5400.0, 4200.0)):
    """an uncompressed Radiance .hdr: a dim sky and a sun disc, texel centres through the inverse of the miss lookup"""
    import struct
    v = 1 - (np.arange(h) + 0.5) / h
    u = (np.arange(w) + 0.5) / w
    lat, phi = (v - 0.5) / 0.3183, (u - 0.5) / 0.1591
    d = np.stack([np.cos(lat)[:, None] * np.cos(phi)[None], np.repeat(np.sin(lat)[:, None], w, 1), np.cos(lat)[:, None] * np.sin(phi)[None]], -1)
    el, az = np.radians(elevation_deg), np.radians(azimuth_deg)
    c = np.array([np.cos(el) * np.cos(az), np.sin(el), np.cos(el) * np.sin(az)])
    rgb = np.where((d @ c >= np.cos(np.radians(radius_deg)))[..., None], np.array(sun), np.array(sky))
    mant, ex = np.frexp(rgb.max(-1))
    sc = mant * 256.0 / rgb.max(-1)
    px = np.concatenate([(rgb * sc[..., None]).astype(np.uint8), (ex + 128).astype(np.uint8)[..., None]], -1)
    with open(path, "wb") as f:
        f.write(b"#?RADIANCE\nFORMAT=32-bit_rle_rgbe\n\n" + f"-Y {h} +X {w}\n".encode() + px.tobytes())
    return path


def main_env(ref_spp, reps):
    import tempfile
    global W, H
    W, H = 960, 540
    ctx = ptx.Context(0)
    s = ptx.Scene.from_arrays(ctx, *[proc.plaza_scene(alpha=False, sun=False)[k] for k in KEYS])
    with tempfile.TemporaryDirectory() as tmp:
        s.set_environment(sun_disc_map(os.path.join(tmp, "sun_disc.hdr")), srgb=False)
    lines = []

    def image(acc, spp):
        return ctx.tonemap_encode(acc, W, H, spp)[..., :3].astype(np.float64) / 255

    def timed(call, spp):
        best, acc, st = 1e30, None, None
        for rep in range(reps + 1):
            acc = zeros()
            t0 = time.perf_counter()
            _, st = call(spp, acc)
            ctx.synchronize()
            if rep:
                best = min(best, time.perf_counter() - t0)
        return best, acc, st
    ref_acc = zeros()
    s.render(W, H, ref_spp, BOUNCES, accum=ref_acc, seed=REF_SEED, want_stats=False)
    ctx.synchronize()
    ref = image(ref_acc, ref_spp)
    del ref_acc

    def mse(acc, spp):
        return float(np.mean((image(acc, spp) - ref) ** 2))

    def call(flags):
        return lambda spp, acc: s.render_nee(W, H, spp, BOUNCES, accum=acc, seed=SEED, flags=flags)
    for spp in (16, 64):
        t_env, a_env, st_env = timed(call(ptx.NEE_ENV_SAMPLES | ptx.NEE_FUSED), spp)
        launches = ctx.timing()["fused_launches"]
        t_un, a_un, st_un = timed(call(ptx.NEE_FUSED), spp)
        t_envu, a_envu, st_envu = timed(call(ptx.NEE_ENV_SAMPLES), spp)
        spp_eq = max(1, int(round(spp * t_env / t_un)))
        t_eq, a_eq, _ = timed(call(ptx.NEE_FUSED), spp_eq)
        same = bool((a_env == a_envu).all()) and all(st_env[k] == st_envu[k] for k in ("rays", "light_samples", "light_visible"))
        lines.append(json.dumps(dict(scene="plaza3_opaque_nosun", map="sun disc 512x256", W=W, H=H, bounces=BOUNCES, spp=spp, n_lights=st_env["n_lights"],
                                     env_s=round(t_env, 4), env_msamples_s=round(W * H * spp / t_env / 1e6, 1), env_rays=st_env["rays"],
                                     env_light_samples=st_env["light_samples"], env_light_visible=st_env["light_visible"], env_mse=mse(a_env, spp),
                                     unflagged_s=round(t_un, 4), unflagged_rays=st_un["rays"], unflagged_mse=mse(a_un, spp),
                                     unflagged_equal_time_spp=spp_eq, unflagged_equal_time_s=round(t_eq, 4), unflagged_equal_time_mse=mse(a_eq, spp_eq),
                                     env_unfused_s=round(t_envu, 4), env_fused_launches=launches, env_fused_bitwise_unfused=same,
                                     env_fused_speedup=round(t_envu / t_env, 3), ref_spp=ref_spp)))
        print(lines[-1], flush=True)
    s.close()
    with open(os.path.join(ROOT, "profiles", "nee_env_bench.txt"), "w") as f:
        f.write("tools/bench_nee.py --env: PTX_NEE_ENV_SAMPLES against the unflagged ptx_render_nee (both PTX_NEE_FUSED), MI355X\n" + "\n".join(lines) + "\n")


def main_sampler_pdf(ref_spp, reps):
    import tempfile
    global W, H
    ctx = ptx.Context(0)
    lines = []
    with tempfile.TemporaryDirectory() as tmp:
        sun_map = sun_disc_map(os.path.join(tmp, "sun_disc.hdr"))
        cases = [("cornell", 1920, 1080, 0, lambda: ptx.Scene.load_gltf(ctx, CORNELL), None),
                 ("plaza3_opaque_nosun", 960, 540, ptx.NEE_ENV_SAMPLES, lambda: ptx.Scene.from_arrays(ctx, *[proc.plaza_scene(alpha=False, sun=False)[k] for k in KEYS]), sun_map)]
        for name, W, H, base, make, env_map in cases:
            s = make()
            if env_map:
                s.set_environment(env_map, srgb=False)
            ref_acc = zeros()
            s.render(W, H, ref_spp, BOUNCES, accum=ref_acc, seed=REF_SEED, want_stats=False)
            ctx.synchronize()
            ref = ctx.tonemap_encode(ref_acc, W, H, ref_spp)[..., :3].astype(np.float64) / 255
            ref_mean = ref_acc.cpu().numpy()[..., :3].astype(np.float64).reshape(-1, 3).mean(0) / ref_spp
            del ref_acc
            forms = {"unfused": base, "unfused_spdf": base | ptx.NEE_SAMPLER_PDF, "fused": base | ptx.NEE_FUSED, "fused_spdf": base | ptx.NEE_FUSED | ptx.NEE_SAMPLER_PDF}
            for spp in (16, 64):
                best = {k: 1e30 for k in forms}
                acc, st, launches = {}, {}, {}
                for rep in range(reps + 1):
                    for k, flags in forms.items():   # the four calls alternate
                        a = zeros()
                        t0 = time.perf_counter()
                        _, st[k] = s.render_nee(W, H, spp, BOUNCES, accum=a, seed=SEED, flags=flags)
                        ctx.synchronize()
                        dt = time.perf_counter() - t0
                        if rep:
                            best[k] = min(best[k], dt)
                        acc[k], launches[k] = a, ctx.timing()["fused_launches"]
                out = dict(scene=name, W=W, H=H, bounces=BOUNCES, spp=spp, n_lights=st["fused"]["n_lights"], base_flags=base, ref_spp=ref_spp,
                           fused_launches=launches["fused_spdf"], spdf_fused_bitwise_unfused=bool((acc["fused_spdf"] == acc["unfused_spdf"]).all()))
                for k in forms:
                    img = ctx.tonemap_encode(acc[k], W, H, spp)[..., :3].astype(np.float64) / 255
                    mean = acc[k].cpu().numpy()[..., :3].astype(np.float64).reshape(-1, 3).mean(0) / spp
                    out[k + "_s"] = round(best[k], 4)
                    out[k + "_mse"] = float(np.mean((img - ref) ** 2))
                    out[k + "_mean_ratio_rgb"] = [round(float(x), 5) for x in mean / ref_mean]
                    out[k + "_light_samples"] = st[k]["light_samples"]
                out["fused_time_ratio_spdf"] = round(best["fused_spdf"] / best["fused"], 4)
                out["unfused_time_ratio_spdf"] = round(best["unfused_spdf"] / best["unfused"], 4)
                lines.append(json.dumps(out))
                print(lines[-1], flush=True)
            s.close()
    with open(os.path.join(ROOT, "profiles", "nee_sampler_pdf_bench.txt"), "w") as f:
        f.write("tools/bench_nee.py --sampler-pdf: PTX_NEE_SAMPLER_PDF against the same ptx_render_nee call without it, fused and unfused, MI355X\n" + "\n".join(lines) + "\n")


def main_ris(ref_spp, reps, spp):
    ctx = ptx.Context(0)
    lines = []
    cases = [("cornell", lambda: ptx.Scene.load_gltf(ctx, CORNELL)),
             ("emitter_cloud", lambda: ptx.Scene.from_arrays(ctx, *[proc.emitter_cloud_scene()[k] for k in KEYS]))]
    for name, make in cases:
        s = make()
        ref_acc = zeros()
        s.render(W, H, ref_spp, BOUNCES, accum=ref_acc, seed=REF_SEED, want_stats=False)
        ctx.synchronize()
        ref = ctx.tonemap_encode(ref_acc, W, H, ref_spp)[..., :3].astype(np.float64) / 255
        del ref_acc

        def mse(acc, n):
            return float(np.mean((ctx.tonemap_encode(acc, W, H, n)[..., :3].astype(np.float64) / 255 - ref) ** 2))

        def timed(forms, n):
            """forms: {key: flags}, run alternately -> {key: (the smallest of `reps` synchronised calls after a warm-up, buffer, stats, launches)}"""
            best = {k: 1e30 for k in forms}
            acc, st, launches = {}, {}, {}
            for rep in range(reps + 1):
                for k, flags in forms.items():
                    a = zeros()
                    t0 = time.perf_counter()
                    _, st[k] = s.render_nee(W, H, n, BOUNCES, accum=a, seed=SEED, flags=flags)
                    ctx.synchronize()
                    dt = time.perf_counter() - t0
                    if rep:
                        best[k] = min(best[k], dt)
                    acc[k], launches[k] = a, ctx.timing()["fused_launches"]
            return {k: (best[k], acc[k], st[k], launches[k]) for k in forms}
        for form, base in (("fused", ptx.NEE_FUSED), ("unfused", 0)):
            t = timed({m: base | ptx.NEE_CANDIDATES(m) for m in (1, 2, 4, 8)}, spp)
            t1 = t[1][0]
            for m, (sec, acc, st, launches) in t.items():
                spp_eq = max(1, int(round(spp * sec / t1)))
                eq_s, eq_acc, _, _ = timed({1: base}, spp_eq)[1] if m > 1 else (sec, acc, None, None)
                lines.append(json.dumps(dict(scene=name, form=form, M=m, W=W, H=H, bounces=BOUNCES, spp=spp, n_lights=st["n_lights"], fused_launches=launches,
                                             s=round(sec, 4), time_ratio_to_m1=round(sec / t1, 4), rays=st["rays"], light_samples_per_sample=round(st["light_samples"] / st["samples"], 4),
                                             light_visible_per_sample=round(st["light_visible"] / st["samples"], 4), mse=mse(acc, spp),
                                             m1_equal_time_spp=spp_eq, m1_equal_time_s=round(eq_s, 4), m1_equal_time_mse=mse(eq_acc, spp_eq), ref_spp=ref_spp)))
                print(lines[-1], flush=True)
        s.close()
    with open(os.path.join(ROOT, "profiles", "nee_ris_bench.txt"), "w") as f:
        f.write("tools/bench_nee.py --ris: PTX_NEE_CANDIDATES(M) against M = 1, fused and unfused, MI355X\n" + "\n".join(lines) + "\n")


def main_punctual(ref_spp, reps, spp):
    ctx = ptx.Context(0)
    for n_lamps in (1, 64):
        d, lamps = proc.lamp_scene(n_lamps, emitters=True, spots=True)
        s = ptx.Scene.from_arrays(ctx, *[d[k] for k in KEYS])
        s.set_punctual_lights(lamps)
        ref_acc = zeros()
        s.render_nee(W, H, ref_spp, BOUNCES, accum=ref_acc, seed=REF_SEED, want_stats=False)
        ctx.synchronize()
        ref = ctx.tonemap_encode(ref_acc, W, H, ref_spp)[..., :3].astype(np.float64) / 255
        del ref_acc
        # the same scene with the light of a punctual sample picked from the light tree (Scene.set_punctual_pick): a scene of its own, so that
        # no call of the alternation uploads anything
        tree = ptx.Scene.from_arrays(ctx, *[d[k] for k in KEYS])
        tree.set_punctual_lights(lamps)
        tree.set_punctual_pick(ptx.PUNCTUAL_PICK_TREE)
        scene_of = {"cdf": s, "tree": tree}
        forms = {(form, pick, m): base | ptx.NEE_CANDIDATES(m) for form, base in (("fused", ptx.NEE_FUSED), ("unfused", 0))
                 for pick, m in (("tree", 1), ("cdf", 1), ("cdf", 4))}

        def mse_of(a, n):
            return float(np.mean((ctx.tonemap_encode(a, W, H, n)[..., :3].astype(np.float64) / 255 - ref) ** 2))

        def timed(forms, n):
            best, acc, st, launches = {k: 1e30 for k in forms}, {}, {}, {}
            for r in range(reps + 1):
                for k, flags in forms.items():
                    a = zeros()
                    t0 = time.perf_counter()
                    _, st[k] = scene_of[k[1]].render_nee(W, H, n, BOUNCES, accum=a, seed=SEED, flags=flags)
                    ctx.synchronize()
                    dt = time.perf_counter() - t0
                    if r:
                        best[k] = min(best[k], dt)
                    acc[k], launches[k] = a, ctx.timing()["fused_launches"]
            return best, acc, st, launches
        best, acc, st, launches = timed(forms, spp)
        for k, sec in best.items():
            form, pick, m = k
            row = dict(scene="lamp_scene", lamps=n_lamps, form=form, pick=pick, M=m, W=W, H=H, bounces=BOUNCES, spp=spp, n_lights=st[k]["n_lights"],
                       fused_launches=launches[k], s=round(sec, 4), msamples_s=round(W * H * spp / sec / 1e6, 1), rays=st[k]["rays"],
                       light_samples_per_sample=round(st[k]["light_samples"] / st[k]["samples"], 4),
                       light_visible_per_sample=round(st[k]["light_visible"] / st[k]["samples"], 4), mse=mse_of(acc[k], spp), ref_spp=ref_spp)
            if pick == "tree":   # what the CDF call (M = 1, same form) reaches in the tree call's time
                spp_eq = max(1, int(round(spp * sec / best[(form, "cdf", 1)])))
                eq_key = (form, "cdf", 1)
                eq_best, eq_acc, _, _ = timed({eq_key: forms[eq_key]}, spp_eq)
                row.update(cdf_equal_time_spp=spp_eq, cdf_equal_time_s=round(eq_best[eq_key], 4), cdf_equal_time_mse=mse_of(eq_acc[eq_key], spp_eq))
            print(json.dumps(row), flush=True)
        s.close()
        tree.close()


def main_light_tree(ref_spp, reps, spp, w, h):
    import torch
    ctx = ptx.Context(0)
    lines = []

    def buf():
        t = torch.zeros((h, w, 4), device="cuda:0")
        torch.cuda.synchronize()   # the fill runs on torch's stream, the library on its own
        return t
    for name, d in (("emitter_field_16", proc.emitter_field_scene(16)), ("emitter_field_256", proc.emitter_field_scene(256)),
                    ("emitter_cloud", proc.emitter_cloud_scene())):
        # one scene per mode, so that no call of the alternation builds or uploads anything
        scene_of = {"cdf": ptx.Scene.from_arrays(ctx, *[d[k] for k in KEYS]), "tree": ptx.Scene.from_arrays(ctx, *[d[k] for k in KEYS])}
        scene_of["tree"].set_light_pick("tree")
        ref_acc = buf()
        scene_of["cdf"].render_nee(w, h, ref_spp, BOUNCES, accum=ref_acc, seed=REF_SEED, want_stats=False)
        ctx.synchronize()
        ref = ctx.tonemap_encode(ref_acc, w, h, ref_spp)[..., :3].astype(np.float64) / 255
        del ref_acc
        forms = {(form, pick, m): base | ptx.NEE_CANDIDATES(m) for form, base in (("fused", ptx.NEE_FUSED), ("unfused", 0))
                 for pick in ("tree", "cdf") for m in (1, 4)}

        def mse_of(a, n):
            return float(np.mean((ctx.tonemap_encode(a, w, h, n)[..., :3].astype(np.float64) / 255 - ref) ** 2))

        def timed(forms, n):
            best, acc, st, launches = {k: 1e30 for k in forms}, {}, {}, {}
            for r in range(reps + 1):
                for k, flags in forms.items():
                    a = buf()
                    t0 = time.perf_counter()
                    _, st[k] = scene_of[k[1]].render_nee(w, h, n, BOUNCES, accum=a, seed=SEED, flags=flags)
                    ctx.synchronize()
                    dt = time.perf_counter() - t0
                    if r:
                        best[k] = min(best[k], dt)
                    acc[k], launches[k] = a, ctx.timing()["fused_launches"]
            return best, acc, st, launches
        best, acc, st, launches = timed(forms, spp)
        for k, sec in best.items():
            form, pick, m = k
            row = dict(scene=name, form=form, pick=pick, M=m, W=w, H=h, bounces=BOUNCES, spp=spp, n_lights=st[k]["n_lights"], fused_launches=launches[k],
                       s=round(sec, 4), msamples_s=round(w * h * spp / sec / 1e6, 1), rays=st[k]["rays"],
                       light_samples_per_sample=round(st[k]["light_samples"] / st[k]["samples"], 4),
                       light_visible_per_sample=round(st[k]["light_visible"] / st[k]["samples"], 4), mse=mse_of(acc[k], spp), ref_spp=ref_spp)
            if pick == "tree":   # what the CDF call (same form, same M) reaches in the tree call's time
                eq_key = (form, "cdf", m)
                spp_eq = max(1, int(round(spp * sec / best[eq_key])))
                eq_best, eq_acc, _, _ = timed({eq_key: forms[eq_key]}, spp_eq)
                row.update(time_ratio_to_cdf=round(sec / best[eq_key], 4), cdf_equal_time_spp=spp_eq, cdf_equal_time_s=round(eq_best[eq_key], 4),
                           cdf_equal_time_mse=mse_of(eq_acc[eq_key], spp_eq))
            lines.append(json.dumps(row))
            print(lines[-1], flush=True)
        for sc in scene_of.values():
            sc.close()
    with open(os.path.join(ROOT, "profiles", "nee_light_tree_bench.txt"), "w") as f:
        f.write("tools/bench_nee.py --light-tree: the light tree over the light list against the CDF over area, fused and unfused, MI355X\n" + "\n".join(lines) + "\n")


def main_motion(reps, spp):
    ctx = ptx.Context(0)
    lines = []
    movers = proc.movers_scene()

    def cornell():
        s = ptx.Scene.load_gltf(ctx, CORNELL)
        begin = s.array(ptx.ARR_MODEL_XFORM).copy()
        k = 1                                  # Cube.001, one of the two boxes (single surface, not the light)
        assert s.array(ptx.ARR_MODEL_SURF)[k, 1] == 1 and not s.array(ptx.ARR_MATERIALS)[s.array(ptx.ARR_MODEL_SURF)[k, 0], 6:9].any()
        begin[k, 0] += 0.3
        begin[k, 2] -= 0.2
        return s, begin, None

    def moving():
        s = ptx.Scene.from_arrays(ctx, *[movers[k] for k in KEYS])
        return s, movers["begin_model_xform"], (movers["begin_camera"][:3], movers["begin_camera"][3:12], movers["begin_camera"][12])
    for name, make in (("cornell_one_box", cornell), ("movers", moving)):
        s, begin, cam = make()
        FM = ptx.NEE_FUSED | ptx.NEE_FUSED_MOTION
        calls = {"static": (False, 0), "motion": (True, 0), "fused_static": (False, ptx.NEE_FUSED), "fused_motion": (True, FM)}
        times = {k: [] for k in calls}
        st, launches, frames = {}, {}, {}
        for rep in range(reps + 1):
            for k, (moving_now, flags) in calls.items():     # the four calls alternate; the motion is set and cleared outside the timed region
                if moving_now:
                    s.set_motion(begin, cam, (0.0, 1.0))
                a = zeros()
                t0 = time.perf_counter()
                _, st[k] = s.render_nee(W, H, spp, BOUNCES, accum=a, seed=SEED, flags=flags)
                ctx.synchronize()
                dt = time.perf_counter() - t0
                launches[k] = ctx.timing()["fused_launches"]
                if moving_now:
                    s.clear_motion()
                if rep:
                    times[k].append(dt)
                else:
                    frames[k] = a.cpu().numpy() if hasattr(a, "cpu") else np.array(a)
        bitwise = bool((frames["fused_motion"].view(np.uint32) == frames["motion"].view(np.uint32)).all())
        lines.append(json.dumps(dict(scene=name, W=W, H=H, bounces=BOUNCES, spp=spp, reps=reps, pipeline=ctx.timing()["pipeline"],
                                     static_s_min=round(min(times["static"]), 4), static_s_max=round(max(times["static"]), 4),
                                     motion_s_min=round(min(times["motion"]), 4), motion_s_max=round(max(times["motion"]), 4),
                                     motion_over_static=round(min(times["motion"]) / min(times["static"]), 4),
                                     static_msamples_s=round(W * H * spp / min(times["static"]) / 1e6, 1), motion_msamples_s=round(W * H * spp / min(times["motion"]) / 1e6, 1),
                                     static_rays=st["static"]["rays"], motion_rays=st["motion"]["rays"], static_n_lights=st["static"]["n_lights"],
                                     motion_n_lights=st["motion"]["n_lights"],
                                     fused_motion_s_min=round(min(times["fused_motion"]), 4), fused_motion_s_max=round(max(times["fused_motion"]), 4),
                                     fused_static_s_min=round(min(times["fused_static"]), 4), fused_static_s_max=round(max(times["fused_static"]), 4),
                                     fused_motion_launches=launches["fused_motion"], fused_static_launches=launches["fused_static"], motion_launches=launches["motion"],
                                     unfused_motion_over_fused_motion=round(min(times["motion"]) / min(times["fused_motion"]), 4),
                                     fused_motion_over_fused_static=round(min(times["fused_motion"]) / min(times["fused_static"]), 4),
                                     fused_motion_msamples_s=round(W * H * spp / min(times["fused_motion"]) / 1e6, 1), fused_motion_rays=st["fused_motion"]["rays"],
                                     fused_motion_frame_is_unfused_motion_frame=bitwise)))
        print(lines[-1], flush=True)
        s.close()
    with open(os.path.join(ROOT, "profiles", "nee_fused_motion_bench.txt"), "w") as f:
        f.write("tools/bench_nee.py --motion: ptx_render_nee under active motion, unfused and with PTX_NEE_FUSED | PTX_NEE_FUSED_MOTION, against the same calls "
                "without motion (unflagged and PTX_NEE_FUSED), the four alternated, MI355X\n" + "\n".join(lines) + "\n")


if __name__ == "__main__":
    if len(sys.argv) > 1 and sys.argv[1] == "--motion":
        main_motion(int(sys.argv[2]) if len(sys.argv) > 2 else 5, int(sys.argv[3]) if len(sys.argv) > 3 else 16)
        sys.exit(0)
    if len(sys.argv) > 1 and sys.argv[1] == "--light-tree":
        av = [int(x) for x in sys.argv[2:]]
        main_light_tree(av[0] if len(av) > 0 else 1024, av[1] if len(av) > 1 else 3, av[2] if len(av) > 2 else 16, av[3] if len(av) > 4 else W, av[4] if len(av) > 4 else H)
        sys.exit(0)
    if len(sys.argv) > 1 and sys.argv[1] == "--punctual":
        main_punctual(int(sys.argv[2]) if len(sys.argv) > 2 else 1024, int(sys.argv[3]) if len(sys.argv) > 3 else 3, int(sys.argv[4]) if len(sys.argv) > 4 else 16)
        sys.exit(0)
    if len(sys.argv) > 1 and sys.argv[1] == "--ris":
        main_ris(int(sys.argv[2]) if len(sys.argv) > 2 else 4096, int(sys.argv[3]) if len(sys.argv) > 3 else 3, int(sys.argv[4]) if len(sys.argv) > 4 else 16)
        sys.exit(0)
    if len(sys.argv) > 1 and sys.argv[1] == "--sampler-pdf":
        main_sampler_pdf(int(sys.argv[2]) if len(sys.argv) > 2 else 1024, int(sys.argv[3]) if len(sys.argv) > 3 else 3)
        sys.exit(0)
    if len(sys.argv) > 1 and sys.argv[1] == "--env":
        main_env(int(sys.argv[2]) if len(sys.argv) > 2 else 1024, int(sys.argv[3]) if len(sys.argv) > 3 else 3)
        sys.exit(0)
    main(int(sys.argv[1]) if len(sys.argv) > 1 else 4096, int(sys.argv[2]) if len(sys.argv) > 2 else 3)
