#!/usr/bin/env python3
"""Kernel time of k_tp_accumulate (ptx_denoise_temporal, and the instantiations of ptx_denoise_temporal_counts) next to the kernel it replaces, k_dn_prepare, and one a-trous iteration.

  tools/bench_temporal.py [W H reps]     Cornell, 8 + 8 spp, device buffers, default 1920 1080 20

The calls are alternated in one process, `reps` rounds after one warm-up round, and the smallest HIP-event time of each is kept:
  accumulate, with history     ptx_denoise_temporal's accumulate_ms with prev given (zero motion: every surface pixel takes four-tap history)
  accumulate, first frame      the same with prev = NULL (no tap is fetched)
  prepare                      ptx_denoise(iterations = 1).kernel_ms - ptx_denoise_temporal(prev = NULL, iterations = 1).filter time: the two
                               differ by k_dn_prepare alone (prefilter and the iteration are the same launches)
  a-trous iteration            ptx_denoise(iterations = 2).kernel_ms - ptx_denoise(iterations = 1).kernel_ms: the iteration at step 2
Bytes per pixel the algorithm needs: accumulate reads the frame's five float4 (80 B) and, with history, each history texel once (40 B: the
four taps of neighbouring pixels overlap), and writes the history (40 B) and the filter's state, guide and re-modulation record (48 B);
prepare reads 64 B and writes 48 B.
  counts, ...                  ptx_denoise_temporal_counts' accumulate_ms on the same buffers (the halves' .w is 8 in every pixel, guide_spp 16): the
                               instantiation with per-pixel counts, without a flag, with each and with both; the same 208 bytes per pixel
  counts search, holes         the same with PTX_TEMPORAL_SEARCH_3X3 on a history whose N is 0 in the 2 x 2 blocks with (x // 2 + y // 2) % 3 == 0: at
                               zero motion those pixels' one tap fails and they search (searched_share, counted as the reprojected pixels the flag
                               adds); the searching pixels fetch 27 texels more, which the 208 bytes do not count
Prints one JSON line.
"""
import importlib
import json
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
ptx = importlib.import_module("distributed-path-tracer_amd")
CORNELL = os.path.join(ROOT, "scenes", "cornell-box", "cornell.gltf")


def main(W, H, reps):
    import torch
    ctx = ptx.Context(0)
    s = ptx.Scene.load_gltf(ctx, CORNELL)

    def mk(c=4):
        t = torch.zeros((H, W, c), device="cuda:0")
        torch.cuda.synchronize()   # the fill runs on torch's stream, the library on its own
        return t
    a, _ = s.render(W, H, 8, 8, accum=mk())
    b, _ = s.render(W, H, 8, 8, accum=mk(), sample0=8)
    A, N, _ = s.render_aov(W, H, 16, albedo=mk(), normal_depth=mk())
    M, _ = s.render_motion(W, H, 16, motion=mk())
    out = mk()
    hists = [(mk(), mk(2), mk()), (mk(), mk(2), mk())]
    ctx.denoise_temporal(a, b, A, N, M, 8, 8, next=hists[0], out=out)
    holed = (hists[0][0].clone(), hists[0][1], hists[0][2])
    yy, xx = torch.meshgrid(torch.arange(H, device="cuda:0"), torch.arange(W, device="cuda:0"), indexing="ij")
    holed[0][..., 3][(xx // 2 + yy // 2) % 3 == 0] = 0
    torch.cuda.synchronize()
    counts_rows = (("counts_history", 0), ("counts_unit", ptx.TEMPORAL_UNIT_NORMALS), ("counts_search", ptx.TEMPORAL_SEARCH_3X3),
                   ("counts_search_unit", ptx.TEMPORAL_SEARCH_3X3 | ptx.TEMPORAL_UNIT_NORMALS))
    shares = {}
    best = {}

    def keep(k, v):
        best[k] = min(best.get(k, 1e9), v)
    for rep in range(reps + 1):   # the first round warms up
        _, _, st = ctx.denoise_temporal(a, b, A, N, M, 8, 8, prev=hists[0], next=hists[1], iterations=1, out=out)
        share = st["reprojected"] / (W * H)
        _, _, s0 = ctx.denoise_temporal(a, b, A, N, M, 8, 8, next=hists[1], iterations=1, out=out)
        for name, flags in counts_rows:
            _, _, sc = ctx.denoise_temporal_counts(a, b, A, N, M, 16, prev=hists[0], next=hists[1], iterations=1, out=out, flags=flags)
            if rep:
                keep(name + "_ms", sc["accumulate_ms"])
        _, _, sc = ctx.denoise_temporal_counts(a, b, A, N, M, 16, next=hists[1], iterations=1, out=out)
        _, _, sh0 = ctx.denoise_temporal_counts(a, b, A, N, M, 16, prev=holed, next=hists[1], iterations=1, out=out)
        _, _, sh1 = ctx.denoise_temporal_counts(a, b, A, N, M, 16, prev=holed, next=hists[1], iterations=1, out=out, flags=ptx.TEMPORAL_SEARCH_3X3)
        shares = dict(holes_reprojected=sh0["reprojected"] / (W * H), holes_search_reprojected=sh1["reprojected"] / (W * H))
        if rep:
            keep("counts_first_ms", sc["accumulate_ms"]), keep("counts_holes_ms", sh0["accumulate_ms"]), keep("counts_search_holes_ms", sh1["accumulate_ms"])
        _, d1 = ctx.denoise(a, b, A, N, 8, 8, iterations=1, out=out)
        _, d2 = ctx.denoise(a, b, A, N, 8, 8, iterations=2, out=out)
        if rep:
            keep("accumulate_history_ms", st["accumulate_ms"]), keep("accumulate_first_ms", s0["accumulate_ms"])
            keep("filter1_after_accumulate_ms", s0["kernel_ms"]), keep("denoise1_ms", d1["kernel_ms"]), keep("denoise2_ms", d2["kernel_ms"])
    n = W * H
    prepare_ms = best["denoise1_ms"] - best["filter1_after_accumulate_ms"]
    gbs = lambda bytes_per_pixel, ms: round(n * bytes_per_pixel / (ms * 1e-3) / 1e9, 1)
    print(json.dumps(dict(W=W, H=H, reps=reps, reprojected_share=round(share, 4),
                          accumulate_history_ms=round(best["accumulate_history_ms"], 4), accumulate_history_bytes_per_pixel=208,
                          accumulate_history_GBs=gbs(208, best["accumulate_history_ms"]),
                          accumulate_first_ms=round(best["accumulate_first_ms"], 4), accumulate_first_bytes_per_pixel=168,
                          accumulate_first_GBs=gbs(168, best["accumulate_first_ms"]),
                          prepare_ms=round(prepare_ms, 4), prepare_bytes_per_pixel=112, prepare_GBs=gbs(112, prepare_ms),
                          atrous_step2_ms=round(best["denoise2_ms"] - best["denoise1_ms"], 4),
                          **{k: round(best[k], 4) for k in sorted(best) if k.startswith("counts_")},
                          **{name + "_GBs": gbs(208, best[name + "_ms"]) for name, _ in counts_rows},
                          counts_first_GBs=gbs(168, best["counts_first_ms"]),
                          searched_share=round(shares["holes_search_reprojected"] - shares["holes_reprojected"], 4),
                          **{k: round(v, 4) for k, v in shares.items()})))


if __name__ == "__main__":
    v = sys.argv[1:]
    main(int(v[0]) if v else 1920, int(v[1]) if len(v) > 1 else 1080, int(v[2]) if len(v) > 2 else 20)
