"""ptx_render_aov restated from the oracle alone, in float32 numpy (tests/test_aov.py states the rules and pins it; tests/test_denoise.py,
tests/test_material_chart.py take guide buffers from it). Not collected (underscore prefix).

The defaults are test_aov's common shape: 96 x 54, tile (13, 9, 67, 35), samples 3 .. 7, seed 0x5EED.
"""
import numpy as np

W, H, TILE, S0, SPP, SEED = 96, 54, (13, 9, 67, 35), 3, 5, 0x5EED
f32 = np.float32
EPS = f32(0.0001)   # math::epsilon


def _len3(v):
    """sqrt((x*x + y*y) + z*z) in float32, the parenthesisation of oracle/pt_oracle.cpp (dot, then length)."""
    v = np.asarray(v, f32)
    return np.sqrt((v[:, 0] * v[:, 0] + v[:, 1] * v[:, 1]) + v[:, 2] * v[:, 2]).astype(f32)


def restate(ora, o, W_=W, H_=H, tile=TILE, sample0=S0, spp=SPP, seed=SEED):
    """-> (albedo_cov [h,w,4], normal_depth [h,w,4], counts) for samples [sample0, sample0 + spp) of the tile; counts: samples, those that
    passed through at least once, the longest pass-through chain, samples that ended on a miss."""
    x0, y0, w, h = tile
    alb, nd = np.zeros((h * w, 4), f32), np.zeros((h * w, 4), f32)
    yy, xx = np.divmod(np.arange(h * w), w)
    pixel = (yy + y0) * W_ + (xx + x0)
    counts = dict(samples=0, through=0, chain=0, miss=0)
    for s in range(sample0, sample0 + spp):
        rays = o.primary_rays(ora.make_cfg(W_, H_, 1, 1, seed=seed, tile=tile), s).reshape(-1, 6)
        origin = rays[:, :3].copy()
        ra, rn = np.zeros((h * w, 4), f32), np.zeros((h * w, 4), f32)
        live, cur, pas = np.arange(h * w), rays.copy(), np.zeros(h * w, np.int64)
        passed = np.zeros(h * w, np.int64)
        while len(live):
            out, idx = o.intersect(cur)
            hit = idx >= 0
            me = np.zeros((len(live), 12), f32)
            for u in np.unique(idx[hit]):
                sel = idx == u
                me[sel] = o.material_eval(int(u), out[sel, 3:5])
            op = me[:, 6]
            through = np.zeros(len(live), bool)
            for k in np.flatnonzero(hit & ~((op == f32(1)) | (np.abs(op - f32(1)) < EPS))):   # !is_approx(opacity, 1)
                through[k] = ora.draws(int(pixel[live[k]]), s, seed, 0, int(pas[k]), 0)[0] > op[k]
            surf = hit & ~through
            ra[live[surf], :3], ra[live[surf], 3] = me[surf, 3:6], f32(1)
            rn[live[surf], :3], rn[live[surf], 3] = out[surf, 11:14], _len3(out[surf, :3] - origin[live[surf]])
            d = cur[through, 3:6]
            nxt = np.concatenate([out[through, :3] + d * EPS, d * (f32(1) / _len3(d))[:, None]], 1).astype(f32)
            pas = pas[through] + 1
            live = live[through]
            passed[live] = pas
            keep = pas <= 4096
            live, cur, pas = live[keep], nxt[keep], pas[keep]
        covered = ra[:, 3] > 0
        alb[covered] += ra[covered]
        nd[covered] += rn[covered]
        counts["samples"] += h * w
        counts["through"] += int((passed > 0).sum())
        counts["chain"] = max(counts["chain"], int(passed.max()))
        counts["miss"] += int((~covered).sum())
    return alb.reshape(h, w, 4), nd.reshape(h, w, 4), counts
