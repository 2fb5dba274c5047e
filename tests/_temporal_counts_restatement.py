"""ptx_denoise_temporal_counts restated in float32 numpy from its specification in include/ptx.h (tests/test_temporal_counts.py states the
rules, tests/test_temporal_counts_gpu.py pins the product to it bit for bit). Step 1 is ptx_denoise_counts', the four taps are
ptx_denoise_temporal's, the blend weighs the frame by its samples; the filter's steps 2 to 5, the synthetic frames and the clamped gather
are tests/_temporal_restatement.py's. Not collected (underscore prefix).
"""
import numpy as np

from _denoise_restatement import _lum, f32
from _temporal_restatement import _gather, filter_tail, motion_sums, synthetic  # noqa: F401  (re-exported for the tests)

i32 = np.int32
SEARCH_3X3, UNIT_NORMALS = 1, 2   # PTX_TEMPORAL_SEARCH_3X3, PTX_TEMPORAL_UNIT_NORMALS


def _unit(v):
    """v.xyz / sqrt((v.x*v.x + v.y*v.y) + v.z*v.z): three divisions by the exact square root; a zero vector gives NaN."""
    l = np.sqrt((v[..., 0] * v[..., 0] + v[..., 1] * v[..., 1]) + v[..., 2] * v[..., 2])
    return v[..., :3] / l[..., None]


def accumulate(a, b, albedo_cov, normal_depth, motion, guide_spp, prev=None, max_history=0, tau_z=0.1, tau_n=0.9, flags=0):
    """Steps 1 to 5 of ptx_denoise_temporal_counts' own part -> dict(col, var, g, alb, alpha: the filter's inputs; next: (color, moments,
    geometry); took: the pixels that took history; searched: those of them that took it through the 3 x 3 search; sw: the sum of the taken
    taps' weights). max_history = 0: the call's default, min(32 * guide_spp, 1048576)."""
    a, b, A, N, M = (np.asarray(x, f32) for x in (a, b, albedo_cov, normal_depth, motion))
    H, W = a.shape[:2]
    ng = f32(guide_spp)
    maxh, tz, tn = f32(max_history if max_history else min(32 * guide_spp, 1048576)), f32(tau_z), f32(tau_n)
    with np.errstate(all="ignore"):
        # 1. the current frame, as ptx_denoise_counts
        na, nb = a[..., 3], b[..., 3]
        n = na + nb
        cov = A[..., 3]
        alb = np.fmax((A[..., :3] + (ng - cov)[..., None]) / ng, f32(0.001))
        col = ((a[..., :3] + b[..., :3]) / n[..., None]) / alb
        d = (_lum((a[..., :3] / na[..., None]) / alb) - _lum((b[..., :3] / nb[..., None]) / alb)) * f32(0.5)
        v0 = d * d
        alpha = (a[..., 3] + b[..., 3]) / n
        hit = cov > 0
        g = np.where(hit[..., None], N / np.where(hit, cov, f32(1))[..., None], f32(0)).astype(f32)
        L = _lum(col)
        LL = L * L
        # 2. reprojection
        took = np.zeros((H, W), bool)
        searched = np.zeros((H, W), bool)
        hist = None
        sw = np.zeros((H, W), f32)
        if prev is not None:
            pc, pm, pg = (np.asarray(x, f32) for x in prev)
            up = _unit(g) if flags & UNIT_NORMALS else g[..., :3]

            def passes(cq, gq):
                """N_q > 0, z_q > 0, the depth test and the normal test of a tap"""
                uq = _unit(gq) if flags & UNIT_NORMALS else gq[..., :3]
                dot = (up[..., 0] * uq[..., 0] + up[..., 1] * uq[..., 1]) + up[..., 2] * uq[..., 2]
                return (cq[..., 3] > 0) & (gq[..., 3] > 0) & (np.abs(zexp - gq[..., 3]) <= tz * np.fmax(zexp, gq[..., 3])) & (dot >= tn)
            yy, xx = np.mgrid[0:H, 0:W]
            have = M[..., 3] > 0
            mvx, mvy, zexp = M[..., 0] / M[..., 3], M[..., 1] / M[..., 3], M[..., 2] / M[..., 3]
            gx = ((xx.astype(f32) + f32(0.5)) + mvx) - f32(0.5)
            gy = ((yy.astype(f32) + f32(0.5)) + mvy) - f32(0.5)
            have = have & (np.abs(gx) < f32(32768)) & (np.abs(gy) < f32(32768))
            flx, fly = np.floor(gx), np.floor(gy)
            wx, wy = gx - flx, gy - fly
            ix = np.where(have, flx, f32(0)).astype(i32)
            iy = np.where(have, fly, f32(0)).astype(i32)
            acc = np.zeros((H, W, 6), f32)   # colour r g b, N, mu1, mu2
            for dy in (0, 1):
                for dx in (0, 1):
                    qx, qy = ix + dx, iy + dy
                    bq = (wx if dx else f32(1) - wx) * (wy if dy else f32(1) - wy)
                    cq, mq, gq = _gather(pc, qx, qy), _gather(pm, qx, qy), _gather(pg, qx, qy)
                    take = have & (qx >= 0) & (qx < W) & (qy >= 0) & (qy < H) & (bq > 0) & passes(cq, gq)
                    hq = np.concatenate([cq, mq], -1)
                    sw = np.where(take, sw + bq, sw)
                    acc = np.where(take[..., None], acc + bq[..., None] * hq, acc)
            if flags & SEARCH_3X3:
                search = have & (sw == 0)
                rx = np.where(search, np.floor(gx + f32(0.5)), f32(0)).astype(i32)
                ry = np.where(search, np.floor(gy + f32(0.5)), f32(0)).astype(i32)
                for dy in (-1, 0, 1):
                    for dx in (-1, 0, 1):
                        qx, qy = rx + dx, ry + dy
                        cq, mq, gq = _gather(pc, qx, qy), _gather(pm, qx, qy), _gather(pg, qx, qy)
                        take = search & (qx >= 0) & (qx < W) & (qy >= 0) & (qy < H) & passes(cq, gq)
                        hq = np.concatenate([cq, mq], -1)
                        sw = np.where(take, sw + f32(1), sw)
                        acc = np.where(take[..., None], acc + hq, acc)
                searched = search & (sw > 0)
            have = have & (sw > 0)
            h = acc / sw[..., None]
            # 3. blend: the frame weighs n of N' samples
            Nh = np.fmin(h[..., 3] + n, np.fmax(maxh, n))
            al = n / Nh
            bc = h[..., :3] + (col - h[..., :3]) * al[..., None]
            b1 = h[..., 4] + (L - h[..., 4]) * al
            b2 = h[..., 5] + (LL - h[..., 5]) * al
            took = have & np.isfinite(((bc[..., 0] + bc[..., 1]) + bc[..., 2]) + (b1 + b2))
            searched &= took
            hist = (bc, b1, b2, Nh)
        if hist is None:
            colp, m1, m2, Np = col, L, LL, n
        else:
            colp = np.where(took[..., None], hist[0], col)
            m1, m2 = np.where(took, hist[1], L), np.where(took, hist[2], LL)
            Np = np.where(took, hist[3], n)
        # 4. the variance the filter starts from
        vf = np.where(Np < f32(4) * n, v0, np.fmax(f32(0), m2 - m1 * m1))
        var = vf * (n / Np)
    nxt = (np.concatenate([colp, Np[..., None]], -1).astype(f32), np.stack([m1, m2], -1).astype(f32), g)
    for x in (colp, var, nxt[0], nxt[1]):
        assert x.dtype == f32, x.dtype
    return dict(col=colp, var=var, g=g, alb=alb, alpha=alpha, next=nxt, took=took, searched=searched, sw=sw)


def restate(a, b, albedo_cov, normal_depth, motion, guide_spp, prev=None, iterations=5, sigma_l=4.0, sigma_n=0.5, sigma_z=0.1, max_history=0,
            tau_z=0.1, tau_n=0.9, flags=0):
    """The specification of ptx_denoise_temporal_counts -> (out [H,W,4], next (color, moments, geometry), took [H,W] bool)."""
    s = accumulate(a, b, albedo_cov, normal_depth, motion, guide_spp, prev, max_history, tau_z, tau_n, flags)
    out = filter_tail(s["col"], s["var"], s["g"], s["alb"], s["alpha"], iterations, sigma_l, sigma_n, sigma_z)
    return out, s["next"], s["took"]
