"""ptx_denoise_temporal restated in float32 numpy from its specification in include/ptx.h (tests/test_temporal.py states the rules,
tests/test_temporal_gpu.py pins the product to it bit for bit). Step 1 and the filter's steps 2 to 5 are written as
tests/_denoise_restatement.py writes them, with its helpers; with prev = None the output is bitwise that module's. Not collected
(underscore prefix).
"""
import numpy as np

from _denoise_restatement import KERN, _bw, _geo, _lum, _shift, f32

i32 = np.int32


def _gather(arr, qx, qy):
    """arr[qy, qx] with the coordinates clamped to the image: what a tap outside fetches is never used."""
    H, W = arr.shape[:2]
    return arr[np.clip(qy, 0, H - 1), np.clip(qx, 0, W - 1)]


def accumulate(a, b, albedo_cov, normal_depth, motion, spp_a, spp_b, prev=None, max_history=32, tau_z=0.1, tau_n=0.9):
    """Steps 1 to 5 of ptx_denoise_temporal's own part -> dict(col, var, g, alb, alpha: the filter's inputs; next: (color, moments,
    geometry); took: the pixels that took history; sw: the sum of the taken taps' bilinear weights)."""
    a, b, A, N, M = (np.asarray(x, f32) for x in (a, b, albedo_cov, normal_depth, motion))
    H, W = a.shape[:2]
    n, na, nb = f32(spp_a + spp_b), f32(spp_a), f32(spp_b)
    maxh, tz, tn = f32(max_history), f32(tau_z), f32(tau_n)
    with np.errstate(all="ignore"):
        # 1. the current frame, as ptx_denoise
        cov = A[..., 3]
        alb = np.fmax((A[..., :3] + (n - cov)[..., None]) / n, f32(0.001))
        col = ((a[..., :3] + b[..., :3]) / n) / alb
        d = (_lum((a[..., :3] / na) / alb) - _lum((b[..., :3] / nb) / alb)) * f32(0.5)
        v0 = d * d
        alpha = (a[..., 3] + b[..., 3]) / n
        hit = cov > 0
        g = np.where(hit[..., None], N / np.where(hit, cov, f32(1))[..., None], f32(0)).astype(f32)
        L = _lum(col)
        LL = L * L
        # 2. reprojection
        took = np.zeros((H, W), bool)
        hist = None
        sw = np.zeros((H, W), f32)
        if prev is not None:
            pc, pm, pg = (np.asarray(x, f32) for x in prev)
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
                    dot = (g[..., 0] * gq[..., 0] + g[..., 1] * gq[..., 1]) + g[..., 2] * gq[..., 2]
                    take = (have & (qx >= 0) & (qx < W) & (qy >= 0) & (qy < H) & (bq > 0) & (cq[..., 3] > 0) & (gq[..., 3] > 0)
                            & (np.abs(zexp - gq[..., 3]) <= tz * np.fmax(zexp, gq[..., 3])) & (dot >= tn))
                    hq = np.concatenate([cq, mq], -1)
                    sw = np.where(take, sw + bq, sw)
                    acc = np.where(take[..., None], acc + bq[..., None] * hq, acc)
            have = have & (sw > 0)
            h = acc / sw[..., None]
            # 3. blend
            Nh = np.fmin(h[..., 3] + f32(1), maxh)
            al = f32(1) / Nh
            bc = h[..., :3] + (col - h[..., :3]) * al[..., None]
            b1 = h[..., 4] + (L - h[..., 4]) * al
            b2 = h[..., 5] + (LL - h[..., 5]) * al
            took = have & np.isfinite(((bc[..., 0] + bc[..., 1]) + bc[..., 2]) + (b1 + b2))
            hist = (bc, b1, b2, Nh)
        if hist is None:
            colp, m1, m2, Np = col, L, LL, np.ones((H, W), f32)
        else:
            colp = np.where(took[..., None], hist[0], col)
            m1, m2 = np.where(took, hist[1], L), np.where(took, hist[2], LL)
            Np = np.where(took, hist[3], f32(1))
        # 4. the variance the filter starts from
        vf = np.where(Np < 4, v0, np.fmax(f32(0), m2 - m1 * m1))
        var = vf * (f32(1) / Np)
    nxt = (np.concatenate([colp, Np[..., None]], -1).astype(f32), np.stack([m1, m2], -1).astype(f32), g)
    for x in (colp, var, nxt[0], nxt[1]):
        assert x.dtype == f32, x.dtype
    return dict(col=colp, var=var, g=g, alb=alb, alpha=alpha, next=nxt, took=took, sw=sw)


def filter_tail(col, v0, g, alb, alpha, iterations=5, sigma_l=4.0, sigma_n=0.5, sigma_z=0.1):
    """Steps 2 to 5 of ptx_denoise's specification on a prepared state -> out [H,W,4]."""
    sl, sn, sz = f32(sigma_l), f32(sigma_n), f32(sigma_z)
    sl2, sn2, sz2 = sl * sl, sn * sn, sz * sz
    with np.errstate(all="ignore"):
        s0, s1 = np.zeros_like(v0), np.zeros_like(v0)
        for dy in (-1, 0, 1):
            for dx in (-1, 0, 1):
                gq, ok = _shift(g, dx, dy)
                vq, _ = _shift(v0, dx, dy)
                w = np.ones_like(v0) if dx == 0 and dy == 0 else _geo(g, gq, sn2, sz2)
                s0 = np.where(ok, s0 + w, s0)
                s1 = np.where(ok, s1 + w * vq, s1)
        var = s1 / s0
        for i in range(iterations):
            step = 1 << i
            L = _lum(col)
            den = (sl2 * var) + f32(1e-8)
            acc, ws, av = np.zeros_like(col), np.zeros_like(var), np.zeros_like(var)
            for dy in range(-2, 3):
                for dx in range(-2, 3):
                    cq, ok = _shift(col, dx * step, dy * step)
                    if not ok.any():
                        continue
                    h = KERN[abs(dx)] * KERN[abs(dy)]
                    if dx == 0 and dy == 0:
                        w = np.full_like(var, h)
                    else:
                        gq, _ = _shift(g, dx * step, dy * step)
                        Lq, _ = _shift(L, dx * step, dy * step)
                        dl = L - Lq
                        w = (h * _geo(g, gq, sn2, sz2)) * _bw((dl * dl) / den)
                    vq, _ = _shift(var, dx * step, dy * step)
                    take = ok & (w > 0)
                    acc = np.where(take[..., None], acc + w[..., None] * cq, acc)
                    ws = np.where(take, ws + w, ws)
                    av = np.where(take, av + (w * w) * vq, av)
            col = acc / ws[..., None]
            var = av / (ws * ws)
        out = np.concatenate([col * alb, alpha[..., None]], -1)
    assert out.dtype == f32, out.dtype
    return out


def synthetic(W, H, spp_a=3, spp_b=5, seed=1):
    """A finite frame: random positive sums; a guide with three planar regions of different unit normals and depth ramps, a cov = 0 block
    and a band of partly covered pixels -> (a, b, albedo_cov, normal_depth)."""
    rng = np.random.default_rng(seed + 1000 * W + H)
    n = spp_a + spp_b
    yy, xx = np.mgrid[0:H, 0:W]
    a = (rng.uniform(0.05, 2.0, (H, W, 4)) * spp_a).astype(f32)
    b = (rng.uniform(0.05, 2.0, (H, W, 4)) * spp_b).astype(f32)
    a[..., 3], b[..., 3] = spp_a, spp_b
    region = np.where(xx * 3 < W, 0, np.where(yy * 2 < H, 1, 2))
    normals = np.array([[0, 0, 1], [0.6, 0, 0.8], [0, 1, 0]], f32)[region]
    depth = (f32(2) + f32(0.03) * xx + f32(0.05) * yy * (region == 2) + f32(1.5) * (region == 1)).astype(f32)
    cov = np.full((H, W), n, f32)
    cov[(yy >= H // 4) & (yy < H // 4 + max(H // 5, 1)) & (xx >= W // 2) & (xx < W // 2 + max(W // 4, 1))] = 0
    band = (yy >= (2 * H) // 3) & (yy < (2 * H) // 3 + 3)
    cov[band] = (1 + (xx[band] % (n - 1))).astype(f32)
    albedo = rng.uniform(0.2, 0.9, (H, W, 3)).astype(f32)
    A = np.concatenate([albedo * cov[..., None], cov[..., None]], -1).astype(f32)
    N = np.concatenate([normals * cov[..., None], (depth * cov)[..., None]], -1).astype(f32)
    return a, b, A, N


def motion_sums(A, N, mvx=0.0, mvy=0.0):
    """The motion sums of a frame whose every surface sample moved by (mvx, mvy) pixels and kept its distance from the camera:
    (mvx * cov, mvy * cov, depth sum, cov). Integer motions and the small integer coverages divide back exactly."""
    cov = A[..., 3]
    return np.stack([f32(mvx) * cov, f32(mvy) * cov, N[..., 3], cov], -1).astype(f32)


def restate(a, b, albedo_cov, normal_depth, motion, spp_a, spp_b, prev=None, iterations=5, sigma_l=4.0, sigma_n=0.5, sigma_z=0.1, max_history=32,
            tau_z=0.1, tau_n=0.9):
    """The specification of ptx_denoise_temporal -> (out [H,W,4], next (color, moments, geometry), took [H,W] bool)."""
    s = accumulate(a, b, albedo_cov, normal_depth, motion, spp_a, spp_b, prev, max_history, tau_z, tau_n)
    out = filter_tail(s["col"], s["var"], s["g"], s["alb"], s["alpha"], iterations, sigma_l, sigma_n, sigma_z)
    return out, s["next"], s["took"]
