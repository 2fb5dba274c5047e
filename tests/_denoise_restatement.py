"""ptx_denoise restated in float32 numpy from its specification in include/ptx.h (tests/test_denoise.py states the rules and pins the
product to it bit for bit; tests/test_multigpu_product.py filters the reduced halves with it). Not collected (underscore prefix).
"""
import numpy as np

f32 = np.float32
KERN = (f32(0.375), f32(0.25), f32(0.0625))


def _shift(arr, dx, dy):
    """q[y, x] = arr[y + dy, x + dx] where that lies inside the image (zeros elsewhere), and the mask of where it does."""
    H, W = arr.shape[:2]
    out, ok = np.zeros_like(arr), np.zeros((H, W), bool)
    y0, y1, x0, x1 = max(0, -dy), min(H, H - dy), max(0, -dx), min(W, W - dx)
    if y0 < y1 and x0 < x1:
        out[y0:y1, x0:x1] = arr[y0 + dy:y1 + dy, x0 + dx:x1 + dx]
        ok[y0:y1, x0:x1] = True
    return out, ok


def _bw(x):
    t = np.fmax(f32(0), f32(1) - x)
    return t * t


def _lum(c):
    return (f32(0.2126) * c[..., 0] + f32(0.7152) * c[..., 1]) + f32(0.0722) * c[..., 2]


def _geo(gp, gq, sn2, sz2):
    dn = gp[..., :3] - gq[..., :3]
    xn = ((dn[..., 0] * dn[..., 0] + dn[..., 1] * dn[..., 1]) + dn[..., 2] * dn[..., 2]) / sn2
    zm = np.fmax(gp[..., 3], gq[..., 3])
    rel = np.where(zm > 0, (gp[..., 3] - gq[..., 3]) / np.where(zm > 0, zm, f32(1)), f32(0))
    xz = (rel * rel) / sz2
    return _bw(xn) * _bw(xz)


def restate(a, b, albedo_cov, normal_depth, spp_a, spp_b, iterations=5, sigma_l=4.0, sigma_n=0.5, sigma_z=0.1):
    """The specification of ptx_denoise in float32 numpy -> out [H,W,4] (filtered means, alpha)."""
    a, b, A, N = (np.asarray(x, f32) for x in (a, b, albedo_cov, normal_depth))
    sl, sn, sz = f32(sigma_l), f32(sigma_n), f32(sigma_z)
    sl2, sn2, sz2 = sl * sl, sn * sn, sz * sz
    n, na, nb = f32(spp_a + spp_b), f32(spp_a), f32(spp_b)
    with np.errstate(all="ignore"):
        # 1. prepare
        cov = A[..., 3]
        alb = np.fmax((A[..., :3] + (n - cov)[..., None]) / n, f32(0.001))
        col = ((a[..., :3] + b[..., :3]) / n) / alb
        d = (_lum((a[..., :3] / na) / alb) - _lum((b[..., :3] / nb) / alb)) * f32(0.5)
        v0 = d * d
        alpha = (a[..., 3] + b[..., 3]) / n
        hit = cov > 0
        g = np.where(hit[..., None], N / np.where(hit, cov, f32(1))[..., None], f32(0)).astype(f32)
        # 3. variance prefilter
        s0, s1 = np.zeros_like(v0), np.zeros_like(v0)
        for dy in (-1, 0, 1):
            for dx in (-1, 0, 1):
                gq, ok = _shift(g, dx, dy)
                vq, _ = _shift(v0, dx, dy)
                w = np.ones_like(v0) if dx == 0 and dy == 0 else _geo(g, gq, sn2, sz2)
                s0 = np.where(ok, s0 + w, s0)
                s1 = np.where(ok, s1 + w * vq, s1)
        var = s1 / s0
        # 4. iterations
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
        # 5. output
        out = np.concatenate([col * alb, alpha[..., None]], -1)
    assert out.dtype == f32, out.dtype
    return out


# the quality case: Cornell 96 x 54, 8 bounces, seed 0x5EED, halves of samples 0..7 and 8..15
QW, QH, QB, QSEED = 96, 54, 8, 0x5EED
