"""ptx_denoise_counts restated in float32 numpy from its specification in include/ptx.h: ptx_denoise's filter with step 1 taking the halves'
per-pixel sample counts from their .w and the guides' count from guide_spp. Steps 2 to 5 are written out again from the text, on the
primitives of tests/_denoise_restatement.py (bw, lum, geo, the shifted views). Not collected (underscore prefix).
"""
import numpy as np

from _denoise_restatement import KERN, _bw, _geo, _lum, _shift

f32 = np.float32


def restate_counts(a, b, albedo_cov, normal_depth, guide_spp, iterations=5, sigma_l=4.0, sigma_n=0.5, sigma_z=0.1):
    """The specification of ptx_denoise_counts in float32 numpy -> out [H,W,4] (filtered means, alpha)."""
    a, b, A, N = (np.asarray(x, f32) for x in (a, b, albedo_cov, normal_depth))
    sl, sn, sz = f32(sigma_l), f32(sigma_n), f32(sigma_z)
    sl2, sn2, sz2 = sl * sl, sn * sn, sz * sz
    ng = f32(guide_spp)
    with np.errstate(all="ignore"):
        # 1. per pixel, with the pixel's own counts
        na, nb = a[..., 3:4], b[..., 3:4]
        n = na + nb
        cov = A[..., 3]
        alb = np.fmax((A[..., :3] + (ng - cov)[..., None]) / ng, f32(0.001))
        col = ((a[..., :3] + b[..., :3]) / n) / alb
        d = (_lum((a[..., :3] / na) / alb) - _lum((b[..., :3] / nb) / alb)) * f32(0.5)
        v0 = d * d
        alpha = (a[..., 3] + b[..., 3]) / n[..., 0]
        hit = cov > 0
        g = np.where(hit[..., None], N / np.where(hit, cov, f32(1))[..., None], f32(0)).astype(f32)
        # 3. variance prefilter, 3 x 3, row-major, the centre with weight 1
        s0, s1 = np.zeros_like(v0), np.zeros_like(v0)
        for dy in (-1, 0, 1):
            for dx in (-1, 0, 1):
                gq, ok = _shift(g, dx, dy)
                vq, _ = _shift(v0, dx, dy)
                w = np.ones_like(v0) if dx == 0 and dy == 0 else _geo(g, gq, sn2, sz2)
                s0 = np.where(ok, s0 + w, s0)
                s1 = np.where(ok, s1 + w * vq, s1)
        var = s1 / s0
        # 4. the iterations: 25 taps at distance 2^i, dy outer
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
        # 5. re-modulate
        out = np.concatenate([col * alb, alpha[..., None]], -1)
    assert out.dtype == f32, out.dtype
    return out


def synthetic(h, w, seed, uniform=None):
    """Half-buffers with random even per-pixel counts (2 .. 32 per half), guides over 8 samples with missed pixels and partly covered ones,
    a depth edge and a few bright outliers. uniform = (spp_a, spp_b): every pixel has those counts and the guides hold spp_a + spp_b samples.
    -> (a, b, albedo_cov, normal_depth, guide_spp)"""
    rng = np.random.default_rng(seed)
    if uniform:
        na, nb = np.full((h, w), uniform[0], f32), np.full((h, w), uniform[1], f32)
        ng = uniform[0] + uniform[1]
    else:
        na, nb = (2 * rng.integers(1, 17, (h, w))).astype(f32), (2 * rng.integers(1, 17, (h, w))).astype(f32)
        ng = 8
    albedo = rng.uniform(0.1, 0.9, (h, w, 3)).astype(f32)
    light = rng.uniform(0.0, 2.0, (h, w, 3)).astype(f32)
    light[rng.random((h, w)) < 0.02] *= f32(20)
    mean = albedo * light

    def half(n_half):
        noise = (f32(1) + f32(0.3) * rng.standard_normal((h, w, 3)).astype(f32))
        return np.concatenate([(mean * noise) * n_half[..., None], n_half[..., None]], -1).astype(f32)
    a, b = half(na), half(nb)
    cov = np.where(rng.random((h, w)) < 0.1, rng.integers(0, ng, (h, w)), ng).astype(f32)
    cov[:, : max(1, w // 9)] = 0                      # missed pixels: the sky
    nrm = rng.standard_normal((h, w, 3)).astype(f32)
    nrm /= np.linalg.norm(nrm, axis=-1, keepdims=True)
    nrm[h // 2:] = (0, 1, 0)                          # a flat region next to a rough one
    z = np.where(np.arange(w)[None, :] < w // 2, 3.0, 7.5).astype(f32) + rng.uniform(0, 0.05, (h, w)).astype(f32)
    A = np.concatenate([albedo * cov[..., None], cov[..., None]], -1).astype(f32)
    N = np.concatenate([nrm * cov[..., None], (z * cov)[..., None]], -1).astype(f32)
    return a, b, A, N, ng
