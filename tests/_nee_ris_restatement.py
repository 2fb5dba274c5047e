"""numpy restatement of PTX_NEE_CANDIDATES' selection rule alone (include/ptx.h: WEIGHT AND SELECTION), for tests/test_nee_ris.py; the
candidates, the loop that keeps one of them and the estimate are in tests/_nee_estimator.py (M).

select: the selection rule on given weights and given uniforms (the frequency test).

R0: the per-pixel sample variance of VARIANCE_CASE at M = 4 over that at M = 1, as test_nee_ris measures it on the estimator's restatement; the
GPU test compares the product's ratio with it.
"""
import numpy as np

f32 = np.float32
VARIANCE_CASE = dict(name="cornell", W=32, H=32, bounces=3, spp=64, seed=0x5EED, M=4)
R0 = 0.9036


def select(Wj, u):
    """The selection rule on weights Wj [n, M] float32 (a weight that is not a positive finite number: a dropped candidate) and uniforms
    u [n, M] float32 -> (chosen index [n] or -1, wsum [n] float32)"""
    n, M = Wj.shape
    wsum, y = np.zeros(n, f32), np.full(n, -1, np.int64)
    for j in range(M):
        w = Wj[:, j]
        keep = (w > 0) & np.isfinite(w)
        wsum = np.where(keep, wsum + w, wsum).astype(f32)
        with np.errstate(all="ignore"):
            take = keep & ((y < 0) | (u[:, j] * wsum < w))
        y = np.where(take, j, y)
    return y, wsum
