"""numpy restatement of the light tree of ptx_render_nee's punctual lights (include/ptx.h: ptx_scene_set_punctual_pick, PUNCTUAL PICK), for
tests/test_nee_punctual_tree.py and tests/test_nee_punctual_tree_gpu.py. Not collected (underscore prefix).

build:      THE TREE as ptx_scene_set_punctual_pick builds it: uint32 [n_nodes, 8], float64 where the text says float64.
importance: THE IMPORTANCE of nodes seen from positions, float32 in the written order, vectorised over (node, position) pairs.
pick:       THE PICK for arrays of (position, u) -> (light, pmf), all descents level by level.
leaf_pmfs:  every light's pmf at the given positions as the product of the branch probabilities, by walking the whole tree with the same
            float32 branch probabilities p and 1 - p the descent uses (so a descent's pmf is bit for bit the entry of the light it ends at).
cdf_pick:   the CDF mode's pick: the first stored entry with u below it, and the difference of the stored entries.

R0: the conditional variance ratio tree / CDF that test_nee_punctual_tree.test_variance_ratio_r0 measures on VARIANCE_CASE; the GPU test's
bar is 2 * R0.
"""
import numpy as np

from _nee_restatement import _clamp, _dot, _fmax2, _fmin2, f32

LEAF = np.uint32(0x80000000)
ONE_BELOW = np.nextafter(f32(1), f32(0))   # 0x1.fffffep-1F
VARIANCE_CASE = dict(lamps=dict(n_lamps=16, spots=True), W=32, H=24, spp=4)
R0 = 0.4402   # measured on the restatement; the CPU test recomputes it and holds it to this figure


def lum_of(lights):
    I = np.asarray(lights, f32).reshape(-1, 16)[:, 8:11].astype(np.float64)
    return (0.2126 * I[:, 0] + 0.7152 * I[:, 1]) + 0.0722 * I[:, 2]


def build(lights):
    """[n, 16] records -> the tree [n_nodes, 8] uint32 (lo.xyz, power, hi.xyz, word 7); [0, 8] without a light of positive luminance"""
    if lights is None or len(lights) == 0:
        return np.zeros((0, 8), np.uint32)
    L = np.asarray(lights, f32).reshape(-1, 16)
    lum = lum_of(L)
    keep = [k for k in range(len(L)) if lum[k] > 0]
    if not keep:
        return np.zeros((0, 8), np.uint32)
    nodes, queue = [None], [(0, keep)]
    while queue:
        i, idx = queue.pop(0)                     # FIFO
        p = L[idx, 0:3]
        lo, hi = p.min(0), p.max(0)
        power = 0.0
        for k in idx:                             # float64, in the node's light order
            power += float(lum[k])
        if len(idx) == 1:
            w7 = np.uint32(LEAF | np.uint32(idx[0]))
        else:
            ext = hi.astype(np.float64) - lo.astype(np.float64)
            ax = int(np.argmax(ext))              # the lowest axis wins a tie
            order = sorted(idx, key=lambda k: (float(L[k, ax]), k))
            half = len(order) // 2
            w7 = np.uint32(len(nodes))
            nodes += [None, None]
            queue += [(int(w7), order[:half]), (int(w7) + 1, order[half:])]
        rec = np.zeros(8, np.uint32)
        rec[0:3], rec[4:7] = lo.view(np.uint32), hi.view(np.uint32)
        rec[3] = np.array([power], np.float64).astype(f32).view(np.uint32)[0]
        rec[7] = w7
        nodes[i] = rec
    return np.stack(nodes)


def light_geom(rec, x):
    """PUNCTUAL SAMPLE's v, dist2, dist, w, att and range test of the records rec [n, 16] seen from x [n, 3] -> (dist2, dist, w, att, in_range)"""
    with np.errstate(all="ignore"):
        v = rec[:, 0:3] - x
        dist2 = _dot(v, v)
        dist = np.sqrt(dist2)
        w = v / dist[:, None]
        cd = _dot(rec[:, 4:7], -w)
        sm = _clamp((cd - rec[:, 12]) / _fmax2(rec[:, 11] - rec[:, 12], f32(1e-6)), f32(0), f32(1))
        att = np.where(rec[:, 7] != 0, sm * sm, f32(1)).astype(f32)
        in_range = (rec[:, 3] == 0) | (dist <= rec[:, 3])
    return dist2, dist, w, att, in_range


def importance(T, lights, node, x):
    """importance of the nodes `node` [n] seen from x [n, 3] float32 -> [n] float32"""
    L = np.asarray(lights, f32).reshape(-1, 16)
    N = T[node]
    lo, hi, power, w7 = N[:, 0:3].view(f32), N[:, 4:7].view(f32), N[:, 3].view(f32), N[:, 7]
    x = np.asarray(x, f32)
    with np.errstate(all="ignore"):
        c = (lo + hi) * f32(0.5)
        d = x - c
        h = (hi - lo) * f32(0.5)
        out = (power / _fmax2(_dot(d, d), _dot(h, h))).astype(f32)
        leaf = (w7 & LEAF) != 0
        if leaf.any():
            dist2, _, _, att, in_range = light_geom(L[(w7[leaf] & ~LEAF).astype(np.int64)], x[leaf])
            out[leaf] = np.where((dist2 > 0) & in_range, (power[leaf] * att) / dist2, f32(0)).astype(f32)
    return out


def branch_p(T, lights, left, x):
    """p of the branches whose left children are `left` [n], seen from x [n, 3]: I_l / (I_l + I_r), 0.5 where the sum is not positive and finite"""
    il, ir = importance(T, lights, left, x), importance(T, lights, left + 1, x)
    with np.errstate(all="ignore"):
        s = il + ir
        return np.where((s > 0) & (s < np.inf), il / s, f32(0.5)).astype(f32)


def pick(T, lights, x, u):
    """x [n, 3], u [n] -> (light [n] int32, pmf [n] float32)"""
    x, u = np.asarray(x, f32).reshape(-1, 3), np.asarray(u, f32).reshape(-1).copy()
    n = len(u)
    node, pmf = np.zeros(n, np.int64), np.ones(n, f32)
    while True:
        w7 = T[node, 7]
        act = np.flatnonzero((w7 & LEAF) == 0)
        if not len(act):
            return (w7 & ~LEAF).astype(np.int32), pmf
        left = w7[act].astype(np.int64)
        p = branch_p(T, lights, left, x[act])
        ua = u[act]
        go_left = ua < p
        with np.errstate(all="ignore"):
            q1 = f32(1) - p
            pmf[act] = np.where(go_left, pmf[act] * p, pmf[act] * q1)
            un = np.where(go_left, ua / p, (ua - p) / q1).astype(f32)
        u[act] = _fmin2(un, ONE_BELOW)
        node[act] = np.where(go_left, left, left + 1)


def leaf_pmfs(T, lights, x):
    """x [n, 3] -> [n, n_lights] float32: every light's pmf from x as the product of the branch probabilities (0 for a light in no leaf)"""
    x = np.asarray(x, f32).reshape(-1, 3)
    n = len(x)
    out = np.zeros((n, len(np.asarray(lights).reshape(-1, 16))), f32)
    stack = [(0, np.ones(n, f32))]
    while stack:
        i, pm = stack.pop()
        w7 = T[i, 7]
        if w7 & LEAF:
            out[:, int(w7 & ~LEAF)] = pm
            continue
        left = np.full(n, int(w7), np.int64)
        p = branch_p(T, lights, left, x)
        stack.append((int(w7), (pm * p).astype(f32)))
        stack.append((int(w7) + 1, (pm * (f32(1) - p)).astype(f32)))
    return out


def depths(T):
    """leaf depths (the root is depth 1)"""
    out, stack = [], [(0, 1)]
    while stack:
        i, d = stack.pop()
        if T[i, 7] & LEAF:
            out.append(d)
        else:
            stack += [(int(T[i, 7]), d + 1), (int(T[i, 7]) + 1, d + 1)]
    return out


def cdf_pick(cdf, u):
    """the CDF mode: stored cdf [n], u [m] -> (light [m] int32, pmf [m] float32 from the stored differences)"""
    cdf = np.asarray(cdf, f32)
    k = np.minimum(np.searchsorted(cdf, np.asarray(u, f32), side="right"), len(cdf) - 1)
    pmf = (cdf - np.concatenate([np.zeros(1, f32), cdf[:-1]])).astype(f32)
    return k.astype(np.int32), pmf[k]
