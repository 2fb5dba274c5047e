"""numpy restatement of the light tree over ptx_render_nee's light list (include/ptx.h: ptx_scene_set_light_pick, LIGHT PICK), for
tests/test_nee_light_tree.py and tests/test_nee_light_tree_gpu.py. Not collected (underscore prefix).

leaves:     per listed triangle, in float64 from the float64 world corners of THE LIGHT LIST: centroid, the float32 box of the corners, power.
build:      THE TREE and the path words as build_lights makes them in tree mode: (uint32 [n_nodes, 8], uint32 [n]).
importance: THE IMPORTANCE of nodes seen from positions, float32 in the written order, one formula for leaves and branches.
pick:       THE PICK for arrays of (position, u) -> (entry, pmf), all descents level by level.
pmf:        THE DIRECTED PMF of given entries at given positions: the walk along the entry's path word.
leaf_pmfs:  every entry's pmf at the given positions, by walking the whole tree with the same float32 p and 1 - p.
cdf_pick:   the CDF mode's pick and the difference of the stored entries.
render_samples: the tree-mode vertex loop of ptx_render_nee for the triangle list (LIGHT SAMPLE, EMISSION WEIGHT, PATH STATE) with SPDF and
            M = 1 .. 16, built from the primitives of _nee_restatement as _nee_estimator.render_samples is. tree=None is the CDF mode, and
            must then equal _nee_estimator.render_samples bit for bit (tests/test_nee_light_tree.py pins it). ENV and PUN are not restated.

R0: the variance ratio tree / CDF that test_nee_light_tree.test_variance_ratio_r0 measures on VARIANCE_CASE; the GPU test's bar is 2 * R0.
"""
import numpy as np

from _nee_pdf_restatement import sampler_pdf
from _nee_restatement import (BLOCK_LIGHT, BLOCK_SUN, BLOCK_SURFACE, EPS, _Attr, _clamp, _closest, _dot, _eval_brdf, _fmax2, _fmin2, _lerp,
                              _material, _mulmv, _normalize, _pbr, _shading_normal, draws, f32, light_list)

LEAF = np.uint32(0x80000000)
ONE_BELOW = np.nextafter(f32(1), f32(0))   # 0x1.fffffep-1F
BLOCK_RIS = 0x100
VARIANCE_CASE = dict(n=64, seed=7, W=32, H=24, spp=4, bounces=2)
R0 = 0.2347   # measured on the restatement; the CPU test recomputes it and holds it to this figure
WRONG = ("area_total",        # A_total kept in p_l (the light sample's and the emission weight's) beside the tree's pmf
         "pmf_at_hit",        # the emission weight's pmf taken at the hit point instead of x_prev
         "no_pmf_emission")   # pmf left out of the emission weight


# ---------------------------------------------------------------------------- the tree
def leaves(a, ll):
    """scene arrays and their light list -> (centroid float64 [n, 3], lo float32 [n, 3], hi float32 [n, 3], power float64 [n])"""
    mats = np.asarray(a.materials, f32)
    n_surf = len(mats)
    model_of = np.zeros(n_surf, np.int64)
    for m, (first, cnt) in enumerate(np.asarray(a.model_surf)):
        model_of[first:first + cnt] = m
    n = len(ll["cdf"])
    cen, lo, hi, power = np.zeros((n, 3)), np.zeros((n, 3), f32), np.zeros((n, 3), f32), np.zeros(n)
    V, Tr, XF, SR = np.asarray(a.vertices, f32), np.asarray(a.triangles), np.asarray(a.model_xform, f32), np.asarray(a.surf_range)
    for k in range(n):
        s, t = int(ll["tris"][k, 0]), int(ll["tris"][k, 1])
        X = XF[model_of[s]].astype(np.float64)
        v0, _, t0, _ = [int(x) for x in SR[s][:4]]
        c = []
        for j in range(3):
            v = V[v0 + int(Tr[t0 + t][j])].astype(np.float64)
            c.append(np.array([(X[3 + i] * v[0] + X[6 + i] * v[1]) + X[9 + i] * v[2] + X[i] for i in range(3)]))
        e1, e2 = c[1] - c[0], c[2] - c[0]
        cr = np.array([e1[1] * e2[2] - e1[2] * e2[1], e1[2] * e2[0] - e1[0] * e2[2], e1[0] * e2[1] - e1[1] * e2[0]])
        area = 0.5 * np.sqrt((cr[0] * cr[0] + cr[1] * cr[1]) + cr[2] * cr[2])
        cen[k] = ((c[0] + c[1]) + c[2]) / 3.0
        C = np.stack(c)
        lo[k], hi[k] = C.min(0).astype(f32), C.max(0).astype(f32)
        em = mats[s, 6:9].astype(np.float64)
        power[k] = area * ((0.2126 * em[0] + 0.7152 * em[1]) + 0.0722 * em[2])
    return cen, lo, hi, power


def build_from_leaves(cen, lo, hi, power):
    """-> (tree uint32 [n_nodes, 8], path uint32 [n]); ([0, 8], [0]) for an empty list"""
    n = len(power)
    if n == 0:
        return np.zeros((0, 8), np.uint32), np.zeros(0, np.uint32)
    path = np.zeros(n, np.uint32)
    nodes, queue = [None], [(0, 0, 0, list(range(n)))]
    while queue:
        i, dep, word, idx = queue.pop(0)                      # FIFO
        blo, bhi = lo[idx].min(0), hi[idx].max(0)
        pw = 0.0
        for k in idx:                                          # float64, in the node's order
            pw += float(power[k])
        if len(idx) == 1:
            w7 = np.uint32(LEAF | np.uint32(idx[0]))
            path[idx[0]] = word
        else:
            ext = cen[idx].max(0) - cen[idx].min(0)
            ax = int(np.argmax(ext))                           # the lowest axis wins a tie
            order = sorted(idx, key=lambda k: (float(cen[k, ax]), k))
            half = len(order) // 2
            w7 = np.uint32(len(nodes))
            nodes += [None, None]
            queue += [(int(w7), dep + 1, word, order[:half]), (int(w7) + 1, dep + 1, word | (1 << dep), order[half:])]
        rec = np.zeros(8, np.uint32)
        rec[0:3], rec[4:7] = blo.astype(f32).view(np.uint32), bhi.astype(f32).view(np.uint32)
        rec[3] = np.array([pw], np.float64).astype(f32).view(np.uint32)[0]
        rec[7] = w7
        nodes[i] = rec
    return np.stack(nodes), path


def build(a, ll=None):
    ll = light_list(a) if ll is None else ll
    return build_from_leaves(*leaves(a, ll))


def importance(T, node, x):
    """importance of the nodes `node` [n] seen from x [n, 3] float32 -> [n] float32; one formula for leaves and branches"""
    N = T[node]
    lo, hi, power = N[:, 0:3].view(f32), N[:, 4:7].view(f32), N[:, 3].view(f32)
    x = np.asarray(x, f32)
    with np.errstate(all="ignore"):
        c = (lo + hi) * f32(0.5)
        d = x - c
        h = (hi - lo) * f32(0.5)
        return (power / _fmax2(_dot(d, d), _dot(h, h))).astype(f32)


def branch_p(T, left, x):
    """p of the branches whose left children are `left` [n], seen from x [n, 3]: I_l / (I_l + I_r), 0.5 where the sum is not positive and finite"""
    il, ir = importance(T, left, x), importance(T, left + 1, x)
    with np.errstate(all="ignore"):
        s = il + ir
        return np.where((s > 0) & (s < np.inf), il / s, f32(0.5)).astype(f32)


def pick(T, x, u):
    """x [n, 3], u [n] -> (entry [n] int32, pmf [n] float32)"""
    x, u = np.asarray(x, f32).reshape(-1, 3), np.asarray(u, f32).reshape(-1).copy()
    n = len(u)
    node, pm = np.zeros(n, np.int64), np.ones(n, f32)
    while True:
        w7 = T[node, 7]
        act = np.flatnonzero((w7 & LEAF) == 0)
        if not len(act):
            return (w7 & ~LEAF).astype(np.int32), pm
        left = w7[act].astype(np.int64)
        p = branch_p(T, left, x[act])
        ua = u[act]
        go_left = ua < p
        with np.errstate(all="ignore"):
            q1 = f32(1) - p
            pm[act] = np.where(go_left, pm[act] * p, pm[act] * q1)
            un = np.where(go_left, ua / p, (ua - p) / q1).astype(f32)
        u[act] = _fmin2(un, ONE_BELOW)
        node[act] = np.where(go_left, left, left + 1)


def pmf(T, path, k, x):
    """entries k [n] at positions x [n, 3] -> pmf_k(x) [n] float32: the walk along path[k]"""
    x = np.asarray(x, f32).reshape(-1, 3)
    word = np.asarray(path, np.uint32)[np.asarray(k, np.int64)].astype(np.int64)
    n = len(x)
    node, pm = np.zeros(n, np.int64), np.ones(n, f32)
    while True:
        w7 = T[node, 7]
        act = np.flatnonzero((w7 & LEAF) == 0)
        if not len(act):
            assert ((w7 & ~LEAF).astype(np.int64) == np.asarray(k, np.int64)).all()   # every path word leads to its own leaf
            return pm
        left = w7[act].astype(np.int64)
        p = branch_p(T, left, x[act])
        go_left = (word[act] & 1) == 0
        pm[act] = np.where(go_left, pm[act] * p, pm[act] * (f32(1) - p)).astype(f32)
        node[act] = np.where(go_left, left, left + 1)
        word[act] >>= 1


def leaf_pmfs(T, x):
    """x [n, 3] -> [n, n_entries] float32: every entry's pmf from x as the product of the branch probabilities"""
    x = np.asarray(x, f32).reshape(-1, 3)
    n = len(x)
    out = np.zeros((n, (len(T) + 1) // 2), f32)
    stack = [(0, np.ones(n, f32))]
    while stack:
        i, pm = stack.pop()
        w7 = T[i, 7]
        if w7 & LEAF:
            out[:, int(w7 & ~LEAF)] = pm
            continue
        p = branch_p(T, np.full(n, int(w7), np.int64), x)
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


def branch_centres(T):
    """the centres (lo + hi) * 0.5 of every node's box [n_nodes, 3] float32"""
    return ((T[:, 0:3].view(f32) + T[:, 4:7].view(f32)) * f32(0.5)).astype(f32)


def cdf_pick(cdf, u):
    """the CDF mode: stored cdf [n], u [m] -> (entry [m] int32, pmf [m] float32 from the stored differences)"""
    cdf = np.asarray(cdf, f32)
    k = np.minimum(np.searchsorted(cdf, np.asarray(u, f32), side="right"), len(cdf) - 1)
    pm = (cdf - np.concatenate([np.zeros(1, f32), cdf[:-1]])).astype(f32)
    return k.astype(np.int32), pm[k]


# ---------------------------------------------------------------------------- the vertex loop
def render_samples(ora, o, a, W, H, spp, bounces, *, tree=None, M=1, spdf=False, seed=0x5EED, env=(1.0, 1.0, 1.0), wrong=(), first=None):
    """The vertex loop of ptx_render_nee for the triangle list (no environment table, no punctual lights). tree: None = the CDF mode, else
    (T, path) of build(). -> dict(rad [H, W, spp, 3] float32 per-sample radiance, v1_listed [H, W, spp] bool: the sample's vertex at depth 1
    lies on a listed triangle, rays, light_samples, light_visible).
    first: None (M = 1 only otherwise), or a dict that receives the depth-0 triangle samples that contribute: ids (s * n_pixels + p), surf,
    tri, x, and what picked the triangle: pos (the vertex's position) and u (r.x of the light block)."""
    assert first is None or M == 1
    wrong = frozenset(wrong)
    assert wrong <= frozenset(WRONG) and (not wrong or tree is not None)
    assert 1 <= M <= 16
    w, h = W, H
    npix, N = w * h, w * h * spp
    env = np.asarray(env, f32)
    env_map = getattr(o, "_env", None) is not None
    attr = _Attr(a)
    model_of = attr.model_of
    mats = np.asarray(a.materials, f32)
    ll = light_list(a)
    n_l = len(ll["cdf"])
    if tree is not None and n_l == 0:
        tree = None                                            # an empty list: the mode is ignored
    if tree is not None:
        TT, path = tree
    A_of = ll["geom"][:, 3] if n_l else np.zeros(0, f32)
    light_key = ll["tris"][:, 0].astype(np.int64) << 32 | ll["tris"][:, 1].astype(np.int64)
    has_sun = a.sun is not None
    O, D = np.zeros((N, 3), f32), np.zeros((N, 3), f32)
    for s in range(spp):
        r = o.primary_rays(ora.make_cfg(W, H, 1, 1, seed=seed, tile=(0, 0, w, h)), s).reshape(-1, 6)
        O[s * npix:(s + 1) * npix], D[s * npix:(s + 1) * npix] = r[:, :3], r[:, 3:]
    p_local = np.tile(np.arange(npix), spp)
    pixel = ((p_local // w) * W + (p_local % w)).astype(np.uint32)
    sample = np.repeat(np.arange(spp), npix).astype(np.uint32)
    T, L = np.ones((N, 3), f32), np.zeros((N, 3), f32)
    PP = np.zeros(N, f32)
    XP = np.zeros((N, 3), f32)                                 # x_prev
    depth, pas = np.zeros(N, np.int64), np.zeros(N, np.int64)
    v1_listed = np.zeros(N, bool)
    live = np.arange(N) if bounces > 0 else np.zeros(0, np.int64)
    stats = dict(rays=0, light_samples=0, light_visible=0)

    def listed(surf, tri):
        if n_l == 0:
            return np.full(len(surf), -1, np.int64)
        key = surf.astype(np.int64) << 32 | tri.astype(np.int64)
        k = np.minimum(np.searchsorted(light_key, key), n_l - 1)
        return np.where(light_key[k] == key, k, -1)

    while len(live):
        out, surf, tri, dist = _closest(o, model_of, np.concatenate([O[live], D[live]], 1))
        stats["rays"] += len(live)
        nxt = np.zeros(len(live), bool)
        miss = surf < 0
        if miss.any():
            gm = live[miss]
            col = o.env_lookup(D[gm], env)[2] if env_map else env
            L[gm] = L[gm] + T[gm] * col
        hi = np.flatnonzero(~miss)
        if len(hi):
            g = live[hi]
            pos, uv, sn = out[hi, 0:3], out[hi, 3:5], out[hi, 11:14]
            sf, tr, di = surf[hi], tri[hi], dist[hi]
            me = _material(o, sf, uv)
            albedo, opacity, rough, metallic, e10 = me[:, 3:6], me[:, 6], me[:, 7], me[:, 8], me[:, 9:12] * f32(10)
            ior, catcher_m = mats[sf, 9], mats[sf, 10] != 0
            d = D[g]
            dep, pa = depth[g], pas[g]
            k_l = listed(sf, tr)
            v1_listed[g[(dep == 1) & (k_l >= 0)]] = True
            last = dep + 1 == bounces
            rnd = draws(ora, pixel[g], sample[g], dep, pa, BLOCK_SURFACE, seed)
            approx1 = (opacity == f32(1)) | (np.abs(opacity - f32(1)) < EPS)
            through = ~approx1 & (rnd[:, 0] > opacity)
            normal, outc = sn, -d
            back = ~through & (_dot(normal, outc) <= 0)
            act = ~through & ~back
            rough = _fmax2(rough, f32(0.05))
            pb = _pbr(ora, normal, outc, normal, rnd[:, 2], rnd[:, 3], rough, 1, ior)
            spec_prob = _fmax2(pb[:, 11], metallic)

            def weight_pdf(c2, wdir, pe):
                if not spdf:
                    return pe
                return sampler_pdf(ora, normal[c2], outc[c2], wdir, rough[c2], spec_prob[c2], ior[c2])
            # ---- sun
            sun_add = np.zeros((len(g), 3), f32)
            pending_dead, add = np.zeros(len(g), bool), np.zeros(len(g), bool)
            if has_sun:
                sun = np.asarray(a.sun, f32)
                sr = draws(ora, pixel[g], sample[g], dep, pa, BLOCK_SUN, seed)
                c0 = _mulmv((sun[0:3][None], sun[3:6][None], sun[6:9][None]), np.array([[0, 0, 1]], f32))
                ct = np.cos((sr[:, 1] * sun[12]).astype(np.float64)).astype(f32)
                c = _pbr(ora, np.repeat(c0, len(g), 0), outc, outc, 0, sr[:, 0], rough, ct, ior)[:, 0:3]
                sampled = act & (_dot(normal, c) > 0)
                si = np.flatnonzero(sampled)
                occl = np.zeros(len(g), bool)
                if len(si):
                    _, ssurf = o.intersect(np.concatenate([pos[si] + c[si] * EPS, _normalize(c[si])], 1))
                    stats["rays"] += len(si)
                    occl[si] = ssurf >= 0
                catcher = catcher_m & (dep == 0)
                lit_catcher = sampled & catcher & ~occl
                pending_dead = sampled & catcher & occl
                through = through | lit_catcher
                add = sampled & ~catcher & ~occl
                if add.any():
                    brdf, _ = _eval_brdf(ora, normal[add], outc[add], c[add], albedo[add], rough[add], metallic[add], spec_prob[add], ior[add])
                    e = sun[9:12]
                    pdf = _lerp(f32(1), f32(1), spec_prob[add])
                    v = brdf * e / _fmax2(pdf, EPS)[:, None]
                    sun_add[add] = T[g[add]] * _clamp(v, f32(0), e)
                act = act & ~lit_catcher & ~pending_dead
            # ---- pass-through: same depth, pass + 1; p_prev and x_prev stay
            ti = np.flatnonzero(through)
            O[g[ti]] = pos[ti] + d[ti] * EPS
            D[g[ti]] = _normalize(d[ti])
            pas[g[ti]] = pa[ti] + 1
            nxt[hi[ti]] = pas[g[ti]] <= 4096
            # ---- emission
            ai = np.flatnonzero(act)
            ga = g[ai]
            em = T[ga] * e10[ai]
            wsel = (k_l[ai] >= 0) & (dep[ai] != 0) & (pa[ai] == 0)
            if wsel.any():
                kk = k_l[ai][wsel]
                cg = np.abs(_dot(ll["geom"][kk, 0:3], d[ai][wsel]))
                dd = di[ai][wsel]
                with np.errstate(all="ignore"):
                    if tree is None:
                        p_l = (dd * dd) / (cg * ll["area"])
                    else:
                        at = pos[ai][wsel] if "pmf_at_hit" in wrong else XP[ga[wsel]]
                        pk = np.ones(len(kk), f32) if "no_pmf_emission" in wrong else pmf(TT, path, kk, at)
                        p_l = (pk * (dd * dd)) / (cg * (ll["area"] if "area_total" in wrong else A_of[kk]))
                    wgt = PP[ga[wsel]] / (PP[ga[wsel]] + p_l)
                em[wsel] = em[wsel] * wgt[:, None]
            L[ga] = L[ga] + em
            sa = np.flatnonzero(add)
            L[g[sa]] = L[g[sa]] + sun_add[sa]
            # ---- the light sample: M candidates, one kept
            ci = ai[~last[ai]]
            gc = g[ci]
            if len(ci):
                nc = len(ci)

                def candidate(j):
                    okc, X, Wd = np.zeros(nc, bool), np.zeros((nc, 3), f32), np.zeros((nc, 3), f32)
                    LS, LT = np.zeros(nc, np.int64), np.zeros(nc, np.int64)
                    if not n_l:
                        return okc, X, Wd, LS, LT
                    rl = draws(ora, pixel[gc], sample[gc], dep[ci], pa[ci], BLOCK_LIGHT + 2 * j, seed)
                    cl = ci
                    if tree is None:
                        k = np.minimum(np.searchsorted(ll["cdf"], rl[:, 0], side="right"), n_l - 1)
                        pm = np.ones(nc, f32)
                    else:
                        k, pm = pick(TT, pos[cl], rl[:, 0])
                        k = k.astype(np.int64)
                    su = np.sqrt(rl[:, 1])
                    beta, gamma = su * (f32(1) - rl[:, 2]), su * rl[:, 2]
                    ls, lt = ll["tris"][k, 0].astype(np.int64), ll["tris"][k, 1].astype(np.int64)
                    ypos, yuv, ynrm, ytan = attr.at(ls, lt, beta, gamma)
                    my = _material(o, ls, yuv)
                    n_y, Le = _shading_normal(ynrm, ytan, my[:, 0:3]), my[:, 9:12] * f32(10)
                    v = ypos - pos[cl]
                    dist2 = _dot(v, v)
                    with np.errstate(all="ignore"):
                        wdir = v / np.sqrt(dist2)[:, None]
                        cg = np.abs(_dot(ll["geom"][k, 0:3], wdir))
                        ok = ((dist2 > 0) & (_dot(normal[cl], wdir) > 0) & (_dot(n_y, -wdir) > 0) & (cg > 0)
                              & (_fmax2(Le[:, 0], _fmax2(Le[:, 1], Le[:, 2])) > 0) & (pm > 0))
                    oi = np.flatnonzero(ok)
                    if len(oi):
                        c2 = cl[oi]
                        brdf, pdf = _eval_brdf(ora, normal[c2], outc[c2], wdir[oi], albedo[c2], rough[c2], metallic[c2], spec_prob[c2], ior[c2])
                        pe = _fmax2(pdf, EPS)
                        qc = _clamp(brdf / pe[:, None], f32(0), f32(1))
                        pw = weight_pdf(c2, wdir[oi], pe)
                        keep = pw > 0
                        c2, oi, qc, pw = c2[keep], oi[keep], qc[keep], pw[keep]
                        with np.errstate(all="ignore"):
                            if tree is None:
                                p_l = dist2[oi] / (cg[oi] * ll["area"])
                            else:
                                p_l = (pm[oi] * dist2[oi]) / (cg[oi] * (ll["area"] if "area_total" in wrong else A_of[k[oi]]))
                            wl = pw / (pw + p_l)
                        X[oi] = ((T[g[c2]] * qc) * wl[:, None]) * Le[oi]
                        Wd[oi], LS[oi], LT[oi], okc[oi] = wdir[oi], ls[oi], lt[oi], True
                    return okc, X, Wd, LS, LT

                if M == 1:
                    chosen, cX, cWd, cLS, cLT = candidate(0)
                else:
                    chosen, cX, cWd = np.zeros(nc, bool), np.zeros((nc, 3), f32), np.zeros((nc, 3), f32)
                    cLS, cLT = np.zeros(nc, np.int64), np.zeros(nc, np.int64)
                    wsum, Wy = np.zeros(nc, f32), np.ones(nc, f32)
                    for j in range(M):
                        okc, X, Wd, LS, LT = candidate(j)
                        Wj = _fmax2(X[:, 0], _fmax2(X[:, 1], X[:, 2]))
                        keep = okc & (Wj > 0) & np.isfinite(Wj)
                        wsum = np.where(keep, wsum + Wj, wsum).astype(f32)
                        u = draws(ora, pixel[gc], sample[gc], dep[ci], pa[ci], BLOCK_RIS + (j >> 2), seed)[:, j & 3]
                        with np.errstate(all="ignore"):
                            take = keep & (~chosen | (u * wsum < Wj))
                        cX[take], cWd[take], cLS[take], cLT[take], Wy[take] = X[take], Wd[take], LS[take], LT[take], Wj[take]
                        chosen = chosen | keep
                    cX = cX * ((wsum / f32(M)) / Wy)[:, None]
                yi = np.flatnonzero(chosen)
                if len(yi):
                    c2 = ci[yi]
                    rays = np.concatenate([pos[c2] + cWd[yi] * EPS, cWd[yi]], 1)
                    _, hs, ht, _ = _closest(o, model_of, rays)
                    stats["rays"] += len(yi)
                    vis = (hs == cLS[yi]) & (ht == cLT[yi])
                    stats["light_samples"] += len(yi)
                    stats["light_visible"] += int(vis.sum())
                    L[g[c2[vis]]] = L[g[c2[vis]]] + cX[yi][vis]
                    if first is not None and "ids" not in first:
                        z = dep[c2] == 0
                        u0 = draws(ora, pixel[g[c2]], sample[g[c2]], dep[c2], pa[c2], BLOCK_LIGHT, seed)[:, 0]   # candidate 0's r.x
                        first.update(ids=g[c2[z]].copy(), surf=cLS[yi][z].copy(), tri=cLT[yi][z].copy(), x=cX[yi][z].copy(), pos=pos[c2[z]].copy(), u=u0[z].copy())
                # ---- BSDF sample
                spec = rnd[ci, 1] < spec_prob[ci]
                inc = np.where(spec[:, None], pb[ci, 6:9], pb[ci, 3:6])
                ok = _dot(normal[ci], inc) > 0
                oi = np.flatnonzero(ok)
                c2 = ci[oi]
                brdf, pdf = _eval_brdf(ora, normal[c2], outc[c2], inc[oi], albedo[c2], rough[c2], metallic[c2], spec_prob[c2], ior[c2])
                pe = _fmax2(pdf, EPS)
                with np.errstate(all="ignore"):
                    qv = brdf / pe[:, None]
                T[g[c2]] = T[g[c2]] * _clamp(qv, f32(0), f32(1))
                ps = weight_pdf(c2, inc[oi], pe)
                PP[g[c2]] = np.where((ps > 0) & np.isfinite(ps), ps, pe)
                XP[g[c2]] = pos[c2]
                O[g[c2]] = pos[c2] + inc[oi] * EPS
                D[g[c2]] = _normalize(inc[oi])
                depth[g[c2]] = dep[c2] + 1
                pas[g[c2]] = 0
                nxt[hi[c2]] = depth[g[c2]] != bounces
        live = live[nxt]

    res = dict(rad=L.reshape(spp, h, w, 3).transpose(1, 2, 0, 3).copy(), v1_listed=v1_listed.reshape(spp, h, w).transpose(1, 2, 0).copy())
    res.update(stats)
    return res
