"""numpy restatement of PTX_NEE_CANDIDATES (include/ptx.h: CANDIDATES, WEIGHT AND SELECTION, ESTIMATE), for tests/test_nee_ris.py.
Built on tests/_nee_pdf_restatement.py as that file is built on tests/_nee_env_restatement.py and tests/_nee_restatement.py: the vertex is
theirs, statement for statement, for both light kinds (tab: the environment table, or None for the triangle list alone) and for both weight
bases (spdf: PTX_NEE_SAMPLER_PDF's ps, or pe). The light sample of a vertex has become a function of the candidate's index j, which moves
the Philox blocks to 3 + 2 j and 4 + 2 j and changes nothing else; the vertex takes M of them, keeps one by the selection rule in float32
with the header's parenthesisation, and traces that one's shadow ray.

M = 1 is the call without the bits: one candidate, no weight, no scale; render_samples(M=1) is _nee_pdf_restatement's frame bit for bit.

select: the selection rule alone, on given weights and given uniforms (the frequency test).
render_samples: per-sample radiance. Two wrong forms, the switches of the power checks: kept_div divides wsum by the number of KEPT
candidates instead of M; emission_m puts M * p_l into the emission weight, as if the BSDF-side density had changed.

R0: the per-pixel sample variance of VARIANCE_CASE at M = 4 over that at M = 1, as test_nee_ris measures it on this restatement; the GPU
test compares the product's ratio with it.
"""
import numpy as np

from _nee_env_restatement import BLOCK_ENV, env_box, env_pdf, sample_env
from _nee_pdf_restatement import sampler_pdf
from _nee_restatement import (BLOCK_LIGHT, BLOCK_SUN, BLOCK_SURFACE, EPS, _Attr, _clamp, _closest, _dot, _eval_brdf, _fmax2, _lerp, _material,
                              _mulmv, _normalize, _pbr, _shading_normal, draws, f32, light_list)

BLOCK_RIS = 0x100
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


def render_samples(ora, o, a, W, H, spp, bounces, tab, M, spdf=False, seed=0x5EED, env=(1.0, 1.0, 1.0), tile=None, sample0=0, lights=True,
                   kept_div=False, emission_m=False):
    """-> dict(rad [h, w, spp, 3] float32, light_samples, light_visible, rays). tab: _nee_env_restatement.table() of the map the oracle
    scene `o` has been given, or None: no environment sample. M: the candidates per vertex, 1 .. 16."""
    assert 1 <= M <= 16
    x0, y0, w, h = tile if tile else (0, 0, W, H)
    npix, N = w * h, w * h * spp
    env = np.asarray(env, f32)
    env_map = getattr(o, "_env", None) is not None
    assert tab is None or env_map
    attr = _Attr(a)
    model_of = attr.model_of
    mats = np.asarray(a.materials, f32)
    ll = light_list(a) if lights else dict(tris=np.zeros((0, 2), np.uint32), cdf=np.zeros(0, f32), geom=np.zeros((0, 4), f32), area=f32(0),
                                           surf_first=np.full(len(mats), -1, np.int32))
    n_l = len(ll["cdf"])
    c_env = (f32(0.5) if n_l else f32(1)) if tab is not None else f32(0)   # without a table (1 - c_env) * p_l is p_l, and is not computed
    light_key = ll["tris"][:, 0].astype(np.int64) << 32 | ll["tris"][:, 1].astype(np.int64)
    has_sun = a.sun is not None
    O, D = np.zeros((N, 3), f32), np.zeros((N, 3), f32)
    for s in range(spp):
        r = o.primary_rays(ora.make_cfg(W, H, 1, 1, seed=seed, tile=(x0, y0, w, h)), sample0 + s).reshape(-1, 6)
        O[s * npix:(s + 1) * npix], D[s * npix:(s + 1) * npix] = r[:, :3], r[:, 3:]
    p_local = np.tile(np.arange(npix), spp)
    pixel = ((y0 + p_local // w) * W + (x0 + p_local % w)).astype(np.uint32)
    sample = (sample0 + np.repeat(np.arange(spp), npix)).astype(np.uint32)
    T, L = np.ones((N, 3), f32), np.zeros((N, 3), f32)
    PP = np.zeros(N, f32)
    depth, pas = np.zeros(N, np.int64), np.zeros(N, np.int64)
    live = np.arange(N) if bounces > 0 else np.zeros(0, np.int64)
    stats = dict(light_samples=0, light_visible=0, rays=0)

    def listed(surf, tri):
        if n_l == 0:
            return np.full(len(surf), -1, np.int64)
        key = surf.astype(np.int64) << 32 | tri.astype(np.int64)
        k = np.minimum(np.searchsorted(light_key, key), n_l - 1)
        return np.where(light_key[k] == key, k, -1)

    def scale_pl(p_l):   # p_l' of a triangle: (1 - c_env) * p_l with a table, p_l without
        return (f32(1) - c_env) * p_l if tab is not None else p_l

    while len(live):
        out, surf, tri, dist = _closest(o, model_of, np.concatenate([O[live], D[live]], 1))
        stats["rays"] += len(live)
        nxt = np.zeros(len(live), bool)
        miss = surf < 0
        if miss.any():   # ---- miss: the environment, weighted against the environment sample of the previous vertex where one exists
            gm = live[miss]
            if env_map:
                uv, _, col = o.env_lookup(D[gm], env)
                add = T[gm] * col
            else:
                add = T[gm] * env
            wsel = (depth[gm] != 0) & (pas[gm] == 0)
            if tab is not None and wsel.any():
                pp = PP[gm[wsel]]
                wm = pp / (pp + c_env * env_pdf(tab, D[gm[wsel]], uv[wsel]))   # env_pdf: a SINGLE candidate's density, whatever M
                add[wsel] = add[wsel] * wm[:, None]
            L[gm] = L[gm] + add
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

            def weight_pdf(c2, wdir, pe):   # what the weights are built on: ps with PTX_NEE_SAMPLER_PDF, pe without
                if not spdf:
                    return pe
                return sampler_pdf(ora, normal[c2], outc[c2], wdir, rough[c2], spec_prob[c2], ior[c2])
            # ---- sun (as _nee_restatement)
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
            ti = np.flatnonzero(through)
            O[g[ti]] = pos[ti] + d[ti] * EPS
            D[g[ti]] = _normalize(d[ti])
            pas[g[ti]] = pa[ti] + 1
            nxt[hi[ti]] = pas[g[ti]] <= 4096
            # ---- emission: the formula is unchanged, p_l is a SINGLE candidate's density, whatever M
            ai = np.flatnonzero(act)
            ga = g[ai]
            em = T[ga] * e10[ai]
            wsel = (k_l[ai] >= 0) & (dep[ai] != 0) & (pa[ai] == 0)
            if wsel.any():
                kk = k_l[ai][wsel]
                cg = np.abs(_dot(ll["geom"][kk, 0:3], d[ai][wsel]))
                with np.errstate(all="ignore"):
                    p_l = scale_pl((di[ai][wsel] * di[ai][wsel]) / (cg * ll["area"]))
                    if emission_m:   # the wrong form
                        p_l = f32(M) * p_l
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
                    """candidate j of every vertex of ci -> (contributes [nc], x [nc, 3], direction [nc, 3], towards the map [nc],
                    surface [nc], triangle [nc]): the unflagged light sample with blocks 3 + 2 j and 4 + 2 j"""
                    okc, X, Wd = np.zeros(nc, bool), np.zeros((nc, 3), f32), np.zeros((nc, 3), f32)
                    is_env, LS, LT = np.zeros(nc, bool), np.zeros(nc, np.int64), np.zeros(nc, np.int64)
                    r, to_env = None, np.zeros(nc, bool)
                    if n_l:
                        r = draws(ora, pixel[gc], sample[gc], dep[ci], pa[ci], BLOCK_LIGHT + 2 * j, seed)
                    if tab is not None:
                        to_env = r[:, 3] < f32(0.5) if n_l else np.ones(nc, bool)
                    ei = np.flatnonzero(to_env)
                    if len(ei):
                        ce = ci[ei]
                        q = draws(ora, pixel[g[ce]], sample[g[ce]], dep[ce], pa[ce], BLOCK_ENV + 2 * j, seed)
                        bi, bj, wdir = sample_env(tab, q)
                        fuv, _, Le = o.env_lookup(wdir, env)
                        fi, fj = env_box(tab, fuv)
                        p = env_pdf(tab, wdir, fuv)
                        ok = (fi == bi) & (fj == bj) & (_dot(normal[ce], wdir) > 0) & (p > 0) & (_fmax2(Le[:, 0], _fmax2(Le[:, 1], Le[:, 2])) > 0)
                        oi = np.flatnonzero(ok)
                        if len(oi):
                            c2 = ce[oi]
                            brdf, pdf = _eval_brdf(ora, normal[c2], outc[c2], wdir[oi], albedo[c2], rough[c2], metallic[c2], spec_prob[c2], ior[c2])
                            pe = _fmax2(pdf, EPS)
                            qc = _clamp(brdf / pe[:, None], f32(0), f32(1))
                            pw = weight_pdf(c2, wdir[oi], pe)
                            keep = pw > 0                       # !(ps > 0): nothing, and no shadow ray
                            c2, oi, qc, pw = c2[keep], oi[keep], qc[keep], pw[keep]
                            wl = pw / (pw + c_env * p[oi])
                            idx = ei[oi]
                            X[idx] = ((T[g[c2]] * qc) * wl[:, None]) * Le[oi]
                            Wd[idx], is_env[idx], okc[idx] = wdir[oi], True, True
                    li = np.flatnonzero(~to_env)
                    if n_l and len(li):
                        cl, rl = ci[li], r[li]
                        k = np.minimum(np.searchsorted(ll["cdf"], rl[:, 0], side="right"), n_l - 1)
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
                            ok = (dist2 > 0) & (_dot(normal[cl], wdir) > 0) & (_dot(n_y, -wdir) > 0) & (cg > 0) & (_fmax2(Le[:, 0], _fmax2(Le[:, 1], Le[:, 2])) > 0)
                        oi = np.flatnonzero(ok)
                        if len(oi):
                            c2 = cl[oi]
                            brdf, pdf = _eval_brdf(ora, normal[c2], outc[c2], wdir[oi], albedo[c2], rough[c2], metallic[c2], spec_prob[c2], ior[c2])
                            pe = _fmax2(pdf, EPS)
                            qc = _clamp(brdf / pe[:, None], f32(0), f32(1))
                            pw = weight_pdf(c2, wdir[oi], pe)
                            keep = pw > 0
                            c2, oi, qc, pw = c2[keep], oi[keep], qc[keep], pw[keep]
                            p_l = scale_pl(dist2[oi] / (cg[oi] * ll["area"]))
                            wl = pw / (pw + p_l)
                            idx = li[oi]
                            X[idx] = ((T[g[c2]] * qc) * wl[:, None]) * Le[oi]
                            Wd[idx], LS[idx], LT[idx], okc[idx] = wdir[oi], ls[oi], lt[oi], True
                    return okc, X, Wd, is_env, LS, LT

                if M == 1:   # the call without the bits: the one sample as it is
                    chosen, cX, cWd, cEnv, cLS, cLT = candidate(0)
                else:
                    chosen, cX, cWd = np.zeros(nc, bool), np.zeros((nc, 3), f32), np.zeros((nc, 3), f32)
                    cEnv, cLS, cLT = np.zeros(nc, bool), np.zeros(nc, np.int64), np.zeros(nc, np.int64)
                    wsum, Wy, n_kept = np.zeros(nc, f32), np.ones(nc, f32), np.zeros(nc, np.int64)
                    for j in range(M):
                        okc, X, Wd, is_env, LS, LT = candidate(j)
                        Wj = _fmax2(X[:, 0], _fmax2(X[:, 1], X[:, 2]))
                        keep = okc & (Wj > 0) & np.isfinite(Wj)
                        wsum = np.where(keep, wsum + Wj, wsum).astype(f32)
                        u = draws(ora, pixel[gc], sample[gc], dep[ci], pa[ci], BLOCK_RIS + (j >> 2), seed)[:, j & 3]
                        with np.errstate(all="ignore"):
                            take = keep & (~chosen | (u * wsum < Wj))
                        cX[take], cWd[take], cEnv[take], cLS[take], cLT[take], Wy[take] = X[take], Wd[take], is_env[take], LS[take], LT[take], Wj[take]
                        chosen = chosen | keep
                        n_kept += keep
                    denom = np.maximum(n_kept, 1).astype(f32) if kept_div else f32(M)   # kept_div: the wrong form
                    cX = cX * ((wsum / denom) / Wy)[:, None]
                yi = np.flatnonzero(chosen)
                if len(yi):
                    c2 = ci[yi]
                    rays = np.concatenate([pos[c2] + cWd[yi] * EPS, cWd[yi]], 1)
                    _, hs, ht, _ = _closest(o, model_of, rays)
                    stats["rays"] += len(yi)
                    vis = np.where(cEnv[yi], hs < 0, (hs == cLS[yi]) & (ht == cLT[yi]))
                    stats["light_samples"] += len(yi)
                    stats["light_visible"] += int(vis.sum())
                    L[g[c2[vis]]] = L[g[c2[vis]]] + cX[yi][vis]
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
                O[g[c2]] = pos[c2] + inc[oi] * EPS
                D[g[c2]] = _normalize(inc[oi])
                depth[g[c2]] = dep[c2] + 1
                pas[g[c2]] = 0
                nxt[hi[c2]] = depth[g[c2]] != bounces
        live = live[nxt]

    res = dict(rad=L.reshape(spp, h, w, 3).transpose(1, 2, 0, 3).copy())
    res.update(stats)
    return res
