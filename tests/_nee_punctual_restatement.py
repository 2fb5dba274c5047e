"""numpy restatement of the punctual lights of ptx_render_nee (include/ptx.h: PUNCTUAL LIGHTS), for tests/test_nee_punctual.py and
tests/test_nee_punctual_gpu.py. Built on tests/_nee_ris_restatement.py as that file is built on _nee_pdf_restatement.py,
_nee_env_restatement.py and _nee_restatement.py: the vertex is theirs, statement for statement, for every light kind (tab), weight basis
(spdf) and candidate count (M). A candidate has become one of three kinds: with lights given, candidate j draws block 0x200 + j and is a
punctual sample iff c_p == 1 or q.x < 0.5; the other strategies' densities carry (1 - c_p), multiplied from the left onto the density as the
older text computes it.

punctual=None (or an empty array, or lights that are all black) is the scene without lights: render_samples is then
_nee_ris_restatement.render_samples bit for bit, since no statement of it is touched.

cdf_of: the CDF as ptx_scene_set_punctual_lights builds it. render_samples: per-sample radiance. Two wrong forms, the switches of the power
checks: forget_bsdf_side leaves (1 - c_p) out of the emission and miss weights; forget_cp leaves 1 / c_p out of x.
"""
import numpy as np

from _nee_env_restatement import BLOCK_ENV, env_box, env_pdf, sample_env
from _nee_pdf_restatement import sampler_pdf
from _nee_ris_restatement import BLOCK_RIS
from _nee_restatement import (BLOCK_LIGHT, BLOCK_SUN, BLOCK_SURFACE, EPS, _Attr, _clamp, _closest, _dot, _eval_brdf, _fmax2, _lerp, _material,
                              _mulmv, _normalize, _pbr, _shading_normal, draws, f32, light_list)

BLOCK_PUNCTUAL = 0x200
KIND_TRI, KIND_ENV, KIND_PUNCTUAL = 0, 1, 2


def cdf_of(lights):
    """[n, 16] records -> the stored CDF [n] float32 (float64 shares of lum(intensity), the last entry 1), or None when there is no light or
    every light is black: ptx_scene_set_punctual_lights then stores none"""
    if lights is None or len(lights) == 0:
        return None
    I = np.asarray(lights, f32).reshape(-1, 16)[:, 8:11].astype(np.float64)
    cum = np.cumsum((0.2126 * I[:, 0] + 0.7152 * I[:, 1]) + 0.0722 * I[:, 2])
    if not cum[-1] > 0:
        return None
    cdf = (cum / cum[-1]).astype(f32)
    cdf[-1] = 1
    return cdf


def render_samples(ora, o, a, W, H, spp, bounces, tab, M, spdf=False, seed=0x5EED, env=(1.0, 1.0, 1.0), tile=None, sample0=0, lights=True,
                   punctual=None, forget_bsdf_side=False, forget_cp=False):
    """-> dict(rad [h, w, spp, 3] float32, light_samples, light_visible, rays). tab: _nee_env_restatement.table() of the map the oracle
    scene `o` has been given, or None: no environment sample. M: the candidates per vertex, 1 .. 16. punctual: [n, 16] records as
    ptx_scene_set_punctual_lights takes them, or None."""
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
    pcdf = cdf_of(punctual)
    pun = pcdf is not None
    if pun:
        PL = np.asarray(punctual, f32).reshape(-1, 16)
        ppmf = (pcdf - np.concatenate([np.zeros(1, f32), pcdf[:-1]])).astype(f32)   # from the stored values
    c_p = (f32(0.5) if (n_l or tab is not None) else f32(1)) if pun else f32(0)
    bsdf_cp = pun and not forget_bsdf_side   # (1 - c_p) in the emission weight and the miss weight
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

    def scale_pl(p_l, cp=pun):   # p_l' of a triangle: (1 - c_env) * p_l with a table, p_l without; with punctual lights (1 - c_p) times that
        p_l = (f32(1) - c_env) * p_l if tab is not None else p_l
        return (f32(1) - c_p) * p_l if cp else p_l

    def scale_pe(p_e, cp=pun):   # the environment sample's density c_env * p; with punctual lights (1 - c_p) times that
        return (f32(1) - c_p) * p_e if cp else p_e

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
                wm = pp / (pp + scale_pe(c_env * env_pdf(tab, D[gm[wsel]], uv[wsel]), bsdf_cp))   # env_pdf: a SINGLE candidate's density, whatever M
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
                    p_l = scale_pl((di[ai][wsel] * di[ai][wsel]) / (cg * ll["area"]), bsdf_cp)
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
                    """candidate j of every vertex of ci -> (contributes [nc], x [nc, 3], direction [nc, 3], kind [nc], surface [nc],
                    triangle [nc], distance of a punctual light [nc]): a punctual sample from block 0x200 + j, or the unflagged light sample
                    with blocks 3 + 2 j and 4 + 2 j"""
                    okc, X, Wd = np.zeros(nc, bool), np.zeros((nc, 3), f32), np.zeros((nc, 3), f32)
                    kind, LS, LT, LD = np.zeros(nc, np.int64), np.zeros(nc, np.int64), np.zeros(nc, np.int64), np.zeros(nc, f32)
                    is_p = np.zeros(nc, bool)
                    if pun:
                        q = draws(ora, pixel[gc], sample[gc], dep[ci], pa[ci], BLOCK_PUNCTUAL + j, seed)
                        is_p = (q[:, 0] < f32(0.5)) if c_p != 1 else np.ones(nc, bool)
                        pi = np.flatnonzero(is_p)
                        if len(pi):
                            cp_ = ci[pi]
                            k = np.minimum(np.searchsorted(pcdf, q[pi, 1], side="right"), len(pcdf) - 1)
                            rec = PL[k]
                            v = rec[:, 0:3] - pos[cp_]
                            dist2 = _dot(v, v)
                            with np.errstate(all="ignore"):
                                dist = np.sqrt(dist2)
                                wdir = v / dist[:, None]
                                cd = _dot(rec[:, 4:7], -wdir)
                                sm = _clamp((cd - rec[:, 12]) / _fmax2(rec[:, 11] - rec[:, 12], f32(1e-6)), f32(0), f32(1))
                                att = np.where(rec[:, 7] != 0, sm * sm, f32(1)).astype(f32)
                                E = (rec[:, 8:11] * att[:, None]) / dist2[:, None]
                                ok = ((dist2 > 0) & (_dot(normal[cp_], wdir) > 0) & (ppmf[k] > 0) & ((rec[:, 3] == 0) | (dist <= rec[:, 3])) & (att > 0)
                                      & (_fmax2(E[:, 0], _fmax2(E[:, 1], E[:, 2])) > 0))
                            oi = np.flatnonzero(ok)
                            if len(oi):
                                c2 = cp_[oi]
                                brdf, pdf = _eval_brdf(ora, normal[c2], outc[c2], wdir[oi], albedo[c2], rough[c2], metallic[c2], spec_prob[c2], ior[c2])
                                pe = _fmax2(pdf, EPS)
                                qc = _clamp(brdf / pe[:, None], f32(0), f32(1))
                                b = qc * pe[:, None]
                                den = ppmf[k[oi]] if forget_cp else c_p * ppmf[k[oi]]   # forget_cp: the wrong form
                                idx = pi[oi]
                                X[idx] = ((T[g[c2]] * b) * E[oi]) / den[:, None]
                                Wd[idx], kind[idx], LD[idx], okc[idx] = wdir[oi], KIND_PUNCTUAL, dist[oi], True
                    r, to_env = None, np.zeros(nc, bool)
                    if n_l:
                        r = draws(ora, pixel[gc], sample[gc], dep[ci], pa[ci], BLOCK_LIGHT + 2 * j, seed)
                    if tab is not None:
                        to_env = r[:, 3] < f32(0.5) if n_l else np.ones(nc, bool)
                    to_env = to_env & ~is_p
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
                            wl = pw / (pw + scale_pe(c_env * p[oi]))
                            idx = ei[oi]
                            X[idx] = ((T[g[c2]] * qc) * wl[:, None]) * Le[oi]
                            Wd[idx], kind[idx], okc[idx] = wdir[oi], KIND_ENV, True
                    li = np.flatnonzero(~to_env & ~is_p)
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
                    return okc, X, Wd, kind, LS, LT, LD

                if M == 1:   # the call without the bits: the one sample as it is
                    chosen, cX, cWd, cKind, cLS, cLT, cLD = candidate(0)
                else:
                    chosen, cX, cWd = np.zeros(nc, bool), np.zeros((nc, 3), f32), np.zeros((nc, 3), f32)
                    cKind, cLS, cLT, cLD = np.zeros(nc, np.int64), np.zeros(nc, np.int64), np.zeros(nc, np.int64), np.zeros(nc, f32)
                    wsum, Wy = np.zeros(nc, f32), np.ones(nc, f32)
                    for j in range(M):
                        okc, X, Wd, kind, LS, LT, LD = candidate(j)
                        Wj = _fmax2(X[:, 0], _fmax2(X[:, 1], X[:, 2]))
                        keep = okc & (Wj > 0) & np.isfinite(Wj)
                        wsum = np.where(keep, wsum + Wj, wsum).astype(f32)
                        u = draws(ora, pixel[gc], sample[gc], dep[ci], pa[ci], BLOCK_RIS + (j >> 2), seed)[:, j & 3]
                        with np.errstate(all="ignore"):
                            take = keep & (~chosen | (u * wsum < Wj))
                        cX[take], cWd[take], cKind[take], cLS[take], cLT[take], cLD[take], Wy[take] = X[take], Wd[take], kind[take], LS[take], LT[take], LD[take], Wj[take]
                        chosen = chosen | keep
                    cX = cX * ((wsum / f32(M)) / Wy)[:, None]
                yi = np.flatnonzero(chosen)
                if len(yi):
                    c2 = ci[yi]
                    rays = np.concatenate([pos[c2] + cWd[yi] * EPS, cWd[yi]], 1)
                    _, hs, ht, hd = _closest(o, model_of, rays)
                    stats["rays"] += len(yi)
                    vis = np.where(cKind[yi] == KIND_ENV, hs < 0, (hs == cLS[yi]) & (ht == cLT[yi]))
                    vis = np.where(cKind[yi] == KIND_PUNCTUAL, (hs < 0) | ~(hd < cLD[yi]), vis)   # nothing nearer than the light
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
