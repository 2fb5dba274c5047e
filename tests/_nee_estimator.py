"""numpy float32 wavefront restatement of ptx_render_nee's estimator (include/ptx.h), the yardstick of every tests/test_nee*.py: ONE vertex for
every light kind and every flag. Not collected (underscore prefix).

Built on the oracle's batch primitives only: OracleScene.intersect (closest hit: position, uv, shading normal, surface),
OracleScene.model_intersect (the same hit's triangle index and distance), material_eval, primary_rays, env_lookup, pt_oracle.pbr (importance
samples, pdfs, Fresnel: every call that goes through libm), pt_oracle.philox and the scene arrays. Everything else is written out on np.float32
arrays in the operation order of the specification (numpy neither contracts nor reorders). What is not the vertex lives in the files it is
imported from: the light list, the hit attributes and the BRDF (_nee_restatement), the environment table's pdf and sampler
(_nee_env_restatement), the sampler's density (_nee_pdf_restatement), the punctual lights' CDF (_nee_punctual_restatement).

The arguments of render_samples and the sections of include/ptx.h they restate:
tab      THE ENVIRONMENT TABLE, THE PDF, SELECTION, ENVIRONMENT SAMPLE, MISS WEIGHT (PTX_NEE_ENV_SAMPLES): _nee_env_restatement.table() of the map
         that the oracle scene has been given with set_environment, or None: no environment sample (the scene may still have a map, whose
         radiance a miss collects: per ray, OracleScene.env_lookup of the direction times the factor, renderer.cpp:443-449).
spdf     THE DENSITY, and where ps takes pe's place (PTX_NEE_SAMPLER_PDF): p_prev = ps(inc) where that is a positive finite number,
         wl = ps / (ps + p_l') for the triangle sample and for the environment sample, and no light sample where !(ps > 0).
M        CANDIDATES, WEIGHT AND SELECTION, ESTIMATE (PTX_NEE_CANDIDATES): the light sample of a vertex is a function of the candidate's index j,
         which moves the Philox blocks to 3 + 2 j and 4 + 2 j and changes nothing else; the vertex takes M of them, keeps one by the selection
         rule in float32 with the header's parenthesisation, and traces that one's shadow ray. M = 1 is the call without the bits: one
         candidate, no weight, no scale.
punctual PUNCTUAL LIGHTS: [n, 16] records as ptx_scene_set_punctual_lights takes them. Candidate j draws block 0x200 + j and is a punctual sample
         iff c_p == 1 or q.x < 0.5; the other strategies' densities carry (1 - c_p), multiplied from the left onto the density as the older
         text computes it. None, an empty array or lights that are all black: the scene without lights, no statement is touched.
lights   False runs with an empty triangle list (PTX_NEE_NO_LIGHT_SAMPLES); with tab=None and no punctual lights that is LIB itself.
fold     "throughput" is the product's order: vertex k's emission, its sun term, its light term, then vertex k + 1. "recursive" (only where no
         light sample is possible) adds a path's vertices back to front as renderer::trace returns them, which is what
         OracleScene.render_samples computes bit for bit.
wrong    names out of WRONG: forms that break the estimator on purpose, the switches of the tests' power checks, each in the domain it was
         written for.
"""
import numpy as np

from _nee_env_restatement import env_box, env_pdf, sample_env
from _nee_pdf_restatement import sampler_pdf
from _nee_punctual_restatement import cdf_of
from _nee_restatement import (BLOCK_LIGHT, BLOCK_SUN, BLOCK_SURFACE, EPS, _Attr, _clamp, _closest, _dot, _eval_brdf, _fmax2, _lerp, _material,
                              _mulmv, _normalize, _pbr, _shading_normal, draws, f32, light_list)

BLOCK_ENV, BLOCK_RIS, BLOCK_PUNCTUAL = 4, 0x100, 0x200   # candidate j: BLOCK_LIGHT + 2 j, BLOCK_ENV + 2 j, BLOCK_RIS + (j >> 2), BLOCK_PUNCTUAL + j
KIND_TRI, KIND_ENV, KIND_PUNCTUAL = 0, 1, 2
WRONG = ("no_mis",             # every weight of the triangle list is 1 (double counting)
         "no_light_term",      # the light term is dropped, the weights stay (energy lost)
         "no_miss_weight",     # wm = 1 (the map's radiance is counted twice)
         "c_env_one",          # every weight is computed with c_env = 1 while the selection still splits the vertices (energy is lost)
         "kept_div",           # wsum is divided by the number of KEPT candidates instead of M
         "emission_m",         # M * p_l in the emission weight, as if the BSDF-side density had changed
         "forget_bsdf_side",   # (1 - c_p) left out of the emission and miss weights
         "forget_cp")          # 1 / c_p left out of a punctual sample's x


def render_samples(ora, o, a, W, H, spp, bounces, *, tab=None, M=1, spdf=False, punctual=None, seed=0x5EED, env=(1.0, 1.0, 1.0), tile=None,
                   sample0=0, lights=True, fold="throughput", wrong=(), light_draws=None, first_env=None):
    """-> dict(rad [h, w, spp, 3] float32 per-sample radiance, v1_listed [h, w, spp] bool: the sample's vertex at depth 1 lies on a listed
    triangle, rays, light_samples, light_visible, env_samples, env_rejected_box: candidates towards the map, and those of them whose direction
    the lookup maps to another box). light_draws: None, or a list that receives, per round, the Philox keys (pixel, sample, depth, pass:
    uint32 [n, 4]) of the vertices that drew a light sample, accepted or not. first_env: None, or a dict that receives the depth-0
    environment samples: ids (sample ids: s * n_pixels + p), wdir, x, visible."""
    wrong = frozenset(wrong)
    assert wrong <= frozenset(WRONG), sorted(wrong - frozenset(WRONG))
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
    # the domains of the switches: those of the estimators they were written for
    one_plain = M == 1 and not spdf and not pun
    assert fold in ("throughput", "recursive") and (fold == "throughput" or not (lights or tab is not None or pun))
    assert not wrong & {"no_mis", "no_light_term"} or (one_plain and tab is None), wrong
    assert not wrong & {"no_miss_weight", "c_env_one"} or (one_plain and tab is not None), wrong
    assert not wrong & {"kept_div", "emission_m"} or (M > 1 and not pun), wrong
    assert not wrong & {"forget_bsdf_side", "forget_cp"} or pun, wrong
    assert light_draws is None or (M == 1 and tab is None and not pun)
    assert first_env is None or (M == 1 and tab is not None and not pun)
    if "c_env_one" in wrong:
        c_env = f32(1)                                # what the weights use; the selection below keeps its share of 0.5
    bsdf_cp = pun and "forget_bsdf_side" not in wrong   # (1 - c_p) in the emission weight and the miss weight
    light_key = ll["tris"][:, 0].astype(np.int64) << 32 | ll["tris"][:, 1].astype(np.int64)
    has_sun = a.sun is not None
    # state by sample id = s * npix + p
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
    v1_listed = np.zeros(N, bool)
    live = np.arange(N) if bounces > 0 else np.zeros(0, np.int64)
    rec = []   # per round, for the recursive fold
    stats = dict(rays=0, light_samples=0, light_visible=0, env_samples=0, env_rejected_box=0)

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
        R = dict(ids=live, kind=np.zeros(len(live), np.int8), e=np.zeros((len(live), 3), f32), dsun=np.zeros((len(live), 3), f32),
                 env=np.zeros((len(live), 3), f32), brdf=np.zeros((len(live), 3), f32), pe=np.ones(len(live), f32),
                 cont=np.zeros(len(live), bool))   # kind 0 zero, 1 miss, 2 pass, 3 vertex
        rec.append(R)
        miss = surf < 0
        R["kind"][miss] = 1
        if miss.any():   # ---- miss: the environment, weighted against the environment sample of the previous vertex where one exists
            gm = live[miss]
            if env_map:
                uv, _, col = o.env_lookup(D[gm], env)
            else:
                col = env
            R["env"][miss] = col
            add = T[gm] * col
            wsel = (depth[gm] != 0) & (pas[gm] == 0)
            if tab is not None and wsel.any() and "no_miss_weight" not in wrong:
                pp = PP[gm[wsel]]
                wm = pp / (pp + scale_pe(c_env * env_pdf(tab, D[gm[wsel]], uv[wsel]), bsdf_cp))   # env_pdf: a SINGLE candidate's density, whatever M
                add[wsel] = add[wsel] * wm[:, None]
            L[gm] = L[gm] + add
        hi = np.flatnonzero(~miss)          # positions within `live`
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
            act = ~through & ~back                                   # vertices that shade
            rough = _fmax2(rough, f32(0.05))
            pb = _pbr(ora, normal, outc, normal, rnd[:, 2], rnd[:, 3], rough, 1, ior)
            spec_prob = _fmax2(pb[:, 11], metallic)

            def weight_pdf(c2, wdir, pe):   # what the weights are built on: ps with PTX_NEE_SAMPLER_PDF, pe without
                if not spdf:
                    return pe
                return sampler_pdf(ora, normal[c2], outc[c2], wdir, rough[c2], spec_prob[c2], ior[c2])
            # ---- sun
            sun_add = np.zeros((len(g), 3), f32)
            sun_raw = np.zeros((len(g), 3), f32)
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
                    sun_raw[add] = _clamp(v, f32(0), e)
                    sun_add[add] = T[g[add]] * sun_raw[add]
                act = act & ~lit_catcher & ~pending_dead
            # ---- pass-through (opacity, or a lit catcher): same depth, pass + 1
            ti = np.flatnonzero(through)
            O[g[ti]] = pos[ti] + d[ti] * EPS
            D[g[ti]] = _normalize(d[ti])
            pas[g[ti]] = pa[ti] + 1
            nxt[hi[ti]] = pas[g[ti]] <= 4096
            R["kind"][hi[ti]] = 2
            # ---- emission, sun: p_l is a SINGLE candidate's density, whatever M; PP is what the previous vertex left
            ai = np.flatnonzero(act)
            ga = g[ai]
            em = T[ga] * e10[ai]
            wsel = (k_l[ai] >= 0) & (dep[ai] != 0) & (pa[ai] == 0)
            if wsel.any() and "no_mis" not in wrong:
                kk = k_l[ai][wsel]
                cg = np.abs(_dot(ll["geom"][kk, 0:3], d[ai][wsel]))
                with np.errstate(all="ignore"):
                    p_l = scale_pl((di[ai][wsel] * di[ai][wsel]) / (cg * ll["area"]), bsdf_cp)
                    if "emission_m" in wrong:
                        p_l = f32(M) * p_l
                    wgt = PP[ga[wsel]] / (PP[ga[wsel]] + p_l)
                em[wsel] = em[wsel] * wgt[:, None]
            L[ga] = L[ga] + em
            sa = np.flatnonzero(add)
            L[g[sa]] = L[g[sa]] + sun_add[sa]
            R["kind"][hi[ai]] = 3
            R["e"][hi[ai]] = e10[ai]
            R["dsun"][hi[ai]] = sun_raw[ai]
            # ---- the vertices that sample a direction. The light sample: M candidates, one kept
            ci = ai[~last[ai]]
            gc = g[ci]
            if len(ci):
                nc = len(ci)

                def candidate(j):
                    """candidate j of every vertex of ci -> (contributes [nc], x [nc, 3], direction [nc, 3], kind [nc], surface [nc],
                    triangle [nc], distance of a punctual light [nc]): a punctual sample from block 0x200 + j, or a sample towards the map or
                    a listed triangle with blocks 3 + 2 j and 4 + 2 j"""
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
                            rec_ = PL[k]
                            v = rec_[:, 0:3] - pos[cp_]
                            dist2 = _dot(v, v)
                            with np.errstate(all="ignore"):
                                dist = np.sqrt(dist2)
                                wdir = v / dist[:, None]
                                cd = _dot(rec_[:, 4:7], -wdir)
                                sm = _clamp((cd - rec_[:, 12]) / _fmax2(rec_[:, 11] - rec_[:, 12], f32(1e-6)), f32(0), f32(1))
                                att = np.where(rec_[:, 7] != 0, sm * sm, f32(1)).astype(f32)
                                E = (rec_[:, 8:11] * att[:, None]) / dist2[:, None]
                                ok = ((dist2 > 0) & (_dot(normal[cp_], wdir) > 0) & (ppmf[k] > 0) & ((rec_[:, 3] == 0) | (dist <= rec_[:, 3])) & (att > 0)
                                      & (_fmax2(E[:, 0], _fmax2(E[:, 1], E[:, 2])) > 0))
                            oi = np.flatnonzero(ok)
                            if len(oi):
                                c2 = cp_[oi]
                                brdf, pdf = _eval_brdf(ora, normal[c2], outc[c2], wdir[oi], albedo[c2], rough[c2], metallic[c2], spec_prob[c2], ior[c2])
                                pe = _fmax2(pdf, EPS)
                                qc = _clamp(brdf / pe[:, None], f32(0), f32(1))
                                b = qc * pe[:, None]
                                den = ppmf[k[oi]] if "forget_cp" in wrong else c_p * ppmf[k[oi]]
                                idx = pi[oi]
                                X[idx] = ((T[g[c2]] * b) * E[oi]) / den[:, None]
                                Wd[idx], kind[idx], LD[idx], okc[idx] = wdir[oi], KIND_PUNCTUAL, dist[oi], True
                    r, to_env = None, np.zeros(nc, bool)
                    if n_l:
                        r = draws(ora, pixel[gc], sample[gc], dep[ci], pa[ci], BLOCK_LIGHT + 2 * j, seed)
                        if light_draws is not None:
                            light_draws.append(np.stack([pixel[gc], sample[gc], dep[ci], pa[ci]], -1).astype(np.uint32))
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
                        same = (fi == bi) & (fj == bj)
                        stats["env_samples"] += len(ei)
                        stats["env_rejected_box"] += int((~same).sum())
                        p = env_pdf(tab, wdir, fuv)
                        ok = same & (_dot(normal[ce], wdir) > 0) & (p > 0) & (_fmax2(Le[:, 0], _fmax2(Le[:, 1], Le[:, 2])) > 0)
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
                            wl = np.ones(len(oi), f32) if "no_mis" in wrong else pw / (pw + p_l)
                            idx = li[oi]
                            X[idx] = ((T[g[c2]] * qc) * wl[:, None]) * Le[oi]
                            Wd[idx], LS[idx], LT[idx], okc[idx] = wdir[oi], ls[oi], lt[oi], True
                    return okc, X, Wd, kind, LS, LT, LD

                if M == 1:   # the call without the bits: the one sample as it is
                    chosen, cX, cWd, cKind, cLS, cLT, cLD = candidate(0)
                else:
                    chosen, cX, cWd = np.zeros(nc, bool), np.zeros((nc, 3), f32), np.zeros((nc, 3), f32)
                    cKind, cLS, cLT, cLD = np.zeros(nc, np.int64), np.zeros(nc, np.int64), np.zeros(nc, np.int64), np.zeros(nc, f32)
                    wsum, Wy, n_kept = np.zeros(nc, f32), np.ones(nc, f32), np.zeros(nc, np.int64)
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
                        n_kept += keep
                    denom = np.maximum(n_kept, 1).astype(f32) if "kept_div" in wrong else f32(M)
                    cX = cX * ((wsum / denom) / Wy)[:, None]
                yi = np.flatnonzero(chosen)
                if len(yi):
                    c2 = ci[yi]
                    rays = np.concatenate([pos[c2] + cWd[yi] * EPS, cWd[yi]], 1)
                    _, hs, ht, hd = _closest(o, model_of, rays)
                    stats["rays"] += len(yi)
                    to_map = cKind[yi] == KIND_ENV
                    vis = np.where(to_map, hs < 0, (hs == cLS[yi]) & (ht == cLT[yi]))
                    vis = np.where(cKind[yi] == KIND_PUNCTUAL, (hs < 0) | ~(hd < cLD[yi]), vis)   # nothing nearer than the light
                    stats["light_samples"] += len(yi)
                    stats["light_visible"] += int(vis.sum())
                    if "no_light_term" not in wrong:
                        L[g[c2[vis]]] = L[g[c2[vis]]] + cX[yi][vis]
                    if first_env is not None and "ids" not in first_env and to_map.any():
                        z = to_map & (dep[c2] == 0)
                        first_env.update(ids=g[c2[z]].copy(), wdir=cWd[yi][z].copy(), x=cX[yi][z].copy(), visible=vis[z].copy())
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
                R["cont"][hi[c2]] = True
                R["brdf"][hi[c2]] = brdf
                R["pe"][hi[c2]] = pe
        live = live[nxt]

    if fold == "recursive":
        val = np.zeros((N, 3), f32)
        for R in reversed(rec):
            ids, kind = R["ids"], R["kind"]
            val[ids[kind == 0]] = 0
            val[ids[kind == 1]] = R["env"][kind == 1]
            v = kind == 3
            iv = ids[v]
            inn = val[iv]
            with np.errstate(all="ignore"):
                ind = _clamp((R["brdf"][v] * inn) / R["pe"][v][:, None], f32(0), inn)
            ind = np.where(R["cont"][v][:, None], ind, f32(0)).astype(f32)
            val[iv] = (R["dsun"][v] + ind) + R["e"][v]
        L = val
    res = dict(rad=L.reshape(spp, h, w, 3).transpose(1, 2, 0, 3).copy(), v1_listed=v1_listed.reshape(spp, h, w).transpose(1, 2, 0).copy())
    res.update(stats)
    return res
