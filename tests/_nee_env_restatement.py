"""numpy restatement of PTX_NEE_ENV_SAMPLES (include/ptx.h: THE ENVIRONMENT TABLE, THE PDF, SELECTION, ENVIRONMENT SAMPLE, MISS WEIGHT), for
tests/test_nee_env.py. Built on tests/_nee_restatement.py: the vertex is that file's, statement for statement, with the flagged
estimator's changes written in; (u, v) and Le of a direction come from the oracle's env_lookup.

build_tables: the table from the texels in float64, as the specification words it (np.roll for the wrapped 3 x 3 footprint).
env_pdf / sample_env: the pdf and the sampler on float32 arrays in the specification's operation order. cos and sin of the sampled
direction are float64 values rounded to float32 (the product's are ocml's cosf / sinf: last-place differences).
render_samples: per-sample radiance. tab=None is the unflagged estimator (delegates to _nee_restatement.render_samples). Switches that
break the estimator on purpose: miss_weight=False sets wm = 1 (the map's radiance is counted twice), use_c_env=False computes every
weight with c_env = 1 while the selection still splits the vertices (energy is lost where both strategies exist).

R0: the ratio of flagged to unflagged per-sample variance that test_nee_env.test_expectation_and_variance_on_the_restatement measures on
VARIANCE_CASE; the GPU test's bar is 2 * R0.
"""
import struct

import numpy as np

import _nee_restatement as R
from _nee_restatement import (BLOCK_LIGHT, BLOCK_SUN, BLOCK_SURFACE, EPS, _Attr, _clamp, _closest, _dot, _eval_brdf, _fmax2, _lerp, _material,
                              _mulmv, _normalize, _pbr, _shading_normal, draws, f32, light_list)

BLOCK_ENV = 4
KU, KV = f32(0.1591), f32(0.3183)

# the scene, frame and map of the variance comparison (CPU: the restatement, GPU: the product), and the restatement's measured ratio
VARIANCE_CASE = dict(name="chart", W=24, H=16, spp=64, bounces=3, seed=0x5EED, env=(1.0, 1.0, 1.0))
R0 = 0.2321   # measured on the restatement; the CPU test recomputes it and holds it to this figure


# ---------------------------------------------------------------------------- maps
def write_hdr(path, rgb):
    """rgb [h, w, 3] float -> an uncompressed (flat) Radiance .hdr file; returns the path. Values are chosen by the tests so that no
    scanline begins with the bytes (2, 2), which would announce a run-length coded line."""
    rgb = np.asarray(rgb, np.float64)
    h, w, _ = rgb.shape
    out = bytearray(b"#?RADIANCE\nFORMAT=32-bit_rle_rgbe\n\n" + f"-Y {h} +X {w}\n".encode())
    for row in rgb:
        for px in row:
            m = float(px.max())
            if m < 1e-32:
                out += bytes(4)
                continue
            mant, ex = np.frexp(m)
            sc = mant * 256.0 / m
            out += struct.pack("4B", int(px[0] * sc), int(px[1] * sc), int(px[2] * sc), int(ex) + 128)
    with open(path, "wb") as f:
        f.write(bytes(out))
    return str(path)


def hot_texel(w=16, h=8, base=0.05, hot=400.0, at=(0, 0)):
    """a dim grey map with one hot texel (column, row) — in a corner the wrapped 3 x 3 footprint reaches both opposite edges"""
    rgb = np.full((h, w, 3), base)
    rgb[at[1], at[0]] = (hot, hot * 0.9, hot * 0.7)
    return rgb


def map_pixels(ptx, s):
    """[h, w, 3] float32: rgb of the scene's environment texels as the kernels' tex_pixel reads them (the last texture of the arrays: sRGB
    table for 8-bit texels, powf for float ones, missing channels 1), or None without a map."""
    tex = s.array(ptx.ARR_TEXTURES).reshape(-1, 4)
    if not len(tex):
        return None
    w, h, cs, off = [int(x) for x in tex[-1]]
    c, srgb, is_f = cs & 255, bool(cs & 0x100), bool(cs & 0x10000)
    if is_f:
        raw = s.array(ptx.ARR_TEXELS_F32)[off:off + w * h * c].reshape(h, w, c).astype(f32)
    else:
        raw = s.array(ptx.ARR_TEXELS)[off:off + w * h * c].reshape(h, w, c).astype(f32) / f32(255)
    with np.errstate(all="ignore"):
        lin = np.power(raw, f32(2.2)) if srgb else raw
    out = np.ones((h, w, 3), f32)
    k = min(c, 3)
    out[..., :k] = lin[..., :k]
    return out


def build_tables(pix):
    """pix [h, w, 3] -> (row_cdf float32 [h], cell_cdf float32 [h, w]); two empty arrays for a black map or None"""
    if pix is None:
        return np.zeros(0, f32), np.zeros((0, 0), f32)
    p = np.asarray(pix, np.float64)
    h, w, _ = p.shape
    lum = (0.2126 * p[..., 0] + 0.7152 * p[..., 1]) + 0.0722 * p[..., 2]
    lum = np.where(lum > 0, lum, 0.0)
    foot = sum(np.roll(lum, (-dj, -di), (0, 1)) for dj in (-1, 0, 1) for di in (-1, 0, 1))
    lat = ((1.0 - (np.arange(h) + 0.5) / h) - 0.5) / 0.3183
    wgt = foot * np.maximum(np.cos(lat), 0.0)[:, None]
    mass = wgt.sum(1)
    total = mass.sum()
    if not total > 0:
        return np.zeros(0, f32), np.zeros((0, 0), f32)
    row = (np.cumsum(mass) / total).astype(f32)
    row[-1] = 1
    cell = np.zeros((h, w), f32)
    nz = mass > 0
    cell[nz] = (np.cumsum(wgt[nz], 1) / mass[nz, None]).astype(f32)
    cell[nz, -1] = 1
    return row, cell


def table(row, cell):
    """the dict the functions below take, from the two arrays (the product's PTX_ARR_ENV_* or build_tables'); None when they are empty"""
    row = np.asarray(row, f32).reshape(-1)
    if not len(row):
        return None
    cell = np.asarray(cell, f32).reshape(len(row), -1)
    return dict(row=row, cell=cell, w=cell.shape[1], h=len(row))


# ---------------------------------------------------------------------------- the pdf and the sampler
def env_box(tab, uv):
    """box (i, j) of the lookup's (u, v) [n, 2]"""
    w, h = tab["w"], tab["h"]
    with np.errstate(all="ignore"):
        fi = np.nan_to_num(uv[:, 0] * f32(w), nan=0.0, posinf=0.0, neginf=0.0)
        fj = np.nan_to_num((f32(1) - uv[:, 1]) * f32(h), nan=0.0, posinf=0.0, neginf=0.0)
    return np.minimum(np.maximum(fi, 0).astype(np.int64), w - 1), np.minimum(np.maximum(fj, 0).astype(np.int64), h - 1)


def box_probability(tab, i, j):
    """P of box (i, j) from the stored float32 differences"""
    row, cell = tab["row"], tab["cell"]
    pr = row[j] - np.where(j > 0, row[np.maximum(j - 1, 0)], f32(0)).astype(f32)
    pc = cell[j, i] - np.where(i > 0, cell[j, np.maximum(i - 1, 0)], f32(0)).astype(f32)
    return (pr * pc).astype(f32)


def env_pdf(tab, d, uv):
    """env_pdf of directions d [n, 3] whose lookup coordinates are uv [n, 2] -> float32 [n]"""
    i, j = env_box(tab, uv)
    P = box_probability(tab, i, j)
    with np.errstate(all="ignore"):
        c = np.sqrt(_fmax2(f32(0), f32(1) - d[:, 1] * d[:, 1]))
        p = ((P * f32(tab["w"] * tab["h"])) * (KU * KV)) / c
    return np.where(c > 0, p, f32(0)).astype(f32)


def sample_env(tab, q):
    """q [n, 4] float32 draws -> (i, j, w_dir [n, 3] float32)"""
    w, h = tab["w"], tab["h"]
    j = np.minimum(np.searchsorted(tab["row"], q[:, 0], side="right"), h - 1)
    i = np.zeros(len(q), np.int64)
    for jj in np.unique(j):
        sel = j == jj
        i[sel] = np.minimum(np.searchsorted(tab["cell"][jj], q[sel, 1], side="right"), w - 1)
    u = (i.astype(f32) + q[:, 2]) / f32(w)
    v = f32(1) - (j.astype(f32) + q[:, 3]) / f32(h)
    phi, lat = (u - f32(0.5)) / KU, (v - f32(0.5)) / KV
    cl, sl = np.cos(lat.astype(np.float64)).astype(f32), np.sin(lat.astype(np.float64)).astype(f32)
    cp, sp = np.cos(phi.astype(np.float64)).astype(f32), np.sin(phi.astype(np.float64)).astype(f32)
    return i, j, np.stack([cl * cp, sl, cl * sp], -1).astype(f32)


# ---------------------------------------------------------------------------- the estimator
def render_samples(ora, o, a, W, H, spp, bounces, tab, seed=0x5EED, env=(1.0, 1.0, 1.0), tile=None, sample0=0, lights=True, miss_weight=True,
                   use_c_env=True, first_env=None):
    """-> dict(rad [h, w, spp, 3] float32, light_samples, light_visible, rays, env_samples, env_rejected_box). tab: table() of the map that
    the oracle scene `o` has been given with set_environment, or None for the unflagged estimator. first_env: None, or a dict that receives
    the depth-0 environment samples: ids (sample ids: s * n_pixels + p), wdir, x, visible."""
    if tab is None:
        r = R.render_samples(ora, o, a, W, H, spp, bounces, seed=seed, env=env, tile=tile, sample0=sample0, lights=lights)
        r.update(env_samples=0, env_rejected_box=0)
        return r
    assert getattr(o, "_env", None) is not None
    x0, y0, w, h = tile if tile else (0, 0, W, H)
    npix, N = w * h, w * h * spp
    env = np.asarray(env, f32)
    attr = _Attr(a)
    model_of = attr.model_of
    mats = np.asarray(a.materials, f32)
    ll = light_list(a) if lights else dict(tris=np.zeros((0, 2), np.uint32), cdf=np.zeros(0, f32), geom=np.zeros((0, 4), f32), area=f32(0),
                                           surf_first=np.full(len(mats), -1, np.int32))
    n_l = len(ll["cdf"])
    c_sel = f32(0.5) if n_l else f32(1)              # the selection's share
    c_env = c_sel if use_c_env else f32(1)           # what the weights use
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
    stats = dict(light_samples=0, light_visible=0, rays=0, env_samples=0, env_rejected_box=0)

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
        if miss.any():   # ---- miss: the map's radiance, weighted against the environment sample of the previous vertex
            gm = live[miss]
            uv, _, col = o.env_lookup(D[gm], env)
            add = T[gm] * col
            wsel = (depth[gm] != 0) & (pas[gm] == 0)
            if wsel.any() and miss_weight:
                pp = PP[gm[wsel]]
                wm = pp / (pp + c_env * env_pdf(tab, D[gm[wsel]], uv[wsel]))
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
            # ---- emission: p_l becomes (1 - c_env) * p_l
            ai = np.flatnonzero(act)
            ga = g[ai]
            em = T[ga] * e10[ai]
            wsel = (k_l[ai] >= 0) & (dep[ai] != 0) & (pa[ai] == 0)
            if wsel.any():
                kk = k_l[ai][wsel]
                cg = np.abs(_dot(ll["geom"][kk, 0:3], d[ai][wsel]))
                with np.errstate(all="ignore"):
                    p_l = (f32(1) - c_env) * ((di[ai][wsel] * di[ai][wsel]) / (cg * ll["area"]))
                    wgt = PP[ga[wsel]] / (PP[ga[wsel]] + p_l)
                em[wsel] = em[wsel] * wgt[:, None]
            L[ga] = L[ga] + em
            sa = np.flatnonzero(add)
            L[g[sa]] = L[g[sa]] + sun_add[sa]
            # ---- the light sample: towards the map, or towards a triangle
            ci = ai[~last[ai]]
            gc = g[ci]
            if len(ci):
                if n_l:
                    r = draws(ora, pixel[gc], sample[gc], dep[ci], pa[ci], BLOCK_LIGHT, seed)
                    to_env = r[:, 3] < f32(0.5)
                else:
                    r, to_env = None, np.ones(len(ci), bool)
                ei = np.flatnonzero(to_env)
                if len(ei):
                    ce = ci[ei]
                    q = draws(ora, pixel[g[ce]], sample[g[ce]], dep[ce], pa[ce], BLOCK_ENV, seed)
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
                        wl = pe / (pe + c_env * p[oi])
                        x = ((T[g[c2]] * qc) * wl[:, None]) * Le[oi]
                        _, hs = o.intersect(np.concatenate([pos[c2] + wdir[oi] * EPS, wdir[oi]], 1))
                        stats["rays"] += len(oi)
                        vis = hs < 0
                        stats["light_samples"] += len(oi)
                        stats["light_visible"] += int(vis.sum())
                        L[g[c2[vis]]] = L[g[c2[vis]]] + x[vis]
                        if first_env is not None and "ids" not in first_env:
                            z = dep[c2] == 0
                            first_env.update(ids=g[c2[z]].copy(), wdir=wdir[oi][z].copy(), x=x[z].copy(), visible=vis[z].copy())
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
                        p_l = (f32(1) - c_env) * (dist2[oi] / (cg[oi] * ll["area"]))
                        wl = pe / (pe + p_l)
                        x = ((T[g[c2]] * qc) * wl[:, None]) * Le[oi]
                        _, hs, ht, _ = _closest(o, model_of, np.concatenate([pos[c2] + wdir[oi] * EPS, wdir[oi]], 1))
                        stats["rays"] += len(oi)
                        vis = (hs == ls[oi]) & (ht == lt[oi])
                        stats["light_samples"] += len(oi)
                        stats["light_visible"] += int(vis.sum())
                        L[g[c2[vis]]] = L[g[c2[vis]]] + x[vis]
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
                PP[g[c2]] = pe
                O[g[c2]] = pos[c2] + inc[oi] * EPS
                D[g[c2]] = _normalize(inc[oi])
                depth[g[c2]] = dep[c2] + 1
                pas[g[c2]] = 0
                nxt[hi[c2]] = depth[g[c2]] != bounces
        live = live[nxt]

    res = dict(rad=L.reshape(spp, h, w, 3).transpose(1, 2, 0, 3).copy())
    res.update(stats)
    return res
