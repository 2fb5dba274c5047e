"""numpy float32 wavefront restatement of ptx_render_nee's estimator and light list (include/ptx.h), for tests/test_nee.py.

Built on the oracle's batch primitives only: OracleScene.intersect (closest hit: position, uv, shading normal, surface),
OracleScene.model_intersect (the same hit's triangle index and distance: the closest hit inside the model of the surface that
OracleScene.intersect reported is that hit), material_eval, primary_rays, pt_oracle.pbr (importance samples, pdfs, Fresnel: every call
that goes through libm), pt_oracle.philox and the scene arrays. Everything else is written out here on np.float32 arrays in the
operation order of the specification (numpy neither contracts nor reorders).

Switches: lights=False runs with an empty list (LIB itself), mis=False sets every weight to 1 (double counting), light_term=False
drops the light term but keeps the weights (energy lost). fold="recursive" (lights=False only) adds a path's vertices back to front
as renderer::trace returns them, which is what OracleScene.render_samples computes bit for bit; fold="throughput" is the product's
order: vertex k's emission, its sun term, its light term, then vertex k + 1.

A miss adds T * env; when the oracle scene has an environment map (OracleScene.set_environment), env is OracleScene.env_lookup of the
ray's direction times the factor, per ray (renderer.cpp:443-449).
"""
import numpy as np

f32 = np.float32
EPS = f32(0.0001)
BLOCK_SURFACE, BLOCK_SUN, BLOCK_JITTER, BLOCK_LIGHT = 0, 1, 2, 3


# ---------------------------------------------------------------------------- float32 helpers (oracle/pt_oracle.cpp:44-72)
def _dot(a, b):
    return a[..., 0] * b[..., 0] + a[..., 1] * b[..., 1] + a[..., 2] * b[..., 2]


def _cross(l, r):
    return np.stack([(l[..., 1] * r[..., 2]) - (l[..., 2] * r[..., 1]), (l[..., 2] * r[..., 0]) - (l[..., 0] * r[..., 2]),
                     (l[..., 0] * r[..., 1]) - (l[..., 1] * r[..., 0])], -1)


def _normalize(a):
    with np.errstate(all="ignore"):
        return a * (f32(1) / np.sqrt(_dot(a, a)))[..., None]


def _fmax2(a, b):   # b > a ? b : a
    return np.where(b > a, b, a).astype(f32)


def _fmin2(a, b):   # b < a ? b : a
    return np.where(b < a, b, a).astype(f32)


def _clamp(x, lo, hi):
    return _fmin2(_fmax2(x, lo), hi)


def _lerp(a, b, w):
    return a + (b - a) * w


def _mulmv(cols, v):
    """mat3 * v with the matrix given as its three columns [..., 3] each: the dot of each ROW with v."""
    bx, by, bz = cols
    return bx * v[..., 0:1] + by * v[..., 1:2] + bz * v[..., 2:3]


def draws(ora, pixel, sample, depth, pas, block, seed):
    n = len(pixel)
    ctr = np.stack([pixel.astype(np.uint32), sample.astype(np.uint32), ((depth.astype(np.uint32) << 16) | np.minimum(pas, 0xFFFF).astype(np.uint32)),
                    np.full(n, block, np.uint32)], -1)
    key = np.tile(np.array([seed & 0xFFFFFFFF, (seed >> 32) & 0xFFFFFFFF], np.uint32), (n, 1))
    r = ora.philox(ctr, key)
    return (r >> 8).astype(f32) * f32(1.0 / 16777216.0)


# ---------------------------------------------------------------------------- the light list (include/ptx.h: THE LIGHT LIST)
def light_list(a):
    """a: the scene arrays (pt_oracle.SceneArrays, or any object with the same fields). -> dict(tris uint32 [n, 2], cdf float32 [n],
    geom float32 [n, 4], area float32, surf_first int32 [n_surf])."""
    mats = np.asarray(a.materials, f32)
    n_surf = len(mats)
    surf_tex = getattr(a, "surf_tex", None)
    model_of = np.zeros(n_surf, np.int64)
    for m, (first, cnt) in enumerate(np.asarray(a.model_surf)):
        model_of[first:first + cnt] = m
    tris, geom, cum, first_of = [], [], [], np.full(n_surf, -1, np.int32)
    total = np.float64(0)
    for s in range(n_surf):
        em, op, catcher = mats[s, 6:9], mats[s, 3], mats[s, 10]
        if not (em > 0).any():
            continue
        op_tex = surf_tex is not None and surf_tex[s][2] >= 0
        if op_tex or not (op == f32(1) or abs(f32(op - f32(1))) < EPS) or catcher != 0:
            continue
        X = np.asarray(a.model_xform, f32)[model_of[s]].astype(np.float64)
        v0, _, t0, nt = [int(x) for x in np.asarray(a.surf_range)[s][:4]]
        for t in range(nt):
            c = []
            for k in range(3):
                v = np.asarray(a.vertices, f32)[v0 + int(a.triangles[t0 + t][k])].astype(np.float64)
                c.append(np.array([(X[3 + j] * v[0] + X[6 + j] * v[1]) + X[9 + j] * v[2] + X[j] for j in range(3)]))
            e1, e2 = c[1] - c[0], c[2] - c[0]
            cr = np.array([e1[1] * e2[2] - e1[2] * e2[1], e1[2] * e2[0] - e1[0] * e2[2], e1[0] * e2[1] - e1[1] * e2[0]])
            ln = np.sqrt((cr[0] * cr[0] + cr[1] * cr[1]) + cr[2] * cr[2])
            area = 0.5 * ln
            if not area > 0:
                continue
            if first_of[s] < 0:
                first_of[s] = len(tris)
            tris.append([s, t])
            geom.append([f32(cr[0] / ln), f32(cr[1] / ln), f32(cr[2] / ln), f32(area)])
            total = total + area
            cum.append(total)
    cdf = np.array([f32(v / total) for v in cum], f32)
    if len(cdf):
        cdf[-1] = f32(1)
    return dict(tris=np.array(tris, np.uint32).reshape(-1, 2), cdf=cdf, geom=np.array(geom, f32).reshape(-1, 4), area=f32(total),
                surf_first=first_of)


# ---------------------------------------------------------------------------- hit attributes at a barycentric point (renderer.cpp:688-715)
class _Attr:
    def __init__(self, a):
        X = np.asarray(a.model_xform, f32)
        n_surf = len(a.surf_range)
        model_of = np.zeros(n_surf, np.int64)
        for m, (first, cnt) in enumerate(np.asarray(a.model_surf)):
            model_of[first:first + cnt] = m
        self.model_of = model_of
        self.origin, self.bx, self.by, self.bz = X[:, 0:3], X[:, 3:6], X[:, 6:9], X[:, 9:12]
        # inverse(basis) (mat3.inl:245-263) as columns; the normal matrix is its transpose, so normal_matrix * v = the dot of each COLUMN of the inverse with v
        x, y, z = self.bx, self.by, self.bz
        det1 = +(y[:, 1] * z[:, 2] - z[:, 1] * y[:, 2])
        det2 = -(x[:, 1] * z[:, 2] - z[:, 1] * x[:, 2])
        det3 = +(x[:, 1] * y[:, 2] - y[:, 1] * x[:, 2])
        det = x[:, 0] * det1 + y[:, 0] * det2 + z[:, 0] * det3
        s = f32(1) / det
        c0 = np.stack([det1, det2, det3], -1)
        c1 = np.stack([-(y[:, 0] * z[:, 2] - z[:, 0] * y[:, 2]), +(x[:, 0] * z[:, 2] - z[:, 0] * x[:, 2]), -(x[:, 0] * y[:, 2] - y[:, 0] * x[:, 2])], -1)
        c2 = np.stack([+(y[:, 0] * z[:, 1] - z[:, 0] * y[:, 1]), -(x[:, 0] * z[:, 1] - z[:, 0] * x[:, 1]), +(x[:, 0] * y[:, 1] - y[:, 0] * x[:, 1])], -1)
        self.inv = [c0 * s[:, None], c1 * s[:, None], c2 * s[:, None]]
        self.verts = np.asarray(a.vertices, f32)
        self.tris = np.asarray(a.triangles, np.int64)
        self.range = np.asarray(a.surf_range, np.int64)[:, :4]

    def at(self, surf, tri, b1, b2):
        """-> pos, uv, nrm, tan of the point (1 - b1 - b2, b1, b2) of triangle `tri` of surface `surf` (arrays)."""
        b0 = f32(1) - b1 - b2
        ids = self.range[surf, 0][:, None] + self.tris[self.range[surf, 2] + tri]
        v1, v2, v3 = self.verts[ids[:, 0]], self.verts[ids[:, 1]], self.verts[ids[:, 2]]

        def mix(lo, hi):
            return v1[:, lo:hi] * b0[:, None] + v2[:, lo:hi] * b1[:, None] + v3[:, lo:hi] * b2[:, None]
        m = self.model_of[surf]
        pos = _mulmv((self.bx[m], self.by[m], self.bz[m]), mix(0, 3)) + self.origin[m]
        uv = mix(3, 5)

        def nmul(v):
            return np.stack([_dot(self.inv[0][m], v), _dot(self.inv[1][m], v), _dot(self.inv[2][m], v)], -1)
        return pos, uv, _normalize(nmul(mix(5, 8))), _normalize(nmul(mix(8, 11)))


def _shading_normal(nrm, tan, nts):
    b = _cross(nrm, tan)
    return tan * nts[:, 0:1] + b * nts[:, 1:2] + nrm * nts[:, 2:3]


def _material(o, surf, uv):
    """material_eval per hit -> [n, 12]: normal_ts(3) albedo(3) opacity roughness metallic emissive(3)"""
    out = np.zeros((len(surf), 12), f32)
    for s in np.unique(surf):
        sel = surf == s
        out[sel] = o.material_eval(int(s), uv[sel])
    return out


def _closest(o, model_of, rays):
    """Closest hits of world rays -> (out [n, 14], surface [n] or -1, triangle [n], distance [n])."""
    out, surf = o.intersect(rays)
    tri = np.full(len(rays), -1, np.int64)
    dist = np.full(len(rays), -1, f32)
    hit = surf >= 0
    for m in np.unique(model_of[surf[hit]]):
        sel = hit & (model_of[np.maximum(surf, 0)] == m)
        mo, mi = o.model_intersect(int(m), rays[sel])
        assert (mi[:, 0] == surf[sel]).all()
        tri[sel] = mi[:, 1]
        dist[sel] = mo[:, 0]
    return out, surf, tri, dist


def _pbr(ora, n, outc, inc, u1, u2, rough, ct, ior):
    k = len(n)
    inp = np.zeros((k, 14), f32)
    inp[:, 0:3], inp[:, 3:6], inp[:, 6:9] = n, outc, inc
    inp[:, 9], inp[:, 10], inp[:, 11], inp[:, 12], inp[:, 13] = u1, u2, rough, ct, ior
    with np.errstate(all="ignore"):
        return ora.pbr(inp)


def _eval_brdf(ora, n, outc, inc, albedo, rough, metallic, spec_prob, ior):
    """BRDF / PDF combination of renderer::trace (renderer.cpp:521-556, 579-606) -> brdf [k, 3], pdf [k]"""
    pb = _pbr(ora, n, outc, inc, 0, 0, rough, 1, ior)
    dpdf, spdf = pb[:, 9], pb[:, 10]
    with np.errstate(all="ignore"):
        dbrdf = dpdf[:, None] * albedo
        fr = _lerp(f32(0.04), albedo, metallic[:, None])
        halfway = _normalize(outc + inc)
        cos_theta = _dot(outc, halfway)
        p5 = np.power((f32(1) - cos_theta).astype(np.float64), 5.0).astype(f32)
        fr = _lerp(fr, f32(1), p5[:, None])
        dbrdf = _lerp(dbrdf, f32(0), metallic[:, None])
        brdf = _lerp(dbrdf, spdf[:, None], fr)
        pdf = _lerp(dpdf, spdf, spec_prob)
    return brdf.astype(f32), pdf.astype(f32)


# ---------------------------------------------------------------------------- the estimator
def render_samples(ora, o, a, W, H, spp, bounces, seed=0x5EED, env=(1.0, 1.0, 1.0), tile=None, sample0=0, lights=True, mis=True,
                   light_term=True, fold="throughput", light_draws=None):
    """-> dict(rad [h, w, spp, 3] float32 per-sample radiance, v1_listed [h, w, spp] bool: the sample's vertex at depth 1 lies on a listed
    triangle, light_samples, light_visible, rays). light_draws: None, or a list that receives, per round, the Philox keys (pixel, sample,
    depth, pass: uint32 [n, 4]) of the vertices that drew a light sample, accepted or not."""
    assert fold in ("throughput", "recursive") and (fold == "throughput" or not lights)
    x0, y0, w, h = tile if tile else (0, 0, W, H)
    npix, N = w * h, w * h * spp
    env = np.asarray(env, f32)
    env_map = getattr(o, "_env", None) is not None
    attr = _Attr(a)
    model_of = attr.model_of
    mats = np.asarray(a.materials, f32)
    ll = light_list(a) if lights else dict(tris=np.zeros((0, 2), np.uint32), cdf=np.zeros(0, f32), geom=np.zeros((0, 4), f32), area=f32(0),
                                           surf_first=np.full(len(mats), -1, np.int32))
    n_l = len(ll["cdf"])
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
    stats = dict(light_samples=0, light_visible=0, rays=0)

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
        R = dict(ids=live, kind=np.zeros(len(live), np.int8), e=np.zeros((len(live), 3), f32), dsun=np.zeros((len(live), 3), f32), env=env,
                 brdf=np.zeros((len(live), 3), f32), pe=np.ones(len(live), f32), cont=np.zeros(len(live), bool))   # kind 0 zero, 1 miss, 2 pass, 3 vertex
        rec.append(R)
        miss = surf < 0
        if env_map and miss.any():
            R["env"] = np.zeros((len(live), 3), f32)
            R["env"][miss] = o.env_lookup(D[live[miss]], env)[2]
            L[live[miss]] = L[live[miss]] + T[live[miss]] * R["env"][miss]
        else:
            L[live[miss]] = L[live[miss]] + T[live[miss]] * env
        R["kind"][miss] = 1
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
            # ---- emission, sun
            ai = np.flatnonzero(act)
            ga = g[ai]
            em = T[ga] * e10[ai]
            wsel = (k_l[ai] >= 0) & (dep[ai] != 0) & (pa[ai] == 0)
            if wsel.any() and mis:
                kk = k_l[ai][wsel]
                cg = np.abs(_dot(ll["geom"][kk, 0:3], d[ai][wsel]))
                with np.errstate(all="ignore"):
                    p_l = (di[ai][wsel] * di[ai][wsel]) / (cg * ll["area"])
                    wgt = PP[ga[wsel]] / (PP[ga[wsel]] + p_l)
                em[wsel] = em[wsel] * wgt[:, None]
            L[ga] = L[ga] + em
            sa = np.flatnonzero(add)
            L[g[sa]] = L[g[sa]] + sun_add[sa]
            R["kind"][hi[ai]] = 3
            R["e"][hi[ai]] = e10[ai]
            R["dsun"][hi[ai]] = sun_raw[ai]
            # ---- the vertices that sample a direction
            ci = ai[~last[ai]]
            gc = g[ci]
            if n_l and len(ci):
                r = draws(ora, pixel[gc], sample[gc], dep[ci], pa[ci], BLOCK_LIGHT, seed)
                if light_draws is not None:
                    light_draws.append(np.stack([pixel[gc], sample[gc], dep[ci], pa[ci]], -1).astype(np.uint32))
                k = np.minimum(np.searchsorted(ll["cdf"], r[:, 0], side="right"), n_l - 1)
                su = np.sqrt(r[:, 1])
                beta, gamma = su * (f32(1) - r[:, 2]), su * r[:, 2]
                ls, lt = ll["tris"][k, 0].astype(np.int64), ll["tris"][k, 1].astype(np.int64)
                ypos, yuv, ynrm, ytan = attr.at(ls, lt, beta, gamma)
                my = _material(o, ls, yuv)
                n_y, Le = _shading_normal(ynrm, ytan, my[:, 0:3]), my[:, 9:12] * f32(10)
                v = ypos - pos[ci]
                dist2 = _dot(v, v)
                with np.errstate(all="ignore"):
                    wdir = v / np.sqrt(dist2)[:, None]
                    cg = np.abs(_dot(ll["geom"][k, 0:3], wdir))
                    ok = (dist2 > 0) & (_dot(normal[ci], wdir) > 0) & (_dot(n_y, -wdir) > 0) & (cg > 0) & (_fmax2(Le[:, 0], _fmax2(Le[:, 1], Le[:, 2])) > 0)
                oi = np.flatnonzero(ok)
                if len(oi):
                    c2 = ci[oi]
                    brdf, pdf = _eval_brdf(ora, normal[c2], outc[c2], wdir[oi], albedo[c2], rough[c2], metallic[c2], spec_prob[c2], ior[c2])
                    pe = _fmax2(pdf, EPS)
                    qc = _clamp(brdf / pe[:, None], f32(0), f32(1))
                    p_l = dist2[oi] / (cg[oi] * ll["area"])
                    wl = pe / (pe + p_l) if mis else np.ones(len(oi), f32)
                    x = ((T[g[c2]] * qc) * wl[:, None]) * Le[oi]
                    _, hs, ht, _ = _closest(o, model_of, np.concatenate([pos[c2] + wdir[oi] * EPS, wdir[oi]], 1))
                    stats["rays"] += len(oi)
                    vis = (hs == ls[oi]) & (ht == lt[oi])
                    stats["light_samples"] += len(oi)
                    stats["light_visible"] += int(vis.sum())
                    if light_term:
                        L[g[c2[vis]]] = L[g[c2[vis]]] + x[vis]
            if len(ci):
                spec = rnd[ci, 1] < spec_prob[ci]
                inc = np.where(spec[:, None], pb[ci, 6:9], pb[ci, 3:6])
                ok = _dot(normal[ci], inc) > 0
                oi = np.flatnonzero(ok)
                c2 = ci[oi]
                brdf, pdf = _eval_brdf(ora, normal[c2], outc[c2], inc[oi], albedo[c2], rough[c2], metallic[c2], spec_prob[c2], ior[c2])
                pe = _fmax2(pdf, EPS)
                with np.errstate(all="ignore"):
                    q = brdf / pe[:, None]
                T[g[c2]] = T[g[c2]] * _clamp(q, f32(0), f32(1))
                PP[g[c2]] = pe
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
            val[ids[kind == 1]] = R["env"] if R["env"].ndim == 1 else R["env"][kind == 1]
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
