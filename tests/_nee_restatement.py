"""What tests/_nee_estimator.py's vertex is built from, in numpy float32: the float32 helpers (oracle/pt_oracle.cpp:44-72), the Philox draws,
the light list (include/ptx.h: THE LIGHT LIST), the attributes of a point of a triangle (renderer.cpp:688-715), the material and closest-hit
batches over the oracle, and the BRDF / PDF combination of renderer::trace (renderer.cpp:521-556, 579-606). Not collected (underscore prefix).

Built on the oracle's batch primitives only: OracleScene.intersect (closest hit: position, uv, shading normal, surface),
OracleScene.model_intersect (the same hit's triangle index and distance: the closest hit inside the model of the surface that
OracleScene.intersect reported is that hit), material_eval, pt_oracle.pbr (importance samples, pdfs, Fresnel: every call that goes through
libm), pt_oracle.philox and the scene arrays. Everything else is written out here on np.float32 arrays in the operation order of the
specification (numpy neither contracts nor reorders).
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
