"""ptx_render_motion restated from the oracle alone, in float32 numpy (tests/test_temporal.py states its rules on the CPU,
tests/test_motion_gpu.py pins the product to it bit for bit). Not collected (underscore prefix).

The walk — camera samples, opacity pass-throughs, the first vertex that does not pass through — is tests/_aov_restatement.restate's. What
the sample's surface adds is the specification of include/ptx.h: the surface comes from the oracle's scene intersection, the triangle and
its barycentrics from the oracle's model intersection of that surface's model, the local corners from the scene arrays.
"""
import numpy as np

from _aov_restatement import EPS, H, S0, SEED, SPP, TILE, W, _len3
from _camera_restatement import _dot, mulmv

f32 = np.float32


class Pose:
    """What project() needs of a camera: origin [3], basis [9] (columns), tan_half_fov as the host's std::tan gives it."""

    def __init__(self, origin, basis, tan_half_fov):
        self.origin, self.basis, self.tan = np.asarray(origin, f32).reshape(3).copy(), np.asarray(basis, f32).reshape(9).copy(), f32(tan_half_fov)

    @classmethod
    def of(cls, cam14):
        """from ARR_CAMERA's 14 floats: origin, basis, yfov, tan_half_fov"""
        c = np.asarray(cam14, f32).reshape(-1)
        return cls(c[0:3], c[3:12], c[13])


def project(pose, W_, H_, p):
    """project(cam, p) of include/ptx.h -> (fx, fy, defined), every operation one float32 operation in the order written"""
    p = np.asarray(p, f32)
    with np.errstate(all="ignore"):
        q = p - pose.origin
        b = pose.basis
        cx, cy, cz = _dot(b[0:3], q), _dot(b[3:6], q), _dot(b[6:9], q)
        iz = f32(0) - cz
        ratio = f32(W_) / f32(H_)
        ndc_x = ((cx / iz) / ratio) / pose.tan
        ndc_y = (cy / iz) / pose.tan
        fx = ((ndc_x + f32(1)) * f32(0.5)) * f32(W_)
        fy = ((f32(1) - ndc_y) * f32(0.5)) * f32(H_)
    return fx.astype(f32), fy.astype(f32), cz < 0


def local_points(o, rays, surf):
    """For rays whose closest hit is on surface surf[i]: the triangle's local corners weighted by the barycentrics, lp = A*b0 + B*b1 + C*b2,
    the surface's model, and the model intersection's distance — from the oracle's model intersection and the scene arrays."""
    a = o.a
    ms = np.asarray(a.model_surf)
    model = np.searchsorted(ms[:, 0] + ms[:, 1], surf, side="right")
    lp, dist = np.zeros((len(rays), 3), f32), np.zeros(len(rays), f32)
    sr, V, T = np.asarray(a.surf_range), np.asarray(a.vertices, f32), np.asarray(a.triangles)
    for m in np.unique(model):
        sel = np.flatnonzero(model == m)
        out, idx = o.model_intersect(int(m), rays[sel])
        assert (idx[:, 0] == surf[sel]).all(), "the model's closest hit is the scene's"
        v0, t0 = sr[idx[:, 0], 0], sr[idx[:, 0], 2]
        tri = T[t0 + idx[:, 1]]
        A, B, C_ = (V[v0 + tri[:, k], :3] for k in range(3))
        b1, b2 = out[:, 2], out[:, 3]
        b0 = f32(1) - b1 - b2
        lp[sel] = (A * b0[:, None] + B * b1[:, None]) + C_ * b2[:, None]
        dist[sel] = out[:, 0]
    return lp, model, dist


def restate(ora, o, prev_pose=None, prev_xform=None, cur_pose=None, W_=W, H_=H, tile=TILE, sample0=S0, spp=SPP, seed=SEED, per_sample=False):
    """-> (motion [h,w,4], counts) for samples [sample0, sample0 + spp) of the tile. o: the oracle scene of the CURRENT frame (a LensOracle
    for a lens: the projections ignore it). prev_pose: the previous camera (None: the current one); prev_xform [n_models,12]: the previous
    model transforms (None: nothing moved). counts: surface samples, samples dropped for a projection, pixels of moved models.
    cur_pose: the current camera where the oracle's arrays do not hold its tan_half_fov (scenes made from a dict).
    per_sample: also the list of (live pixel indices, pos, pos_prev, record) per sample, for the semantic checks."""
    x0, y0, w, h = tile
    if cur_pose is None:
        cur_pose = Pose.of(o.a.camera)
    assert cur_pose.tan > 0, "the arrays hold no tan_half_fov: pass cur_pose"
    if prev_pose is None:
        prev_pose = cur_pose
    xf_cur = np.asarray(o.a.model_xform, f32).reshape(-1, 12)
    xf_prev = None if prev_xform is None else np.asarray(prev_xform, f32).reshape(-1, 12)
    moved = np.zeros(len(xf_cur), bool) if xf_prev is None else (xf_prev.view(np.uint32) != xf_cur.view(np.uint32)).any(1)
    mot = np.zeros((h * w, 4), f32)
    yy, xx = np.divmod(np.arange(h * w), w)
    pixel = (yy + y0) * W_ + (xx + x0)
    counts = dict(surface=0, dropped=0, moved=0)
    samples = []
    for s in range(sample0, sample0 + spp):
        rays = o.primary_rays(ora.make_cfg(W_, H_, 1, 1, seed=seed, tile=tile), s).reshape(-1, 6)
        rec = np.zeros((h * w, 4), f32)
        live, cur, pas = np.arange(h * w), rays.copy(), np.zeros(h * w, np.int64)
        while len(live):
            out, idx = o.intersect(cur)
            hit = idx >= 0
            op = np.ones(len(live), f32)
            for u in np.unique(idx[hit]):
                sel = idx == u
                op[sel] = o.material_eval(int(u), out[sel, 3:5])[:, 6]
            through = np.zeros(len(live), bool)
            for k in np.flatnonzero(hit & ~((op == f32(1)) | (np.abs(op - f32(1)) < EPS))):   # !is_approx(opacity, 1)
                through[k] = ora.draws(int(pixel[live[k]]), s, seed, 0, int(pas[k]), 0)[0] > op[k]
            surf = hit & ~through
            if surf.any():
                pos = out[surf, :3]
                lp, model, dist = local_points(o, cur[surf], idx[surf])
                # the local point gives the oracle's position back, bit for bit: triangle, barycentrics and corners are the hit's own
                again = mulmv(xf_cur[model, 3:12].T, lp) + xf_cur[model, 0:3]
                assert (again.view(np.uint32) == pos.view(np.uint32)).all(), "hit_attributes' position from the local point"
                # ... and the two intersections agree on the distance (the model's is length(basis * (local direction * t)))
                assert np.allclose(dist, _len3(pos - cur[surf, :3]), rtol=1e-3, atol=1e-4), "model and scene intersection disagree on the distance"
                pos_prev = pos.copy()
                mv = moved[model]
                if mv.any():
                    pos_prev[mv] = mulmv(xf_prev[model[mv], 3:12].T, lp[mv]) + xf_prev[model[mv], 0:3]
                fxc, fyc, okc = project(cur_pose, W_, H_, pos)
                fxp, fyp, okp = project(prev_pose, W_, H_, pos_prev)
                ok = okc & okp
                r = np.stack([fxp - fxc, fyp - fyc, _len3(pos_prev - prev_pose.origin), np.ones(len(pos), f32)], 1).astype(f32)
                r[~ok] = 0
                rec[live[surf]] = r
                counts["surface"] += int(surf.sum())
                counts["dropped"] += int((~ok).sum())
                counts["moved"] += int(mv.sum())
                if per_sample:
                    samples.append((s, live[surf], pos, pos_prev, r))
            d = cur[through, 3:6]
            nxt = np.concatenate([out[through, :3] + d * EPS, d * (f32(1) / _len3(d))[:, None]], 1).astype(f32)
            pas = pas[through] + 1
            live = live[through]
            keep = pas <= 4096
            live, cur, pas = live[keep], nxt[keep], pas[keep]
        took = rec[:, 3] > 0
        mot[took] += rec[took]
    mot = mot.reshape(h, w, 4)
    return (mot, counts, samples) if per_sample else (mot, counts)
