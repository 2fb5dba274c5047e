"""The camera of include/ptx.h (THE LENS, THE APERTURE TABLE) restated in float32 numpy: the pinhole ray of scene::camera::get_ray, the thin
lens with its polygonal aperture, and a proxy around an OracleScene whose primary_rays are lens rays, so that the restatements that take
their camera rays from primary_rays (tests/_aov_restatement.restate, tests/_nee_estimator.render_samples) restate the lens renders as they
are. Not collected (underscore prefix).

Every operation is one float32 operation, in the order the header writes them. tan_half_fov is taken from ARR_CAMERA [13] (std::tan of the
float): numpy's tan of a float32 need not give the same bits, which tests/test_camera_lens.py pins.
"""
import numpy as np

f32 = np.float32


def _dot(a, b):
    return (a[..., 0] * b[..., 0] + a[..., 1] * b[..., 1]) + a[..., 2] * b[..., 2]


def normalize(a):
    """a * (1.0f / sqrt(dot(a, a))) — math/vec3.inl:251"""
    a = np.asarray(a, f32)
    return (a * (f32(1) / np.sqrt(_dot(a, a)))[..., None]).astype(f32)


def mulmv(m, v):
    """column-major 3 x 3 times vector: each row dotted with v, left to right (math/mat3.inl:219-224)"""
    m = np.asarray(m, f32)
    v = np.asarray(v, f32)
    return np.stack([(m[r] * v[..., 0] + m[3 + r] * v[..., 1]) + m[6 + r] * v[..., 2] for r in range(3)], -1).astype(f32)


def aperture_table(radius, blades, rotation):
    """[blades + 1, 2] float32: corners in float64 from the stored float32 fields, the last entry a copy of the first"""
    R, rot = float(f32(radius)), float(f32(rotation))
    t = np.zeros((blades + 1, 2), f32)
    for k in range(blades):
        th = rot + 2.0 * np.pi * k / blades
        t[k] = (f32(R * np.cos(th)), f32(R * np.sin(th)))
    t[blades] = t[0]
    return t


class Camera:
    """origin [3], basis [9], tan_half_fov and the lens as stored (blades resolved: 0 means 16)"""

    def __init__(self, cam14, lens_radius=0.0, focus_distance=0.0, blades=0, blade_rotation=0.0):
        c = np.asarray(cam14, f32)
        self.origin, self.basis, self.tan = c[0:3].copy(), c[3:12].copy(), f32(c[13])
        self.R, self.F = f32(lens_radius), f32(focus_distance)
        self.n = (blades or 16) if self.R > 0 else 0
        self.table = aperture_table(self.R, self.n, blade_rotation) if self.R > 0 else np.zeros((0, 2), f32)

    def _dir(self, ndc_x, ndc_y, ratio):
        dx, dy = self.tan * np.asarray(ndc_x, f32), self.tan * np.asarray(ndc_y, f32)
        dx = dx * np.asarray(ratio, f32)
        return normalize(np.stack([dx, dy, np.full_like(dx, -1)], -1))

    def pinhole(self, ndc_x, ndc_y, ratio):
        """camera::get_ray -> [n, 6]"""
        d = self._dir(ndc_x, ndc_y, ratio)
        o = mulmv(self.basis, np.zeros_like(d)) + self.origin
        return np.concatenate([o, normalize(mulmv(self.basis, d))], -1).astype(f32)

    def lens_parts(self, ndc_x, ndc_y, ratio, u, v):
        """the lens branch in camera space -> (pf, lp, dl)"""
        u, v = np.asarray(u, f32), np.asarray(v, f32)
        d = self._dir(ndc_x, ndc_y, ratio)
        t = self.F / (f32(0) - d[..., 2])
        pf = (d * t[..., None]).astype(f32)
        a = u * f32(self.n)
        k = np.minimum(a.astype(np.uint32), np.uint32(self.n - 1))
        su = np.sqrt(a - k.astype(f32))
        beta, gamma = su * (f32(1) - v), su * v
        v0, v1 = self.table[k], self.table[k + 1]
        lp = np.stack([beta * v0[..., 0] + gamma * v1[..., 0], beta * v0[..., 1] + gamma * v1[..., 1], np.zeros_like(beta)], -1).astype(f32)
        return pf, lp, normalize(pf - lp)

    def rays(self, ndc_x, ndc_y, ratio, u, v):
        """camera_ray's branch: the lens ray, or without a lens the pinhole ray -> [n, 6]"""
        if not self.R > 0:
            return self.pinhole(ndc_x, ndc_y, ratio)
        _, lp, dl = self.lens_parts(ndc_x, ndc_y, ratio, u, v)
        o = mulmv(self.basis, lp) + self.origin
        return np.concatenate([o, normalize(mulmv(self.basis, dl))], -1).astype(f32)

    def primary_rays(self, ora, cfg, sample):
        """the camera rays of sample `sample` of the cfg's tile -> [h, w, 6]; the draws are pt_oracle.draws' block 2"""
        W, H = cfg.W, cfg.H
        seed = cfg.seed_lo | (cfg.seed_hi << 32)
        yy, xx = np.divmod(np.arange(cfg.h * cfg.w), cfg.w)
        xx, yy = xx + cfg.x0, yy + cfg.y0
        j = np.stack([ora.draws(int(y) * W + int(x), sample, seed, 0, 0, 2) for x, y in zip(xx, yy)]).astype(f32)
        if cfg.integrator == 1 and sample == 0:
            j[:, :2] = 0   # worker.cpp:125-126: the first sample is not offset; the lens draws stay
        ndc_x = ((xx.astype(f32) + j[:, 0]) / f32(W)) * f32(2) - f32(1)
        ndc_y = -(((yy.astype(f32) + j[:, 1]) / f32(H)) * f32(2) - f32(1))
        ratio = np.full(len(xx), f32(W) / f32(H), f32)
        return self.rays(ndc_x, ndc_y, ratio, j[:, 2], j[:, 3]).reshape(cfg.h, cfg.w, 6)


class LensOracle:
    """An OracleScene whose camera rays are `camera`'s: primary_rays is restated here, everything else is the oracle's."""

    def __init__(self, ora, o, camera):
        self._ora, self._o, self.camera = ora, o, camera

    def primary_rays(self, cfg, sample):
        return self.camera.primary_rays(self._ora, cfg, sample)

    def __getattr__(self, name):
        return getattr(self._o, name)


# ---------------------------------------------------------------------------- moved model transforms (ptx_scene_set_model_xforms)
def _rot(axis, angle):
    a = np.asarray(axis, np.float64) / np.linalg.norm(axis)
    K = np.array([[0, -a[2], a[1]], [a[2], 0, -a[0]], [-a[1], a[0], 0]])
    return np.eye(3) + np.sin(angle) * K + (1 - np.cos(angle)) * K @ K


def moved_xforms(x, share=True):
    """Every model rotated, translated and scaled non-uniformly; with `share`, the last model takes the first one's transform, so that the
    number of distinct ray spaces changes."""
    x = np.asarray(x, f32).reshape(-1, 12)
    out = x.copy()
    for m in range(len(x)):
        B = x[m, 3:12].astype(np.float64).reshape(3, 3).T            # columns x, y, z
        M = _rot([0.3 + m, 1.0, 0.2 * m], 0.4 + 0.3 * m) @ np.diag([1.0 + 0.1 * m, 0.8, 1.25])
        out[m, 3:12] = (M @ B).T.reshape(-1).astype(f32)
        out[m, 0:3] = (M @ x[m, 0:3].astype(np.float64) + [0.05 * m, 0.02, -0.03 * m]).astype(f32)
    if share and len(x) > 1:
        out[-1] = out[0]
    return out
