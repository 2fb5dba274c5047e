"""What tests/test_nee_fused_motion_gpu.py builds on: scenes of one fused route and the movers under a shutter. Routed and with_motion
restate the helpers of tests/test_motion_blur_gpu.py (test modules are not imported). Not collected (underscore prefix); import by name."""
import numpy as np

from _motion_common import begin_camera
from _routes import ROUTE_VARS, forced_routes, route_named, under_force_global, use_route
from conftest import product_from_dict

f32 = np.float32
FUSED_ROUTES = ("lds fused", "hybrid", "global fused")


def hybrid_budget(ptx, mp, create):
    """one byte short of what the resident arrays take (tests/test_camera_lens_gpu.py's recipe for a partly resident scene); create() makes
    a host-only scene under the switches that are set"""
    budget = int(create().array(ptx.ARR_RES_PLAN)[0]) - 1
    mp.setenv("PTX_LDS_BUDGET", str(budget))
    fits = create().info()["lds_resident"] == 1
    mp.delenv("PTX_LDS_BUDGET")
    if fits:
        mp.setenv("PTX_LDS_LEAF_ORDER", "0")
        budget = int(create().array(ptx.ARR_RES_PLAN)[0]) - 1
        mp.delenv("PTX_LDS_LEAF_ORDER")
    return budget


class Routed:
    """scenes of one route ("lds fused", "hybrid", "global fused", "queue"): make(d) creates one from a scene dict under the route's creation
    switches and asserts its residency; the route's call switches stay set"""

    def __init__(self, ptx, ctx, mp, route, d0):
        self.ptx, self.ctx, self.mp, self.route = ptx, ctx, mp, route
        for k in ROUTE_VARS:
            mp.delenv(k, raising=False)
        self.budget = hybrid_budget(ptx, mp, lambda: product_from_dict(ptx, None, d0)) if route == "hybrid" else None
        if route == "hybrid":
            mp.setenv("PTX_WAVEFRONT", "0")
            self.pipeline, self.resident = 0, 2
        else:
            r = route_named(forced_routes(1), route)
            use_route(mp, r)
            self.force_global, self.pipeline, self.resident = r.force_global, r.pipeline, r.resident

    def creating(self, fn):
        """fn() under the route's creation switches: creating a scene, and every call that uploads one again (the residency choice is made
        again at every upload)"""
        if self.route != "hybrid":
            return under_force_global(self.mp, self.force_global, fn)
        self.mp.setenv("PTX_LDS_BUDGET", str(self.budget))
        try:
            return fn()
        finally:
            self.mp.delenv("PTX_LDS_BUDGET")

    def make(self, d):
        s = self.creating(lambda: product_from_dict(self.ptx, self.ctx, d))
        assert s.info()["lds_resident"] == self.resident, (self.route, s.info())
        return s


def with_motion(R, d, shutter, models=True, camera=True, lens=None):
    """the movers `d` on route R under a shutter: models and camera moving, or one of the two alone"""
    a = R.make(d)
    if lens:
        a.set_camera(d["camera"][:3], d["camera"][3:12], d["camera"][12], *lens)
    a.set_motion(d["begin_model_xform"] if models else None, begin_camera(d) if camera else None, shutter)
    return a


def turned(xform, degrees, shift):
    """[n, 12] transforms (origin, basis columns) turned about y by `degrees` and moved by `shift`, in float32: begin keys a little off"""
    x = np.array(xform, f32).reshape(-1, 12).copy()
    a = np.deg2rad(degrees)
    rot = np.array([[np.cos(a), 0, np.sin(a)], [0, 1, 0], [-np.sin(a), 0, np.cos(a)]])
    for m in x:
        basis = m[3:12].reshape(3, 3).T.astype(np.float64)   # columns -> matrix
        m[3:12] = (rot @ basis).T.reshape(9).astype(f32)
        m[:3] = (m[:3].astype(np.float64) + np.asarray(shift)).astype(f32)
    return x
