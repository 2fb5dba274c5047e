"""Motion blur on the GPU (include/ptx.h: MOTION): a time per ray in the intersect batch, and ptx_render_nee, ptx_render_adaptive_nee and
ptx_render_aov under a shutter.

The handle every test holds on to is the stated consequence of the specification: a ray of time u sees, bit for bit, the scene set to the
transforms x(u) with no motion. x(u) comes from Scene.motion_state, the function the kernels use (tests/test_motion_blur.py pins it to
a + (b - a) * u in numpy float32), and the static scene is created fresh from those arrays. With a degenerate shutter a whole frame is the
static scene's frame; with an open shutter every single sample is the static scene's sample at the sample's own restated time. All
comparisons are bitwise but the analytic one at the end, whose bound is worked out there.
"""
import numpy as np
import pytest

from _common import _bits, _proc, _same
from _motion_common import begin_camera as _begin_camera, movers as _movers, sample_time
from _nee_env_restatement import write_hdr
from _routes import ROUTE_VARS, clean_env, ctx, forced_routes, route_named, under_force_global, use_route  # noqa: F401
from conftest import product_from_dict

f32 = np.float32
pytestmark = pytest.mark.gpu

TIMES = f32([0.0, 0.3, 0.75, 1.0])
OUTPUTS = ("distance", "surface", "triangle", "b0", "b1", "b2", "px", "py", "pz", "nx", "ny", "nz", "u", "v")


def _rays(n=4096, seed=5):
    """rays aimed at the movers from all around: origins on a sphere about the scene's middle, targets inside the box the movers sweep"""
    rng = np.random.default_rng(seed)
    w = rng.standard_normal((n, 3))
    w[:, 1] = np.abs(w[:, 1]) + 0.05
    o = np.array([0.0, 0.6, 0.0]) + 6.0 * w / np.linalg.norm(w, axis=1, keepdims=True)
    t = rng.uniform([-2.0, 0.0, -1.5], [2.0, 1.6, 1.8], (n, 3))
    d = (t - o).astype(f32)
    d /= np.sqrt((d * d).sum(1, dtype=f32))[:, None]
    return o.astype(f32), d.astype(f32)


def _hybrid_budget(ptx, mp, d):
    """one byte short of what the resident arrays take: tests/test_camera_lens_gpu.py's recipe for a scene that is partly resident"""
    budget = int(product_from_dict(ptx, None, d).array(ptx.ARR_RES_PLAN)[0]) - 1
    mp.setenv("PTX_LDS_BUDGET", str(budget))
    fits = product_from_dict(ptx, None, d).info()["lds_resident"] == 1
    mp.delenv("PTX_LDS_BUDGET")
    if fits:
        mp.setenv("PTX_LDS_LEAF_ORDER", "0")
        budget = int(product_from_dict(ptx, None, d).array(ptx.ARR_RES_PLAN)[0]) - 1
        mp.delenv("PTX_LDS_LEAF_ORDER")
    return budget


class Routed:
    """scenes of one route ("lds fused", "hybrid", "global fused", "queue"): make(d) creates one under the route's creation switches and
    asserts its residency; the route's call switches stay set"""

    def __init__(self, ptx, ctx, mp, route, d0):
        self.ptx, self.ctx, self.mp, self.route = ptx, ctx, mp, route
        for k in ROUTE_VARS:
            mp.delenv(k, raising=False)
        self.budget = _hybrid_budget(ptx, mp, d0) if route == "hybrid" else None
        if route == "hybrid":
            mp.setenv("PTX_WAVEFRONT", "0")
            self.pipeline, self.resident = 0, 2
        else:
            r = route_named(forced_routes(1), route)
            use_route(mp, r)
            self.force_global, self.pipeline, self.resident = r.force_global, r.pipeline, r.resident

    def make(self, d):
        if self.route == "hybrid":
            self.mp.setenv("PTX_LDS_BUDGET", str(self.budget))
            try:
                s = product_from_dict(self.ptx, self.ctx, d)
            finally:
                self.mp.delenv("PTX_LDS_BUDGET")
        else:
            s = under_force_global(self.mp, self.force_global, lambda: product_from_dict(self.ptx, self.ctx, d))
        assert s.info()["lds_resident"] == self.resident, (self.route, s.info())
        return s

    def assert_pipeline(self, s, what):
        """the pipeline from a tiny ptx_render under the same switches (ptx_intersect_batch routes its rays with ptx_render's rule)"""
        s.render(16, 12, 1, 2)
        assert self.ctx.timing()["pipeline"] == self.pipeline, (what, self.route)


def _static_at(R, d, x):
    return R.make(dict(d, model_xform=x))


def _compare_groups(R, d, a, o, dr, time, got, what):
    """every output of the timed batch, group by group, against ptx_intersect_batch on the scene set to x(u)"""
    n_hit = 0
    for u in np.unique(time):
        idx = np.nonzero(time == u)[0]
        x, _ = a.motion_state(float(u))
        b = _static_at(R, d, x)
        want = b.intersect(o[idx], dr[idx])
        R.assert_pipeline(b, what)
        for k in OUTPUTS:
            if got[k].dtype == np.int32:
                np.testing.assert_array_equal(got[k][idx], want[k], err_msg=f"{what}: u = {u}: {k}")
            else:
                _same(got[k][idx], want[k], f"{what}: u = {u}: {k}")
        n_hit += int((want["surface"] >= 0).sum())
        b.close()
    return n_hit


# ---------------------------------------------------------------------------- 1. the timed batch
@pytest.mark.parametrize("route", ["lds fused", "hybrid", "global fused", "queue"])
def test_timed_batch_is_the_static_scene_at_each_time(ptx, ctx, clean_env, route):
    """4096 rays, time cycling lane by lane through {0, 0.3, 0.75, 1}: every wave holds all four. Fails on the parent for want of the entry
    point; with wave-uniform or static transforms the groups at 0.3 and 0.75 differ."""
    d = _movers()
    R = Routed(ptx, ctx, clean_env, route, d)
    a = R.make(d)
    a.set_motion(d["begin_model_xform"], _begin_camera(d))
    assert a.info()["lds_resident"] == R.resident   # setting the motion does not decide the residency again
    o, dr = _rays()
    time = np.tile(TIMES, len(o) // 4)
    got = a.intersect_motion(o, dr, time)
    n_hit = _compare_groups(R, d, a, o, dr, time, got, route)
    assert n_hit > len(o) // 2, n_hit
    # the movers are hit, and at different places at different times: the middle groups are not the scene at u = 1
    still = a.intersect(o, dr)
    moving = np.isin(still["surface"], [2, 3, 4, 5, 6, 7, 8, 9])
    assert moving.sum() > 200, moving.sum()
    mid = (time == TIMES[1]) | (time == TIMES[2])
    assert (_bits(got["distance"])[mid] != _bits(still["distance"])[mid]).sum() > 100
    # ptx_intersect_batch itself stays the scene at u = 1: the current transforms
    cur = R.make(d)
    want = cur.intersect(o, dr)
    for k in OUTPUTS:
        _same(still[k].astype(f32), want[k].astype(f32), f"{route}: ptx_intersect_batch under motion: {k}")
    cur.close(), a.close()


def test_timed_batch_with_a_small_pool_repeats_its_slices(ptx, ctx, clean_env):
    """the queue route with the pair pool forced to its smallest: a slice overflows and is repeated smaller, times and all"""
    d = _movers()
    R = Routed(ptx, ctx, clean_env, "queue", d)
    a = R.make(d)
    a.set_motion(d["begin_model_xform"])
    rng = np.random.default_rng(11)
    o, dr = _rays(1 << 20, seed=7)   # more than a pair per ray: more than the pool
    time = rng.choice(TIMES[1:3], len(o)).astype(f32)
    # a fresh scene has no pairs-per-ray measurement: the guess decides the first slice, which then takes the whole batch and overflows
    clean_env.setenv("PTX_WF_PAIRS_M", "1")
    clean_env.setenv("PTX_WF_RATIO_GUESS", "0.25")
    before = ctx.timing()["pool_overflows"]
    got = a.intersect_motion(o, dr, time, attributes=False)
    overflows = ctx.timing()["pool_overflows"] - before
    clean_env.delenv("PTX_WF_PAIRS_M")
    clean_env.delenv("PTX_WF_RATIO_GUESS")
    assert overflows >= 1, overflows
    want = a.intersect_motion(o, dr, time, attributes=False)
    for k in ("distance", "surface", "triangle", "b0", "b1", "b2"):
        _same(got[k].astype(f32), want[k].astype(f32), f"small pool: {k}")
    sub = slice(0, 8192)
    _compare_groups(R, d, a, o[sub], dr[sub], time[sub], {k: v[sub] for k, v in a.intersect_motion(o[sub], dr[sub], time[sub]).items()}, "small pool")
    a.close()


def test_timed_batch_on_device_pointers(ptx, ctx, clean_env):
    torch = pytest.importorskip("torch")
    d = _movers()
    R = Routed(ptx, ctx, clean_env, "lds fused", d)
    a = R.make(d)
    a.set_motion(d["begin_model_xform"])
    o, dr = _rays(1024, seed=3)
    time = np.tile(TIMES, len(o) // 4)
    host = a.intersect_motion(o, dr, time)
    dev = a.intersect_motion(torch.from_numpy(o).cuda(), torch.from_numpy(dr).cuda(), torch.from_numpy(time).cuda())
    for k in OUTPUTS:
        _same(dev[k].cpu().numpy().astype(f32), host[k].astype(f32), f"device pointers: {k}")
    a.close()


@pytest.mark.parametrize("route", ["lds fused", "queue"])
def test_times_are_ignored_without_active_motion(ptx, ctx, clean_env, route):
    """never given motion, motion with all keys equal, motion of the camera alone, and cleared motion: arbitrary times give ptx_intersect_batch"""
    d = _movers()
    R = Routed(ptx, ctx, clean_env, route, d)
    a = R.make(d)
    o, dr = _rays(1024, seed=9)
    time = np.random.default_rng(1).uniform(-1, 2, len(o)).astype(f32)
    want = a.intersect(o, dr)

    def check(what):
        got = a.intersect_motion(o, dr, time)
        for k in OUTPUTS:
            _same(got[k].astype(f32), want[k].astype(f32), f"{route}: {what}: {k}")

    check("never given motion")
    a.set_motion(d["model_xform"])
    assert not a.array(ptx.ARR_MOTION_MOVED).any()
    check("all keys equal")
    a.set_motion(None, _begin_camera(d))
    check("the camera alone moves")
    a.set_motion(d["begin_model_xform"])
    a.clear_motion()
    check("cleared")
    a.close()


# ---------------------------------------------------------------------------- frames under a shutter
W, H, SPP, B, SEED = 16, 12, 3, 3, 0x5EED
STAT_KEYS = ("rays", "samples", "light_samples", "light_visible")


def _static_frame_scene(R, d, a, u, lens=None):
    """a fresh scene set to x(u) and camera(u) of the moving scene `a`, no motion"""
    x, cam = a.motion_state(float(u))
    b = R.make(dict(d, model_xform=x))
    b.set_camera(cam[:3], cam[3:], d["camera"][12], *(lens or ()))
    return b


def _with_motion(R, d, shutter, lens=None):
    a = R.make(d)
    if lens:
        a.set_camera(d["camera"][:3], d["camera"][3:12], d["camera"][12], *lens)
    a.set_motion(d["begin_model_xform"], _begin_camera(d), shutter)
    return a


# 2. a degenerate shutter: the whole frame is the static scene's
@pytest.mark.parametrize("route", ["lds fused", "global fused", "queue"])
@pytest.mark.parametrize("u", [0.0, 0.3, 1.0])
def test_degenerate_shutter_is_the_static_scene(ptx, ctx, clean_env, route, u):
    """lights on static models only; ptx_render_nee and both guide buffers, and the stats"""
    d = _movers()
    R = Routed(ptx, ctx, clean_env, route, d)
    a = _with_motion(R, d, (u, u))
    b = _static_frame_scene(R, d, a, u)
    got, gst = a.render_nee(W, H, SPP, B, seed=SEED)
    assert ctx.timing()["pipeline"] == R.pipeline
    want, wst = b.render_nee(W, H, SPP, B, seed=SEED)
    _same(got, want, f"{route}: u = {u}: ptx_render_nee")
    assert all(gst[k] == wst[k] for k in STAT_KEYS), (gst, wst)
    assert gst["light_samples"] > 0 and gst["n_lights"] == wst["n_lights"] == 2
    ga, gn, _ = a.render_aov(W, H, SPP, seed=SEED)
    wa, wn, _ = b.render_aov(W, H, SPP, seed=SEED)
    _same(ga, wa, f"{route}: u = {u}: albedo_cov")
    _same(gn, wn, f"{route}: u = {u}: normal_depth")
    assert ga[..., 3].sum() > 0
    a.close(), b.close()


VARIANTS = {
    "lens": dict(lens=(0.08, 5.0, 6, 0.3)),
    "sun and pass-through": dict(scene=(False, True, True)),
    "env samples": dict(flags="NEE_ENV_SAMPLES", env_map=True),
    "sampler pdf": dict(flags="NEE_SAMPLER_PDF"),
    "candidates": dict(candidates=4),
    "punctual": dict(punctual=True),
    "emissive mover, no light samples": dict(scene=(True, False, False), flags="NEE_NO_LIGHT_SAMPLES"),
    "emissive mover": dict(scene=(True, False, False)),
}


@pytest.fixture(scope="module")
def env_map(tmp_path_factory):
    """a small Radiance map: grey with one hot texel"""
    rgb = np.full((8, 16, 3), 0.5)
    rgb[1, 3] = [40.0, 36.0, 24.0]
    return write_hdr(str(tmp_path_factory.mktemp("motion_env") / "hot.hdr"), rgb)


@pytest.mark.parametrize("name", list(VARIANTS))
def test_degenerate_shutter_variants(ptx, ctx, clean_env, env_map, name):
    """each estimator variant once, at u = 0.3 on the LDS route. The emissive mover is unlisted under motion: with light samples the
    static scene lists it, so the frames are compared only where the two light lists are equal (PTX_NEE_NO_LIGHT_SAMPLES)."""
    v = VARIANTS[name]
    u = 0.3
    d = _movers(*v.get("scene", ()))
    R = Routed(ptx, ctx, clean_env, "lds fused", d)
    a = _with_motion(R, d, (u, u), v.get("lens"))
    b = _static_frame_scene(R, d, a, u, v.get("lens"))
    flags = getattr(ptx, v["flags"]) if "flags" in v else 0
    for s in (a, b):
        if v.get("env_map"):
            s.set_environment(env_map, srgb=False)
        if v.get("punctual"):
            s.set_punctual_lights(np.array([[0.5, 2.0, 1.0, 0, 0, -1, 0, 0, 6, 5, 4, 0, 0, 0, 0, 0], [-1.0, 1.5, 2.0, 0, 0, -1, 0, 0, 2, 3, 4, 0, 0, 0, 0, 0]], f32))
    kw = dict(seed=SEED, flags=flags, candidates=v.get("candidates", 1))
    got, gst = a.render_nee(W, H, SPP, B, **kw)
    want, wst = b.render_nee(W, H, SPP, B, **kw)
    if name == "emissive mover":
        # the static scene lists the mover's 12 triangles, the moving scene does not: not the same estimator, and not compared
        assert gst["n_lights"] == 2 and wst["n_lights"] == 14
        lib, _ = a.render_nee(W, H, SPP, B, seed=SEED, flags=ptx.NEE_NO_LIGHT_SAMPLES)
        assert np.isfinite(got).all() and (_bits(got) != _bits(lib)).any()
    else:
        _same(got, want, f"{name}: ptx_render_nee")
        assert all(gst[k] == wst[k] for k in STAT_KEYS), (name, gst, wst)
        if "NO_LIGHT" not in v.get("flags", ""):
            assert gst["light_samples"] > 0
    ga, gn, _ = a.render_aov(W, H, SPP, seed=SEED)
    wa, wn, _ = b.render_aov(W, H, SPP, seed=SEED)
    _same(ga, wa, f"{name}: albedo_cov")
    _same(gn, wn, f"{name}: normal_depth")
    a.close(), b.close()


# 3. an open shutter, sample by sample
@pytest.mark.parametrize("route", ["lds fused", "queue"])
def test_open_shutter_sample_by_sample(ptx, ctx, ora, clean_env, route):
    """Shutter (0.2, 0.9), 12 x 8, 2 spp: each of the 192 samples is the static scene's sample at the sample's own restated time. A
    wave-uniform or per-pixel time fails here."""
    w, h, spp, shutter = 12, 8, 2, (0.2, 0.9)
    d = _movers()
    R = Routed(ptx, ctx, clean_env, route, d)
    a = _with_motion(R, d, shutter)
    frame, _ = a.render_nee(w, h, spp, B, seed=SEED)
    ga, gn, _ = a.render_aov(w, h, spp, seed=SEED)
    b = R.make(d)
    want = np.zeros_like(frame)
    wa, wn = np.zeros_like(ga), np.zeros_like(gn)
    times = set()
    for y in range(h):
        for x in range(w):
            for s in range(spp):
                u = sample_time(ora, y * w + x, s, SEED, shutter)
                times.add(float(u))
                xs, cam = a.motion_state(float(u))
                if route == "queue":
                    clean_env.setenv("PTX_FORCE_GLOBAL", "1")   # the residency choice is made again at every upload
                b.set_model_xforms(xs)
                clean_env.delenv("PTX_FORCE_GLOBAL", raising=False)
                b.set_camera(cam[:3], cam[3:], d["camera"][12])
                one, _ = b.render_nee(w, h, 1, B, seed=SEED, tile=(x, y, 1, 1), sample0=s, want_stats=False)
                want[y, x] += one[0, 0]
                oa, on, _ = b.render_aov(w, h, 1, seed=SEED, tile=(x, y, 1, 1), sample0=s, want_stats=False)
                if oa[0, 0, 3] != 0:
                    wa[y, x] += oa[0, 0]
                    wn[y, x] += on[0, 0]
    assert len(times) > 150 and min(times) >= 0.2 and max(times) <= 0.9
    assert b.info()["lds_resident"] == R.resident
    _same(frame, want, f"{route}: the frame is its samples, each at its own time")
    _same(ga, wa, f"{route}: albedo_cov")
    _same(gn, wn, f"{route}: normal_depth")
    still, _ = b.render_nee(w, h, spp, B, seed=SEED)
    assert (_bits(frame) != _bits(still)).any()
    a.close(), b.close()


# 4. composition under motion
def test_composition_under_motion(ptx, ctx, clean_env):
    torch = pytest.importorskip("torch")
    d = _movers()
    R = Routed(ptx, ctx, clean_env, "lds fused", d)
    a = _with_motion(R, d, (0.1, 0.8))
    spp = 4
    full, fst = a.render_nee(W, H, spp, B, seed=SEED)
    tiles = np.zeros_like(full)
    for (x0, y0, w, h) in ((0, 0, 7, 12), (7, 0, 9, 5), (7, 5, 9, 7)):
        t, _ = a.render_nee(W, H, spp, B, seed=SEED, tile=(x0, y0, w, h))
        tiles[y0:y0 + h, x0:x0 + w] = t
    _same(tiles, full, "tiles")
    acc = np.zeros_like(full)
    for s0, n in ((0, 1), (1, 2), (3, 1)):
        a.render_nee(W, H, n, B, accum=acc, seed=SEED, sample0=s0)
    _same(acc, full, "ascending sample ranges")
    one, _ = a.render_nee(W, H, spp, B, seed=SEED, spp_per_pass=1)
    _same(one, full, "spp_per_pass = 1")
    for count in (2, 3):
        acc = np.zeros_like(full)
        for k in range(count):
            a.render_nee(W, H, spp, B, accum=acc, seed=SEED, shard=(k, count, 4))
        _same(acc, full, f"{count} shards")
    dev = torch.zeros((H, W, 4), dtype=torch.float32, device="cuda")
    a.render_nee(W, H, spp, B, accum=dev, seed=SEED)
    ctx.synchronize()
    _same(dev.cpu().numpy(), full, "device buffer")
    # the adaptive loop with a threshold nothing exceeds: every pixel takes min_spp, split into the two half ranges
    ha, hb, ast = a.render_adaptive_nee(W, H, spp, B, min_spp=spp, threshold=float("inf"), seed=SEED)
    wa_, _ = a.render_nee(W, H, spp // 2, B, seed=SEED)
    wb_, _ = a.render_nee(W, H, spp - spp // 2, B, seed=SEED, sample0=spp // 2)
    _same(ha, wa_, "adaptive: first half")
    _same(hb, wb_, "adaptive: second half")
    a.close()


# 5. routing and refusals
def test_fused_flag_and_refusals(ptx, ctx, clean_env):
    d = _movers()
    R = Routed(ptx, ctx, clean_env, "lds fused", d)
    never = R.make(d)
    a = R.make(d)
    kw = dict(seed=SEED)
    base, _ = never.render_nee(W, H, SPP, B, flags=ptx.NEE_FUSED, **kw)
    passes = ctx.timing()["fused_launches"]
    assert passes >= 1
    a.set_motion(d["begin_model_xform"], _begin_camera(d), (0.2, 0.9))
    plain, _ = a.render_nee(W, H, SPP, B, **kw)
    flagged, _ = a.render_nee(W, H, SPP, B, flags=ptx.NEE_FUSED, **kw)
    assert ctx.timing()["fused_launches"] == 0 and ctx.timing()["pipeline"] == 0
    _same(flagged, plain, "PTX_NEE_FUSED is ignored under active motion")
    assert (_bits(plain) != _bits(base)).any()
    refused = {
        "ptx_render": lambda s: s.render(W, H, 1, B, **kw),
        "ptx_render_transparent": lambda s: s.render_transparent(W, H, 1, B, **kw),
        "ptx_render_adaptive": lambda s: s.render_adaptive(W, H, 2, B, min_spp=2, **kw),
        "ptx_render_motion": lambda s: s.render_motion(W, H, 1, **kw),
        "ptx_render_emission": lambda s: s.render_emission(W, H, 1, **kw),
        "worker ptx_render": lambda s: s.render(W, H, 1, B, integrator=ptx.INTEGRATOR_WORKER, **kw),
        "worker ptx_render_nee": lambda s: s.render_nee(W, H, 1, B, integrator=ptx.INTEGRATOR_WORKER, **kw),
    }
    before = {k: f(never) for k, f in refused.items() if not k.startswith("worker ptx_render_")}
    for k, f in refused.items():
        with pytest.raises(ptx.PtxError) as e:
            f(a)
        assert e.value.code == ptx.ERR_UNSUPPORTED, k
        if not k.startswith("worker ptx_render_"):
            assert "ptx_render_nee" in str(e.value), (k, str(e.value))

    def first(r):
        return r[0] if isinstance(r, tuple) else r

    for what in ("cleared", "inactive"):
        if what == "cleared":
            a.clear_motion()
        else:
            a.set_motion(d["model_xform"], (d["camera"][:3], d["camera"][3:12], d["camera"][12]), (0.2, 0.9))
        again, _ = a.render_nee(W, H, SPP, B, flags=ptx.NEE_FUSED, **kw)
        assert ctx.timing()["fused_launches"] == passes, what
        _same(again, base, f"{what}: the frame of a scene never given motion")
        for k, want in before.items():
            _same(first(refused[k](a)), first(want), f"{what}: {k} renders as before")
    a.close(), never.close()


# 6. blur is there: analytic, no reference frame
def test_a_translating_quad_covers_half_the_shutter(ptx, ctx, clean_env):
    """Two opaque quads slide along x in the plane z = 0 in front of a static camera that looks down -z from z = D; quad A fills the upper
    half of the frame's height, quad B the lower half. A pixel is p wide in that plane.
    Quad A has speed v = 50 p per unit of u and width w = v / 2, and starts so that its leading edge passes the centre xc of the chosen pixel
    at u = 0.25; its trailing edge then passes at u = 0.75, and the pixel is covered for u in (0.25, 0.75): coverage 0.5. An edge takes p / v
    of u to cross the pixel's footprint, twice: the footprint is only partly covered over a share 2 p / v = 0.04 < 0.05 of u.
    Bound: 5 sigma of a binomial with n = 1024, p = 0.5 (5 sqrt(0.25 / 1024) = 0.078), widened by that share. The band A sweeps is
    1.5 v = 75 p wide in a frame of 128 p: pixels of the upper rows outside it read 0. Quad B is 40 p wide and moves by 10 p: the pixels of
    the lower rows it covers at both ends of its way read n. One time for all samples would read 0 or n in the chosen pixel."""
    Wf, Hf, n = 128, 8, 1024
    yfov, D = 0.3, 4.0
    half_h = D * np.tan(yfov / 2)                   # half the frame's height in the plane z = 0
    half_w = half_h * Wf / Hf
    p = 2 * half_w / Wf                             # a pixel's footprint
    v = 50 * p
    w = v / 2
    share = 2 * p / v
    assert share < 0.05
    px, py = 64, 2
    x_of = lambda q: (q + 0.5) / Wf * 2 * half_w - half_w   # a pixel's centre in the plane
    xc = x_of(px)
    c0 = (xc - w / 2) - v * 0.25                    # A's centre at u = 0: the leading (+x) edge reaches xc at u = 0.25
    c1 = c0 + v
    b0, b1, wb = x_of(20), x_of(20) + 10 * p, 40 * p

    def quad(width, y_lo, y_hi):
        q = np.zeros((4, 11), f32)
        q[:, :3] = [[-width / 2, y_lo, 0], [width / 2, y_lo, 0], [width / 2, y_hi, 0], [-width / 2, y_hi, 0]]
        q[:, 3:5] = [[0, 0], [1, 0], [1, 1], [0, 1]]
        q[:, 5:8] = [0, 0, 1]
        q[:, 8:11] = [1, 0, 0]
        return q

    ident = [1, 0, 0, 0, 1, 0, 0, 0, 1]
    grey = [0.8, 0.8, 0.8, 1.0, 0.5, 0.0, 0, 0, 0, 1.33, 0.0]
    d = dict(model_xform=f32([[c1, 0, 0] + ident, [b1, 0, 0] + ident]), model_surf=np.array([[0, 1], [1, 1]], np.int32),
             surf_range=np.array([[0, 4, 0, 2], [4, 4, 2, 2]], np.int32), vertices=np.concatenate([quad(w, 0.0, 2 * half_h), quad(wb, -2 * half_h, 0.0)]),
             triangles=np.array([[0, 1, 2], [0, 2, 3], [0, 1, 2], [0, 2, 3]], np.uint32), materials=f32([grey, grey]),
             camera=f32([0, 0, D, 1, 0, 0, 0, 1, 0, 0, 0, 1, yfov]), sun=None)
    R = Routed(ptx, ctx, clean_env, "lds fused", d)
    s = R.make(d)
    s.set_motion(f32([[c0, 0, 0] + ident, [b0, 0, 0] + ident]), None, (0.0, 1.0))
    alb, _, _ = s.render_aov(Wf, Hf, n, seed=SEED)
    cov = alb[..., 3] / n
    bound = 5 * np.sqrt(0.25 / n) + share
    print("coverage of the chosen pixel", cov[py, px], "bound", bound)
    assert abs(cov[py, px] - 0.5) <= bound, (cov[py, px], bound)
    assert 0 < alb[py, px, 3] < n
    upper, lower = [1, 2], [5, 6]                   # rows well inside each half
    outside = [q for q in range(Wf) if x_of(q) + p < c0 - w / 2 or x_of(q) - p > c1 + w / 2]
    always = [q for q in range(Wf) if b1 - wb / 2 + p < x_of(q) < b0 + wb / 2 - p]
    assert len(outside) > 20 and len(always) > 20, (len(outside), len(always))
    assert (alb[np.ix_(upper, outside)][..., 3] == 0).all()
    assert (alb[np.ix_(lower, always)][..., 3] == n).all()
    s.close()
