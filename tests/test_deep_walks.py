"""Deep KD walks and the far bound of a popped stack entry, on every route, against the oracle and the compiled reference.

core::mesh::intersect (mesh.cpp:300-405) sets a subtree aside at every "both children" step. The kernels keep those pending entries
in two separate stacks: mesh_traverse (device_core.hpp: 3 entries in registers, 24 in a lane-interleaved global area; the fused
kernels, their deferral and shadow sweeps, ptx_render_aov, ptx_intersect_batch on the fused route) and k_wf_traverse2
(wavefront.hip: 4 entries in LDS, the rest in 16-byte rows; the queue pipeline). Cornell's rays reach 8 pending entries, the
reference's jack-of-blades 12. procedural.corner_cluster_scene is a mesh whose SAH tree is a comb down to the builder's depth limit:
rays from its innermost cell reach 20 to 22 pending entries, a quarter of a million of them at once, so that the spill rows of every
wave slot are live together.

The second subject is the interval a popped entry resumes with. The reference stores (node, min_dist, max_dist); a walker that
keeps (node, min_dist) and rebuilds max_dist from the entry beneath is NOT equivalent: at a "both children" step whose far child
is absent (an empty-space cut) the reference cuts max_dist to the split distance and pushes nothing, so the next push stores a
bound that no entry's min_dist repeats. The oracle has that walker as a foil (mesh_intersect_recon): the CPU search below finds
rays on which it returns other records than the reference's walk (corner-aimed rays at scales 1e6 and 1e7, where float error
exceeds the builder's 1e-4 cut margin), and the GPU tests run exactly those rays on every route.

What the CPU search found (120 000 corner-aimed candidates per scale, mesh 60 / 0.8 / 0.1): 1 differing ray at scale 1e3, 135 at
1e6, 83 at 1e7 (the first 64 are kept); 94-95 % of the candidates have a pop whose rebuilt bound differs from the stored one.
mesh_traverse rebuilt its bounds that way: on the MI355X it returned other records than the oracle on 1 / 53 / 56 of the kept rays
at 1e3 / 1e6 / 1e7 (exactly the rays on which the foil still differs once the reference has normalised their directions) and on 1
and 9 rays of the 262 144-ray batches at 1e3 and 1e6, while the queue walk, which stores the bound, returned the oracle's. It now
leaves a placeholder entry behind at such a step, which makes the rebuilt bound the stored one.
"""
import functools
import os

import numpy as np
import pytest

from _checks import _check_records, _same_hits
from _common import _bits, _proc
from _routes import assert_route, clean_env, ctx, forced_routes, under_force_global  # noqa: F401  (clean_env and ctx are fixtures)
from conftest import GOLD, kd_stream_packed, kd_stream_preorder, oracle_from_dict, product_from_dict
from oracle import deep_walk as dw

N_BATCH = 262_144                  # > 8 waves per CU on 256 CUs
W, H, SPP, B = 64, 36, 3, 5
FIXTURE = os.path.join(GOLD, "deep_walk_vectors.npz")
VARIANT = dict(surfaces=9, backdrop=48)      # 9 clusters and a 4608-triangle backdrop in one model: hybrid residency, queue pipeline by default


# ---------------------------------------------------------------------------- shared, computed once, never modified
@functools.lru_cache(maxsize=None)
def _scene(cfg, scale, sun=False, variant=False):
    from oracle import pt_oracle as ora
    d = _proc().corner_cluster_scene(*cfg, scale, sun=sun, **(VARIANT if variant else {}))
    return d, oracle_from_dict(ora, d)


@functools.lru_cache(maxsize=None)
def _deep_batch(scale):
    """The rays of the 262 144-ray batch at `scale` with the oracle's records and per-ray pending depth (surface 0 = the cluster)."""
    d, o = _scene(dw.DEEP, scale)
    rays, is_deep = dw.deep_rays(scale, N_BATCH)
    out, idx = o.intersect(rays)
    _, midx, depth, hist = o.mesh_intersect(0, rays, stats=True)
    for a in (rays, is_deep, out, idx, depth):
        a.setflags(write=False)
    return rays, is_deep, out, idx, depth, hist


@functools.lru_cache(maxsize=None)
def _corner_found(scale):
    """-> (the kept differing rays, how many the search found, share of candidates with a differing rebuilt bound)"""
    d, o = _scene(dw.CORNER, scale)
    cand, differ, popped = dw.corner_search(o, scale)
    keep = cand[np.flatnonzero(differ)[:dw.CORNER_KEEP]]
    keep.setflags(write=False)
    return keep, int(differ.sum()), float(popped.mean())


def _tree_depth(kd):
    """Levels below the root of the oracle's pre-order tree."""
    dep = np.zeros(len(kd["type"]), np.int64)
    for i in range(len(dep)):
        if kd["type"][i] == 0:
            for c in (kd["left"][i], kd["right"][i]):
                if c >= 0:
                    dep[c] = dep[i] + 1
    return int(dep.max())


# ---------------------------------------------------------------------------- the generator (no GPU)
def test_corner_cluster_follows_its_recipe():
    n, ratio, size, scale = 17, 0.8, 0.1, 1e3
    d = _proc().corner_cluster_scene(n, ratio, size, scale, seed=4)
    u = np.random.default_rng(4).uniform(-1.0, 1.0, (n, 3, 3))
    s = scale * ratio ** np.arange(n)
    want = s[:, None, None] * (1 + size * u)
    p = d["vertices"][:, :3].reshape(n, 3, 3)
    assert d["vertices"].dtype == np.float32 and d["vertices"].shape == (3 * n, 11)
    np.testing.assert_allclose(p, want, rtol=2e-6)                     # float32 arithmetic on float32 factors
    assert d["triangles"].tolist() == np.arange(3 * n).reshape(-1, 3).tolist()
    assert d["model_xform"].tolist() == [[0, 0, 0, 1, 0, 0, 0, 1, 0, 0, 0, 1]] and d["model_surf"].tolist() == [[0, 1]] and d["sun"] is None
    np.testing.assert_allclose(np.linalg.norm(d["vertices"][:, 5:8], axis=1), 1, atol=1e-5)
    cam = d["camera"]
    assert (cam[:3] > 0).all() and (cam[:3] < p[-1].min()).all()       # inside the innermost cell
    np.testing.assert_allclose(-cam[9:12], np.ones(3) / np.sqrt(3), atol=1e-6)   # -z looks along (1, 1, 1)
    again = _proc().corner_cluster_scene(n, ratio, size, scale, seed=4)
    for k in ("vertices", "triangles", "materials", "camera"):
        np.testing.assert_array_equal(d[k], again[k])
    assert _proc().corner_cluster_scene(n, ratio, size, scale, seed=4, sun=True)["sun"].shape == (13,)
    v = _proc().corner_cluster_scene(n, ratio, size, scale, seed=4, **VARIANT)
    assert v["model_surf"].tolist() == [[0, 10]] and v["surf_range"][:, 3].tolist() == [n] * 9 + [2 * 48 * 48]
    np.testing.assert_array_equal(v["vertices"][:3 * n], d["vertices"])           # surface j is the cluster of seed + j
    np.testing.assert_array_equal(v["vertices"][3 * n:6 * n], _proc().corner_cluster_scene(n, ratio, size, scale, seed=5)["vertices"])
    rays = _proc().corner_cluster_rays(n, ratio, size, scale, 500, seed=4)
    assert rays.dtype == np.float32 and (rays[:, :3] > 0).all() and (rays[:, :3] < p[-1].min()).all()
    np.testing.assert_allclose(np.linalg.norm(rays[:, 3:], axis=1), 1, atol=1e-6)


def test_residency_of_the_cluster_scenes(ptx):
    """The routes the GPU tests expect without switches: the single cluster is LDS-resident (fused kernel), the ten-surface variant hybrid
    (its backdrop does not fit) with a model of more than eight surfaces (queue pipeline)."""
    assert product_from_dict(ptx, None, _scene(dw.DEEP, 1e3)[0]).info()["lds_resident"] == 1
    info = product_from_dict(ptx, None, _scene(dw.DEEP, 1e3, True, True)[0]).info()
    assert info["lds_resident"] == 2 and info["n_surfaces"] == 10 and info["n_models"] == 1 and info["has_sun"] == 1


# ---------------------------------------------------------------------------- D.1: the oracle pinned to the compiled reference
def _fixture():
    if not os.path.exists(FIXTURE):
        pytest.skip("tests/golden/deep_walk_vectors.npz is missing: build oracle/_ref and run oracle/make_golden.py --only-deep-walk")
    return dict(np.load(FIXTURE))


def _fixture_scene(ora, g, tag):
    a = ora.SceneArrays()
    for k in ("model_xform", "model_surf", "surf_range", "vertices", "triangles", "materials"):
        setattr(a, k, g[f"{tag}_{k}"])
    a.camera = np.zeros(14, np.float32)
    a.camera[3:12] = np.eye(3).ravel()
    a.camera[12] = 1
    return ora.OracleScene(a)


FIXTURE_TAGS = [("deep_1e3", dw.DEEP, 1e3)] + [(f"corner_{dw.scale_tag(sc)}", dw.CORNER, sc) for sc in dw.CORNER_SCALES]


@pytest.mark.parametrize("tag,cfg,scale", FIXTURE_TAGS, ids=[t[0] for t in FIXTURE_TAGS])
def test_oracle_equals_the_reference_on_the_cluster(ora, tag, cfg, scale):
    """renderer::intersect and model::intersect of the compiled reference (frozen records) against the oracle, bit for bit, on deep rays
    and on the corner-aimed rays: the oracle's walk is the reference's walk on this mesh. The frozen differing rays still tell the two
    CPU walkers apart as the reference holds them (it normalises every direction once more)."""
    g = _fixture()
    d = _proc().corner_cluster_scene(*cfg, scale)
    np.testing.assert_array_equal(_bits(g[tag + "_vertices"][:, :8]), _bits(d["vertices"][:, :8]))      # the mesh the GPU tests use
    np.testing.assert_array_equal(g[tag + "_triangles"], d["triangles"])
    o = _fixture_scene(ora, g, tag)
    rays = g[tag + "_rays"]
    assert len(rays) >= 1000 or tag.startswith("corner")
    out, idx = o.intersect(rays)
    np.testing.assert_array_equal(idx, g[tag + "_scene_idx"])
    np.testing.assert_array_equal(_bits(out), _bits(g[tag + "_scene_out"]))
    mo, mi = o.model_intersect(0, rays)
    np.testing.assert_array_equal(mi, g[tag + "_model_idx"][:, 0])
    np.testing.assert_array_equal(_bits(mo), _bits(g[tag + "_model_out"][:, 0]))
    hit = idx >= 0
    assert 0.05 < hit.mean() and (~hit).sum() > 0
    if tag.startswith("corner"):
        k = int(g[tag + "_n_differ"])
        a, ai = o.mesh_intersect(0, rays[:k])
        b, bi, _ = o.mesh_intersect_recon(0, rays[:k])
        still = int(dw.records_differ(a, ai, b, bi).sum())
        print(f"{tag}: {k} differing rays frozen, {still} still differ as the reference holds them")
        if scale >= 1e6:
            assert k == dw.CORNER_KEEP and still >= 8


# ---------------------------------------------------------------------------- D.2: what the GPU ray sets cover, by the oracle's count
@pytest.mark.parametrize("scale", dw.DEEP_SCALES, ids=[dw.scale_tag(s) for s in dw.DEEP_SCALES])
def test_deep_rays_cover_the_pending_stack(ptx, scale):
    """Conditions on the exact rays of test_deep_batch_every_route, from the oracle's walk alone."""
    d, o = _scene(dw.DEEP, scale)
    rays, is_deep, out, idx, depth, hist = _deep_batch(scale)
    kd = o.kd(0)
    assert _tree_depth(kd) == 25                                       # the builder's limit (mesh.hpp:34): 25 levels below the root
    s = product_from_dict(ptx, None, d)
    assert s.info()["kd_max_depth"] == _tree_depth(kd) + 1             # the product counts levels, root included
    nodes, refs, rg = s.array(ptx.ARR_KD_NODES), s.array(ptx.ARR_KD_REFS), s.array(ptx.ARR_SURF_RANGE)
    np.testing.assert_array_equal(kd_stream_packed(nodes, refs, rg[0, 4], int(rg[0, 2])), kd_stream_preorder(kd))
    want = dw.DEEP_PENDING[scale]
    deep = depth[is_deep]
    print(f"scale {scale:g}: deepest pending stack {depth.max()}, {(deep >= want).mean():.1%} of the deep rays reach {want}, "
          f"{(idx[is_deep] >= 0).mean():.1%} of them hit; histogram {hist[:26].tolist()}")
    assert want >= 18 and (deep >= want).mean() >= 0.01
    assert set(range(int(depth.max()) + 1)) <= set(np.unique(depth).tolist())      # a ray at every depth up to the maximum
    per_ray = np.bincount(depth, minlength=32)                                       # the histogram counts the walks that enter the box
    assert (per_ray[1:] == hist[1:].astype(np.int64)).all() and int(hist[0]) <= per_ray[0]
    assert 0.05 <= (idx[is_deep] >= 0).mean() <= 0.5                                 # most walks pop their whole stack
    assert depth.max() <= 25                                                         # the bound behind the kernels' 27 entries
    # more than kRegStack + one full row set: spill rows of mesh_traverse up to depth - 4, of the queue walk up to depth - 5
    assert depth.max() - 3 >= 16


def test_small_batch_rays_are_at_the_maximum_depth():
    rays, is_deep, out, idx, depth, hist = _deep_batch(1e3)
    at_max = np.flatnonzero(depth == depth.max())
    assert len(at_max) >= 65 and depth.max() >= dw.DEEP_PENDING[1e3]


# ---------------------------------------------------------------------------- D.3: rays that tell the two walkers apart
@pytest.mark.parametrize("scale", dw.CORNER_SCALES, ids=[dw.scale_tag(s) for s in dw.CORNER_SCALES])
def test_corner_rays_tell_stored_from_rebuilt_bounds(scale):
    """The search of the two CPU walkers (fixed seed). At 1e3 float error stays below the builder's 1e-4 cut margin and next to nothing
    differs; at 1e6 and 1e7 the search must find its rays. Independent of results: on more than half of all candidates some pop's
    rebuilt bound is not the stored one, which is the falsity of `max_dist of an entry = min_dist of the entry beneath`."""
    keep, found, popped = _corner_found(scale)
    print(f"scale {scale:g}: {found} of {dw.CORNER_CANDIDATES} corner-aimed rays differ between the walkers, {len(keep)} kept; "
          f"{popped:.1%} have a pop whose rebuilt bound differs")
    assert popped > 0.5
    if scale >= 1e6:
        assert len(keep) == dw.CORNER_KEEP >= 8
    # the kept rays are the frozen ones (the fixture holds them as given and as the reference used them)
    if os.path.exists(FIXTURE):
        g = np.load(FIXTURE)
        tag = f"corner_{dw.scale_tag(scale)}"
        np.testing.assert_array_equal(_bits(g[tag + "_rays_in"][:int(g[tag + "_n_differ"])]), _bits(keep))


def test_the_two_walkers_agree_where_no_bound_differs(ora):
    """The foil is the reference's walk except for the rebuilt bound: wherever no pop differed, the records are equal."""
    d, o = _scene(dw.CORNER, 1e7)
    rays = dw.corner_rays(1e7, 20_000, rng_seed=9)
    a, ai = o.mesh_intersect(0, rays)
    b, bi, popped = o.mesh_intersect_recon(0, rays)
    same = ~popped
    assert same.sum() > 200
    assert not dw.records_differ(a[same], ai[same], b[same], bi[same]).any()


# ---------------------------------------------------------------------------- GPU
def _route_scenes(ptx, ctx, mp, d, n_surf=1):
    """(name, scene, expected pipeline) per forced route, each asserted from the scene's residency and from the pipeline a tiny render
    reports; leaves PTX_WAVEFRONT set for the route when the caller iterates (generator). The scenes are the test's own: created under the
    route's PTX_WAVEFRONT, one LDS scene for the test."""
    s_lds = None
    for route in forced_routes(n_surf):
        mp.setenv("PTX_WAVEFRONT", route.env["PTX_WAVEFRONT"])
        if route.force_global:
            s = under_force_global(mp, True, lambda: product_from_dict(ptx, ctx, d))
        else:
            s = s_lds = s_lds or product_from_dict(ptx, ctx, d)
        assert_route(ctx, s, route, route.name)
        yield route.name, s, route.pipeline


@pytest.mark.gpu
@pytest.mark.parametrize("scale", dw.DEEP_SCALES, ids=[dw.scale_tag(s) for s in dw.DEEP_SCALES])
def test_deep_batch_every_route(ptx, ctx, ora, clean_env, scale):
    """ptx_intersect_batch on 262 144 rays whose walks hold up to 20-22 pending entries (test_deep_rays_cover_the_pending_stack), on the
    LDS fused, global fused and queue routes: every record the oracle's, no ray excluded, and the routes bitwise equal."""
    d, o = _scene(dw.DEEP, scale)
    rays, is_deep, out, idx, depth, hist = _deep_batch(scale)
    first = None
    for name, s, pipeline in _route_scenes(ptx, ctx, clean_env, d):
        hits = s.intersect(rays[:, :3], rays[:, 3:])
        _check_records(hits, o, rays, out, idx)
        if first is None:
            first = hits
        else:
            _same_hits(hits, first, name)


@pytest.mark.gpu
@pytest.mark.parametrize("scale", dw.CORNER_SCALES, ids=[dw.scale_tag(s) for s in dw.CORNER_SCALES])
def test_differing_rays_every_route(ptx, ctx, ora, clean_env, scale):
    """The rays on which a walk with rebuilt far bounds returns other records than the reference's (the CPU search above), mixed at
    random positions into a batch of ordinary deep rays of the same mesh: every record of every route is the oracle's, and on the
    frozen rays the compiled reference's."""
    d, o = _scene(dw.CORNER, scale)
    keep, found, _ = _corner_found(scale)
    if scale >= 1e6:
        assert len(keep) >= 8
    rng = np.random.default_rng(5)
    rays = dw.deep_rays(scale, 16_384, cfg=dw.CORNER)[0].copy()
    at = rng.choice(len(rays), len(keep), replace=False)
    rays[at] = keep
    out, idx = o.intersect(rays)
    g = dict(np.load(FIXTURE)) if os.path.exists(FIXTURE) else None
    tag = f"corner_{dw.scale_tag(scale)}"
    first = None
    for name, s, pipeline in _route_scenes(ptx, ctx, clean_env, d):
        hits = s.intersect(rays[:, :3], rays[:, 3:])
        wrong = hits["surface"][at] != idx[at]
        wrong |= (_bits(hits["distance"][at]) != _bits(o.model_intersect(0, rays[at])[0][:, 0])) & (idx[at] >= 0)
        print(f"scale {scale:g}, {name}: {int(wrong.sum())} of the {len(at)} differing rays are not the oracle's")
        _check_records(hits, o, rays, out, idx)
        if first is None:
            first = hits
        else:
            _same_hits(hits, first, name)
        if g is not None:
            fr = g[tag + "_rays"]
            fh = s.intersect(fr[:, :3], fr[:, 3:])
            fi, fo, fm, fmi = g[tag + "_scene_idx"], g[tag + "_scene_out"], g[tag + "_model_out"][:, 0], g[tag + "_model_idx"][:, 0]
            hit = fi >= 0
            np.testing.assert_array_equal(fh["surface"], fi, err_msg=name)
            np.testing.assert_array_equal(_bits(fh["distance"][hit]), _bits(fm[hit, 0]), err_msg=name)
            np.testing.assert_array_equal(fh["triangle"][hit], fmi[hit, 1], err_msg=name)
            np.testing.assert_array_equal(_bits(np.stack([fh["b0"], fh["b1"], fh["b2"]], 1)[hit]), _bits(fm[hit, 1:4]), err_msg=name)
            np.testing.assert_array_equal(_bits(np.stack([fh["px"], fh["py"], fh["pz"]], 1)[hit]), _bits(fo[hit, 0:3]), err_msg=name)
            np.testing.assert_array_equal(_bits(np.stack([fh["nx"], fh["ny"], fh["nz"]], 1)[hit]), _bits(fo[hit, 11:14]), err_msg=name)


def _render_checks(ptx, ctx, ora, mp, s, o, what, pipeline, ref, state):
    """Per-sample radiance of both integrators against the oracle (test_unit_limits' criterion), and frame, ray count and guide buffers
    bitwise those of the first route (`state` carries them)."""
    for ig in (0, 1):
        got = np.zeros_like(ref[ig])
        for k in range(SPP):
            a, _ = s.render(W, H, 1, B, sample0=k, integrator=ig)
            assert ctx.timing()["pipeline"] == pipeline, what
            got[:, :, k] = a[..., :3]
        assert np.isfinite(got).all()
        err = np.abs(got - ref[ig]).max(-1) / np.maximum(np.abs(ref[ig]).max(-1), 1e-3)
        print(f"{what} integrator {ig}: {(err < 1e-3).mean():.4%} of samples agree")
        assert (err < 1e-3).mean() > 0.995, f"{what} integrator {ig}: {(err < 1e-3).mean():.4%} of samples agree"
        frame, st = s.render(W, H, SPP, B, integrator=ig)
        assert ctx.timing()["pipeline"] == pipeline, what
        if ("frame", ig) not in state:
            state["frame", ig], state["rays", ig] = frame, st["rays"]
        else:
            np.testing.assert_array_equal(_bits(frame), _bits(state["frame", ig]), err_msg=f"{what} integrator {ig}")
            assert st["rays"] == state["rays", ig], what
    alb, nd, _ = s.render_aov(W, H, SPP)
    if "aov" not in state:
        state["aov"] = (alb, nd)
        assert (alb[..., 3] > 0).any()
    else:
        np.testing.assert_array_equal(_bits(alb), _bits(state["aov"][0]), err_msg=what)
        np.testing.assert_array_equal(_bits(nd), _bits(state["aov"][1]), err_msg=what)


@pytest.mark.gpu
@pytest.mark.parametrize("sun", [False, True], ids=["no-sun", "sun"])
def test_renders_of_the_cluster_every_route(ptx, ctx, ora, clean_env, sun):
    """64 x 36, 3 samples, 5 bounces from inside the innermost cell: the walk inside k_render_pass, its deferral sweeps, the shadow
    any-hit sweep (with a sun) and the queue steps, all on walks of up to 20 pending entries."""
    d, o = _scene(dw.DEEP, 1e3, sun)
    prim = o.primary_rays(ora.make_cfg(W, H, 1, B), 0).reshape(-1, 6)
    _, _, depth, _ = o.mesh_intersect(0, prim, stats=True)
    assert depth.max() >= 18 and (depth >= 16).mean() > 0.1           # the camera's own rays walk deep
    ref = {ig: o.render_samples(ora.make_cfg(W, H, SPP, B, integrator=ig), threads=0) for ig in (0, 1)}
    state = {}
    for name, s, pipeline in _route_scenes(ptx, ctx, clean_env, d):
        assert s.info()["has_sun"] == int(sun)
        for un in (["0", "1"] if pipeline == 0 else [None]):
            if un is None:
                clean_env.delenv("PTX_SURFACE_UNITS", raising=False)
            else:
                clean_env.setenv("PTX_SURFACE_UNITS", un)
            _render_checks(ptx, ctx, ora, clean_env, s, o, f"{name} units={un}", pipeline, ref, state)


@pytest.mark.gpu
def test_ten_surface_variant_default_route_and_deferral(ptx, ctx, ora, clean_env):
    """Nine clusters and a backdrop in one model: the queue pipeline without switches, then the fused (hybrid) kernel with and without
    surface units, whose deferral sweeps walk the clusters. Deep rays against the oracle, renders against the oracle, everything
    bitwise across the three."""
    d, o = _scene(dw.DEEP, 1e3, True, True)
    rays = dw.deep_rays(1e3, 32_768)[0]
    out, idx, st = o.intersect(rays, stats=True)
    hist = st[6:38]
    assert int(np.flatnonzero(hist).max()) >= 18 and len(np.unique(idx[idx >= 0])) == 10
    ref = {ig: o.render_samples(ora.make_cfg(W, H, SPP, B, integrator=ig), threads=0) for ig in (0, 1)}
    s = product_from_dict(ptx, ctx, d)
    assert s.info()["lds_resident"] == 2
    state, first = {}, None
    for what, wf, un, pipeline in (("default", None, None, 1), ("fused units=0", "0", "0", 0), ("fused units=1", "0", "1", 0)):
        for var, val in (("PTX_WAVEFRONT", wf), ("PTX_SURFACE_UNITS", un)):
            if val is None:
                clean_env.delenv(var, raising=False)
            else:
                clean_env.setenv(var, val)
        hits = s.intersect(rays[:, :3], rays[:, 3:])
        _check_records(hits, o, rays, out, idx)
        if first is None:
            first = hits
        else:
            _same_hits(hits, first, what)
        _render_checks(ptx, ctx, ora, clean_env, s, o, what, pipeline, ref, state)


@pytest.mark.gpu
@pytest.mark.parametrize("n", [1, 65])
def test_small_batches_at_the_maximum_depth(ptx, ctx, ora, clean_env, n):
    """One ray, and 65 (one full wave and one lane of the next): every walk at the maximum pending depth, so a wave's single busy lane
    spills while its neighbours are idle."""
    d, o = _scene(dw.DEEP, 1e3)
    all_rays, _, _, _, depth, _ = _deep_batch(1e3)
    rays = all_rays[np.flatnonzero(depth == depth.max())[:n]]
    assert len(rays) == n
    out, idx = o.intersect(rays)
    first = None
    for name, s, pipeline in _route_scenes(ptx, ctx, clean_env, d):
        hits = s.intersect(rays[:, :3], rays[:, 3:])
        _check_records(hits, o, rays, out, idx)
        if first is None:
            first = hits
        else:
            _same_hits(hits, first, name)
