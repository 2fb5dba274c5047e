"""PTX_INTEGRATOR_WORKER pinned to the COMPILED HOST worker of the reference.

oracle/host_harness.cpp links the reference's own src/processors/worker/*.cpp and src/scene/*.cpp, unmodified, against stand-in
headers (oracle/host_stubs/) and runs the worker's stage functions on one thread, one sample at a time. Its records are the fixtures
tests/golden/worker_trace.npz, worker_frame.npz and worker_scene.npz (oracle/make_golden.py --only-worker). Here

  * the oracle's trace_worker replays the reference's three std::mt19937 streams (jitter / sun cone / shading: core::rand() is a
    `static` function, one copy per translation unit) and must return the recorded colour BITS of every sample (CPU);
  * the oracle's restatement of the glTF loader with the scene_work primitive filter must give the arrays the HOST loader built (CPU);
  * the device kernels, on every route, must give the recorded bits of the frames no random draw reaches (GPU).

meta = [ORACLE_SEED, k of the jitter / sun-cone / shading stream, X, Y, spp, bounces]: the k-th mt19937 that is seeded gets the seed
ORACLE_SEED + 7919 k; 0xFFFFFFFF = the run never seeded that stream.
"""
import os

import numpy as np
import pytest

from _common import _bits
from _routes import Scenes, clean_env, ctx, each_route  # noqa: F401  (clean_env and ctx are fixtures)
from conftest import CORNELL, GOLD, JACK, ROOT

NEVER = 0xFFFFFFFF
CHART = os.path.join(GOLD, "chart")
TRACE_SCENES = {"cornell": CORNELL, "jack": JACK, "chart": os.path.join(CHART, "chart.gltf"), "chart_facing": os.path.join(CHART, "chart_facing.gltf")}
FRAME_SCENES = {"cornell_3spp": CORNELL, "cornell_first": CORNELL, "chart_plain_first": os.path.join(CHART, "chart_plain.gltf")}
LIT = os.path.join(GOLD, "textures", "lit.gltf")
SCENE_WORK = {"lit_047": (LIT, {"lit": [0, 4, 7]}), "lit_rest": (LIT, {"lit": [1, 2, 3, 5, 6, 8, 9]}),
              "chart": (os.path.join(CHART, "chart.gltf"), None),
              "cornell_work": (CORNELL, {"Cube.003": [0, 2], "Sphere": [0], "No.Such.Mesh": [0]})}
HOST_HARNESS = os.path.join(ROOT, "oracle", "_ref", "host_harness")


def _seed(meta, i):
    return None if int(meta[i]) == NEVER else (int(meta[0]) + 7919 * int(meta[i])) & 0xFFFFFFFF


@pytest.fixture(scope="module")
def gold_wt():
    return dict(np.load(os.path.join(GOLD, "worker_trace.npz")))


@pytest.fixture(scope="module")
def gold_wf():
    return dict(np.load(os.path.join(GOLD, "worker_frame.npz")))


@pytest.fixture(scope="module")
def gold_ws():
    return dict(np.load(os.path.join(GOLD, "worker_scene.npz")))


_oracles, _replays = {}, {}


def _oracle(ora, path):
    if path not in _oracles:
        _oracles[path] = ora.OracleScene(ora.load_gltf(path))
    return _oracles[path]


def _replay(ora, gold_wt, tag):
    """(rgba, draws per stream, counts) of the oracle's replay of one worker_trace tag in the reference's argument order; computed once."""
    if tag not in _replays:
        meta = gold_wt[tag + "_meta"]
        _replays[tag] = _oracle(ora, TRACE_SCENES[tag]).trace_worker_mt(gold_wt[tag + "_rays"], int(meta[7]), (_seed(meta, 2), _seed(meta, 3)))
    return _replays[tag]


# ---------------------------------------------------------------------------- the estimator's composition, bit for bit
@pytest.mark.parametrize("tag", list(TRACE_SCENES))
def test_worker_composition_bit_exact(tag, gold_wt, ora):
    """The stage pipeline as a whole — INTERSECT's sun sample (intersection_worker.cpp:22-39), the shadow query (:49-67), SHADING
    (shading_worker.cpp:27-199: emissive before the opacity test, the catcher rule, the direct term, the [0, 10] throughput clamp,
    Russian roulette below bounce_count - 2, uint8_t bounce) — against the compiled worker: 2000 Cornell rays x 8 bounces, 4000
    jack-of-blades x 6, 4000 on the flat material chart and 10 000 between the facing charts x 6. The oracle draws from the reference's
    own streams at the points where it calls core::rand() and must return the same BITS for every ray. The streams are sequential over
    all rays: one draw too many or too few anywhere shifts everything after it.
    Two call sites pass two rand() calls as arguments of one call (intersection_worker.cpp:26, shading_worker.cpp:149); g++ evaluates
    both right to left, and the other order at either site disagrees on more than 2 % of the rows. Cornell has no sun: its sun-cone
    stream is never seeded and the oracle must not draw from it, so that site has no order to get wrong there."""
    sc = _oracle(ora, TRACE_SCENES[tag])
    rays, ref, meta = gold_wt[tag + "_rays"], gold_wt[tag + "_out"], gold_wt[tag + "_meta"]
    seeds = (_seed(meta, 2), _seed(meta, 3))
    assert int(meta[1]) == NEVER and seeds[1] is not None and (seeds[0] is not None) == (sc.a.sun is not None)
    out, n_draws, _ = _replay(ora, gold_wt, tag)
    assert n_draws[1] > len(rays) // 4 and (ref[:, :3].max(1) > 0).sum() > 50      # the fixture does shade surfaces
    np.testing.assert_array_equal(_bits(out), _bits(ref))
    assert (ref[:, 3] == 1).all()                                                  # shading_worker.cpp:36, 43, 91
    differ = lambda rtl: (_bits(sc.trace_worker_mt(rays, int(meta[7]), seeds, args_rtl=rtl)[0]) != _bits(ref)).any(1).mean()
    assert differ((True, False)) > 0.02
    if seeds[0] is None:
        assert n_draws[0] == 0
    else:
        assert n_draws[0] > 0 and differ((False, True)) > 0.02


def test_worker_fixtures_reach_every_branch(gold_wt, ora):
    """Counted by the oracle during the bit-exact replays: every material of both charts is the first hit of >= 20 rays; >= 50 opacity
    pass-throughs, >= 20 lit catcher pass-throughs, >= 20 catcher samples turned black, >= 50 paths ended by Russian roulette and >= 50
    vertices that survived it and were divided by p.
    The [0, 10] throughput clamp (shading_worker.cpp:175) was NEVER active: no vertex of the 20 000 paths had a component of brdf / pdf
    x throughput outside [0, 10], so these fixtures pin that the clamp leaves such values alone, not what it does to others."""
    total = {}
    for tag in TRACE_SCENES:
        _, _, c = _replay(ora, gold_wt, tag)
        if tag.startswith("chart"):
            assert c["first_hit"].min() >= 20, (tag, c["first_hit"].tolist())
        for k in ora.OracleScene.WORKER_COUNTS:
            total[k] = total.get(k, 0) + c[k]
    print(total)
    assert total["opacity_pass"] >= 50 and total["catcher_lit"] >= 20 and total["catcher_black"] >= 20, total
    assert total["rr_ended"] >= 50 and total["rr_survived"] >= 50, total
    assert total["shadow_rays"] >= 1000 and total["clamp_active"] == 0, total


# ---------------------------------------------------------------------------- generate_rays + the pipeline: whole frames
@pytest.mark.parametrize("tag", list(FRAME_SCENES))
def test_worker_frame_replays_bit_exact(tag, gold_wf, ora):
    """worker::generate_rays as it is (worker.cpp:114-149): samples in its order (x outer, y, sample) with its uuid; sample 0 of a
    pixel carries no jitter and draws nothing (with spp = 1 the jitter stream is never seeded), later samples carry the jitter
    stream's pair, drawn right to left like the other pairs. The function the oracle's primary_rays goes through gives the recorded
    camera rays bit for bit at those offsets, primary_rays(integrator = 1) itself gives sample 0's, and the colours replay bit for bit."""
    sc = _oracle(ora, FRAME_SCENES[tag])
    uuid, rays, ref, meta = (gold_wf[f"{tag}_{k}"] for k in ("uuid", "rays", "out", "meta"))
    X, Y, spp, b = (int(v) for v in meta[4:8])
    seeds = tuple(_seed(meta, i) for i in (1, 2, 3))
    assert (seeds[0] is None) == (spp == 1) and len(rays) == X * Y * spp
    u, off, r, out = sc.trace_worker_frame_mt(X, Y, spp, b, seeds)
    np.testing.assert_array_equal(u, uuid)
    off = off.reshape(X, Y, spp, 2)
    assert (off[:, :, 0] == 0).all()
    np.testing.assert_array_equal(_bits(r), _bits(rays))
    np.testing.assert_array_equal(_bits(out), _bits(ref))
    # sample 0 through the oracle's own entry point: [H, W, 6], against the fixture's x-outer order
    first = sc.primary_rays(ora.make_cfg(X, Y, 1, b, integrator=1), 0)
    np.testing.assert_array_equal(_bits(first.transpose(1, 0, 2)), _bits(rays.reshape(X, Y, spp, 6)[:, :, 0]))
    if spp > 1:
        assert (off[:, :, 1:] > 0).mean() > 0.99 and (off < 1).all()
        other = sc.trace_worker_frame_mt(X, Y, spp, b, seeds, args_rtl=(False, True, True))[2].reshape(X, Y, spp, 6)
        got = rays.reshape(X, Y, spp, 6)
        assert (_bits(other[:, :, 1:]) != _bits(got[:, :, 1:])).any(-1).mean() > 0.99
        np.testing.assert_array_equal(_bits(other[:, :, 0]), _bits(got[:, :, 0]))


def test_first_sample_at_one_bounce_is_a_function_of_the_scene(gold_wf, ora):
    """The two frames the device test compares with: un-jittered, one bounce — emission x 10 of the first hit, the environment factor
    on a miss, 0 behind a back face; no draw reaches the colour (the chart has no sun and no patch a ray passes through; Cornell neither).
    So the oracle's counter-based render_samples, the one the kernels are compared with everywhere else, gives the same bits."""
    for tag in ("cornell_first", "chart_plain_first"):
        sc = _oracle(ora, FRAME_SCENES[tag])
        meta = gold_wf[tag + "_meta"]
        X, Y, spp, b = (int(v) for v in meta[4:8])
        assert (spp, b) == (1, 1) and sc.a.sun is None and (sc.a.materials[:, 3] == 1).all() and not sc.a.materials[:, 10].any()
        ref = gold_wf[tag + "_out"].reshape(X, Y, 4).transpose(1, 0, 2)
        got = sc.render_samples(ora.make_cfg(X, Y, 1, 1, integrator=1), threads=0)[:, :, 0]
        np.testing.assert_array_equal(_bits(got), _bits(ref[..., :3]))
        # Cornell is a closed box: black walls and the light's 10; the chart: black patches, the environment (and the back face's
        # emissive 0.1 x 10, added before the back-face test), the two emissive patches
        values = np.unique(ref[..., :3].reshape(-1, 3), axis=0).tolist()
        want = [[0, 0, 0], [10, 10, 10]] if tag == "cornell_first" else [[0, 0, 0], [1, 1, 1], [2, 4, 8], [5, 3, 1]]
        assert values == want and (ref[..., :3] > 0).any(-1).sum() >= 16, values


# ---------------------------------------------------------------------------- the HOST loader and its primitive filter
@pytest.mark.parametrize("tag", list(SCENE_WORK))
def test_host_loader_and_primitive_filter(tag, gold_ws, ora):
    """cloud::distributed_scene::load_scene (src/scene/load_gltf.cpp) under scene_work filters: the oracle's load_gltf(work = ...) gives
    the arrays the HOST loader built (models in the order its intersect() visits them, unlisted meshes as empty models), and the
    oracle's intersect on the stored rays gives the recorded position, uv, normal, tangent and shading-normal bits of
    distributed_scene::intersect; intersect_min_result (src/scene/intersect.cpp:9-79) returns the same position and the shading normal."""
    path, work = SCENE_WORK[tag]
    g = {k[len(tag) + 1:]: v for k, v in gold_ws.items() if k.startswith(tag + "_")}
    a = ora.load_gltf(path, work=work)
    assert "\n".join(a.model_names) + "\n" == g["model_names"].tobytes().decode()
    for k in ("model_xform", "vertices", "materials", "camera"):
        np.testing.assert_array_equal(_bits(getattr(a, k)), _bits(g[k]), err_msg=k)
    for k in ("model_surf", "surf_range", "triangles", "material_tex"):
        np.testing.assert_array_equal(getattr(a, k), g[k], err_msg=k)
    if a.sun is None:
        assert g["sun"].size == 0
    else:
        np.testing.assert_array_equal(_bits(a.sun), _bits(g["sun"]))
    if work is not None:
        listed = sum(len(v) for v in work.values())
        assert 0 < len(a.surf_range) <= listed * 2 and len(a.surf_range) < len(ora.load_gltf(path).surf_range)
    out, idx = ora.OracleScene(a).intersect(g["ws_rays"])
    np.testing.assert_array_equal(idx, g["ws_idx"])
    np.testing.assert_array_equal(_bits(out), _bits(g["ws_out"]))
    hit = idx >= 0
    assert hit.sum() >= 100 and (~hit).sum() >= 20 and len(np.unique(idx[hit])) >= min(3, len(a.surf_range))
    mn = g["ws_min"]
    np.testing.assert_array_equal(mn[:, 0] != 0, hit)
    np.testing.assert_array_equal(_bits(mn[hit, 2:5]), _bits(out[hit, 0:3]))
    np.testing.assert_array_equal(_bits(mn[hit, 5:8]), _bits(out[hit, 11:14]))
    assert (mn[~hit, 1] == np.finfo(np.float32).max).all()


def test_regenerating_a_fixture_gives_the_committed_bytes(gold_wf, tmp_path):
    """Where the compiled worker exists (oracle/_ref/host_harness, built by pt_oracle.build() next to the reference), running it
    again gives the committed arrays byte for byte."""
    if not os.path.exists(HOST_HARNESS):
        pytest.skip("oracle/_ref/host_harness is not built here (needs the reference's sources)")
    from oracle import make_golden
    got = make_golden.worker_frame_arrays(dict(os.environ), "cornell_3spp", str(tmp_path))
    assert set(got) == {k for k in gold_wf if k.startswith("cornell_3spp_")}
    for k, v in got.items():
        assert v.dtype == gold_wf[k].dtype and v.shape == gold_wf[k].shape and v.tobytes() == gold_wf[k].tobytes(), k


# ---------------------------------------------------------------------------- GPU: the kernels against compiled worker output
@pytest.mark.gpu
@pytest.mark.parametrize("tag", ["cornell_first", "chart_plain_first"])
def test_gpu_first_sample_is_bitwise_the_compiled_worker(ptx, ctx, gold_wf, clean_env, tag):
    """ptx_render with integrator = 1, spp = 1, sample0 = 0, bounces = 1 against worker_frame.npz, ZERO tolerance, on every route (the
    default-choice routes of tests/_routes.py): the product's own glTF loader, camera, un-jittered primary ray, closest hit, material
    lookup, emissive x 10 / environment / back face, straight against what the reference's worker computed."""
    meta = gold_wf[tag + "_meta"]
    X, Y, spp, b = (int(v) for v in meta[4:8])
    ref = gold_wf[tag + "_out"].reshape(X, Y, 4).transpose(1, 0, 2)
    scenes = Scenes(lambda ptx, ctx, tag: ptx.Scene.load_gltf(ctx, FRAME_SCENES[tag]))      # this test's own
    for r, s in each_route(scenes, ptx, ctx, clean_env, tag):
        route, pipeline = r.name, r.pipeline
        a, _ = s.render(X, Y, spp, b, env=(1.0, 1.0, 1.0), sample0=0, integrator=1)
        assert ctx.timing()["pipeline"] == pipeline, route
        np.testing.assert_array_equal(_bits(a), _bits(ref), err_msg=f"{tag} / {route}")
