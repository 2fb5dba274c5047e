"""The fused kernel's sweeps at their boundaries: pass sizes around the wave width and the chunk size, pixel-list passes, and the other
kernels that share the walk (mesh_traverse / spill_get, device_core.hpp).

k_render_pass walks a wave's stream 64 entries at a time; every sweep has a last wave-iteration with 1 to 64 live lanes, a wave takes
its paths in chunks, and the loads and stores of one wave-iteration are in flight while the next begins (the walk no longer waits for
vector memory: spill_get completes its load inside its rare branch, the EXTEND sweep consumes its entry where it loads it). None of
that may change a bit of any frame, whatever the number of camera paths a pass holds: 1 lane in the last iteration, exactly full, one
over, one entry past a chunk.

  1. Cornell tiles and sample settings whose passes hold 1 ... 4097 camera paths against the same pixels of the full 96 x 54 frame at the
     same sample count (the library promises equality for any tiling and pass size); ray counts add up over a partition of the frame.
  2. Interleaved tile sharding (multigpu.render_tiles, world = 3, every rank in turn on the one GPU): pixel-list passes whose sizes are no
     multiples of 64; the sum is the plain frame.
  3. The hybrid plaza (SUN variants: a shadow sweep between SHADE and the next EXTEND) against the same scene in the global-memory
     kernels, and both against the oracle sample by sample.
The spill rows themselves (20-22 pending entries inside k_render_pass, its deferral and shadow sweeps, on the LDS, global and queue
routes) are tests/test_deep_walks.py::test_renders_of_the_cluster_every_route.
Everything is bitwise except the comparison with the oracle.
"""
import importlib

import numpy as np
import pytest

from _common import _proc
from _routes import ctx, under_force_global  # noqa: F401  (ctx is a fixture)
from conftest import CORNELL, oracle_from_dict, product_from_dict

W, H, B = 96, 54, 8
VARS = ("PTX_WAVEFRONT", "PTX_FORCE_GLOBAL", "PTX_SURFACE_UNITS", "PTX_NO_HYBRID", "PTX_LDS_LEAF_ORDER", "PTX_LDS_BUDGET", "PTX_NO_HOT_HITREC")

# (camera paths per pass, tile (x, y, w, h), spp, spp_per_pass): w * h * spp_per_pass paths in every pass. 127, 683 (2049 = 3 * 683) and
# 241 (4097 = 17 * 241) are primes larger than the frame is wide, so those counts come from the sample count
PASSES = [
    (1, (5, 7, 1, 1), 4, 1),
    (63, (3, 2, 21, 3), 4, 1),
    (64, (10, 20, 64, 1), 4, 1),
    (65, (31, 49, 13, 5), 4, 1),
    (127, (95, 53, 1, 1), 127, 127),
    (128, (0, 0, 32, 2), 4, 2),
    (129, (7, 11, 43, 3), 4, 1),
    (2047, (0, 0, 89, 23), 4, 1),
    (2048, (32, 0, 64, 32), 4, 1),
    (2049, (40, 30, 3, 1), 683, 683),
    (4097, (79, 37, 17, 1), 241, 241),
]
# a partition of the frame: its upper left tile is the 2047-path one
PARTITION = [(0, 0, 89, 23), (89, 0, 7, 23), (0, 23, 96, 31)]


@pytest.fixture
def env(monkeypatch):
    for v in VARS:
        monkeypatch.delenv(v, raising=False)
    return monkeypatch


@pytest.fixture(scope="module")
def cornell(ptx, ctx):
    return ptx.Scene.load_gltf(ctx, CORNELL)


_full = {}


def _full_frame(scene, spp, bounces):
    """The full frame at (spp, bounces) with the library's own pass size: rendered once, read-only afterwards."""
    if (spp, bounces) not in _full:
        frame, st = scene.render(W, H, spp, bounces)
        frame.setflags(write=False)
        _full[spp, bounces] = (frame, st["rays"])
    return _full[spp, bounces]


def _cut(frame, tile):
    x, y, w, h = tile
    return np.ascontiguousarray(frame[y:y + h, x:x + w])


# ---------------------------------------------------------------------------- 1. sweep boundaries
def test_pass_sizes_are_what_they_claim():
    for n, (x, y, w, h), spp, per_pass in PASSES:
        assert w * h * per_pass == n and spp % per_pass == 0 and x + w <= W and y + h <= H, n
    assert [p[0] for p in PASSES] == [1, 63, 64, 65, 127, 128, 129, 2047, 2048, 2049, 4097]
    cover = np.zeros((H, W), int)
    for x, y, w, h in PARTITION:
        cover[y:y + h, x:x + w] += 1
    assert (cover == 1).all() and PARTITION[0] == PASSES[7][1]


@pytest.mark.gpu
@pytest.mark.parametrize("n, tile, spp, per_pass", PASSES, ids=[str(p[0]) for p in PASSES])
def test_pass_of_n_paths_equals_the_full_frame(cornell, env, n, tile, spp, per_pass):
    full, _ = _full_frame(cornell, spp, B)
    got, st = cornell.render(W, H, spp, B, tile=tile, spp_per_pass=per_pass)
    assert st["passes"] == spp // per_pass and st["samples"] == tile[2] * tile[3] * spp
    assert got.tobytes() == _cut(full, tile).tobytes()
    assert np.isfinite(got).all() and (got[..., 3] == spp).all() and st["rays"] >= st["samples"]


@pytest.mark.gpu
@pytest.mark.parametrize("bounces", [0, 1, 8])
def test_partition_adds_up(cornell, env, bounces):
    """One sample per pass in every tile (2047, 161 and 2976 paths), four samples; bounces 0 and 1 have no second step."""
    full, rays = _full_frame(cornell, 4, bounces)
    total = 0
    for tile in PARTITION:
        got, st = cornell.render(W, H, 4, bounces, tile=tile, spp_per_pass=1)
        assert st["passes"] == 4
        assert got.tobytes() == _cut(full, tile).tobytes(), tile
        total += st["rays"]
    assert total == rays
    if bounces < 2:
        assert rays == bounces * W * H * 4          # one ray per path and step, and no step after the first
    else:
        assert rays > 2 * W * H * 4


@pytest.mark.gpu
@pytest.mark.parametrize("bounces", [0, 1])
@pytest.mark.parametrize("n, tile, spp, per_pass", [PASSES[i] for i in (0, 3, 6, 8)], ids=[str(PASSES[i][0]) for i in (0, 3, 6, 8)])
def test_short_paths_at_the_boundaries(cornell, env, bounces, n, tile, spp, per_pass):
    full, _ = _full_frame(cornell, spp, bounces)
    got, st = cornell.render(W, H, spp, bounces, tile=tile, spp_per_pass=per_pass)
    assert got.tobytes() == _cut(full, tile).tobytes()
    assert st["rays"] == bounces * tile[2] * tile[3] * spp


# ---------------------------------------------------------------------------- 2. pixel-list passes
@pytest.mark.gpu
def test_interleaved_tiles_of_three_ranks_sum_to_the_frame(ptx, cornell, env):
    mg = importlib.import_module("distributed-path-tracer_amd.multigpu")
    full, rays = _full_frame(cornell, 4, B)
    world, ts = 3, 20                      # 5 x 3 tiles of 20 x 20 (16 wide / 14 high at the edges), dealt out in turn
    total, n_rays = np.zeros((H, W, 4), np.float32), 0
    for rank in range(world):
        n_px = int(mg.tile_mask(rank, world, W, H, ts).sum())
        assert n_px % 64 != 0 and n_px > 64, (rank, n_px)          # 1800, 1680, 1704 pixels: the last wave-iteration of a pass is ragged
        acc = np.zeros((H, W, 4), np.float32)
        st = mg.render_tiles(cornell, W, H, 4, B, acc, rank, world, tile=ts, spp_per_pass=1)
        assert st["samples"] == n_px * 4 and st["passes"] == 4
        assert (acc[~mg.tile_mask(rank, world, W, H, ts)] == 0).all()
        total += acc
        n_rays += st["rays"]
    assert total.tobytes() == full.tobytes() and n_rays == rays


# ---------------------------------------------------------------------------- 3. the other kernels that share the walk
@pytest.mark.gpu
def test_hybrid_and_global_plaza_agree_and_match_the_oracle(ptx, ctx, ora, env):
    d = _proc().plaza_scene(level=3, sun=True, alpha=False)
    spp = 4
    env.setenv("PTX_WAVEFRONT", "0")
    hyb = product_from_dict(ptx, ctx, d)
    glb = under_force_global(env, True, lambda: product_from_dict(ptx, ctx, d))
    assert hyb.info()["lds_resident"] == 2 and glb.info()["lds_resident"] == 0 and hyb.info()["has_sun"] == 1
    frames = {}
    for name, s in (("hybrid", hyb), ("global", glb)):
        frame, st = s.render(W, H, spp, B)
        assert ctx.timing()["pipeline"] == 0, name                    # the fused kernel, not the queue pipeline
        smp = np.zeros((H, W, spp, 3), np.float32)
        for k in range(spp):
            a, _ = s.render(W, H, 1, B, sample0=k)
            smp[:, :, k] = a[..., :3]
        frames[name] = (frame, st["rays"], smp)
    assert frames["hybrid"][0].tobytes() == frames["global"][0].tobytes() and frames["hybrid"][1] == frames["global"][1]
    assert frames["hybrid"][2].tobytes() == frames["global"][2].tobytes()
    assert frames["hybrid"][1] > W * H * spp
    # tests/test_gpu_parity.py::test_per_sample_radiance_matches_oracle's tolerance
    ref = oracle_from_dict(ora, d).render_samples(ora.make_cfg(W, H, spp, B), threads=0)
    for name in frames:
        got = frames[name][2]
        assert np.isfinite(got).all()
        err = np.abs(got - ref).max(-1) / np.maximum(np.abs(ref).max(-1), 1e-3)
        print(f"{name}: {(err < 1e-3).mean():.4%} of samples within 1e-3, {(err < 1e-5).mean():.4%} within 1e-5")
        assert (err < 1e-3).mean() > 0.995, name
        assert (err < 1e-5).mean() > 0.98, name
    hyb.close()
    glb.close()
