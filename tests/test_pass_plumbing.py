"""The host plumbing every render entry point shares (csrc/api_internal.hpp: the pass frame, Staged, the workspace carver) gives the same
bytes whichever way a frame is asked for.

Per entry point the baseline is the host-buffer, single-pass frame with stats requested — the configuration the per-feature tests pin
against the oracle or the restatement (test_gpu_parity, test_transparent_background, test_aov, test_nee, test_adaptive). Asserted bitwise
equal to it: torch device buffers with stats = NULL (the call returns without a sync), an uneven last pass, an odd tile against the same
crop, two interleaved shards rendered into one buffer. Cornell runs on the fused kernel and through the queue pipeline (two of
tests/_routes.py's DEFAULT_ROUTES); the alpha chart with a sun makes ptx_render_aov's pass-through rounds and ptx_render_nee's second
read-back of a round run.
tests/test_nee.py::test_composition_bitwise_on_cornell and its siblings in test_aov / test_adaptive hold the wider sweeps per feature.
"""
import numpy as np
import pytest

from _nee_common import SEED, _make
from _routes import DEFAULT_ROUTES, Scenes, clean_env, ctx, use_route  # noqa: F401  (clean_env and ctx are fixtures)

ENTRIES = ("render", "render_transparent", "render_aov", "render_nee")
TILE = (5, 3, 17, 11)
ROUTES = [r for r in DEFAULT_ROUTES if r.name in ("lds fused", "queue")]
SCENES = Scenes(_make)


def _scene(ptx, ctx, mp, name, force_global):
    return SCENES.get(ptx, ctx, mp, name, force_global)


def _frame(s, entry, W, H, spp, bounces, device=False, shards=(None,), min_spp=2, **kw):
    """(the entry point's output buffers as numpy arrays, the last call's stats). device: torch tensors on the GPU, stats = NULL, then
    ptx_ctx_synchronize. shards: one call per entry, all into the same buffers."""
    x0, y0, w, h = kw.get("tile") or (0, 0, W, H)
    shapes = [(h, w, 4), (h, w)] if entry == "render_transparent" else [(h, w, 4)] * (1 if entry in ("render", "render_nee") else 2)
    if device:
        import torch
        bufs = [torch.zeros(sh, dtype=torch.uint8 if len(sh) == 2 else torch.float32, device="cuda") for sh in shapes]
    else:
        bufs = [np.zeros(sh, np.uint8 if len(sh) == 2 else np.float32) for sh in shapes]
    kw.update(seed=SEED, want_stats=not device)
    for shard in shards:
        kw["shard"] = shard
        if entry == "render":
            st = s.render(W, H, spp, bounces, accum=bufs[0], **kw)[-1]
        elif entry == "render_nee":
            st = s.render_nee(W, H, spp, bounces, accum=bufs[0], **kw)[-1]
        elif entry == "render_transparent":
            st = s.render_transparent(W, H, spp, bounces, pixels=bufs[0], claimed=bufs[1], **kw)[-1]
        elif entry == "render_aov":
            st = s.render_aov(W, H, spp, albedo=bufs[0], normal_depth=bufs[1], **kw)[-1]
        else:
            st = s.render_adaptive(W, H, spp, bounces, min_spp=min_spp, threshold=0.0, a=bufs[0], b=bufs[1], **kw)[-1]
    assert (st is None) == device
    if device:
        s.ctx.synchronize()
        return [b.cpu().numpy() for b in bufs], st
    return bufs, st


def _same(got, want, what):
    assert len(got) == len(want)
    for g, w in zip(got, want):
        np.testing.assert_array_equal(np.ascontiguousarray(g).view(np.uint8), np.ascontiguousarray(w).view(np.uint8), err_msg=what)


def _check_entry(s, entry, W, H, spp, bounces, what):
    base, st = _frame(s, entry, W, H, spp, bounces)
    assert st["passes"] == 1 and st["samples"] == W * H * spp and any(b.any() for b in base), what
    _same(_frame(s, entry, W, H, spp, bounces, device=True)[0], base, f"{what}: device buffers, stats = NULL")
    got, st = _frame(s, entry, W, H, spp, bounces, spp_per_pass=2)
    assert st["passes"] == (spp + 1) // 2 and spp % 2 == 1
    _same(got, base, f"{what}: spp_per_pass = 2")
    x0, y0, w, h = TILE
    for device in (False, True):
        _same(_frame(s, entry, W, H, spp, bounces, device=device, tile=TILE)[0], [b[y0:y0 + h, x0:x0 + w] for b in base], f"{what}: tile, device = {device}")
    for device in (False, True):
        _same(_frame(s, entry, W, H, spp, bounces, device=device, shards=[(0, 2, 8), (1, 2, 8)])[0], base, f"{what}: two shards into one buffer, device = {device}")


@pytest.mark.gpu
@pytest.mark.parametrize("route", ROUTES, ids=lambda r: r.name)
@pytest.mark.parametrize("entry", ENTRIES)
def test_cornell_frames_are_bitwise_the_baseline(ptx, ctx, clean_env, entry, route):
    name, force_global, env, resident, pipeline = route
    s = _scene(ptx, ctx, clean_env, "cornell", force_global)
    use_route(clean_env, route)
    assert s.info()["lds_resident"] == resident
    s.render(8, 8, 1, 1)
    assert ctx.timing()["pipeline"] == pipeline, name
    _check_entry(s, entry, 32, 24, 3, 3, f"cornell / {name} / {entry}")


@pytest.mark.gpu
@pytest.mark.parametrize("entry", ["render_aov", "render_nee"])
def test_alpha_chart_rounds_are_bitwise_the_baseline(ptx, ctx, clean_env, entry):
    s = _scene(ptx, ctx, clean_env, "chart_alpha_sun", False)
    _check_entry(s, entry, 48, 40, 3, 3, f"chart_alpha_sun / {entry}")


@pytest.mark.gpu
@pytest.mark.parametrize("route", ROUTES, ids=lambda r: r.name)
@pytest.mark.parametrize("min_spp,spp", [(2, 6), (4, 8)])
def test_adaptive_subset_rounds(ptx, ctx, clean_env, route, min_spp, spp):
    """threshold = 0: every round after the first renders the active list (PixelSubset) into the halves staged once. min_spp = 4 gives
    halves of two samples, which spp_per_pass = 1 cuts into two passes each."""
    name, force_global, env, resident, pipeline = route
    s = _scene(ptx, ctx, clean_env, "cornell", force_global)
    base, st = _frame(s, "render_adaptive", 32, 24, spp, 3, min_spp=min_spp)
    assert st["rounds"] == 1 + (spp - min_spp) // min_spp and 0 < st["active_last"] and st["samples"] > 32 * 24 * min_spp
    _same(_frame(s, "render_adaptive", 32, 24, spp, 3, min_spp=min_spp, device=True)[0], base, f"{name}: device buffers")
    got, st1 = _frame(s, "render_adaptive", 32, 24, spp, 3, min_spp=min_spp, spp_per_pass=1)
    assert st1["passes"] == st["passes"] * (min_spp // 2)
    _same(got, base, f"{name}: spp_per_pass = 1")
