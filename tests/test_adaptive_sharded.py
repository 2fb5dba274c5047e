"""ptx_render_adaptive and ptx_render_adaptive_nee over interleaved tile shards (ptx_ctx_set_mask_exchange): the sum of the ranks' half-buffers
is bitwise the unsharded call's result.

CPU: the sharded loop of include/ptx.h restated in numpy (tests/_adaptive_shard_restatement.py) and run on the oracle's samples: all ranks in
lockstep give, summed, the bits of the unsharded replay (tests/_adaptive_restatement.py). The same replay shows that the inputs the GPU tests
use can tell a working exchange from a missing one: in every case some pixel is kept active ONLY by a noisy pixel another rank owns, and an
exchange that merges nothing gives another frame.

GPU, one process: rank q's call is given a scripted callback that plays the other ranks. From the product's own ptx_render / ptx_render_nee
snapshots of the rounds' half ranges the unsharded replay gives each round's full noisy mask M_r; the callback checks that the bytes the library
hands it are M_r restricted to q's pixels, and writes M_r back. Nothing blocks, and no threads are needed.

Common shape: 4 bounces, seed 0x5EED, 8 samples first, 8 per round.
"""
import collections
import ctypes as C
import importlib

import numpy as np
import pytest

import _adaptive_restatement as AR
import _adaptive_shard_restatement as SR
from _common import _bits, _proc, _same
from _nee_common import _oracle
from _nee_estimator import render_samples
from _routes import Route, Scenes, assert_route, clean_env, ctx, use_route  # noqa: F401  (clean_env and ctx are fixtures)
from conftest import CORNELL, oracle_from_dict, product_from_dict

B, SEED, MIN, STEP = 4, 0x5EED, 8, 8
f32 = np.float32
FUSED = 4

# name; scene; image size; the rendered rectangle (x0, y0, w, h); shard tile; threshold; cap; world sizes; the route of the GPU test; estimator
Case = collections.namedtuple("Case", "name scene W H rect tile thr cap worlds route nee")
CASES = [
    # tile 16 inside the decision's 32 x 32 tiles; the bottom tile row is 6 pixels high
    Case("plaza", "plaza", 96, 54, (0, 0, 96, 54), 16, 0.1, 64, (2, 3), Route("plaza", False, {}, 1, 0), False),
    # tile 12 cuts the decision's 8 x 8 blocks, and the rectangle's origin is no multiple of anything
    Case("plaza_rect", "plaza", 64, 48, (8, 4, 40, 30), 12, 0.1, 64, (2, 3), Route("plaza", False, {}, 1, 0), False),
    # two tiles for three ranks: rank 0 owns 64 columns, rank 1 one column, rank 2 nothing
    Case("thin", "atrium", 65, 7, (0, 0, 65, 7), 64, 0.1, 64, (3,), Route("atrium", True, {"PTX_WF_PAIRS_M": "1"}, 0, 1), False),
    Case("atrium_queue", "atrium", 48, 32, (0, 0, 48, 32), 8, 0.1, 40, (2, 3), Route("atrium", True, {"PTX_WF_PAIRS_M": "1"}, 0, 1), False),
    Case("cornell_nee", "cornell", 48, 27, (0, 0, 48, 27), 16, 0.2, 40, (2, 3), Route("cornell", False, {}, 1, 0), True),
]
CASE_IDS = [c.name for c in CASES]


def _mg():
    return importlib.import_module("distributed-path-tracer_amd.multigpu")


def _scene_dict(name):
    return {"plaza": lambda: _proc().plaza_scene(level=2, sun=True, alpha=False), "atrium": lambda: _proc().atrium_scene(detail=2)}[name]()


# ---------------------------------------------------------------------------- CPU: symbols and refusals
def test_symbols_are_declared_and_exported_and_a_null_context_is_refused(ptx):
    L = ptx.lib()
    for name in ("ptx_ctx_set_mask_exchange", "ptx_ctx_get_mask_exchange_stats"):
        assert name in ptx.declared_symbols() and hasattr(L, name), name
    assert hasattr(ptx.Context, "set_mask_exchange") and hasattr(ptx.Context, "mask_exchange_stats") and hasattr(_mg(), "render_adaptive_tiles")
    mask = np.zeros(16, np.uint8)
    fn = ptx.MASK_EXCHANGE_FN(lambda user, m, n: 0)
    assert L.ptx_ctx_set_mask_exchange(None, fn, None, mask.ctypes.data, mask.size) == ptx.ERR_INVALID
    assert "ptx_ctx_set_mask_exchange" in L.ptx_last_error().decode()
    assert L.ptx_ctx_set_mask_exchange(None, ptx.MASK_EXCHANGE_FN(), None, None, 0) == ptx.ERR_INVALID
    calls, ms = C.c_uint64(), C.c_double()
    assert L.ptx_ctx_get_mask_exchange_stats(None, C.byref(calls), C.byref(ms)) == ptx.ERR_INVALID
    assert "ptx_ctx_get_mask_exchange_stats" in L.ptx_last_error().decode()


def test_a_host_only_scene_points_at_the_setter(ptx):
    """No context, no registration: the refusal of shard_count > 1 stays, and its message names the way out."""
    s = product_from_dict(ptx, None, _proc().plaza_scene(1, sun=False, alpha=False))
    for call in (lambda: s.render_adaptive(96, 54, 40, B, shard=(0, 2, 16)), lambda: s.render_adaptive_nee(96, 54, 40, B, shard=(0, 2, 16))):
        with pytest.raises(ptx.PtxError) as e:
            call()
        assert e.value.code == ptx.ERR_UNSUPPORTED and "ptx_ctx_set_mask_exchange" in str(e.value), str(e.value)


def test_render_adaptive_tiles_refuses_the_transparent_blend():
    with pytest.raises(ValueError):
        _mg().render_adaptive_tiles(None, 8, 8, 8, 1, None, None, 0, 2, transparent=True)


# ---------------------------------------------------------------------------- CPU: ownership
def test_ownership_restated_equals_tile_mask():
    mg = _mg()
    for c in CASES:
        x0, y0, w, h = c.rect
        for world in (1, 2, 3, 5):
            masks = [SR.own_mask(q, world, c.W, c.rect, c.tile) for q in range(world)]
            assert (np.sum(masks, axis=0) == 1).all(), (c.name, world)
            for q, m in enumerate(masks):
                np.testing.assert_array_equal(m, mg.tile_mask(q, world, c.W, c.H, c.tile)[y0:y0 + h, x0:x0 + w], err_msg=f"{c.name} rank {q} of {world}")
    assert not SR.own_mask(2, 3, 65, (0, 0, 65, 7), 64).any() and SR.own_mask(1, 3, 65, (0, 0, 65, 7), 64).sum() == 7
    # tile 12 cuts 8 x 8 blocks: some block of the rectangle holds pixels of two ranks
    m = SR.own_mask(0, 2, 64, (8, 4, 40, 30), 12)
    assert any(0 < m[by:by + 8, bx:bx + 8].sum() < m[by:by + 8, bx:bx + 8].size for by in range(0, 30, 8) for bx in range(0, 40, 8))


# ---------------------------------------------------------------------------- CPU: the sharded loop on the oracle's samples
_sim = {}


def _oracle_samples(ora, c):
    """Per-sample radiance [H,W,cap,3] of the case's whole image from the oracle (ptx_render's estimator) or from the restated light-sampling
    estimator. Never modified."""
    key = (c.scene, c.W, c.H, c.cap, c.nee)
    if key not in _sim:
        if c.nee:
            o, a = _oracle(ora, c.scene)
            s = render_samples(ora, o, a, c.W, c.H, c.cap, B, seed=SEED)["rad"]
        else:
            if ("scene", c.scene) not in _sim:
                _sim["scene", c.scene] = oracle_from_dict(ora, _scene_dict(c.scene))
            s = _sim["scene", c.scene].render_samples(ora.make_cfg(c.W, c.H, c.cap, B, seed=SEED))
        s.setflags(write=False)
        _sim[key] = s
    return _sim[key]


def _running_sums(samples, cap):
    """[(A_r, B_r)]: the half-buffers of every pixel after round r, each sample added on its own, in order; w counts them."""
    h, w = samples.shape[:2]
    a, b = np.zeros((h, w, 4), f32), np.zeros((h, w, 4), f32)
    out, given = [], 0
    for k in AR.round_sizes(cap, MIN, STEP):
        for buf, s0 in ((a, given), (b, given + k // 2)):
            for s in range(s0, s0 + k // 2):
                buf += np.concatenate([samples[:, :, s], np.ones((h, w, 1), f32)], -1)
        given += k
        out.append((a.copy(), b.copy()))
    return out


def _oracle_snaps(ora, c):
    if ("snaps", c.name) not in _sim:
        _sim["snaps", c.name] = AR.crop(_running_sums(_oracle_samples(ora, c), c.cap), c.rect)
    return _sim["snaps", c.name]


def _check_replay(snaps, c, world, tile):
    """The lockstep replay against the unsharded one. -> the ranks"""
    want_a, want_b, want_rounds, want_last = AR.replay(snaps, c.thr)
    ranks = SR.replay_sharded(snaps, c.thr, world, tile, c.rect, c.W)
    what = f"{c.name} world {world} tile {tile}"
    _same(np.sum([q["a"] for q in ranks], axis=0, dtype=f32), want_a, what + ": sum of A")
    _same(np.sum([q["b"] for q in ranks], axis=0, dtype=f32), want_b, what + ": sum of B")
    assert [q["rounds"] for q in ranks] == [want_rounds] * world, what
    assert sum(q["active_last"] for q in ranks) == want_last, what
    for q in ranks:
        assert not q["a"][~q["own"]].any() and not q["b"][~q["own"]].any(), what
        _same(q["a"][q["own"]], want_a[q["own"]], what + ": own pixels of A")
    return ranks


@pytest.mark.parametrize("world", [2, 3])
@pytest.mark.parametrize("tile", [16, 12])
def test_simulation_on_the_oracle_plaza(ora, world, tile):
    """Measured on the oracle (96 x 54, threshold 0.1, cap 64): 8 rounds on every rank, 232 pixels active after the last decision, split
    121 + 111 over two ranks of 16-pixel tiles and 53 + 95 + 84 over three ranks of 12-pixel tiles."""
    c = CASES[0]
    ranks = _check_replay(_oracle_snaps(ora, c), c, world, tile)
    assert ranks[0]["rounds"] >= 3 and all(q["own"].any() for q in ranks)


def test_simulation_on_a_rectangle_and_on_a_frame_with_an_idle_rank(ora):
    c = CASES[1]
    for world in c.worlds:
        _check_replay(_oracle_snaps(ora, c), c, world, c.tile)
    c = CASES[2]
    ranks = _check_replay(_oracle_snaps(ora, c), c, 3, c.tile)
    assert [int(q["own"].sum()) for q in ranks] == [448, 7, 0]
    assert ranks[2]["rounds"] == ranks[0]["rounds"] > 1 and ranks[2]["active_last"] == 0 and len(ranks[2]["sent"]) == ranks[0]["rounds"]
    assert not any(m.any() for m in ranks[2]["sent"])   # it sends zeros in every round, and still sends


def _input_conditions(snaps, c, world):
    """What makes a case able to show a broken exchange; asserted on the CPU on the oracle's samples and on the GPU on the product's own."""
    what = f"{c.name} world {world}"
    ranks = SR.replay_sharded(snaps, c.thr, world, c.tile, c.rect, c.W)
    cross = [sum(q["cross"]) for q in ranks]
    assert sum(cross) > 0, f"{what}: no pixel is kept active only by a noisy pixel of another rank"
    alone = SR.replay_sharded(snaps, c.thr, world, c.tile, c.rect, c.W, merge=False)
    differs = [q for q in range(world) if not (np.array_equal(_bits(alone[q]["a"]), _bits(ranks[q]["a"])) and np.array_equal(_bits(alone[q]["b"]), _bits(ranks[q]["b"])))]
    assert differs, f"{what}: an exchange that merges nothing gives the same frame"
    return cross, differs


@pytest.mark.parametrize("c", CASES, ids=CASE_IDS)
def test_the_cases_can_show_a_missing_exchange(ora, c):
    """Measured on the oracle's samples, own pixels kept active only across a shard border, summed over the rounds, per rank: plaza 49 + 73 and
    40 + 47 + 35; plaza_rect 26 + 40 and 17 + 31 + 18; thin (atrium) 6 + 8 + 0; atrium_queue 27 + 40 and 28 + 22 + 17; cornell_nee 37 + 41 and
    26 + 23 + 4. The same 65 x 7 frame of the plaza has none (its last column is sky), which is why the thin frame is the atrium's."""
    snaps = _oracle_snaps(ora, c)
    for world in c.worlds:
        cross, differs = _input_conditions(snaps, c, world)
        print(f"{c.name} world {world}: kept active across a border, per rank {cross}; ranks whose frame differs without a merge {differs}")


# ---------------------------------------------------------------------------- GPU
def _make(ptx, ctx, name):
    return ptx.Scene.load_gltf(ctx, CORNELL) if name == "cornell" else product_from_dict(ptx, ctx, _scene_dict(name))


SCENES = Scenes(_make)
_snaps, _whole = {}, {}


def _scene(ptx, ctx, mp, c):
    s = SCENES.get(ptx, ctx, mp, c.scene, c.route.force_global)
    use_route(mp, c.route)
    assert_route(ctx, s, c.route, c.name)
    return s


def _render(s, c, flags, **kw):
    spp = kw.pop("spp")
    if c.nee:
        return s.render_nee(c.W, c.H, spp, B, flags=flags, **kw)
    return s.render(c.W, c.H, spp, B, **kw)


def _adaptive(s, c, flags, **kw):
    if c.nee:
        return s.render_adaptive_nee(c.W, c.H, c.cap, B, MIN, STEP, c.thr, seed=SEED, tile=c.rect, flags=flags, **kw)
    return s.render_adaptive(c.W, c.H, c.cap, B, MIN, STEP, c.thr, seed=SEED, tile=c.rect, **kw)


def _product_snaps(s, c, flags=0):
    """The product's own ptx_render / ptx_render_nee of the rounds' half ranges of the rectangle, snapshotted after every round. Cached; never
    modified."""
    key = (c.name, flags)
    if key not in _snaps:
        x0, y0, w, h = c.rect
        a, b = np.zeros((h, w, 4), f32), np.zeros((h, w, 4), f32)
        out, given = [], 0
        for k in AR.round_sizes(c.cap, MIN, STEP):
            _render(s, c, flags, spp=k // 2, accum=a, seed=SEED, sample0=given, tile=c.rect, want_stats=False)
            _render(s, c, flags, spp=k // 2, accum=b, seed=SEED, sample0=given + k // 2, tile=c.rect, want_stats=False)
            given += k
            fa, fb = a.copy(), b.copy()
            fa.setflags(write=False), fb.setflags(write=False)
            out.append((fa, fb))
        _snaps[key] = out
    return _snaps[key]


def _unsharded(s, c, flags=0):
    """The unsharded call's (a, b, stats) and the noisy masks M_r of its rounds, from the replay of the snapshots (which the call is checked
    against first). Cached; never modified."""
    key = (c.name, flags)
    if key not in _whole:
        snaps = _product_snaps(s, c, flags)
        a, b, st = _adaptive(s, c, flags)
        want_a, want_b, want_rounds, want_last = AR.replay(snaps, c.thr)
        _same(a, want_a, f"{c.name}: the unsharded call against the replay, A"), _same(b, want_b, f"{c.name}: the unsharded call against the replay, B")
        assert st["rounds"] == want_rounds and st["active_last"] == want_last
        one = SR.replay_sharded(snaps, c.thr, 1, c.tile, c.rect, c.W)[0]
        assert one["rounds"] == want_rounds
        a.setflags(write=False), b.setflags(write=False)
        _whole[key] = (a, b, st, one["sent"])
    return _whole[key]


def _host(x):
    return x if isinstance(x, np.ndarray) else x.cpu().numpy()


def _zeros(kind, shape, dtype=np.float32):
    if kind == "host":
        return np.zeros(shape, dtype)
    import torch
    t = torch.zeros(shape, dtype=torch.uint8 if dtype == np.uint8 else torch.float32, device="cuda:0")
    torch.cuda.synchronize()
    return t


def _rank(ctx, s, c, q, world, M, flags=0, merge=True, kind="host", mask_kind=None, fail_at=None, mask_bytes=None, shard=None, **kw):
    """Rank q's call with the scripted exchange. -> dict(a, b, st, log of the callback's complaints, its calls, the library's count of them,
    err: the PtxError or None)"""
    x0, y0, w, h = c.rect
    own = SR.own_mask(q, world, c.W, c.rect, c.tile)
    a, b = _zeros(kind, (h, w, 4)), _zeros(kind, (h, w, 4))
    mask = _zeros(mask_kind or kind, (mask_bytes if mask_bytes is not None else w * h,), np.uint8)
    log, calls = [], [0]

    def exchange(buf, n_bytes):
        r = calls[0]
        calls[0] += 1
        if fail_at is not None and r == fail_at:
            return 7
        if not merge:   # the negative control: every rank keeps its own bytes
            return 0
        if n_bytes != w * h or r >= len(M):
            log.append((q, r, "bytes or round", n_bytes))
            return 1
        got = _host(buf)[:n_bytes]
        if not np.array_equal(got, (M[r] * own).ravel()):
            log.append((q, r, "the incoming bytes are not the round's noisy mask restricted to the rank's pixels", int(got.sum()), int((M[r] * own).sum())))
            return 2
        if isinstance(buf, np.ndarray):
            buf[:n_bytes] = M[r].ravel()
        else:
            import torch
            buf[:n_bytes].copy_(torch.from_numpy(np.ascontiguousarray(M[r].ravel())))
            torch.cuda.synchronize()
        return 0

    ctx.set_mask_exchange(exchange, mask)
    st, err = None, None
    try:
        _, _, st = _adaptive(s, c, flags, a=a, b=b, shard=shard or (q, world, c.tile), **kw)
    except Exception as e:   # PtxError: the caller looks at it
        err = e
    finally:
        ctx.set_mask_exchange(None)
    ctx.synchronize()
    return dict(a=_host(a), b=_host(b), st=st, log=log, calls=calls[0], lib=ctx.mask_exchange_stats(), err=err, own=own)


SUMMED = ("rays", "samples", "active_last")


def _check_world(ctx, s, c, world, flags=0, **kw):
    ua, ub, ust, M = _unsharded(s, c, flags)
    what = f"{c.name} world {world} flags {flags} {kw}"
    want = SR.replay_sharded(_product_snaps(s, c, flags), c.thr, world, c.tile, c.rect, c.W)
    got = [_rank(ctx, s, c, q, world, M, flags, **kw) for q in range(world)]
    for q, g in enumerate(got):
        w_ = f"{what} rank {q}"
        assert g["err"] is None and not g["log"], (w_, g["err"], g["log"])
        own = g["own"]
        _same(g["a"][own], ua[own], w_ + ": own pixels of A"), _same(g["b"][own], ub[own], w_ + ": own pixels of B")
        assert not g["a"][~own].any() and not g["b"][~own].any(), w_ + ": other ranks' pixels are not zero any more"
        _same(g["a"], want[q]["a"], w_ + ": A against the lockstep replay"), _same(g["b"], want[q]["b"], w_ + ": B against the lockstep replay")
        assert g["st"]["rounds"] == ust["rounds"] == g["calls"] == g["lib"]["calls"], (w_, g["st"], g["calls"], g["lib"])
        assert g["st"]["active_last"] == want[q]["active_last"] and g["st"]["samples"] == (g["a"][..., 3] + g["b"][..., 3]).sum(), (w_, g["st"])
        assert g["lib"]["wall_ms"] > 0 and g["st"]["select_ms"] > 0, (w_, g["lib"], g["st"])
    _same(np.sum([g["a"] for g in got], axis=0, dtype=f32), ua, what + ": sum of A")
    _same(np.sum([g["b"] for g in got], axis=0, dtype=f32), ub, what + ": sum of B")
    for k in SUMMED + (("light_samples", "light_visible") if c.nee else ()):
        assert sum(g["st"][k] for g in got) == ust[k], (what, k, [g["st"][k] for g in got], ust[k])
    return got


@pytest.mark.gpu
@pytest.mark.parametrize("c", CASES[:4], ids=CASE_IDS[:4])
def test_sharded_ranks_sum_to_the_unsharded_call(ptx, ctx, clean_env, c):
    s = _scene(ptx, ctx, clean_env, c)
    snaps = _product_snaps(s, c)
    assert ctx.timing()["pipeline"] == c.route.pipeline
    for world in c.worlds:
        cross, differs = _input_conditions(snaps, c, world)   # the product's own samples meet them too
        got = _check_world(ctx, s, c, world)
        print(f"{c.name} world {world}: rounds {got[0]['st']['rounds']}, own active_last {[g['st']['active_last'] for g in got]}, across a border {cross}")
        # the negative control: the same calls with an exchange that merges nothing
        _, _, _, M = _unsharded(s, c)
        alone = SR.replay_sharded(snaps, c.thr, world, c.tile, c.rect, c.W, merge=False)
        for q in differs:
            g = _rank(ctx, s, c, q, world, M, merge=False)
            assert g["err"] is None and g["calls"] == alone[q]["rounds"], (q, g["err"], g["calls"], alone[q]["rounds"])
            _same(g["a"], alone[q]["a"], f"{c.name} world {world} rank {q}: without a merge, A"), _same(g["b"], alone[q]["b"], f"{c.name} world {world} rank {q}: without a merge, B")
            ua, ub = _unsharded(s, c)[:2]
            assert not (np.array_equal(_bits(g["a"][g["own"]]), _bits(ua[g["own"]])) and np.array_equal(_bits(g["b"][g["own"]]), _bits(ub[g["own"]]))), (c.name, world, q)
    if c.name == "thin":   # the rank without pixels renders nothing and takes part in every exchange
        idle = got[2]
        assert not idle["own"].any() and idle["st"]["samples"] == 0 and idle["st"]["rays"] == 0 and idle["calls"] == got[0]["st"]["rounds"] > 1


@pytest.mark.gpu
def test_light_sampling_estimator_fused_unfused_and_small_passes(ptx, ctx, clean_env):
    c = CASES[4]
    s = _scene(ptx, ctx, clean_env, c)
    for world in c.worlds:
        _input_conditions(_product_snaps(s, c, 0), c, world)
        for flags in (0, FUSED):
            got = _check_world(ctx, s, c, world, flags)
            assert ctx.timing()["fused_launches"] == (got[-1]["st"]["passes"] if flags else 0)
    _check_world(ctx, s, c, 3, FUSED, spp_per_pass=3)   # passes of 3, 3 and 2 samples: the halves' split falls inside the second


@pytest.mark.gpu
def test_mask_and_buffers_of_different_kinds(ptx, ctx, clean_env):
    c = CASES[0]
    s = _scene(ptx, ctx, clean_env, c)
    _check_world(ctx, s, c, 2, kind="dev", mask_kind="host")
    _check_world(ctx, s, c, 2, kind="host", mask_kind="dev")
    _check_world(ctx, s, c, 2, kind="dev")


@pytest.mark.gpu
def test_a_failing_exchange_ends_the_call_and_the_next_call_works(ptx, ctx, clean_env):
    c = CASES[0]
    s = _scene(ptx, ctx, clean_env, c)
    ua, ub, ust, M = _unsharded(s, c)
    snaps = _product_snaps(s, c)
    for kind in ("host", "dev"):
        g = _rank(ctx, s, c, 1, 2, M, fail_at=1, kind=kind)
        assert g["err"] is not None and g["err"].code == ptx.ERR_HIP and "mask exchange failed (status 7)" in str(g["err"]), g["err"]
        assert g["calls"] == 2 and g["lib"]["calls"] == 2 and not g["log"]
        # the buffers hold the completed rounds: two
        two = SR.replay_sharded(snaps[:2], c.thr, 2, c.tile, c.rect, c.W)[1]
        _same(g["a"], two["a"], f"{kind}: A after the failure"), _same(g["b"], two["b"], f"{kind}: B after the failure")
    # an exception inside the Python callback is a failure too, and is kept
    def boom(mask, n):
        raise RuntimeError("boom")
    ctx.set_mask_exchange(boom, np.zeros(96 * 54, np.uint8))
    with pytest.raises(ptx.PtxError) as e:
        s.render_adaptive(c.W, c.H, c.cap, B, MIN, STEP, c.thr, seed=SEED, shard=(0, 2, c.tile))
    ctx.set_mask_exchange(None)
    assert e.value.code == ptx.ERR_HIP and "status -1" in str(e.value) and isinstance(ctx.mask_exchange_error, RuntimeError)
    _check_world(ctx, s, c, 2)


@pytest.mark.gpu
def test_refusals_and_the_ignored_registration(ptx, ctx, clean_env):
    c = CASES[0]
    s = _scene(ptx, ctx, clean_env, c)
    ua, ub, ust, M = _unsharded(s, c)
    x0, y0, w, h = c.rect
    # a mask one byte short: refused before any device work, the callback is never called
    g = _rank(ctx, s, c, 0, 2, M, mask_bytes=w * h - 1)
    assert g["err"] is not None and g["err"].code == ptx.ERR_INVALID and "mask" in str(g["err"]) and g["calls"] == 0, g["err"]
    assert not g["a"].any() and not g["b"].any()
    # no registration: today's refusal, with the pointer to the setter
    for call in (lambda: s.render_adaptive(c.W, c.H, c.cap, B, shard=(0, 2, c.tile)), lambda: s.render_adaptive_nee(c.W, c.H, c.cap, B, shard=(0, 2, c.tile))):
        with pytest.raises(ptx.PtxError) as e:
            call()
        assert e.value.code == ptx.ERR_UNSUPPORTED and "ptx_ctx_set_mask_exchange" in str(e.value)
    # a callback without a mask
    L = ptx.lib()
    fn = ptx.MASK_EXCHANGE_FN(lambda user, m, n: 0)
    assert L.ptx_ctx_set_mask_exchange(ctx.h, fn, None, None, 0) == ptx.ERR_INVALID and "mask" in L.ptx_last_error().decode()
    # shard_count 0 and 1 with a registration: the unsharded bits, and the exchange is never called
    for shard in ((0, 0, 0), (0, 1, c.tile)):
        g = _rank(ctx, s, c, 0, 1, M, shard=shard)
        assert g["err"] is None and g["calls"] == 0 and g["lib"]["calls"] == 0, (shard, g["err"], g["calls"])
        _same(g["a"], ua, f"shard {shard}: A"), _same(g["b"], ub, f"shard {shard}: B")
        assert all(g["st"][k] == ust[k] for k in SUMMED + ("rounds", "passes")), (g["st"], ust)
