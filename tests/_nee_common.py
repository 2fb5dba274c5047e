"""What the ptx_render_nee test files share (tests/test_nee.py, test_nee_fused.py, test_nee_lights.py, test_nee_env.py, test_pass_plumbing.py):
the small scenes with their oracles, the batch statistic for "same expectation", the error measure, the check of a light list, and the
unflagged / PTX_NEE_FUSED pair. Not collected (underscore prefix); every assert carries its own message, since pytest does not rewrite
asserts here. Oracles and flat arrays are kept here once; product scenes live on a context and are kept per test module (tests/_routes.py).
"""
import numpy as np

from _common import _bits, _proc
from conftest import CORNELL, JACK, oracle_from_dict, product_from_dict

SEED = 0x5EED
SAME_STATS = ("rays", "samples", "n_lights", "light_area", "light_samples", "light_visible")

# ---------------------------------------------------------------------------- scenes, built once
_dicts, _oracles = {}, {}
_MAKERS = {"chart": lambda p: p.chart_scene(facing=True, alpha=False), "chart_alpha": lambda p: p.chart_scene(facing=True, alpha=True),
           "chart_sun": lambda p: p.chart_scene(facing=True, sun=0.5), "chart_alpha_sun": lambda p: p.chart_scene(facing=True, alpha=True, sun=0.004732),
           "plaza": lambda p: p.plaza_scene(level=1, sun=True, alpha=True), "plaza_opaque": lambda p: p.plaza_scene(level=1, sun=True, alpha=False),
           "atrium": lambda p: p.atrium_scene(0)}


def _dict(name):
    if name not in _dicts:
        _dicts[name] = _MAKERS[name](_proc())
    return _dicts[name]


def _oracle(ora, name):
    """(oracle scene, its arrays)"""
    if name not in _oracles:
        if name == "cornell":
            a = ora.load_gltf(CORNELL)
            _oracles[name] = (ora.OracleScene(a), a)
        elif name == "jack":
            a = ora.load_gltf(JACK)
            _oracles[name] = (ora.OracleScene(a), a)
        else:
            o = oracle_from_dict(ora, _dict(name))
            _oracles[name] = (o, o.a)
    return _oracles[name]


def _host_scene(ptx, name, ctx=None):
    if name == "cornell":
        return ptx.Scene.load_gltf(ctx, CORNELL)
    if name == "jack":
        return ptx.Scene.load_gltf(ctx, JACK)
    return product_from_dict(ptx, ctx, _dict(name))


def _make(ptx, ctx, name):
    """_host_scene in the argument order of tests/_routes.py's Scenes"""
    return _host_scene(ptx, name, ctx)


# ---------------------------------------------------------------------------- checks
def _check_list(ll, n_surf):
    n = len(ll["cdf"])
    assert ll["tris"].shape == (n, 2) and ll["geom"].shape == (n, 4) and n > 0, (ll["tris"].shape, ll["geom"].shape, n)
    assert (np.diff(ll["cdf"]) >= 0).all() and ll["cdf"][-1] == 1 and ll["cdf"][0] > 0, ("cdf", ll["cdf"][0], ll["cdf"][-1])
    share = abs(float(ll["geom"][:, 3].astype(np.float64).sum()) / float(ll["area"]) - 1)
    assert (ll["geom"][:, 3] > 0).all() and share < 1e-5, ("areas", float(ll["geom"][:, 3].min()), share)
    np.testing.assert_allclose(np.linalg.norm(ll["geom"][:, :3].astype(np.float64), axis=1), 1, atol=1e-6)
    key = ll["tris"][:, 0].astype(np.int64) << 32 | ll["tris"][:, 1]
    assert (np.diff(key) > 0).all() and ll["tris"][:, 0].max() < n_surf, ("order or surface id", int(ll["tris"][:, 0].max()), n_surf)


def _batch_stat(frames):
    """frames [K, h, w, 3] batch means per pixel -> (means [K, 5, 3]: the frame and its four quadrants)"""
    K, h, w, _ = frames.shape
    regions = [frames, frames[:, :h // 2, :w // 2], frames[:, :h // 2, w // 2:], frames[:, h // 2:, :w // 2], frames[:, h // 2:, w // 2:]]
    return np.stack([r.reshape(K, -1, 3).mean(1, dtype=np.float64) for r in regions], 1)


def _same_expectation(a, b):
    """|m_a - m_b| <= 4 sqrt(s2_a / K + s2_b / K) on the frame mean of each channel, 5 sigma on the quadrants. -> (ok, worst z frame, worst z quadrant)"""
    K = len(a)
    z = np.abs(a.mean(0) - b.mean(0)) / np.sqrt(a.var(0, ddof=1) / K + b.var(0, ddof=1) / K)
    return bool((z[0] <= 4).all() and (z[1:] <= 5).all()), float(z[0].max()), float(z[1:].max())


K_BATCH = 16


def _err(got, ref):
    return np.abs(got - ref).max(-1) / np.maximum(np.abs(ref).max(-1), 1e-3)


def _pair(ptx, ctx, s, W, H, spp, bounces, fused=True, flags=0, **kw):
    """the unflagged and the flagged call: asserts bitwise equal frames, equal stats and what ptx_ctx_get_timing tells about the route"""
    want, st0 = s.render_nee(W, H, spp, bounces, seed=SEED, flags=flags, **kw)
    tm0 = ctx.timing()
    assert tm0["fused_launches"] == 0, ("the unflagged call launched the fused kernel", tm0)
    got, st = s.render_nee(W, H, spp, bounces, seed=SEED, flags=flags | ptx.NEE_FUSED, **kw)
    tm = ctx.timing()
    np.testing.assert_array_equal(_bits(got), _bits(want))
    assert all(st[k] == st0[k] for k in SAME_STATS), (st, st0)
    if fused:
        assert tm["pipeline"] == 0 and tm["fused_launches"] == st["passes"] > 0 and tm["fused_ms"] == st["kernel_ms"], (tm, st)
    else:
        assert tm["pipeline"] == 1 and tm["fused_launches"] == 0 and st["passes"] == st0["passes"], (tm, st, st0)
    return got, st
