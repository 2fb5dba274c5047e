"""Checks and small scene builders that more than one test file uses. Not collected (underscore prefix).

Pytest does not rewrite asserts outside test files: every assert here carries its own message.
"""
import os

import numpy as np

from _common import _bits, _proc
from conftest import CORNELL, oracle_from_dict, product_from_dict


def _check_hits(hits, oracle_out, oracle_idx):
    np.testing.assert_array_equal(hits["surface"], oracle_idx)
    hit = oracle_idx >= 0
    pos = np.stack([hits["px"], hits["py"], hits["pz"]], 1)
    nrm = np.stack([hits["nx"], hits["ny"], hits["nz"]], 1)
    uv = np.stack([hits["u"], hits["v"]], 1)
    np.testing.assert_array_equal(_bits(pos[hit]), _bits(oracle_out[hit, 0:3]))
    np.testing.assert_array_equal(_bits(uv[hit]), _bits(oracle_out[hit, 3:5]))
    np.testing.assert_array_equal(_bits(nrm[hit]), _bits(oracle_out[hit, 11:14]))
    missed = hits["distance"][~hit]
    assert (missed == -1).all(), ("distance of a miss is not -1", missed[missed != -1][:8])


def _scene_parity(ptx, ctx, ora, d, W, H, spp, b, n_rays=60_000, seed=11):
    s = product_from_dict(ptx, ctx, d)
    o = oracle_from_dict(ora, d)
    cfg = ora.make_cfg(W, H, 1, b)
    prim = o.primary_rays(cfg, 0).reshape(-1, 6)
    out, idx = o.intersect(prim)
    rng = np.random.default_rng(seed)
    hit = idx >= 0
    k = min(n_rays, int(hit.sum()))
    sel = rng.choice(np.flatnonzero(hit), k, replace=True)
    dd = rng.standard_normal((k, 3)).astype(np.float32)
    dd /= np.linalg.norm(dd, axis=1, keepdims=True).astype(np.float32)
    dd = np.where((dd * out[sel, 11:14]).sum(1, keepdims=True) < 0, -dd, dd).astype(np.float32)
    sec = np.concatenate([out[sel, :3] + out[sel, 11:14] * np.float32(1e-4), dd], 1).astype(np.float32)
    rays = np.concatenate([prim, sec])
    out, idx = o.intersect(rays)
    hits = s.intersect(rays[:, :3], rays[:, 3:])
    _check_hits(hits, out, idx)
    ref = o.render_samples(ora.make_cfg(W, H, spp, b), threads=0)
    got = np.zeros_like(ref)
    for kk in range(spp):
        a, _ = s.render(W, H, 1, b, sample0=kk)
        got[:, :, kk] = a[..., :3]
    err = np.abs(got - ref).max(-1) / np.maximum(np.abs(ref).max(-1), 1e-3)
    assert (err < 1e-3).mean() > 0.995, f"{(err < 1e-3).mean():.4%} of samples agree"
    return s, o


def _check_records(hits, o, rays, out, idx):
    """Surface, position, uv and shading normal (_check_hits), then distance, triangle and barycentrics against the winning model's
    model::intersect record (the first model wins ties, renderer.cpp:645-671)."""
    _check_hits(hits, out, idx)
    n_models = o.n_models
    mo = np.zeros((len(rays), n_models, 4), np.float32)
    mi = np.zeros((len(rays), n_models, 2), np.int32)
    for m in range(n_models):
        mo[:, m], mi[:, m] = o.model_intersect(m, rays)
    hit = idx >= 0
    win = np.argmax((mi[:, :, 0] == idx[:, None]) & (mo[:, :, 0] >= 0), axis=1)
    r = np.arange(len(rays))
    np.testing.assert_array_equal(_bits(hits["distance"][hit]), _bits(mo[r, win, 0][hit]))
    np.testing.assert_array_equal(hits["triangle"][hit], mi[r, win, 1][hit])
    bary = np.stack([hits["b0"], hits["b1"], hits["b2"]], 1)
    np.testing.assert_array_equal(_bits(bary[hit]), _bits(mo[r, win, 1:4][hit]))


def _same_hits(a, b, what):
    assert a.keys() == b.keys(), (what, sorted(a), sorted(b))
    for k in a:
        np.testing.assert_array_equal(np.asarray(a[k]).view(np.uint32), np.asarray(b[k]).view(np.uint32), err_msg=f"{what}: {k}")


def _glass_stack(n_layers, opacity):
    """n_layers quads one behind the other in front of the camera, all with the same opacity (< 1: every hit may pass through,
    renderer.cpp:466-472), nothing else: flat arrays for Scene.from_arrays / the oracle."""
    proc = _proc()
    d = proc.plaza_scene(level=0, sun=False, alpha=False)
    verts, tris = [], []
    for k in range(n_layers):
        z = -2.0 - 0.01 * k
        q = np.zeros((4, 11), np.float32)
        q[:, :3] = [[-50, -50, z], [50, -50, z], [50, 50, z], [-50, 50, z]]
        q[:, 7] = 1.0                      # normal +z (towards the camera)
        q[:, 8] = 1.0                      # tangent +x
        verts.append(q)
        tris.append(np.array([[0, 1, 2], [0, 2, 3]], np.uint32) + 4 * k)
    cam = np.zeros(13, np.float32)
    cam[3] = cam[7] = cam[11] = 1.0        # identity basis at the origin, looking down -z
    cam[12] = 0.6
    return dict(model_xform=np.array([[0, 0, 0, 1, 0, 0, 0, 1, 0, 0, 0, 1]], np.float32), model_surf=np.array([[0, 1]], np.int32),
                surf_range=np.array([[0, 4 * n_layers, 0, 2 * n_layers]], np.int32), vertices=np.concatenate(verts), triangles=np.concatenate(tris),
                materials=np.array([[0.8, 0.8, 0.8, opacity, 0.5, 0.0, 0, 0, 0, 1.33, 0]], np.float32), camera=cam, sun=None)


def _event(tmp_path, work, samples=5, bounces=3, X=48, Y=32):
    """The reference worker's Lambda event for Cornell under tmp_path -> (event.json, the local scene root)."""
    import json, shutil
    root = tmp_path / "scene-root"
    root.mkdir()
    shutil.copyfile(CORNELL, root / "scene.gltf")                       # the worker downloads <scene_root>scene.gltf (worker.cpp:108-112)
    shutil.copyfile(os.path.join(os.path.dirname(CORNELL), "cornell.bin"), root / "cornell.bin")
    ev = {"scene_info": {"work": work, "total_size": 0.05}, "scene_bucket": "distributed-path-tracer", "scene_root": "scenes/cornell-box/",
          "worker_id": "1", "sqs_queue_arn": "", "sns_topic_arn": "", "num_workers": 1, "samples": samples, "bounces": bounces, "X": X, "Y": Y}
    p = tmp_path / "event.json"
    p.write_text(json.dumps(ev, indent=4))
    return str(p), str(root)
