"""Texture lookups and material getters (csrc/device_core.hpp tex_sample / material_eval) against the reference, on the device.

tests/golden/textures/ is a small synthetic glTF scene written by `python oracle/make_golden.py --only-textures`: one quad per
material, textures of the sizes where the reference's wrap differs from an ordinary one (1x1, 1x5, 7x1, 3x5, 37x53, 255x3; one
16x16 control), every PNG flavour the loader accepts (grey, grey+alpha, RGB, RGBA, palette with and without tRNS, 16-bit and 1-bit
grey), two Radiance .hdr files (emissive, loaded as sRGB; metallic-roughness, linear), OPAQUE and BLEND base colours, an
untextured material, and two files whose first use fixes their sRGB flag for a later slot. tests/golden/tex_vectors.npz holds
material::get_* of the compiled reference at per-surface uvs: a random set, every texel edge and centre, signed zeros, 1 and its
neighbours, values out to +-1e4, |u w| in every range of the float -> int64 -> uint32 conversion, infinities and NaN.

Bars: bit-exact, NaN compared as NaN; the one exception is a float texel of an sRGB image, which goes through ocml's powf on the
device and glibc's in the reference (SRGB_FLOAT_ULP). ptx_material_eval_batch returns emissive * 10, as the integrators use it.
"""
import os

import numpy as np
import pytest

from _checks import _check_hits
from _common import _bits
from _routes import Route, clean_env, ctx, under_force_global  # noqa: F401  (clean_env and ctx are fixtures)
from conftest import GOLD

TEX_GLTF = os.path.join(GOLD, "textures", "textures.gltf")
K_SRGB, K_FLOAT = 1 << 8, 1 << 16
# (slot of surf_tex, output columns, channels read): normal, albedo, opacity (.w), roughness (.y), metallic (.z), emissive
SLOT_COLS = ((0, slice(0, 3), (0, 1, 2)), (1, slice(3, 6), (0, 1, 2)), (2, slice(6, 7), (3,)), (4, slice(7, 8), (1,)),
             (5, slice(8, 9), (2,)), (6, slice(9, 12), (0, 1, 2)))
# ocml powf vs glibc powf on sRGB float texels, after the bilinear blend and the factors, in ulps of the channel's scale (_powf_scale;
# measured at most 3):
# a 1-ulp texel difference stays about 1 ulp at that scale, but lerp's a + (b - a) w cancels where the taps differ, so in ulps of the
# output itself it can grow without a useful bound (the tests print both histograms)
SRGB_FLOAT_ULP = 4


def _device_form(ref):
    """The reference's getters as ptx_material_eval_batch returns them: emissive * 10 (renderer.cpp:462)."""
    out = np.array(ref, np.float32, copy=True)
    out[..., 9:12] = np.float32(10) * out[..., 9:12]
    return out


def _mismatch(got, want):
    """Elements that differ: bitwise, except that NaN equals NaN (whatever its payload)."""
    return ~((_bits(got) == _bits(want)) | (np.isnan(got) & np.isnan(want)))


def _powf_mask(tex, surf_tex):
    """[n_surf, 12]: output elements fed by a float texel of an image loaded as sRGB (colour channels only: image.cpp:124-141)."""
    m = np.zeros((len(surf_tex), 12), bool)
    for s, row in enumerate(surf_tex):
        for slot, cols, chans in SLOT_COLS:
            t = int(row[slot])
            if t >= 0 and (int(tex[t][2]) & K_FLOAT) and (int(tex[t][2]) & K_SRGB) and min(chans) < 3:
                m[s, cols] = True
    return m


def _powf_scale(arrays, mask):
    """[n_surf, 12]: where `mask` is set, the largest value the element can take — the largest sRGB-decoded texel of its channel
    times its factor (x 2 for the normal map, x 10 for emissive)."""
    a = arrays
    out = np.zeros(mask.shape, np.float32)
    fac = lambda s: np.concatenate([[2, 2, 2], a.materials[s, 0:3], [1], a.materials[s, 4:6], np.float32(10) * a.materials[s, 6:9]])
    for s, row in enumerate(a.surf_tex):
        for slot, cols, chans in SLOT_COLS:
            if row[slot] >= 0 and mask[s, cols].any():
                im = np.asarray(a.images[row[slot]], np.float64)
                out[s, cols] = [im[..., c].max() ** 2.2 * f for c, f in zip(chans, fac(s)[cols])]
    return out


def _powf_err(got, ref, scale):
    """(|got - ref| in ulps of the output, in ulps of `scale`), NaN against NaN counted as 0."""
    from conftest import ulp_diff
    d = np.abs(got.astype(np.float64) - ref.astype(np.float64)) / np.spacing(np.asarray(scale, np.float32)).astype(np.float64)
    return ulp_diff(got, ref), np.where(np.isnan(got) & np.isnan(ref), 0, np.ceil(d)).astype(np.int64)


def _hist(u):
    return {int(k): int(c) for k, c in zip(*np.unique(u, return_counts=True))}


@pytest.fixture(scope="module")
def tex_gold():
    return dict(np.load(os.path.join(GOLD, "tex_vectors.npz")))


@pytest.fixture(scope="module")
def tex_oracle(ora):
    return ora.OracleScene(ora.load_gltf(TEX_GLTF))


@pytest.fixture(scope="module")
def tex_host(ptx):
    s = ptx.Scene.load_gltf(None, TEX_GLTF)
    return s.array(ptx.ARR_TEXTURES), s.array(ptx.ARR_SURF_TEX)


# ---------------------------------------------------------------------------- CPU: the fixture and the oracle
def test_texture_fixture_covers_what_it_claims(ptx, ora, tex_host, tex_gold):
    """Channel counts 1-4, 8-bit and float texels, sizes that are not powers of two, both sRGB flags on each kind, the flag of a
    file's first use kept, an untextured surface, OPAQUE and BLEND base colours, and every uv class — in the product's loader and
    the oracle's alike."""
    tex, st = tex_host
    a = ora.load_gltf(TEX_GLTF)
    np.testing.assert_array_equal(st, a.surf_tex)
    assert [bool(int(t[2]) & K_SRGB) for t in tex] == a.image_srgb
    assert [(int(t[0]), int(t[1]), int(t[2]) & 255) for t in tex] == [(im.shape[1], im.shape[0], im.shape[2]) for im in a.images]
    assert {int(t[2]) & 255 for t in tex} == {1, 2, 3, 4}
    sizes = {(int(t[0]), int(t[1])) for t in tex}
    assert {(1, 1), (1, 5), (7, 1), (3, 5), (37, 53), (255, 3), (16, 16)} <= sizes
    kinds = {(bool(int(t[2]) & K_FLOAT), bool(int(t[2]) & K_SRGB)) for t in tex}
    assert kinds == {(False, False), (False, True), (True, False), (True, True)}
    assert (st < 0).all(1).sum() == 1                                          # the untextured material
    assert ((st[:, 1] >= 0) & (st[:, 2] == st[:, 1])).sum() >= 3               # BLEND: base colour also the opacity texture
    assert ((st[:, 1] >= 0) & (st[:, 2] < 0)).sum() >= 3                       # OPAQUE
    paths = [os.path.basename(p) for p in a.image_paths]
    assert not a.image_srgb[paths.index("rgb_37x53.png")]                      # normal map first, base colour later: stays linear
    assert a.image_srgb[paths.index("la_1x5.png")]                             # base colour first, normal map later: stays sRGB
    uv = tex_gold["mat_in"].reshape(-1, 2)
    assert uv.shape[0] == tex_gold["mat_out"].reshape(-1, 12).shape[0] and len(tex_gold["mat_in"]) == len(st)
    mag = np.abs(uv[np.isfinite(uv)].astype(np.float64)) * 255
    for lo, hi in ((2.0 ** 24, 2.0 ** 31), (2.0 ** 31, 2.0 ** 32), (2.0 ** 32, 2.0 ** 63), (2.0 ** 63, np.inf)):
        assert ((mag >= lo) & (mag < hi)).sum() >= 4, (lo, hi)
    assert np.isnan(uv).any() and np.isposinf(uv).any() and np.isneginf(uv).any() and (_bits(uv) == 0x80000000).any()
    total = sum(os.path.getsize(os.path.join(GOLD, "textures", f)) for f in os.listdir(os.path.join(GOLD, "textures")))
    assert total < 200 * 1024


def test_texture_fixture_lookups_bit_exact_in_the_oracle(tex_oracle, tex_gold):
    """oracle material_eval (float texels included, sRGB ones through glibc's powf as in the reference) = the reference, bit for bit."""
    uv, ref = tex_gold["mat_in"], tex_gold["mat_out"]
    n_nan = 0
    for s in range(len(uv)):
        got = tex_oracle.material_eval(s, uv[s])
        bad = _mismatch(got, ref[s])
        assert not bad.any(), f"surface {s}: {bad.any(1).sum()} uvs differ, first {uv[s][bad.any(1)][:4]}"
        n_nan += int(np.isnan(ref[s]).any(1).sum())
    assert n_nan > 0


# ---------------------------------------------------------------------------- GPU: ptx_material_eval_batch
@pytest.fixture(scope="module")
def tex_scene(ptx, ctx):
    return ptx.Scene.load_gltf(ctx, TEX_GLTF)


@pytest.mark.gpu
def test_jack_material_lookups_on_the_device(ctx, gold_jack):
    """Every surface of the 17-texture asset at the reference's 256 uvs: bit for bit."""
    import importlib
    from conftest import JACK
    ptx = importlib.import_module("distributed-path-tracer_amd")
    s = ptx.Scene.load_gltf(ctx, JACK)
    uv, ref = gold_jack["mat_in"], _device_form(gold_jack["mat_out"])
    assert len(uv) == s.info()["n_surfaces"]
    for k in range(len(uv)):
        got = s.material_eval(k, uv[k])
        bad = _mismatch(got, ref[k])
        assert not bad.any(), f"surface {k}: {bad.any(1).sum()} uvs differ, first {uv[k][bad.any(1)][:4]}"


@pytest.mark.gpu
def test_texture_fixture_on_the_device_against_reference(ora, tex_scene, tex_host, tex_gold):
    """The reference's vectors on the fixture scene, every surface in one batch: bit for bit, except the elements fed by sRGB float
    texels (the emissive .hdr), which are held to SRGB_FLOAT_ULP ulps of the channel's scale. Measured on MI355X, of those 4398
    elements: in ulps of the channel scale 0: 3220, 1: 1117, 2: 61; in ulps of the output itself 0: 3220, 1: 806, 2: 295, 3: 49,
    4: 24, 8: 3, 9: 1. NaN inputs give NaN outputs wherever a texture is read."""
    tex, st = tex_host
    uv, ref = tex_gold["mat_in"], _device_form(tex_gold["mat_out"])
    ns, n = uv.shape[:2]
    surf = np.repeat(np.arange(ns, dtype=np.int32), n)
    got = tex_scene.material_eval(surf, uv.reshape(-1, 2)).reshape(ns, n, 12)
    pw = np.broadcast_to(_powf_mask(tex, st)[:, None, :], got.shape)
    assert pw.any()
    bad = _mismatch(got, ref) & ~pw
    for s in range(ns):
        assert not bad[s].any(), f"surface {s}: {bad[s].any(1).sum()} uvs differ, first {uv[s][bad[s].any(1)][:4]} {got[s][bad[s].any(1)][:2]} {ref[s][bad[s].any(1)][:2]}"
    sc = np.broadcast_to(_powf_scale(ora.load_gltf(TEX_GLTF), _powf_mask(tex, st))[:, None, :], got.shape)
    u, us = _powf_err(got[pw], ref[pw], sc[pw])
    print("\nsRGB float texels: ulps of the output", _hist(u), "ulps of the channel scale", _hist(us))
    assert us.max() <= SRGB_FLOAT_ULP
    assert (np.isnan(got) == np.isnan(ref)).all()
    nan_in = np.isnan(uv).any(-1)
    assert np.isnan(got[nan_in][:, 0]).sum() > 0


@pytest.mark.gpu
def test_material_eval_batch_bad_surface_ids_and_device_buffers(ptx, tex_scene, tex_gold):
    """Surface ids outside [0, n_surfaces) give rows of NaNs; device buffers give the host result; mixed pointer kinds are refused."""
    import torch
    ns = tex_scene.info()["n_surfaces"]
    uv = np.float32([[0.25, 0.75]] * 5)
    got = tex_scene.material_eval(np.int32([-1, ns, 2 ** 31 - 1, -2 ** 31, 0]), uv)
    assert np.isnan(got[:4]).all() and np.isfinite(got[4]).all()
    uv = tex_gold["mat_in"].reshape(-1, 2)
    surf = np.repeat(np.arange(ns, dtype=np.int32), tex_gold["mat_in"].shape[1])
    host = tex_scene.material_eval(surf, uv)
    d_s, d_uv = torch.from_numpy(surf).cuda(), torch.from_numpy(uv).cuda()
    d_out = torch.zeros((len(uv), 12), dtype=torch.float32, device="cuda")
    L = ptx.lib()
    ptx._check(L.ptx_material_eval_batch(tex_scene.h, d_s.data_ptr(), d_uv.data_ptr(), len(uv), d_out.data_ptr()))
    torch.cuda.synchronize()
    np.testing.assert_array_equal(_bits(d_out.cpu().numpy()), _bits(host))
    h_out = np.zeros((len(uv), 12), np.float32)
    assert L.ptx_material_eval_batch(tex_scene.h, surf.ctypes.data, d_uv.data_ptr(), len(uv), h_out.ctypes.data) == ptx.ERR_INVALID
    assert L.ptx_material_eval_batch(tex_scene.h, surf.ctypes.data, uv.ctypes.data, 0, h_out.ctypes.data) == ptx.OK


def _sweep_uvs(rng, n):
    """uvs for the random sweep: most in the scene's vertex range, some out to +-1e4, some random bit patterns (every magnitude,
    infinities, NaNs)."""
    a = rng.uniform(-2.3, 3.7, (n, 2)).astype(np.float32)
    k = n // 5
    a[:k] = rng.uniform(-1e4, 1e4, (k, 2)).astype(np.float32)
    a[k:2 * k] = rng.integers(0, 2 ** 32, (k, 2), dtype=np.uint64).astype(np.uint32).view(np.float32)
    return a


@pytest.mark.gpu
def test_random_uv_sweep_against_the_oracle(ora, tex_scene, tex_oracle, tex_host):
    """100 k uvs per surface, device against oracle: bit for bit with the same exceptions as the reference vectors. Measured on
    MI355X, of the 300 000 sRGB float elements: in ulps of the channel scale 0: 215 372, 1: 80 441, 2: 3 964, 3: 223; in ulps of
    the output up to 255 (lerp's cancellation next to a small tap)."""
    tex, st = tex_host
    rng = np.random.default_rng(17)
    pw = _powf_mask(tex, st)
    scale = _powf_scale(ora.load_gltf(TEX_GLTF), pw)
    hist, hist_s = {}, {}
    for s in range(len(st)):
        uv = _sweep_uvs(rng, 100_000)
        got = tex_scene.material_eval(s, uv)
        ref = _device_form(tex_oracle.material_eval(s, uv))
        bad = _mismatch(got, ref) & ~pw[s][None, :]
        assert not bad.any(), f"surface {s}: {bad.any(1).sum()} uvs differ, first {uv[bad.any(1)][:4]} {got[bad.any(1)][:2]} {ref[bad.any(1)][:2]}"
        assert (np.isnan(got) == np.isnan(ref)).all(), s
        if pw[s].any():
            u, us = _powf_err(got[:, pw[s]], ref[:, pw[s]], np.broadcast_to(scale[s, pw[s]], (len(uv), int(pw[s].sum()))))
            for h, x in ((hist, u), (hist_s, us)):
                for k, c in _hist(x).items():
                    h[k] = h.get(k, 0) + c
    print("\nsRGB float texels: ulps of the output", hist, "ulps of the channel scale", hist_s)
    assert max(hist_s) <= SRGB_FLOAT_ULP


# ---------------------------------------------------------------------------- GPU: renders of the fixture scene on every route
# this file's table: every route with PTX_WAVEFRONT set (as the forced routes of tests/_routes.py), the queue route last
ROUTES = [Route("lds fused", False, {"PTX_WAVEFRONT": "0"}, 1, 0), Route("global fused", True, {"PTX_WAVEFRONT": "0"}, 0, 0),
          Route("queue", True, {"PTX_WAVEFRONT": "1"}, 0, 1)]
W, H, SPP = 96, 54, 4
FW, FH, FSPP = 160, 90, 8


def _route_scenes(ptx, ctx, mp, sun):
    out = []
    for r in ROUTES:
        s = under_force_global(mp, r.force_global, lambda: ptx.Scene.load_gltf(ctx, TEX_GLTF, sun_light_index=0 if sun else 1))
        info = s.info()
        assert info["lds_resident"] == r.resident and info["has_sun"] == int(sun) and info["n_textures"] == 12, r.name
        out.append((r.name, s, r.env["PTX_WAVEFRONT"], r.pipeline))
    return out


def _samples(s, ctx, mp, wf, pipeline, bounces, integrator, what):
    mp.setenv("PTX_WAVEFRONT", wf)
    got = np.zeros((H, W, SPP, 3), np.float32)
    for k in range(SPP):
        a, _ = s.render(W, H, 1, bounces, sample0=k, integrator=integrator)
        assert ctx.timing()["pipeline"] == pipeline, what
        got[:, :, k] = a[..., :3]
    return got


@pytest.mark.gpu
@pytest.mark.parametrize("sun", [False, True], ids=["nosun", "sun"])
def test_fixture_scene_on_every_route(ptx, ctx, ora, tex_host, clean_env, sun):
    """The fixture scene through the LDS fused kernel, the global fused kernel (PTX_FORCE_GLOBAL at creation) and the queue
    pipeline (PTX_WAVEFRONT=1), each asserted from the residency and the pipeline the render reports. The camera sees every quad;
    vertex uvs span about [-2.3, 3.7] (one quad exactly [0, 1]); three BLEND quads stand in front of other quads.
      * hit records (normal maps of odd sizes and channel counts included): bit for bit against the oracle;
      * 1 bounce, no sun: per-sample radiance bit for bit against the oracle with both integrators (camera ray, hit record, Philox
        draws, the opacity test, the normal map's sign test and the emissive lookup — no libm call), except the samples whose
        camera ray hits the sRGB .hdr emissive quad;
      * 4 bounces: >= 99.5 % of samples within 1e-3, ray counts within 1e-4, the three routes bitwise equal to each other."""
    mp = clean_env
    o = ora.OracleScene(ora.load_gltf(TEX_GLTF, sun_light_index=0 if sun else 1))
    routes = _route_scenes(ptx, ctx, mp, sun)
    ns = routes[0][1].info()["n_surfaces"]
    hdr_surf = int(np.flatnonzero(_powf_mask(*tex_host).any(1))[0])
    prim = o.primary_rays(ora.make_cfg(FW, FH, 1, 4), 0).reshape(-1, 6)
    out, idx = o.intersect(prim)
    assert set(np.unique(idx)) == set(range(-1, ns))                          # every quad in view, and background
    rng = np.random.default_rng(3)
    sel = rng.choice(np.flatnonzero(idx >= 0), 20_000)
    dd = rng.standard_normal((len(sel), 3)).astype(np.float32)
    dd /= np.linalg.norm(dd, axis=1, keepdims=True).astype(np.float32)
    rays = np.concatenate([prim, np.concatenate([out[sel, :3] + dd * np.float32(1e-3), dd], 1)]).astype(np.float32)
    out, idx = o.intersect(rays)
    for name, s, wf, pipeline in routes:
        mp.setenv("PTX_WAVEFRONT", wf)
        _check_hits(s.intersect(rays[:, :3], rays[:, 3:]), out, idx)
    for ig in (0, 1):
        if not sun:
            ref = o.render_samples(ora.make_cfg(W, H, SPP, 1, integrator=ig), threads=16)
            keep = np.ones((H, W, SPP), bool)
            for k in range(SPP):
                _, hit = o.intersect(o.primary_rays(ora.make_cfg(W, H, 1, 1, integrator=ig), k).reshape(-1, 6))
                keep[:, :, k] = (hit != hdr_surf).reshape(H, W)
            assert (ref[keep] != 0).any(1).mean() > 0.3 and (~keep).sum() > 100
            for name, s, wf, pipeline in routes:
                got = _samples(s, ctx, mp, wf, pipeline, 1, ig, name)
                bad = _mismatch(got, ref).any(-1) & keep
                assert not bad.any(), f"{name} integrator {ig}, 1 bounce: {bad.sum()} of {keep.sum()} samples differ"
        ref = o.render_samples(ora.make_cfg(W, H, SPP, 4, integrator=ig), threads=16)
        oray = int(o.render(ora.make_cfg(FW, FH, FSPP, 4, integrator=ig), threads=16)[1][0])
        frame0 = rays0 = None
        for name, s, wf, pipeline in routes:
            got = _samples(s, ctx, mp, wf, pipeline, 4, ig, name)
            assert np.isfinite(got).all()
            err = np.abs(got - ref).max(-1) / np.maximum(np.abs(ref).max(-1), 1e-3)
            assert (err < 1e-3).mean() > 0.995, f"{name} integrator {ig}: {(err < 1e-3).mean():.4%} of samples agree"
            frame, st = s.render(FW, FH, FSPP, 4, integrator=ig)
            assert ctx.timing()["pipeline"] == pipeline, name
            assert abs(st["rays"] - oray) <= 1e-4 * oray, (name, ig, st["rays"], oray)
            if frame0 is None:
                frame0, rays0 = frame, st["rays"]
            else:
                np.testing.assert_array_equal(_bits(frame), _bits(frame0), err_msg=f"{name} integrator {ig}")
                assert st["rays"] == rays0, name
