"""ptx_render_emission, ptx_emission_split and ptx_emission_merge restated in float32 numpy (tests/test_emission.py states their rules on
the CPU, tests/test_emission_gpu.py pins the product to them bit for bit). Not collected (underscore prefix).

The walk — camera samples, opacity pass-throughs, the first vertex that does not pass through — is tests/_aov_restatement.restate's, copied
because that one does not keep the ray that found the surface. What the sample's surface adds is the specification of include/ptx.h: the
material's emission (OracleScene.material_eval, floats 9 .. 11: get_emissive, here times 10 as renderer.cpp:462 has it) when the restated shading normal faces the ray.
"""
import numpy as np

from _aov_restatement import EPS, H, S0, SEED, SPP, TILE, W, _len3

f32 = np.float32
# Cornell's only emitter, the ceiling light, lies above the common tile (rows 0 .. 8 of the 54): the same tile moved to the top row
CORNELL_TILE = (13, 0, 67, 35)
# tests/golden/textures/lit.gltf without its sun and without primitive 1 (emit_hdr_srgb): that emitter's float texture is sRGB-decoded with
# powf, which differs between the device's and the host's libm. What stays: a palette-textured emitter behind a normal map, a factor-only
# emitter, one whose texture is black, and the two BLEND primitives (one of them emissive) that pass samples through.
# At the common tile only the factor-only emitter is in sight; LIT_TILE, the same size towards the top left corner, holds the textured one.
LIT_TILE = (3, 2, 67, 35)
LIT_LOAD = dict(sun_light_index=0xFFFFFFFF, work={"lit": [0, 2, 3, 4, 5, 6, 7, 8, 9]})


def restate(ora, o, W_=W, H_=H, tile=TILE, sample0=S0, spp=SPP, seed=SEED, per_sample=False):
    """-> (emission [h,w,4], counts) for samples [sample0, sample0 + spp) of the tile. counts: samples that ended on a surface, of those the
    back-facing ones, the recording ones with a non-zero emission, of those the ones that came through a pass-through; samples that passed
    through at least once; samples that ended on a miss. per_sample: also the list of each sample's records [h*w,4] (zeros where nothing
    was recorded)."""
    x0, y0, w, h = tile
    em = np.zeros((h * w, 4), f32)
    yy, xx = np.divmod(np.arange(h * w), w)
    pixel = (yy + y0) * W_ + (xx + x0)
    counts = dict(surface=0, back=0, emissive=0, emissive_through=0, through=0, miss=0)
    records = []
    for s in range(sample0, sample0 + spp):
        rays = o.primary_rays(ora.make_cfg(W_, H_, 1, 1, seed=seed, tile=tile), s).reshape(-1, 6)
        rec = np.zeros((h * w, 4), f32)
        ended = np.zeros(h * w, bool)
        live, cur, pas = np.arange(h * w), rays.copy(), np.zeros(h * w, np.int64)
        passed = np.zeros(h * w, np.int64)
        while len(live):
            out, idx = o.intersect(cur)
            hit = idx >= 0
            me = np.zeros((len(live), 12), f32)
            for u in np.unique(idx[hit]):
                sel = idx == u
                me[sel] = o.material_eval(int(u), out[sel, 3:5])
            op = me[:, 6]
            through = np.zeros(len(live), bool)
            for k in np.flatnonzero(hit & ~((op == f32(1)) | (np.abs(op - f32(1)) < EPS))):   # !is_approx(opacity, 1)
                through[k] = ora.draws(int(pixel[live[k]]), s, seed, 0, int(pas[k]), 0)[0] > op[k]
            surf = hit & ~through
            n, oc = out[surf, 11:14], -cur[surf, 3:6]   # the shading normal; outcoming = -d of the ray that found the surface
            front = ((n[:, 0] * oc[:, 0] + n[:, 1] * oc[:, 1]) + n[:, 2] * oc[:, 2]) > 0
            e10 = (me[surf, 9:12] * f32(10)).astype(f32)   # material_eval gives get_emissive(uv); renderer.cpp:462 multiplies by 10
            r = np.concatenate([e10, np.ones((int(surf.sum()), 1), f32)], 1).astype(f32)
            r[~front] = 0
            rec[live[surf]] = r
            ended[live[surf]] = True
            lit = front & (me[surf, 9:12] != 0).any(1)
            counts["surface"] += int(surf.sum())
            counts["back"] += int((~front).sum())
            counts["emissive"] += int(lit.sum())
            counts["emissive_through"] += int((lit & (pas[surf] > 0)).sum())
            d = cur[through, 3:6]
            nxt = np.concatenate([out[through, :3] + d * EPS, d * (f32(1) / _len3(d))[:, None]], 1).astype(f32)
            pas = pas[through] + 1
            live = live[through]
            passed[live] = pas
            keep = pas <= 4096
            live, cur, pas = live[keep], nxt[keep], pas[keep]
        took = rec[:, 3] > 0
        em[took] += rec[took]
        counts["through"] += int((passed > 0).sum())
        counts["miss"] += int((~ended).sum())
        records.append(rec)
    em = em.reshape(h, w, 4)
    return (em, counts, records) if per_sample else (em, counts)


def _mean(emission, guide_spp):
    with np.errstate(all="ignore"):
        return (np.asarray(emission, f32)[..., :3] / f32(guide_spp)).astype(f32)


def split(emission, guide_spp, a, b=None):
    """ptx_emission_split on copies: per channel with e = emission / float(guide_spp) > 0, x.c = x.c - (x.w * e.c); every other bit kept.
    -> (a, b) (b None when not given)"""
    e = _mean(emission, guide_spp)
    with np.errstate(all="ignore"):
        on = e > 0
    out = []
    for x in (a, b):
        if x is None:
            out.append(None)
            continue
        x = np.array(x, f32)
        with np.errstate(all="ignore"):
            prod = (x[..., 3:4] * e).astype(f32)
            x[..., :3] = np.where(on, (x[..., :3] - prod).astype(f32), x[..., :3])
        out.append(x)
    return out[0], out[1]


def merge(emission, guide_spp, out):
    """ptx_emission_merge on a copy: per channel with e > 0, out.c = out.c + e.c; every other bit kept."""
    e = _mean(emission, guide_spp)
    out = np.array(out, f32)
    with np.errstate(all="ignore"):
        out[..., :3] = np.where(e > 0, (out[..., :3] + e).astype(f32), out[..., :3])
    return out


def checker_frame(W_=20, H_=12, n_half=4):
    """Consequence (b)'s frame, every factor dyadic: e a one-pixel checker of (2, 0.5, 0.25) (0 elsewhere), counts n_half + n_half,
    a = n*e + d and b = n*e - d with d = +-4 in an unrelated pattern (3-pixel stripes), albedo 0.5, flat normals and depth.
    -> (a, b, albedo_cov, normal_depth, emission sums over 2 * n_half samples, e [H,W,3])"""
    yy, xx = np.mgrid[0:H_, 0:W_]
    e = np.where(((xx + yy) % 2 == 0)[..., None], np.array([2, 0.5, 0.25], f32), f32(0)).astype(f32)
    d = np.where((((xx // 3) + 2 * yy) % 2 == 0), f32(4), f32(-4))[..., None].astype(f32)
    n = f32(n_half)
    a, b = np.zeros((H_, W_, 4), f32), np.zeros((H_, W_, 4), f32)
    a[..., :3], b[..., :3] = n * e + d, n * e - d
    a[..., 3] = b[..., 3] = n
    ng = 2 * n_half
    A, N = np.zeros((H_, W_, 4), f32), np.zeros((H_, W_, 4), f32)
    A[..., :3], A[..., 3] = f32(0.5) * ng, ng
    N[..., 2], N[..., 3] = ng, f32(2) * ng
    em = np.zeros((H_, W_, 4), f32)
    em[..., :3], em[..., 3] = e * f32(ng), ng
    return a, b, A, N, em, e
