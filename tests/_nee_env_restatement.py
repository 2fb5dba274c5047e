"""numpy restatement of PTX_NEE_ENV_SAMPLES' table, pdf and sampler (include/ptx.h: THE ENVIRONMENT TABLE, THE PDF, ENVIRONMENT SAMPLE), for
tests/_nee_estimator.py and tests/test_nee_env.py; the estimator's use of them (SELECTION, MISS WEIGHT) is in tests/_nee_estimator.py. (u, v) and
Le of a direction come from the oracle's env_lookup.

build_tables: the table from the texels in float64, as the specification words it (np.roll for the wrapped 3 x 3 footprint).
env_pdf / sample_env: the pdf and the sampler on float32 arrays in the specification's operation order. cos and sin of the sampled
direction are float64 values rounded to float32 (the product's are ocml's cosf / sinf: last-place differences).

R0: the ratio of flagged to unflagged per-sample variance that test_nee_env.test_expectation_and_variance_on_the_restatement measures on
VARIANCE_CASE; the GPU test's bar is 2 * R0.
"""
import struct

import numpy as np

from _nee_restatement import _fmax2, f32

KU, KV = f32(0.1591), f32(0.3183)

# the scene, frame and map of the variance comparison (CPU: the restatement, GPU: the product), and the restatement's measured ratio
VARIANCE_CASE = dict(name="chart", W=24, H=16, spp=64, bounces=3, seed=0x5EED, env=(1.0, 1.0, 1.0))
R0 = 0.2321   # measured on the restatement; the CPU test recomputes it and holds it to this figure


# ---------------------------------------------------------------------------- maps
def write_hdr(path, rgb):
    """rgb [h, w, 3] float -> an uncompressed (flat) Radiance .hdr file; returns the path. Values are chosen by the tests so that no
    scanline begins with the bytes (2, 2), which would announce a run-length coded line."""
    rgb = np.asarray(rgb, np.float64)
    h, w, _ = rgb.shape
    out = bytearray(b"#?RADIANCE\nFORMAT=32-bit_rle_rgbe\n\n" + f"-Y {h} +X {w}\n".encode())
    for row in rgb:
        for px in row:
            m = float(px.max())
            if m < 1e-32:
                out += bytes(4)
                continue
            mant, ex = np.frexp(m)
            sc = mant * 256.0 / m
            out += struct.pack("4B", int(px[0] * sc), int(px[1] * sc), int(px[2] * sc), int(ex) + 128)
    with open(path, "wb") as f:
        f.write(bytes(out))
    return str(path)


def hot_texel(w=16, h=8, base=0.05, hot=400.0, at=(0, 0)):
    """a dim grey map with one hot texel (column, row) — in a corner the wrapped 3 x 3 footprint reaches both opposite edges"""
    rgb = np.full((h, w, 3), base)
    rgb[at[1], at[0]] = (hot, hot * 0.9, hot * 0.7)
    return rgb


def map_pixels(ptx, s):
    """[h, w, 3] float32: rgb of the scene's environment texels as the kernels' tex_pixel reads them (the last texture of the arrays: sRGB
    table for 8-bit texels, powf for float ones, missing channels 1), or None without a map."""
    tex = s.array(ptx.ARR_TEXTURES).reshape(-1, 4)
    if not len(tex):
        return None
    w, h, cs, off = [int(x) for x in tex[-1]]
    c, srgb, is_f = cs & 255, bool(cs & 0x100), bool(cs & 0x10000)
    if is_f:
        raw = s.array(ptx.ARR_TEXELS_F32)[off:off + w * h * c].reshape(h, w, c).astype(f32)
    else:
        raw = s.array(ptx.ARR_TEXELS)[off:off + w * h * c].reshape(h, w, c).astype(f32) / f32(255)
    with np.errstate(all="ignore"):
        lin = np.power(raw, f32(2.2)) if srgb else raw
    out = np.ones((h, w, 3), f32)
    k = min(c, 3)
    out[..., :k] = lin[..., :k]
    return out


def build_tables(pix):
    """pix [h, w, 3] -> (row_cdf float32 [h], cell_cdf float32 [h, w]); two empty arrays for a black map or None"""
    if pix is None:
        return np.zeros(0, f32), np.zeros((0, 0), f32)
    p = np.asarray(pix, np.float64)
    h, w, _ = p.shape
    lum = (0.2126 * p[..., 0] + 0.7152 * p[..., 1]) + 0.0722 * p[..., 2]
    lum = np.where(lum > 0, lum, 0.0)
    foot = sum(np.roll(lum, (-dj, -di), (0, 1)) for dj in (-1, 0, 1) for di in (-1, 0, 1))
    lat = ((1.0 - (np.arange(h) + 0.5) / h) - 0.5) / 0.3183
    wgt = foot * np.maximum(np.cos(lat), 0.0)[:, None]
    mass = wgt.sum(1)
    total = mass.sum()
    if not total > 0:
        return np.zeros(0, f32), np.zeros((0, 0), f32)
    row = (np.cumsum(mass) / total).astype(f32)
    row[-1] = 1
    cell = np.zeros((h, w), f32)
    nz = mass > 0
    cell[nz] = (np.cumsum(wgt[nz], 1) / mass[nz, None]).astype(f32)
    cell[nz, -1] = 1
    return row, cell


def table(row, cell):
    """the dict the functions below take, from the two arrays (the product's PTX_ARR_ENV_* or build_tables'); None when they are empty"""
    row = np.asarray(row, f32).reshape(-1)
    if not len(row):
        return None
    cell = np.asarray(cell, f32).reshape(len(row), -1)
    return dict(row=row, cell=cell, w=cell.shape[1], h=len(row))


# ---------------------------------------------------------------------------- the pdf and the sampler
def env_box(tab, uv):
    """box (i, j) of the lookup's (u, v) [n, 2]"""
    w, h = tab["w"], tab["h"]
    with np.errstate(all="ignore"):
        fi = np.nan_to_num(uv[:, 0] * f32(w), nan=0.0, posinf=0.0, neginf=0.0)
        fj = np.nan_to_num((f32(1) - uv[:, 1]) * f32(h), nan=0.0, posinf=0.0, neginf=0.0)
    return np.minimum(np.maximum(fi, 0).astype(np.int64), w - 1), np.minimum(np.maximum(fj, 0).astype(np.int64), h - 1)


def box_probability(tab, i, j):
    """P of box (i, j) from the stored float32 differences"""
    row, cell = tab["row"], tab["cell"]
    pr = row[j] - np.where(j > 0, row[np.maximum(j - 1, 0)], f32(0)).astype(f32)
    pc = cell[j, i] - np.where(i > 0, cell[j, np.maximum(i - 1, 0)], f32(0)).astype(f32)
    return (pr * pc).astype(f32)


def env_pdf(tab, d, uv):
    """env_pdf of directions d [n, 3] whose lookup coordinates are uv [n, 2] -> float32 [n]"""
    i, j = env_box(tab, uv)
    P = box_probability(tab, i, j)
    with np.errstate(all="ignore"):
        c = np.sqrt(_fmax2(f32(0), f32(1) - d[:, 1] * d[:, 1]))
        p = ((P * f32(tab["w"] * tab["h"])) * (KU * KV)) / c
    return np.where(c > 0, p, f32(0)).astype(f32)


def sample_env(tab, q):
    """q [n, 4] float32 draws -> (i, j, w_dir [n, 3] float32)"""
    w, h = tab["w"], tab["h"]
    j = np.minimum(np.searchsorted(tab["row"], q[:, 0], side="right"), h - 1)
    i = np.zeros(len(q), np.int64)
    for jj in np.unique(j):
        sel = j == jj
        i[sel] = np.minimum(np.searchsorted(tab["cell"][jj], q[sel, 1], side="right"), w - 1)
    u = (i.astype(f32) + q[:, 2]) / f32(w)
    v = f32(1) - (j.astype(f32) + q[:, 3]) / f32(h)
    phi, lat = (u - f32(0.5)) / KU, (v - f32(0.5)) / KV
    cl, sl = np.cos(lat.astype(np.float64)).astype(f32), np.sin(lat.astype(np.float64)).astype(f32)
    cp, sp = np.cos(phi.astype(np.float64)).astype(f32), np.sin(phi.astype(np.float64)).astype(f32)
    return i, j, np.stack([cl * cp, sl, cl * sp], -1).astype(f32)
