"""The adaptive loop's stopping rule restated in float32 numpy from its specification in include/ptx.h (ptx_render_adaptive; the same text
governs ptx_render_adaptive_nee), with the round sizes and the replay of the loop on full-frame snapshots. Every operation is a float32 numpy
operation in the written parenthesisation; `np.fmax` is the max that returns the other operand when one is NaN. Nothing here goes through libm,
so the product is held to bitwise equality. Not collected (underscore prefix).
"""
import numpy as np

f32 = np.float32


def restate_noisy(a, b, thr):
    """[h,w] bool: the two halves' means disagree by more than thr (NaN: noisy)."""
    a, b = np.asarray(a, f32), np.asarray(b, f32)
    with np.errstate(all="ignore"):
        ma = [a[..., c] / a[..., 3] for c in range(3)]
        mb = [b[..., c] / b[..., 3] for c in range(3)]
        d = (np.abs(ma[0] - mb[0]) + np.abs(ma[1] - mb[1])) + np.abs(ma[2] - mb[2])
        m = ((ma[0] + mb[0]) + (ma[1] + mb[1])) + (ma[2] + mb[2])
        e2 = ((d * d) * f32(0.25)) / np.fmax(m * f32(0.5), f32(0.01))
        assert e2.dtype == np.float32
        return ~(e2 <= f32(thr) * f32(thr))


def restate_order(h, w):
    """The tile-local indices ly * w + lx of an h x w rectangle in list order: 32 x 32 tiles row-major, anchored at the rectangle's origin;
    inside a tile its 8 x 8 blocks row-major; inside a block rows."""
    out = []
    for ty in range(0, h, 32):
        for tx in range(0, w, 32):
            for by in range(ty, min(ty + 32, h), 8):
                for bx in range(tx, min(tx + 32, w), 8):
                    ys, xs = np.arange(by, min(by + 8, h)), np.arange(bx, min(bx + 8, w))
                    out.append((ys[:, None] * w + xs[None, :]).ravel())
    return np.concatenate(out).astype(np.uint32)


def restate_select(a, b, done, thr):
    """One decision. -> (done' [h,w] uint8, the active list uint32). active = !done && (a noisy pixel in the 3 x 3 block clipped to the
    rectangle); done' = done | !active."""
    noisy = restate_noisy(a, b, thr)
    h, w = noisy.shape
    pad = np.zeros((h + 2, w + 2), bool)
    pad[1:-1, 1:-1] = noisy
    near = np.zeros((h, w), bool)
    for dy in range(3):
        for dx in range(3):
            near |= pad[dy:dy + h, dx:dx + w]
    active = (np.asarray(done) == 0) & near
    order = restate_order(h, w)
    return np.where(active, 0, 1).astype(np.uint8), order[active.ravel()[order]]


def restate_mean(a, b=None):
    a = np.asarray(a, f32)
    with np.errstate(all="ignore"):
        if b is None:
            return (a / a[..., 3:4]).astype(f32)
        b = np.asarray(b, f32)
        return ((a + b) / (a[..., 3:4] + b[..., 3:4])).astype(f32)


def round_sizes(cap, min_spp, step):
    """The samples of round 0, 1, ...: min_spp, then min(step, what is left to the cap)."""
    out, given = [], 0
    while given < cap:
        out.append(min_spp if not given else min(step, cap - given))
        given += out[-1]
    return out


def replay(snaps, thr):
    """The loop on full-rectangle snapshots [(A_r, B_r)] of the rounds: -> (a, b, rounds, active_last). A pixel active after round r - 1 takes
    round r's snapshot; a stopped one keeps what it has."""
    a, b = snaps[0][0].copy(), snaps[0][1].copy()
    done = np.zeros(a.shape[:2], np.uint8)
    for r in range(len(snaps)):
        if r:
            act = done == 0
            a[act], b[act] = snaps[r][0][act], snaps[r][1][act]
        done, pix = restate_select(a, b, done, thr)
        assert len(pix) == int((done == 0).sum()), (len(pix), int((done == 0).sum()))
        if not len(pix):
            break
    return a, b, r + 1, len(pix)


def crop(snaps, tile):
    x0, y0, w, h = tile
    return [(fa[y0:y0 + h, x0:x0 + w], fb[y0:y0 + h, x0:x0 + w]) for fa, fb in snaps]
