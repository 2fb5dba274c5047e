"""The sharded adaptive loop restated in numpy from its specification in include/ptx.h (ptx_ctx_set_mask_exchange), on top of the unsharded
restatement (_adaptive_restatement.py): the ownership mask, the noisy bytes a rank sends, the decision of the whole rectangle from a merged
mask, the rank's own list, and the replay of all ranks in lockstep on full-rectangle snapshots. Not collected (underscore prefix).
"""
import numpy as np

from _adaptive_restatement import f32, restate_noisy, restate_order


def own_mask(rank, world, W, rect, tile=64):
    """[h,w] bool: the pixels of the rectangle (x0, y0, w, h) of an image W wide that `rank` owns. Written out pixel by pixel from the header's
    formula, on purpose not through multigpu.tile_mask (the tests assert the two equal)."""
    x0, y0, w, h = rect
    ts = tile if tile else 64
    tiles_x = (W + ts - 1) // ts
    out = np.zeros((h, w), bool)
    for ly in range(h):
        for lx in range(w):
            out[ly, lx] = (((y0 + ly) // ts) * tiles_x + (x0 + lx) // ts) % world == rank
    return out


def sent_mask(a, b, thr, own):
    """[h,w] uint8: what a rank writes before the exchange: noisy_p for its own pixels, 0 for the others (whose sums are zeros here: 0 / 0 is
    a NaN, which the unmasked rule would call noisy)."""
    return (restate_noisy(a, b, thr) & own).astype(np.uint8)


def near(mask):
    """[h,w] bool: some pixel of the 3 x 3 block, clipped to the rectangle, has a nonzero byte."""
    m = np.asarray(mask) != 0
    h, w = m.shape
    pad = np.zeros((h + 2, w + 2), bool)
    pad[1:-1, 1:-1] = m
    out = np.zeros((h, w), bool)
    for dy in range(3):
        for dx in range(3):
            out |= pad[dy:dy + h, dx:dx + w]
    return out


def decide(merged, done, own):
    """The decision of the WHOLE rectangle from the merged mask (nonzero = noisy). -> (done' [h,w] uint8 over all pixels, the number of all
    active pixels, the rank's own active list in the specified order)."""
    active = (np.asarray(done) == 0) & near(merged)
    h, w = active.shape
    order = restate_order(h, w)
    return np.where(active, 0, 1).astype(np.uint8), int(active.sum()), order[(active & own).ravel()[order]]


def replay_sharded(snaps, thr, world, tile, rect, W, merge=True):
    """All ranks of the sharded loop in lockstep on the rectangle's snapshots [(A_r, B_r)] (running sums after round r of EVERY pixel; a pixel
    that is rendered in round r takes round r's values, which are its own running sums because a stopped pixel never restarts).
    merge=False: an exchange that hands every rank its own bytes back.
    -> one dict per rank: a, b (zero outside the own pixels), rounds, active_last (own), sent (the bytes it wrote, per round), merged (what it
    read back, per round), cross (per round: own pixels kept active ONLY by a noisy pixel another rank owns)."""
    h, w = snaps[0][0].shape[:2]
    assert rect[2:] == (w, h), (rect, w, h)
    ranks = []
    for q in range(world):
        own = own_mask(q, world, W, rect, tile)
        ranks.append(dict(own=own, a=np.zeros((h, w, 4), f32), b=np.zeros((h, w, 4), f32), done=np.zeros((h, w), np.uint8), todo=own.copy(), rounds=0,
                          active_last=0, sent=[], merged=[], cross=[], over=False))
    assert (np.sum([r["own"] for r in ranks], axis=0) == 1).all()
    for r in range(len(snaps)):
        live = [q for q in ranks if not q["over"]]
        if not live:
            break
        for q in live:
            m = q["todo"]
            q["a"][m], q["b"][m] = snaps[r][0][m], snaps[r][1][m]
            q["sent"].append(sent_mask(q["a"], q["b"], thr, q["own"]))
            q["rounds"] += 1
        union = np.maximum.reduce([q["sent"][-1] for q in live])
        for q in live:
            merged = union if merge else q["sent"][-1]
            q["merged"].append(merged)
            before = q["done"] == 0
            q["cross"].append(int((q["own"] & before & near(merged) & ~near(q["sent"][-1])).sum()))
            q["done"], n_all, pix = decide(merged, q["done"], q["own"])
            q["todo"] = np.zeros((h, w), bool)
            q["todo"].ravel()[pix] = True
            q["active_last"] = len(pix)
            q["over"] = n_all == 0
        if merge:
            assert len({q["over"] for q in ranks}) == 1 and len({q["rounds"] for q in ranks}) == 1   # no second collective is needed
            assert all((q["done"] == ranks[0]["done"]).all() for q in ranks)
    return ranks
