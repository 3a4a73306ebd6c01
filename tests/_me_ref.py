"""Motion search by block matching in numpy: the CPU yardstick of me_kernels.hip, built on _mc_ref.

The cost of a candidate restates od_mv_est_bma_sad (src/mcenc.c:2224-2264): od_mc_predict1fmv8_c of one vector on
the B x B block centred on a grid point (src/mcenc.c:2589-2611; _mc_ref.predict1), then od_enc_sad against the
source picture clipped to the picture (src/mcenc.c:1615-1679).  tests/test_me_ref.py pins bma_sad to values the
compiled reference gave (tests/golden/me.npz).  The search over candidates is the fixed one include/daala_hip.h
defines for odhip_me_search: all full-pel offsets within `range` in all slots, then rounds of eight sub-pel
neighbours, each won by the smallest (cost, |mvx| + |mvy|, slot, mvy, mvx); candidates outside the legal range are
never evaluated."""
import numpy as np
from numpy.lib.stride_tricks import sliding_window_view

import _mc_ref as R


def block_of(vx, vy, log_size):
    """(bx, by, B): the block centred on grid point (vx, vy)."""
    blk = 8 << log_size
    return 8*vx - blk//2, 8*vy - blk//2, blk


def clip_of(bx, by, blk, pic_w, pic_h):
    """The part of the block inside the picture as picture coordinates (x0, x1, y0, y1), or None."""
    x0, x1, y0, y1 = max(bx, 0), min(bx + blk, pic_w), max(by, 0), min(by + blk, pic_h)
    return None if x1 <= x0 or y1 <= y0 else (x0, x1, y0, y1)


def bma_sad(src, pic_w, pic_h, ref, vx, vy, log_size, mvx, mvy):
    """SAD of one candidate: src is the picture (at least pic_h x pic_w), ref an unpadded coded-size plane."""
    bx, by, blk = block_of(vx, vy, log_size)
    c = clip_of(bx, by, blk, pic_w, pic_h)
    if c is None:
        return 0
    x0, x1, y0, y1 = c
    pred = R.predict1(ref, bx, by, mvx, mvy, blk, 0)
    return int(np.abs(pred[y0 - by:y1 - by, x0 - bx:x1 - bx] - src[y0:y1, x0:x1].astype(np.int64)).sum())


def window_ok(v, mv, lg, dec, n):
    """One axis of _mc_ref.grid_in_range: the window of a leaf of 1 << lg grid steps at grid position v."""
    pad, blk = R.BORDER >> dec, 8 << lg >> dec
    x0 = (v << 3 >> dec) + (R.scale_mv(mv, dec) >> 3) - 2
    return x0 >= -pad and x0 + blk + 5 <= (n << 3 >> dec) + pad


def mv_ok(v, mv, lg, n):
    """One axis of the legality predicate: both leaves of the size inside the frame that have the point at v as
    a corner keep their windows inside the border, at dec 0 and dec 1."""
    for lv in (v, v - (1 << lg)):
        if 0 <= lv < n and not (window_ok(lv, mv, lg, 0, n) and window_ok(lv, mv, lg, 1, n)):
            return False
    return True


def legal(coded_w, coded_h, vx, vy, lg, mvx, mvy):
    return mv_ok(vx, mvx, lg, coded_w >> 3) and mv_ok(vy, mvy, lg, coded_h >> 3)


def limits(coded_w, coded_h, lg, vx, vy):
    """Full-pel (xmin, xmax, ymin, ymax) legal for the point."""
    out = []
    for v, n in ((vx, coded_w >> 3), (vy, coded_h >> 3)):
        lo = hi = 0
        while mv_ok(v, 8*(lo - 1), lg, n):
            lo -= 1
        while mv_ok(v, 8*(hi + 1), lg, n):
            hi += 1
        out += [lo, hi]
    return tuple(out)


def fullpel_sads(src, pic_w, pic_h, ref, vx, vy, log_size, rng):
    """bma_sad of every full-pel offset [dy + rng][dx + rng] at once: at phase 0 predict1 copies the window."""
    bx, by, blk = block_of(vx, vy, log_size)
    side = 2*rng + 1
    c = clip_of(bx, by, blk, pic_w, pic_h)
    if c is None:
        return np.zeros((side, side), np.int64)
    x0, x1, y0, y1 = c
    win = R.window(ref, x0 - rng, y0 - rng, x1 - x0 + 2*rng, y1 - y0 + 2*rng).astype(np.int16)
    views = sliding_window_view(win, (y1 - y0, x1 - x0))
    return np.abs(views - src[y0:y1, x0:x1].astype(np.int16)).sum(axis=(2, 3), dtype=np.int64)


def search_picture(src, pic_w, pic_h, refs, log_size, rng, res, lam):
    """One picture: (grid MV_POINT [nv + 1][nh + 1], cost uint32 of the same shape)."""
    coded_h, coded_w = refs[0].shape
    nh, nv = coded_w >> 3, coded_h >> 3
    grid = np.zeros((nv + 1, nh + 1), R.MV_POINT)
    cost = np.zeros((nv + 1, nh + 1), np.uint32)
    offs = np.arange(-rng, rng + 1)
    for vy in range(0, nv + 1, 1 << log_size):
        oky = np.array([mv_ok(vy, 8*d, log_size, nv) for d in offs])
        for vx in range(0, nh + 1, 1 << log_size):
            okx = np.array([mv_ok(vx, 8*d, log_size, nh) for d in offs])
            keys = []
            for slot, ref in enumerate(refs):
                sads = fullpel_sads(src, pic_w, pic_h, ref, vx, vy, log_size, rng)
                for iy, ix in zip(*np.nonzero(oky[:, None] & okx[None, :])):
                    mvx, mvy = 8*int(offs[ix]), 8*int(offs[iy])
                    l1 = abs(mvx) + abs(mvy)
                    keys.append((8*int(sads[iy, ix]) + lam*l1, l1, slot, mvy, mvx))
            best = min(keys)
            step = 4
            while step >= 1 << res:
                _, _, slot, cy, cx = best
                for dy in (-step, 0, step):
                    for dx in (-step, 0, step):
                        mvx, mvy = cx + dx, cy + dy
                        if (dx or dy) and legal(coded_w, coded_h, vx, vy, log_size, mvx, mvy):
                            sad = bma_sad(src, pic_w, pic_h, refs[slot], vx, vy, log_size, mvx, mvy)
                            l1 = abs(mvx) + abs(mvy)
                            best = min(best, (8*sad + lam*l1, l1, slot, mvy, mvx))
                step >>= 1
            grid[vy, vx] = (best[4], best[3], 1, best[2], 0)
            cost[vy, vx] = best[0]
    return grid, cost


def search(src, pic_w, pic_h, refs, log_size, rng, res, lam):
    """src [F][>= pic_h][>= pic_w], refs: per slot [F][coded_h][coded_w].  (grid [F][nv + 1][nh + 1], cost)."""
    out = [search_picture(src[f], pic_w, pic_h, [r[f] for r in refs], log_size, rng, res, lam)
           for f in range(src.shape[0])]
    return np.stack([g for g, _ in out]), np.stack([c for _, c in out])


# ---- content for the tests ----
def smooth_noise(rng, h, w, gain=2.5):
    """Noise low-passed with a 5-tap binomial in both directions, stretched back over the 8-bit range."""
    a = rng.randint(0, 256, size=(h + 4, w + 4)).astype(np.float64)
    k = np.array([1, 4, 6, 4, 1], np.float64)/16
    a = sum(a[i:i + h]*k[i] for i in range(5))
    a = sum(a[:, i:i + w]*k[i] for i in range(5))
    return np.clip((a - 128)*gain + 128, 0, 255).astype(np.uint8)


def displaced(ref, mvx, mvy):
    """The whole plane `ref` predicted with one vector: what every block's candidate (mvx, mvy) predicts."""
    h, w = ref.shape
    return R.predict1(ref, 0, 0, mvx, mvy, max(h, w), 0)[:h, :w].astype(np.uint8)
