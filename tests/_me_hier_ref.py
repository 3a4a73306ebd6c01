"""The coarse-to-fine motion search in numpy: the CPU yardstick of odhip_me_search3 / odhip_me_costs3 /
odhip_me_downsample (me_kernels.hip), built on _me_ref, _me_cost_ref and _mc_ref.

The pyramid halves a plane with (a + b + c + d + 2) >> 2 over clamped 2 x 2 cells; a level j is searched as a plane of
decimation j: block (bx >> j, by >> j) of size B >> j, the vector v as the sample offset v / (8 << j), the clip to
OD_PLANE_SZ(pic, j) - what _me_cost_ref.plane_dist does at dec = j on a full-pel vector, which tests/test_me_hier_ref.py
ties level_sads to.  Each slot descends on its own from level `levels` to 1 under cost 8 (D << 2j) + lam |v|_1; level
0 is stage 1 of _me_cost_ref.search round every slot's own centre, then its stage 2.  include/daala_hip.h has the
definition."""
import numpy as np
from numpy.lib.stride_tricks import sliding_window_view

import _mc_ref as R
import _me_ref as M
import _me_cost_ref as C


def halve(p):
    """One level up: ((h + 1) >> 1) x ((w + 1) >> 1), an odd last row or column replicated."""
    h, w = p.shape
    q = R.window(p, 0, 0, (w + 1) & ~1, (h + 1) & ~1)
    return ((q[0::2, 0::2] + q[0::2, 1::2] + q[1::2, 0::2] + q[1::2, 1::2] + 2) >> 2).astype(np.uint8)


def pyramid(p, levels):
    """[level 0 .. levels]; every level is the halving of the one below (level 2 rounds twice)."""
    out = [np.ascontiguousarray(p)]
    for _ in range(levels):
        out.append(halve(out[-1]))
    return out


def level_sads(src, pic_w, pic_h, ref, vx, vy, log_size, level, cx, cy, rad):
    """D_level of every offset [dy + rad][dx + rad] round the centre (cx, cy), all in level samples: src / ref are
    level `level` of the picture / the reference plane, (pic_w, pic_h) the LUMA picture size at level 0."""
    bx, by, blk = C.plane_block(vx, vy, log_size, level)
    side = 2*rad + 1
    c = M.clip_of(bx, by, blk, C.plane_sz(pic_w, level), C.plane_sz(pic_h, level))
    if c is None:
        return np.zeros((side, side), np.int64)
    x0, x1, y0, y1 = c
    win = R.window(ref, x0 + cx - rad, y0 + cy - rad, x1 - x0 + 2*rad, y1 - y0 + 2*rad).astype(np.int16)
    views = sliding_window_view(win, (y1 - y0, x1 - x0))
    return np.abs(views - src[y0:y1, x0:x1].astype(np.int16)).sum(axis=(2, 3), dtype=np.int64)


def chroma_sads(src, pic_w, pic_h, ref, vx, vy, log_size, cx, cy, rad, dec):
    """A chroma plane's SAD at the full-pel luma offsets (cx + dx, cy + dy), [dy + rad][dx + rad].  At dec = 1 the
    ABSOLUTE luma offset x is the chroma vector 4 x: sample offset x >> 1 at phase 4 (x & 1)."""
    if dec == 0:
        return level_sads(src, pic_w, pic_h, ref, vx, vy, log_size, 0, cx, cy, rad)
    side = 2*rad + 1
    c = C.plane_clip(vx, vy, log_size, dec, pic_w, pic_h)
    if c is None:
        return np.zeros((side, side), np.int64)
    x0, x1, y0, y1 = c
    lox, loy = (cx - rad) >> 1, (cy - rad) >> 1
    nco = max(((cx + rad) >> 1) - lox, ((cy + rad) >> 1) - loy) + 1
    s = max(x1 - x0, y1 - y0) + nco - 1
    win = R.window(ref, x0 + lox - 2, y0 + loy - 2, s + 5, s + 5)
    blk = src[y0:y1, x0:x1].astype(np.int64)
    per = {}
    for fy in (0, 1):
        for fx in (0, 1):
            plane = R.predict1_window(win, 4*fx, 4*fy, 0)
            views = sliding_window_view(plane, blk.shape)[:nco, :nco]
            per[fy, fx] = np.abs(views - blk).sum(axis=(2, 3), dtype=np.int64)
    out = np.zeros((side, side), np.int64)
    for iy in range(side):
        ay = cy - rad + iy
        for ix in range(side):
            ax = cx - rad + ix
            out[iy, ix] = per[ay & 1, ax & 1][(ay >> 1) - loy, (ax >> 1) - lox]
    return out


def _keys(dist, scale, lam, slot, vx, vy, lg, nh, nv, c, step, rad):
    """The keys of the legal candidates c + step (dx, dy) at distortions dist[dy + rad][dx + rad] << scale."""
    offs = range(-rad, rad + 1)
    okx = [M.mv_ok(vx, c[0] + step*d, lg, nh) for d in offs]
    oky = [M.mv_ok(vy, c[1] + step*d, lg, nv) for d in offs]
    keys = []
    for iy, dy in enumerate(offs):
        for ix, dx in enumerate(offs):
            if okx[ix] and oky[iy]:
                mvx, mvy = c[0] + step*dx, c[1] + step*dy
                l1 = abs(mvx) + abs(mvy)
                keys.append((8*(int(dist[iy, ix]) << scale) + lam*l1, l1, slot, mvy, mvx))
    return keys


def search_picture(srcs, pic_w, pic_h, refs, log_size, rng, res, lam, lam_subpel, flags, cdec, levels, refine,
                   centres=None):
    """One picture: srcs = (Y, Cb, Cr) pictures, refs: per slot (Y, Cb, Cr) planes.  (grid, cost); `centres`, a dict,
    receives {(vx, vy, slot): the level-0 centre}."""
    coded_h, coded_w = refs[0][0].shape
    nh, nv = coded_w >> 3, coded_h >> 3
    chroma = bool(flags & C.CHROMA)
    metric = C.SATD_METRIC if flags & C.SATD else C.SAD_METRIC
    src_pyr = pyramid(srcs[0][:pic_h, :pic_w], levels)
    ref_pyr = [pyramid(r[0], levels) for r in refs]
    grid = np.zeros((nv + 1, nh + 1), R.MV_POINT)
    cost = np.zeros((nv + 1, nh + 1), np.uint32)
    for vy in range(0, nv + 1, 1 << log_size):
        for vx in range(0, nh + 1, 1 << log_size):
            keys = []
            for slot, ref in enumerate(refs):
                c = (0, 0)
                for j in range(levels, 0, -1):
                    rad, step = (rng if j == levels else refine), 8 << j
                    d = level_sads(src_pyr[j], pic_w, pic_h, ref_pyr[slot][j], vx, vy, log_size, j, c[0]//step,
                                   c[1]//step, rad)
                    best = min(_keys(d, 2*j, lam, slot, vx, vy, log_size, nh, nv, c, step, rad))
                    c = (best[4], best[3])
                if centres is not None:
                    centres[vx, vy, slot] = c
                rad = refine if levels else rng
                dist = level_sads(srcs[0], pic_w, pic_h, ref[0], vx, vy, log_size, 0, c[0] >> 3, c[1] >> 3, rad)
                if chroma:
                    for pl in (1, 2):
                        dist = dist + (chroma_sads(srcs[pl], pic_w, pic_h, ref[pl], vx, vy, log_size, c[0] >> 3,
                                                   c[1] >> 3, rad, cdec) >> 2)
                keys += _keys(dist, 0, lam, slot, vx, vy, log_size, nh, nv, c, 8, rad)
            best = min(keys)

            def key2(slot, mvx, mvy):
                d = C.total(C.cand_dist(srcs, pic_w, pic_h, refs[slot], vx, vy, log_size, mvx, mvy, cdec, metric,
                                        chroma))
                l1 = abs(mvx) + abs(mvy)
                return (8*d + lam_subpel*l1, l1, slot, mvy, mvx)

            if res < 3:
                best = key2(best[2], best[4], best[3])
            step = 4
            while step >= 1 << res:
                _, _, slot, cy, cx = best
                for dy in (-step, 0, step):
                    for dx in (-step, 0, step):
                        mvx, mvy = cx + dx, cy + dy
                        if (dx or dy) and M.legal(coded_w, coded_h, vx, vy, log_size, mvx, mvy):
                            best = min(best, key2(slot, mvx, mvy))
                step >>= 1
            grid[vy, vx] = (best[4], best[3], 1, best[2], 0)
            cost[vy, vx] = best[0]
    return grid, cost


def search(src, csrc, pic_w, pic_h, refs, crefs, log_size, rng, res, lam, lam_subpel, flags, cdec, levels, refine):
    """src [F][..], csrc [2F][..] or None without CHROMA, refs / crefs per slot as _me_cost_ref.search takes them.
    (grid [F][nv + 1][nh + 1], cost)."""
    nf = src.shape[0]
    if csrc is None:
        csrc, crefs = [None]*(2*nf), [[None]*(2*nf) for _ in refs]
    out = [search_picture((src[f], csrc[f], csrc[nf + f]), pic_w, pic_h,
                          [(r[f], c[f], c[nf + f]) for r, c in zip(refs, crefs)], log_size, rng, res, lam, lam_subpel,
                          flags, cdec, levels, refine) for f in range(nf)]
    return np.stack([g for g, _ in out]), np.stack([c for _, c in out])


def planted():
    """The planted displacement of the issue: (src [1][180][250], refs: two slots [1][192][256], the vector, the
    points whose block and match lie inside picture and frame)."""
    w, h, pw, ph = 256, 192, 250, 180
    rng = np.random.RandomState(3)
    big = M.smooth_noise(rng, h + 256, w + 256)
    slot1 = big[128:128 + h, 128:128 + w]
    src = big[128 - 45:128 - 45 + ph, 128 + 70:128 + 70 + pw]
    slot0 = M.smooth_noise(rng, h, w)
    mv = (560, -360)
    pts = []
    for vy in range(0, h//8 + 1, 4):
        for vx in range(0, w//8 + 1, 4):
            bx, by, blk = M.block_of(vx, vy, 2)
            if (bx >= 0 and by >= 0 and bx + blk <= pw and by + blk <= ph and 0 <= bx + 70 and bx + 70 + blk <= w
                    and 0 <= by - 45 and by - 45 + blk <= h):
                pts.append((vx, vy))
    return (np.ascontiguousarray(src)[None], [np.ascontiguousarray(slot0)[None], np.ascontiguousarray(slot1)[None]],
            mv, pts)
