"""The motion search's cost with chroma planes and SATD in numpy: the CPU yardstick of odhip_me_search2 /
odhip_me_costs2 (me_kernels.hip), built on _me_ref and _mc_ref.

Per plane with decimation d (0 luma, cdec for Cb and Cr) a candidate's distortion restates od_mv_est_bma_sad with
OD_MC_USE_CHROMA (src/mcenc.c:2224-2264) and od_enc_sad / od_enc_satd (src/mcenc.c:1615-1748): the block at
(bx >> d, by >> d) of size B >> d, the vector od_mc_scale_mv(mv, d), od_mc_predict1fmv8_c (_mc_ref.predict1), the
clip to the plane's picture size OD_PLANE_SZ, then SAD, or SATD by the CLIPPED size: 4x4 -> the 4x4 Hadamard,
(sum + 2) >> 2; a square of 8 .. 64 -> per 8x8 tile (sum + 4) >> 3; any other rectangle -> SAD.
dist = D_Y + (D_Cb >> 2) + (D_Cr >> 2); cost = 8 dist + lambda (|mvx| + |mvy|).  tests/test_me_cost_ref.py pins
plane_dist to values the compiled reference gave (tests/golden/me_cost.npz).  The search is _me_ref's with stage 1
always on SAD under `lam` and stage 2 on the flagged metric under `lam_subpel`, starting from the stage-1 winner
costed again."""
import numpy as np
from numpy.lib.stride_tricks import sliding_window_view

import _mc_ref as R
import _me_ref as M

CHROMA, SATD = 1, 2
SAD_METRIC, SATD_METRIC = 0, 1


def plane_sz(n, dec):
    return (n + (1 << dec) - 1) >> dec


def hadamard(n):
    h = np.array([[1]], np.int64)
    while h.shape[0] < n:
        h = np.block([[h, h], [h, -h]])
    return h


H4, H8 = hadamard(4), hadamard(8)


def satd_of(diff):
    """od_enc_satd's dispatch on a clipped difference rectangle."""
    h, w = diff.shape
    diff = diff.astype(np.int64)
    if w == h == 4:
        return (int(np.abs(H4 @ diff @ H4).sum()) + 2) >> 2
    if w == h and w in (8, 16, 32, 64):
        return sum((int(np.abs(H8 @ diff[y:y + 8, x:x + 8] @ H8).sum()) + 4) >> 3
                   for y in range(0, h, 8) for x in range(0, w, 8))
    return int(np.abs(diff).sum())


def plane_block(vx, vy, lg, dec):
    bx, by, blk = M.block_of(vx, vy, lg)
    return bx >> dec, by >> dec, blk >> dec


def plane_clip(vx, vy, lg, dec, pic_w, pic_h):
    """The clipped rectangle in the plane's picture coordinates (x0, x1, y0, y1), or None; pic_w, pic_h are luma's."""
    px, py, n = plane_block(vx, vy, lg, dec)
    return M.clip_of(px, py, n, plane_sz(pic_w, dec), plane_sz(pic_h, dec))


def plane_dist(src, pic_w, pic_h, ref, vx, vy, lg, mvx, mvy, dec, metric):
    """One plane's distortion: src is the plane's picture, ref its unpadded coded-size plane, (pic_w, pic_h) the LUMA
    picture size, (mvx, mvy) the luma vector."""
    px, py, n = plane_block(vx, vy, lg, dec)
    c = plane_clip(vx, vy, lg, dec, pic_w, pic_h)
    if c is None:
        return 0
    x0, x1, y0, y1 = c
    pred = R.predict1(ref, px, py, R.scale_mv(mvx, dec), R.scale_mv(mvy, dec), n, 0)
    diff = pred[y0 - py:y1 - py, x0 - px:x1 - px] - src[y0:y1, x0:x1].astype(np.int64)
    return satd_of(diff) if metric == SATD_METRIC else int(np.abs(diff).sum())


def cand_dist(srcs, pic_w, pic_h, refs, vx, vy, lg, mvx, mvy, cdec, metric, chroma=True):
    """(D_Y, D_Cb, D_Cr), unshifted; srcs / refs: the three planes' pictures / reference planes.  Chroma is 0
    without `chroma`."""
    out = [plane_dist(srcs[0], pic_w, pic_h, refs[0], vx, vy, lg, mvx, mvy, 0, metric), 0, 0]
    if chroma:
        for pl in (1, 2):
            out[pl] = plane_dist(srcs[pl], pic_w, pic_h, refs[pl], vx, vy, lg, mvx, mvy, cdec, metric)
    return tuple(out)


def total(d):
    return d[0] + (d[1] >> 2) + (d[2] >> 2)


def fullpel_chroma_sads(src, pic_w, pic_h, ref, vx, vy, lg, rng, dec):
    """A chroma plane's SAD at every full-pel luma offset [dy + rng][dx + rng].  At dec = 0 chroma slides like luma;
    at dec = 1 the luma offset dx is the chroma vector 4 dx: sample offset dx >> 1 at phase 4 (dx & 1), so the four
    half-pel planes of the window are built once and each is slid."""
    if dec == 0:
        return M.fullpel_sads(src, pic_w, pic_h, ref, vx, vy, lg, rng)
    side = 2*rng + 1
    c = plane_clip(vx, vy, lg, dec, pic_w, pic_h)
    if c is None:
        return np.zeros((side, side), np.int64)
    x0, x1, y0, y1 = c
    rc = (rng + 1) >> 1
    nco = (rng >> 1) + rc + 1
    s = max(x1 - x0, y1 - y0) + nco - 1
    win = R.window(ref, x0 - rc - 2, y0 - rc - 2, s + 5, s + 5)
    blk = src[y0:y1, x0:x1].astype(np.int64)
    per = {}
    for fy in (0, 1):
        for fx in (0, 1):
            plane = R.predict1_window(win, 4*fx, 4*fy, 0)
            views = sliding_window_view(plane, blk.shape)[:nco, :nco]
            per[fy, fx] = np.abs(views - blk).sum(axis=(2, 3), dtype=np.int64)
    offs = np.arange(-rng, rng + 1)
    out = np.zeros((side, side), np.int64)
    for fy in (0, 1):
        for fx in (0, 1):
            ys, xs = offs[(offs & 1) == fy], offs[(offs & 1) == fx]
            if ys.size and xs.size:
                out[np.ix_(ys + rng, xs + rng)] = per[fy, fx][np.ix_((ys >> 1) + rc, (xs >> 1) + rc)]
    return out


def search_picture(srcs, pic_w, pic_h, refs, log_size, rng, res, lam, lam_subpel, flags, cdec):
    """One picture: srcs = (Y, Cb, Cr) pictures, refs: per slot (Y, Cb, Cr) planes.  (grid, cost)."""
    coded_h, coded_w = refs[0][0].shape
    nh, nv = coded_w >> 3, coded_h >> 3
    chroma = bool(flags & CHROMA)
    metric = SATD_METRIC if flags & SATD else SAD_METRIC
    grid = np.zeros((nv + 1, nh + 1), R.MV_POINT)
    cost = np.zeros((nv + 1, nh + 1), np.uint32)
    offs = np.arange(-rng, rng + 1)
    for vy in range(0, nv + 1, 1 << log_size):
        oky = np.array([M.mv_ok(vy, 8*d, log_size, nv) for d in offs])
        for vx in range(0, nh + 1, 1 << log_size):
            okx = np.array([M.mv_ok(vx, 8*d, log_size, nh) for d in offs])
            keys = []
            for slot, ref in enumerate(refs):
                dist = M.fullpel_sads(srcs[0], pic_w, pic_h, ref[0], vx, vy, log_size, rng)
                if chroma:
                    for pl in (1, 2):
                        dist = dist + (fullpel_chroma_sads(srcs[pl], pic_w, pic_h, ref[pl], vx, vy, log_size, rng,
                                                           cdec) >> 2)
                for iy, ix in zip(*np.nonzero(oky[:, None] & okx[None, :])):
                    mvx, mvy = 8*int(offs[ix]), 8*int(offs[iy])
                    l1 = abs(mvx) + abs(mvy)
                    keys.append((8*int(dist[iy, ix]) + lam*l1, l1, slot, mvy, mvx))
            best = min(keys)

            def key2(slot, mvx, mvy):
                d = total(cand_dist(srcs, pic_w, pic_h, refs[slot], vx, vy, log_size, mvx, mvy, cdec, metric, chroma))
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


def search(src, csrc, pic_w, pic_h, refs, crefs, log_size, rng, res, lam, lam_subpel, flags, cdec):
    """src [F][..], csrc [2F][..] (all Cb, then all Cr), refs / crefs: per slot [F][H][W] / [2F][H >> cdec][W >> cdec].
    (grid [F][nv + 1][nh + 1], cost)."""
    nf = src.shape[0]
    out = [search_picture((src[f], csrc[f], csrc[nf + f]), pic_w, pic_h,
                          [(r[f], c[f], c[nf + f]) for r, c in zip(refs, crefs)], log_size, rng, res, lam,
                          lam_subpel, flags, cdec) for f in range(nf)]
    return np.stack([g for g, _ in out]), np.stack([c for _, c in out])


def load_golden(path):
    """tests/golden/me_cost.npz as a dict: planes and pictures per cdec, cases, sad, satd."""
    with np.load(path) as z:
        return {k: z[k] for k in z.files}


def golden_planes(g, cdec):
    """((Y, Cb, Cr) pictures, (Y, Cb, Cr) coded-size planes) of a chroma format."""
    tag = "444" if cdec == 0 else "420"
    return ((g["src_y"], g["src_cb_" + tag], g["src_cr_" + tag]),
            (g["ref_y"], g["ref_cb_" + tag], g["ref_cr_" + tag]))


def golden_classes(g):
    """Which classes of clipped size the recorded cases hold: a dict of counts (the golden tool and
    tests/test_me_cost_ref.py assert each is nonzero)."""
    n = dict(whole={}, luma_square={}, nonsquare=0, empty=0, chroma4x4=0, chroma_narrow=0)
    for cdec, pic, vx, vy, lg, mvx, mvy in g["cases"].tolist():
        pw, ph = g["pics"][pic].tolist()
        blk = 8 << lg
        c = plane_clip(vx, vy, lg, 0, pw, ph)
        if c is None:
            n["empty"] += 1
            continue
        w, h = c[1] - c[0], c[3] - c[2]
        if w == h == blk:
            n["whole"][blk] = n["whole"].get(blk, 0) + 1
        elif w == h:
            n["luma_square"][w] = n["luma_square"].get(w, 0) + 1
        else:
            n["nonsquare"] += 1
        cc = plane_clip(vx, vy, lg, cdec, pw, ph)
        if cdec == 1 and lg == 0 and cc is not None:
            cw, ch = cc[1] - cc[0], cc[3] - cc[2]
            n["chroma4x4"] += cw == ch == 4
            n["chroma_narrow"] += cw < 4
    return n


def assert_classes(n):
    assert set(n["whole"]) == {8, 16, 32, 64}, n
    assert set(n["luma_square"]) >= {4, 8, 16, 32}, n
    assert n["nonsquare"] and n["empty"] and n["chroma4x4"] and n["chroma_narrow"], n
