"""The motion search at variable block sizes in numpy: the CPU yardstick of odhip_me_search_vbs (me_kernels.hip), built on
_me_hier_ref, _me_cost_ref, _me_ref, _mc_ref and _mc_patterns.  include/daala_hip.h has the definition; in short:

  legality  a component is legal for the point at v when a leaf of 1 << log_max steps at the origin of every cell of that
            size inside the frame whose closed extent holds v keeps its window inside the border (mv_ok_cells);
  1.  per size lg = log_min .. log_max the uniform coarse-to-fine search (G_lg, C_lg) under that legality;
  2.  P_lg = the overlapped-block prediction of G_lg (_mc_ref.mc_predict_plane);
  3.  d_lg = the SAD of P_lg against the picture per 8x8 cell, clipped to the picture;
  4.  a cell of size lg > log_min splits iff 8 D_{lg-1} + penalty < 8 D_lg;
  5.  valid = _mc_patterns.build(centres: above log_max always, else the decision; every edge the rule allows);
  6.  a valid point takes its record from G_s, s the smallest leaf of the pattern with the point among its corners.

_me_hier_ref.search_picture has the uniform search but its legality predicate is fixed, so the search is restated here
with the predicate as a parameter; with _me_ref.mv_ok it is that search (tests/test_me_vbs_ref.py holds it to it)."""
import numpy as np

import _mc_ref as R
import _mc_patterns as P
import _me_ref as M
import _me_cost_ref as C
import _me_hier_ref as HR


def mv_ok_cells(v, mv, lg_top, n):
    """One axis of the legality predicate of a grid whose largest leaves have 1 << lg_top steps."""
    size = 1 << lg_top
    cells = [v & ~(size - 1)]
    if v % size == 0:
        cells.append(v - size)
    return all(M.window_ok(c, mv, lg_top, 0, n) and M.window_ok(c, mv, lg_top, 1, n) for c in cells if 0 <= c < n)


def search_picture(srcs, pic_w, pic_h, refs, log_size, rng, res, lam, lam_subpel, flags, cdec, levels, refine, ok):
    """_me_hier_ref.search_picture under the axis predicate ok(v, mv, n)."""
    coded_h, coded_w = refs[0][0].shape
    nh, nv = coded_w >> 3, coded_h >> 3
    chroma = bool(flags & C.CHROMA)
    metric = C.SATD_METRIC if flags & C.SATD else C.SAD_METRIC
    src_pyr = HR.pyramid(srcs[0][:pic_h, :pic_w], levels)
    ref_pyr = [HR.pyramid(r[0], levels) for r in refs]
    grid = np.zeros((nv + 1, nh + 1), R.MV_POINT)
    cost = np.zeros((nv + 1, nh + 1), np.uint32)

    def keys_of(dist, scale, lam_, slot, vx, vy, c, step, rad):
        offs = range(-rad, rad + 1)
        okx = [ok(vx, c[0] + step*d, nh) for d in offs]
        oky = [ok(vy, c[1] + step*d, nv) for d in offs]
        out = []
        for iy, dy in enumerate(offs):
            for ix, dx in enumerate(offs):
                if okx[ix] and oky[iy]:
                    mvx, mvy = c[0] + step*dx, c[1] + step*dy
                    l1 = abs(mvx) + abs(mvy)
                    out.append((8*(int(dist[iy, ix]) << scale) + lam_*l1, l1, slot, mvy, mvx))
        return out

    for vy in range(0, nv + 1, 1 << log_size):
        for vx in range(0, nh + 1, 1 << log_size):
            keys = []
            for slot, ref in enumerate(refs):
                c = (0, 0)
                for j in range(levels, 0, -1):
                    rad, step = (rng if j == levels else refine), 8 << j
                    d = HR.level_sads(src_pyr[j], pic_w, pic_h, ref_pyr[slot][j], vx, vy, log_size, j, c[0]//step,
                                     c[1]//step, rad)
                    best = min(keys_of(d, 2*j, lam, slot, vx, vy, c, step, rad))
                    c = (best[4], best[3])
                rad = refine if levels else rng
                dist = HR.level_sads(srcs[0], pic_w, pic_h, ref[0], vx, vy, log_size, 0, c[0] >> 3, c[1] >> 3, rad)
                if chroma:
                    for pl in (1, 2):
                        dist = dist + (HR.chroma_sads(srcs[pl], pic_w, pic_h, ref[pl], vx, vy, log_size, c[0] >> 3,
                                                     c[1] >> 3, rad, cdec) >> 2)
                keys += keys_of(dist, 0, lam, slot, vx, vy, c, 8, rad)
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
                        if (dx or dy) and ok(vx, mvx, nh) and ok(vy, mvy, nv):
                            best = min(best, key2(slot, mvx, mvy))
                step >>= 1
            grid[vy, vx] = (best[4], best[3], 1, best[2], 0)
            cost[vy, vx] = best[0]
    return grid, cost


def uniform(src, csrc, pic_w, pic_h, refs, crefs, lg, log_max, rng, res, lam, lam_subpel, flags, cdec, levels, refine):
    """Step 1 at one size: (G_lg [F][nv + 1][nh + 1], C_lg), levels cut to lg + 1, legality of cells of log_max."""
    nf = src.shape[0]
    if csrc is None:
        csrc, crefs = [None]*(2*nf), [[None]*(2*nf) for _ in refs]

    def ok(v, mv, n):
        return mv_ok_cells(v, mv, log_max, n)

    out = [search_picture((src[f], csrc[f], csrc[nf + f]), pic_w, pic_h,
                          [(r[f], c[f], c[nf + f]) for r, c in zip(refs, crefs)], lg, rng, res, lam, lam_subpel, flags,
                          cdec, min(levels, lg + 1), refine, ok) for f in range(nf)]
    return np.stack([g for g, _ in out]), np.stack([c for _, c in out])


def predict(refs, grid):
    """Step 2: [F][coded_h][coded_w] luma predictions of grid [F][..]."""
    return np.stack([R.mc_predict_plane([r[f] for r in refs], grid[f], 0, 0) for f in range(grid.shape[0])])


def cell_dist(src, pic_w, pic_h, pred):
    """Step 3: [F][coded_h/8][coded_w/8], the SAD per 8x8 cell over the part of it inside the picture."""
    nf, h, w = pred.shape
    diff = np.zeros((nf, h, w), np.int64)
    diff[:, :pic_h, :pic_w] = np.abs(pred[:, :pic_h, :pic_w].astype(np.int64) - src[:, :pic_h, :pic_w])
    return diff.reshape(nf, h//8, 8, w//8, 8).sum(axis=(2, 4))


def cell_sum(d, lg, x, y):
    """D of the cell of 1 << lg steps at grid origin (x, y)."""
    return int(d[y:y + (1 << lg), x:x + (1 << lg)].sum())


def splits(d, log_min, log_max, penalty, lg, x, y):
    """Step 4's comparison for the cell of size lg at origin (x, y) of one picture; d = {lg: [nv][nh]}."""
    if lg > log_max:
        return True
    if lg <= log_min:
        return False
    return 8*cell_sum(d[lg - 1], lg, x, y) + penalty < 8*cell_sum(d[lg], lg, x, y)


def pattern(d, coded_w, coded_h, log_min, log_max, penalty):
    """Step 5 for one picture."""
    def want_centre(lg, x, y):
        half = 1 << lg >> 1
        return splits(d, log_min, log_max, penalty, lg, x - half, y - half)

    return P.build(coded_w, coded_h, want_centre, lambda lg, x, y: True)


def closed_form_valid(split, coded_w, coded_h):
    """The pattern of _mc_patterns.build(centres: split(lg, x, y) of the cell at origin (x, y); every edge) without a
    pass per size or an order, as the library's kernel computes it (me_vbs.cuh): S_3(c) = split(c); S_lg(c) = split(c)
    and S_lg+1 of c's parent and of the two cells of the parent's size across c's two outer edges of the parent, a cell
    outside the frame counting as split; an edge midpoint is valid iff S_lg of both cells that share the edge."""
    nh, nv = coded_w >> 3, coded_h >> 3

    def centre(lg, x, y):                       # of the cell of size lg that holds the 8x8 cell (x, y)
        if not (0 <= x < nh and 0 <= y < nv):
            return True
        m = (1 << lg) - 1
        if not split(lg, x & ~m, y & ~m):
            return False
        if lg == 3:
            return True
        size = 2 << lg
        px, py = x & ~(size - 1), y & ~(size - 1)
        nx = px + size if x & (1 << lg) else px - 1
        ny = py + size if y & (1 << lg) else py - 1
        return centre(lg + 1, x, y) and centre(lg + 1, nx, y) and centre(lg + 1, x, ny)

    valid = np.zeros((nv + 1, nh + 1), np.uint8)
    for y in range(nv + 1):
        for x in range(nh + 1):
            tz = min(3, ((x | y | 8) & -(x | y | 8)).bit_length() - 1)
            if tz == 3:
                valid[y, x] = 1
                continue
            lg, ox, oy = tz + 1, x >> tz & 1, y >> tz & 1
            if ox and oy:
                valid[y, x] = centre(lg, x, y)
            elif ox:
                valid[y, x] = centre(lg, x, y - 1) and centre(lg, x, y)
            else:
                valid[y, x] = centre(lg, x - 1, y) and centre(lg, x, y)
    return valid


def point_sizes(valid):
    """Step 6: {(x, y): s} of the points that are an own corner of a leaf."""
    out = {}
    for vx, vy, lg, _, _ in R.leaves(valid):
        for k in range(4):
            pt = (vx + (R.CORNER_DX[k] << lg), vy + (R.CORNER_DY[k] << lg))
            out[pt] = min(out.get(pt, 4), lg)
    return out


def compose(uni, dist, coded_w, coded_h, log_min, log_max, penalty):
    """Steps 4 to 6 from the uniform searches uni = {lg: (G, C)} and the d arrays dist = {lg: [F][nv][nh]}:
    (grid, cost, [the leaves of every picture])."""
    nf = uni[log_max][0].shape[0]
    grid = np.zeros_like(uni[log_max][0])
    cost = np.zeros_like(uni[log_max][1])
    leaves = []
    for f in range(nf):
        valid = pattern({lg: dist[lg][f] for lg in dist}, coded_w, coded_h, log_min, log_max, penalty)
        sizes = point_sizes(valid)
        for y, x in zip(*np.nonzero(valid)):
            s = sizes[int(x), int(y)]          # (a valid point that no leaf has as a corner would be a KeyError)
            assert log_min <= s <= log_max and uni[s][0][f, y, x]["valid"]
            grid[f, y, x] = uni[s][0][f, y, x]
            cost[f, y, x] = uni[s][1][f, y, x]
        leaves.append(R.leaves(valid))
    return grid, cost, leaves


def search(src, csrc, pic_w, pic_h, refs, crefs, log_min, log_max, rng, res, lam, lam_subpel, flags, cdec, levels,
           refine, penalty, uni=None):
    """The whole call: dict(grid, cost, cell_dist [nsizes][F][nv][nh], leaves, uni).  `uni`, a dict {lg: (G, C)}, holds
    uniform searches of this content and log_max that are already known; what is missing is added to it."""
    coded_h, coded_w = refs[0].shape[1:]
    uni = {} if uni is None else uni
    dist = {}
    for lg in range(log_min, log_max + 1):
        if lg not in uni:
            uni[lg] = uniform(src, csrc, pic_w, pic_h, refs, crefs, lg, log_max, rng, res, lam, lam_subpel, flags, cdec,
                              levels, refine)
        if log_min < log_max:
            dist[lg] = cell_dist(src, pic_w, pic_h, predict(refs, uni[lg][0]))
    if log_min == log_max:
        return dict(grid=uni[log_max][0], cost=uni[log_max][1], cell_dist=None, uni=uni,
                    leaves=[R.leaves(g["valid"]) for g in uni[log_max][0]])
    grid, cost, leaves = compose(uni, dist, coded_w, coded_h, log_min, log_max, penalty)
    return dict(grid=grid, cost=cost, cell_dist=np.stack([dist[lg] for lg in sorted(dist)]).astype(np.uint32),
                leaves=leaves, uni=uni)


def check_grid(grid, dec, nrefs):
    """odhip_mc_check_grid of one picture's grid in numpy: every leaf's corners (_mc_ref.vertex) are points of the
    grid in a slot that exists, and no window leaves the border."""
    nv, nh = grid.shape[0] - 1, grid.shape[1] - 1
    for vx, vy, lg, oc, s in R.leaves(grid["valid"]):
        for k in range(4):
            dx, dy = R.vertex(oc, s, k)
            x, y = vx + (dx << lg), vy + (dy << lg)
            if not (0 <= x <= nh and 0 <= y <= nv) or grid["ref"][y, x] >= nrefs:
                return False
            if not (M.window_ok(vx, int(grid["mvx"][y, x]), lg, dec, nh)
                    and M.window_ok(vy, int(grid["mvy"][y, x]), lg, dec, nv)):
                return False
    return True


# ---- content for the tests ----
W, H, PW, PH, F = 128, 64, 120, 56, 2
PATCHES = ((0, 40, 20, 30, 24, 5, -4), (1, 66, 14, 36, 30, -6, 3))
SHIFTS = ((2, -1), (-3, 2), (1, 3))


def scene(nslots=2, seed=4, patches=PATCHES, w=W, h=H, pw=PW, ph=PH):
    """(src [2][ph][pw], csrc [4][ph/2][pw/2], refs: nslots x [2][h][w], crefs: nslots x [4][h/2][w/2]), 4:2:0, coded
    w x h, pictures pw x ph.
    Luma: a smooth scene; slot k is the scene moved by SHIFTS[k] pixels; the pictures are the scene itself but for the
    patches, (picture, x, y, w, h, dx, dy), which show the scene moved by another (dx, dy) - a patch displaced
    differently from its background, which every block size matches but for the picture's edges.  Chroma: two more
    scenes, moved by half the shifts rounded down, no patch.  tests/test_me_vbs_ref.py asserts that seed and patches
    give leaves of all four sizes and a split and an unsplit cell at every size."""
    rng = np.random.RandomState(seed)
    big = [M.smooth_noise(rng, h + 64, w + 64) for _ in range(3)]

    def cut(pl, dx, dy):
        d = 1 if pl else 0
        return big[pl][32 + dy:32 + dy + (h >> d), 32 + dx:32 + dx + (w >> d)]

    src = np.stack([cut(0, 0, 0), cut(0, 0, 0)]).copy()
    for pic, x, y, pw_, ph_, dx, dy in patches:
        src[pic, y:y + ph_, x:x + pw_] = cut(0, dx, dy)[y:y + ph_, x:x + pw_]
    csrc = np.stack([cut(1, 0, 0)]*2 + [cut(2, 0, 0)]*2)[:, :(ph + 1) >> 1, :(pw + 1) >> 1]
    refs = [np.ascontiguousarray(np.stack([cut(0, dx, dy)]*2)) for dx, dy in SHIFTS[:nslots]]
    crefs = [np.ascontiguousarray(np.stack([cut(1, dx >> 1, dy >> 1)]*2 + [cut(2, dx >> 1, dy >> 1)]*2))
             for dx, dy in SHIFTS[:nslots]]
    return np.ascontiguousarray(src[:, :ph, :pw]), np.ascontiguousarray(csrc), refs, crefs


def border_scene(seed=9, edge="left", w=None, h=None, pw=None, ph=None):
    """(src [1][ph][pw], refs: one slot [1][h][w]); by default coded 128 x 64 for the edges "left" and "right", 64 wide
    x 128 tall for "top" and "bottom", and a picture of the coded size.
    "left": every row of the picture is flat at the value the reference has in its first two columns (two, so that the
    halved plane's border has it too), at most 100, and the rest of the reference is at least 156 - so the more of a
    block lies in the replicated border left of the frame, the better it matches.  The 8x8 block of the point at
    x = 64 lies there whole from -68 pixels on, which a leaf of 8 pixels may take and a leaf of 64 pixels at the
    frame's left edge, whose corner that point is, may not (its window would start before -64).
    "right" is that scene mirrored, "top" its transpose and "bottom" the transpose of "right": the border that matches
    lies beyond that edge, and the point is the one in the middle of that axis."""
    tall = edge in ("top", "bottom")
    w = (H if tall else W) if w is None else w
    h = (W if tall else H) if h is None else h
    rows, cols = (w, h) if tall else (h, w)    # of the "left" scene this one is made from
    rng = np.random.RandomState(seed)
    ref = (156 + rng.randint(0, 100, size=(rows, cols))).astype(np.uint8)
    ref[:, :2] = (M.smooth_noise(rng, rows, 8)[:, :1].astype(int)*100//255).astype(np.uint8)
    src = np.repeat(ref[:, :1], cols, axis=1)
    if edge in ("right", "bottom"):
        src, ref = src[:, ::-1], ref[:, ::-1]
    else:
        assert edge in ("left", "top"), edge
    if tall:
        src, ref = src.T, ref.T
    src = src[:h if ph is None else ph, :w if pw is None else pw]
    return np.ascontiguousarray(src)[None], [np.ascontiguousarray(ref)[None]]
