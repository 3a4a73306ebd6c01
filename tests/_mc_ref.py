"""Motion compensation from a motion-vector grid in numpy: the CPU yardstick of mc_kernels.hip.

A restatement in our own words of what the reference does in od_state_mc_predict (the walk of the grid's
quadtree, src/state.c:627-722, 932-959), od_mc_predict1fmv8/16_c (src/mc.c:94-340) and the two bilinear blends
(src/mc.c:352-404, 1056-1200).  tests/test_mc_host.py pins it to recorded outputs of od_state_mc_predict
(tests/golden/mc.npz) and, where the compiled reference is present, to its leaf functions.

Grids are structured arrays (MV_POINT) of shape [nv + 1][nh + 1], nh = coded_w/8; reference planes are unpadded
coded-size planes, read with clamped coordinates."""
import numpy as np

MV_POINT = np.dtype([("mvx", "<i4"), ("mvy", "<i4"), ("valid", "u1"), ("ref", "u1"), ("reserved", "<u2")])
LOG_MVB_MAX = 3
BORDER = 64
TAPS = np.array([[0, 0, 128, 0, 0, 0], [1, -9, 122, 18, -5, 1], [3, -15, 112, 37, -11, 2],
                 [3, -18, 97, 58, -15, 3], [4, -20, 80, 80, -20, 4], [3, -15, 58, 97, -18, 3],
                 [2, -11, 37, 112, -15, 3], [1, -5, 18, 122, -9, 1]], np.int64)
CORNER_DX = (0, 1, 1, 0)        # clockwise from the upper left
CORNER_DY = (0, 0, 1, 1)


def leaf_desc(vx, vy, lg, oc, s):
    return vx | vy << 12 | lg << 24 | oc << 26 | s << 28


def vertex(oc, s, k):
    """Grid point of corner k, in leaf sizes from the leaf's upper left: the block's own corner, moved one step
    further from the outside corner when the neighbour across that edge is not split."""
    x, y = CORNER_DX[k], CORNER_DY[k]
    for bit, n in ((1, (oc + 1) & 3), (2, (oc + 3) & 3)):
        if not s & bit and k == n:
            x += CORNER_DX[k] - CORNER_DX[oc]
            y += CORNER_DY[k] - CORNER_DY[oc]
    return x, y


def leaves(valid):
    """[(vx, vy, lg, oc, s)] of a grid's `valid` flags ([nv + 1][nh + 1]), by recursion from the 64x64 cells."""
    nv, nh = valid.shape[0] - 1, valid.shape[1] - 1
    out = []

    def walk(vx, vy, lg):
        half = 1 << lg >> 1
        if lg > 0 and valid[vy + half, vx + half]:
            for dy in (0, half):
                for dx in (0, half):
                    walk(vx + dx, vy + dy, lg - 1)
            return
        oc, s = 0, 3
        if lg < LOG_MVB_MAX:
            m = (2 << lg) - 1
            oc = int(vx & m != 0)
            if vy & m:
                oc = 3 - oc
            k1, k3 = (oc + 1) & 3, (oc + 3) & 3
            s = int(bool(valid[vy + (CORNER_DY[k1] << lg), vx + (CORNER_DX[k1] << lg)])) \
                | int(bool(valid[vy + (CORNER_DY[k3] << lg), vx + (CORNER_DX[k3] << lg)])) << 1
        out.append((vx, vy, lg, oc, s))

    for vy in range(0, nv, 1 << LOG_MVB_MAX):
        for vx in range(0, nh, 1 << LOG_MVB_MAX):
            walk(vx, vy, LOG_MVB_MAX)
    return out


def scale_mv(v, dec):
    """v / 2**dec, ties to even."""
    return (v + (((1 << dec) + (v >> dec & 1) - 1) >> 1)) >> dec


def window(plane, x0, y0, w, h):
    """plane[y0 : y0 + h, x0 : x0 + w] with coordinates clamped to the plane."""
    ys = np.clip(np.arange(y0, y0 + h), 0, plane.shape[0] - 1)
    xs = np.clip(np.arange(x0, x0 + w), 0, plane.shape[1] - 1)
    return plane[np.ix_(ys, xs)].astype(np.int64)


def predict1_window(win, fx, fy, fpr):
    """One vector's prediction from its (blk + 5)^2 source window (rows / columns -2 .. blk + 2) and the
    vector's eighth-pel phases.  8-bit: first pass kept in int16; full precision (int16 at 12 bits): int32."""
    n = win.shape[0] - 5
    if fx == 0 and fy == 0:
        return win[2:2 + n, 2:2 + n].copy()
    mid_c = 128 << 4 if fpr else 128
    if fx:
        mid = sum(win[:, t:t + n]*TAPS[fx, t] for t in range(6)) - (mid_c << 7)
    else:
        mid = (win[:, 2:2 + n] - mid_c)*128
    mid = mid.astype(np.int32 if fpr else np.int16).astype(np.int64)
    if fy:
        v = (sum(mid[t:t + n]*TAPS[fy, t] for t in range(6)) + (1 << 13)) >> 14
    else:
        v = (mid[2:2 + n] + 64) >> 7
    return np.clip(v + mid_c, 0, 4095 if fpr else 255)


def predict1(plane, bx, by, mvx, mvy, blk, fpr):
    win = window(plane, bx + (mvx >> 3) - 2, by + (mvy >> 3) - 2, blk + 5, blk + 5)
    return predict1_window(win, mvx & 7, mvy & 7, fpr)


def blend(pred, oc, s, lb):
    """The four corner predictions of a 2**lb block, bilinearly weighted."""
    n = 1 << lb
    j, i = np.mgrid[0:n, 0:n].astype(np.int64)
    p = [q.astype(np.int64) for q in pred]
    if s == 3:
        a = (p[0] << lb) + (p[1] - p[0])*i
        b = (p[3] << lb) + (p[2] - p[3])*i
        return ((a << lb) + (b - a)*j + (1 << (2*lb - 1))) >> 2*lb
    w = split_weights(oc, s, lb, i, j)
    return ((p[0] << (2*lb + 1)) + (p[1] - p[0])*w[1] + (p[2] - p[0])*w[2] + (p[3] - p[0])*w[3]
            + (1 << 2*lb)) >> (2*lb + 1)


def split_weights(oc, s, lb, i, j):
    """Weights (times 2 << 2*lb) of the four corners where a neighbour leaf is larger: the corner on the far
    side of an unsplit edge gives half its weight to the outside corner."""
    c0 = [2 << 2*lb, 0, 0, 0]
    ci = [-(2 << lb), 2 << lb, 0, 0]
    cj = [-(2 << lb), 0, 0, 2 << lb]
    cij = [2, -2, 2, -2]
    for bit, n in ((1, (oc + 1) & 3), (2, (oc + 3) & 3)):
        if not s & bit:
            for c in (c0, ci, cj, cij):
                c[n] >>= 1
                c[oc] += c[n]
    return [c0[k] + cj[k]*j + (ci[k] + cij[k]*j)*i for k in range(4)]


def mc_predict_plane(refs, grid, dec, fpr):
    """refs: list of coded-size planes (one per slot) of this plane's decimation; grid: MV_POINT [nv+1][nh+1]."""
    h, w = refs[0].shape
    out = np.zeros((h, w), refs[0].dtype)
    for vx, vy, lg, oc, s in leaves(grid["valid"]):
        lb = lg + 3 - dec
        bx, by = vx << 3 >> dec, vy << 3 >> dec
        pred = []
        seen = {}
        for k in range(4):
            dx, dy = vertex(oc, s, k)
            pt = grid[vy + (dy << lg), vx + (dx << lg)]
            key = (int(pt["ref"]), scale_mv(int(pt["mvx"]), dec), scale_mv(int(pt["mvy"]), dec))
            if key not in seen:
                seen[key] = predict1(refs[key[0]], bx, by, key[1], key[2], 1 << lb, fpr)
            pred.append(seen[key])
        out[by:by + (1 << lb), bx:bx + (1 << lb)] = blend(pred, oc, s, lb)
    return out


def grid_in_range(grid, dec):
    """Does every filter window of every leaf corner stay inside the 64-sample border of the coded frame?"""
    nv, nh = grid.shape[0] - 1, grid.shape[1] - 1
    w, h, pad = nh << 3 >> dec, nv << 3 >> dec, BORDER >> dec
    for vx, vy, lg, oc, s in leaves(grid["valid"]):
        blk = 8 << lg >> dec
        for k in range(4):
            dx, dy = vertex(oc, s, k)
            pt = grid[vy + (dy << lg), vx + (dx << lg)]
            x0 = (vx << 3 >> dec) + (scale_mv(int(pt["mvx"]), dec) >> 3) - 2
            y0 = (vy << 3 >> dec) + (scale_mv(int(pt["mvy"]), dec) >> 3) - 2
            if x0 < -pad or x0 + blk + 5 > w + pad or y0 < -pad or y0 + blk + 5 > h + pad:
                return False
    return True


def load_cases(path):
    """tests/golden/mc.npz (tools/make_golden_mc.py) as a list of dicts: name, c444, fpr, coded w / h, refs[slot][pli],
    grid, pred[pli] - what od_state_mc_predict made of them."""
    z = np.load(path)
    info = {str(c): z[str(c) + "_info"] for c in z["cases"]}
    out = []
    for name in (str(n) for n in z["names"]):
        case = next(c for c in info if name.startswith(c + "_f"))
        _, _, cw, ch, c444, fpr = (int(v) for v in info[case])
        frame = str(z[name + "_refs"])
        out.append(dict(name=name, c444=c444, fpr=fpr, w=cw, h=ch, grid=z[name + "_grid"],
                        refs=[[z["%s_ref%d_%d" % (frame, s, p)] for p in range(3)] for s in range(2)],
                        pred=[z["%s_pred%d" % (name, p)] for p in range(3)]))
    return out


def random_grid(valid, rng, decs, nrefs=2, reach=62):
    """A grid on a given `valid` pattern with random slots and vectors inside the legal range."""
    g = np.zeros(valid.shape, MV_POINT)
    g["valid"] = valid
    g["ref"] = rng.randint(0, nrefs, size=valid.shape)
    g["mvx"] = rng.randint(-reach*8, reach*8 + 1, size=valid.shape)
    g["mvy"] = rng.randint(-reach*8, reach*8 + 1, size=valid.shape)
    for _ in range(200):
        if all(grid_in_range(g, dec) for dec in decs):
            return g
        for dec in decs:
            shrink_offenders(g, dec, rng)
    raise AssertionError("no legal grid found")


def shrink_offenders(grid, dec, rng):
    nv, nh = grid.shape[0] - 1, grid.shape[1] - 1
    w, h, pad = nh << 3 >> dec, nv << 3 >> dec, BORDER >> dec
    for vx, vy, lg, oc, s in leaves(grid["valid"]):
        blk = 8 << lg >> dec
        for k in range(4):
            dx, dy = vertex(oc, s, k)
            pt = grid[vy + (dy << lg), vx + (dx << lg)]
            x0 = (vx << 3 >> dec) + (scale_mv(int(pt["mvx"]), dec) >> 3) - 2
            y0 = (vy << 3 >> dec) + (scale_mv(int(pt["mvy"]), dec) >> 3) - 2
            if x0 < -pad or x0 + blk + 5 > w + pad or y0 < -pad or y0 + blk + 5 > h + pad:
                pt["mvx"] = int(pt["mvx"]*rng.uniform(0.6, 0.95))
                pt["mvy"] = int(pt["mvy"]*rng.uniform(0.6, 0.95))
