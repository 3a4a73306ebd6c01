"""`valid` patterns of motion-vector grids that follow the reference's rule for its grid, built so that together they
hold every kind of leaf (log size, outside corner, split flags) the walk of mc_walk.cuh can meet, and the largest
legal vector component of a leaf: the one that puts its filter window exactly on the 64-sample border.

The rule, with points every 8 luma pixels and cells of 64, 32 and 16 pixels (lg = 3, 2, 1):
  A.  points at multiples of 8 grid steps are valid;
  B.  a cell's centre may be valid only if the cell's four corners are;
  C.  an edge midpoint may be valid only if both ends of the edge are valid and every cell inside the frame that
      shares the edge is split (its centre is valid).
Every point of a grid has exactly one of these roles.  build() walks the sizes from 64 down, asks a callback at every
point the rule allows, and so can only make patterns that keep it; rule_violations() checks any pattern.

Everything here is deterministic: the random patterns draw from numpy's RandomState with fixed seeds."""
import numpy as np

import _mc_ref as R


def build(w, h, want_centre, want_edge):
    """valid [h/8 + 1][w/8 + 1] of a coded w x h frame.  want_centre(lg, x, y) / want_edge(lg, x, y) decide the centre /
    the edge midpoint at grid point (x, y) of a cell of 1 << lg grid steps; they are asked only where the rule allows
    the point, in a fixed order."""
    nh, nv = w >> 3, h >> 3
    valid = np.zeros((nv + 1, nh + 1), np.uint8)
    valid[::8, ::8] = 1
    for lg in (3, 2, 1):
        size, half = 1 << lg, 1 << lg >> 1

        def split(x, y):
            return not (0 <= x < nh and 0 <= y < nv) or valid[y + half, x + half]

        for y in range(0, nv, size):
            for x in range(0, nh, size):
                if (valid[y, x] and valid[y, x + size] and valid[y + size, x] and valid[y + size, x + size]
                        and want_centre(lg, x + half, y + half)):
                    valid[y + half, x + half] = 1
        for y in range(0, nv + 1, size):           # edges along x, between the cells above and below
            for x in range(0, nh, size):
                if (valid[y, x] and valid[y, x + size] and split(x, y - size) and split(x, y)
                        and want_edge(lg, x + half, y)):
                    valid[y, x + half] = 1
        for y in range(0, nv, size):               # edges along y, between the cells left and right
            for x in range(0, nh + 1, size):
                if (valid[y, x] and valid[y + size, x] and split(x - size, y) and split(x, y)
                        and want_edge(lg, x, y + half)):
                    valid[y + half, x] = 1
    return valid


def rule_violations(valid):
    """[(rule, lg, x, y)] of the points of a pattern that break rule A, B or C."""
    nv, nh = valid.shape[0] - 1, valid.shape[1] - 1
    bad = [("A", 3, x, y) for y in range(0, nv + 1, 8) for x in range(0, nh + 1, 8) if not valid[y, x]]
    for lg in (3, 2, 1):
        size, half = 1 << lg, 1 << lg >> 1

        def split(x, y):
            return not (0 <= x < nh and 0 <= y < nv) or valid[y + half, x + half]

        for y in range(0, nv, size):
            for x in range(0, nh, size):
                if valid[y + half, x + half] and not (valid[y, x] and valid[y, x + size] and valid[y + size, x]
                                                      and valid[y + size, x + size]):
                    bad.append(("B", lg, x + half, y + half))
        for y in range(0, nv + 1, size):
            for x in range(0, nh, size):
                if valid[y, x + half] and not (valid[y, x] and valid[y, x + size] and split(x, y - size)
                                               and split(x, y)):
                    bad.append(("C", lg, x + half, y))
        for y in range(0, nv, size):
            for x in range(0, nh + 1, size):
                if valid[y + half, x] and not (valid[y, x] and valid[y + size, x] and split(x - size, y)
                                               and split(x, y)):
                    bad.append(("C", lg, x, y + half))
    return bad


def unread_points(valid):
    """[(leaf, corner)] whose grid point (_mc_ref.vertex) lies outside the grid or is not valid."""
    nv, nh = valid.shape[0] - 1, valid.shape[1] - 1
    bad = []
    for vx, vy, lg, oc, s in R.leaves(valid):
        for k in range(4):
            dx, dy = R.vertex(oc, s, k)
            x, y = vx + (dx << lg), vy + (dy << lg)
            if not (0 <= x <= nh and 0 <= y <= nv and valid[y, x]):
                bad.append(((vx, vy, lg, oc, s), k))
    return bad


def kinds(valid):
    """The kinds of leaf of a pattern: (lg, oc, s), a 64 x 64 leaf being (3, 0, 3)."""
    return {(lg, oc, s) for _, _, lg, oc, s in R.leaves(valid)}


ALL_KINDS = {(lg, oc, s) for lg in range(3) for oc in range(4) for s in range(4)} | {(3, 0, 3)}


def random_pattern(w, h, seed, p_split, p_edge):
    """Centres valid with probability p_split[3 - lg], edge midpoints with p_edge[3 - lg], wherever the rule allows."""
    rng = np.random.RandomState(seed)
    return build(w, h, lambda lg, x, y: rng.rand() < p_split[3 - lg], lambda lg, x, y: rng.rand() < p_edge[3 - lg])


def quadrant_pattern():
    """128 x 128, directed: every 32 x 32 kind.  All four 64 x 64 cells are split and none of their quadrants is; a
    quadrant's split flags are two of its cell's four edge midpoints, and the cells' midpoints (top, right, bottom,
    left) are 1111, 0101 / 1010, 0000 - which the shared edges allow and which give each outside corner all four flag
    pairs."""
    edges = {(4, 0), (0, 4), (4, 8), (8, 4),            # the upper left cell: all four
             (16, 4),                                   # the upper right cell: right (and left, shared)
             (4, 16)}                                   # the lower left cell: bottom (and top, shared)
    return build(128, 128, lambda lg, x, y: lg == 3, lambda lg, x, y: lg == 3 and (x, y) in edges)


def border_pattern():
    """128 x 128, for windows on the border: the upper left and the lower right 64 x 64 cell are leaves, the other two
    are split at random (seed picked by a search), and leaves of all four sizes lie along each of the four sides -
    which tests/test_mc_patterns_host.py asserts."""
    rng = np.random.RandomState(2)
    return build(128, 128, lambda lg, x, y: (x, y) in ((12, 4), (4, 12)) if lg == 3 else rng.rand() < 0.7,
                 lambda lg, x, y: rng.rand() < 0.7)


def side_sizes(valid):
    """{(axis, side): the log sizes of the leaves along that side of the frame}."""
    nv, nh = valid.shape[0] - 1, valid.shape[1] - 1
    out = {(axis, side): set() for axis in (0, 1) for side in (0, 1)}
    for vx, vy, lg, oc, s in R.leaves(valid):
        for axis, v, n in ((0, vx, nh), (1, vy, nv)):
            if v == 0:
                out[axis, 0].add(lg)
            if v + (1 << lg) == n:
                out[axis, 1].add(lg)
    return out


def uniform_pattern(w, h, lg):
    """Every leaf of 1 << lg grid steps: the pattern of a motion search's grid."""
    return build(w, h, lambda l, x, y: l > lg, lambda l, x, y: l > lg)


# (name, coded w, coded h, the pattern).  The random ones were picked by a search over seeds for the kinds the directed
# one lacks; tests/test_mc_patterns_host.py asserts that together they hold ALL_KINDS.
PATTERN_SPECS = (
    ("quadrants", 128, 128, quadrant_pattern),
    ("random_192x128", 192, 128, lambda: random_pattern(192, 128, 36, (0.9, 0.9, 0.8), (0.8, 0.7, 0.5))),
    ("random_128x128", 128, 128, lambda: random_pattern(128, 128, 2, (1, 0.7, 0.5), (0.6, 0.6, 0.5))),
)


def patterns():
    """[(name, w, h, valid)]"""
    return [(name, w, h, fn()) for name, w, h, fn in PATTERN_SPECS]


def axis_extreme(v, lg, dec, n, side):
    """The largest legal component (1/8 luma pel) towards `side` (0: negative, 1: positive) of a leaf of 1 << lg grid
    steps at grid position v on an axis of n grid steps, at a plane's decimation: the leaf's (blk + 5)-sample filter
    window then has its first sample at -pad (side 0) or ends at the plane's size + pad (side 1).  One more step -
    an eighth-pel at dec = 0, the next component that changes scale_mv(.) >> 3 at dec = 1 - is outside."""
    pad, blk, base = R.BORDER >> dec, 8 << lg >> dec, v << 3 >> dec
    if side == 0:
        lim = -pad + 2 - base                       # the least scale_mv(mv) >> 3
        mv = 8*lim << dec
        while R.scale_mv(mv - 1, dec) >> 3 >= lim:
            mv -= 1
    else:
        lim = (n << 3 >> dec) + pad - blk - 3 - base
        mv = (8*lim + 7) << dec
        while R.scale_mv(mv + 1, dec) >> 3 <= lim:
            mv += 1
    return mv


def window_start(v, mv, dec):
    """First sample of the filter window of a leaf at grid position v under the component mv, on one axis."""
    return (v << 3 >> dec) + (R.scale_mv(mv, dec) >> 3) - 2


def readers(valid):
    """{(x, y): [(vx, vy, lg)]}: the leaves that read each grid point."""
    out = {}
    for vx, vy, lg, oc, s in R.leaves(valid):
        for k in range(4):
            dx, dy = R.vertex(oc, s, k)
            out.setdefault((vx + (dx << lg), vy + (dy << lg)), []).append((vx, vy, lg))
    return out


def push_to_side(grid, dec, axis, side):
    """Gives every point that a leaf along one side of the frame reads (axis 0: x, side 0: the left / top) the
    component that is extreme for the most confined leaf reading it.  Returns {lg: the points (x, y) at which a leaf
    of that size along the side has a window exactly on the border}."""
    valid = grid["valid"]
    nv, nh = valid.shape[0] - 1, valid.shape[1] - 1
    n, name = (nh, "mvx") if axis == 0 else (nv, "mvy")
    read = readers(valid)

    def on_side(leaf):
        v = leaf[axis]
        return v == 0 if side == 0 else v + (1 << leaf[2]) == n

    for (x, y), by in read.items():
        if any(on_side(leaf) for leaf in by):
            ext = [axis_extreme(leaf[axis], leaf[2], dec, n, side) for leaf in by]
            grid[name][y, x] = max(ext) if side == 0 else min(ext)
    pad, size = R.BORDER >> dec, n << 3 >> dec
    hits = {}
    for (x, y), by in read.items():
        for leaf in by:
            x0 = window_start(leaf[axis], int(grid[name][y, x]), dec)
            blk = 8 << leaf[2] >> dec
            if on_side(leaf) and (x0 == -pad if side == 0 else x0 + blk + 5 == size + pad):
                hits.setdefault(leaf[2], []).append((x, y))
    return hits
