"""CPU restatement of FastSSIM as the reference's RD tool computes it (calc_ssim :445-463 of tools/dump_fastssim.c),
written from its formulas.

A plane pair of w x h samples at depth 8, 10 or 12 gives four levels.  Level 0 is the 2x2 SUM of the pair at
ceil(w/2) x ceil(h/2), a missing right or bottom neighbour replaced by the last sample; level l > 0 the 2x2 sum of
level l - 1, again at the rounded-up size, and `max` - (1 << depth) - 1 times 4 at level 0 - times 4 again.

THE TOOL'S DEFECT, NOT COPIED: for levels 1..3 the tool clamps the neighbour at w2 and h2, where w2 - 1 and h2 - 1 are
the last column and row.  A level of odd width gives it the first sample of the next row, a level of odd height one row
past the level (another plane's first row, or the bytes of an array of doubles).  This restatement, like the library,
clamps levels 1..3 the way level 0 is clamped; it equals the tool for exactly the sizes where the tool's reads stay
inside the level - levels 0, 1 and 2 even in both directions, i.e. ceil(w/2) and ceil(h/2) multiples of 8
(tool_reads_inside).  1920 x 1080 is not such a size (540 -> 270 -> 135 rows): the tool's own 1080p numbers contain
that foreign row.

Every level: gradient magnitudes g = 4*max(g1, g2) + min(g1, g2) of the two diagonal differences on the
(w - 1) x (h - 1) interior, zero outside; the three sums of gx^2, gy^2, gx*gy under the fixed 8 x 8 integer window
TABLE (total 104), which is what the tool's sliding scheme of doubling, halving and subtracting columns over an 8-row
ring buffer computes (loops_window is a literal port of those loops; tests/test_fastssim_host.py compares the two);
the term (2*mugxgy + c2)/(mugx2 + mugy2 + c2).  The sums are mathematical integers: 104*g^2 <= 104*(5*4095*256)^2 <
2^52, so int64 here and the tool's doubles agree exactly in any summation order.  At level 3 the term is multiplied by
the luminance term over 8 x 8 BOX sums with clamped coordinates, held in `unsigned` (modulo 2^32); the tool slides muy
along a row with x's column sums, so muy(j, i) = muy(j, 0) + mux(j, i) - mux(j, 0) modulo 2^32, which wraps whenever x
darkens along a row by more than muy(j, 0).

The tool adds the terms of a level into one running double in raster order (np.cumsum reproduces it), divides by
w_l*h_l and multiplies the powers FS_WEIGHTS[l] in level order, starting from 1.

The reference's Y4M reader takes 8 and 10 bits only: depth 12, and sizes outside tool_reads_inside, have this
restatement as their only yardstick.

Also: the seeded clip pairs of tests/golden/fastssim.npz and the tool's printed lines.
"""
import math
import struct

import numpy as np

import _metrics_ref as M

K1 = 0.01 * 0.01                    # SSIM_K1
K2 = 0.03 * 0.03                    # SSIM_K2
LEVELS = 4
MIN_SIZE = 16                       # level 3 of 16 x 16 is 1 x 1
WEIGHTS = (0.2989654541015625, 0.3141326904296875, 0.2473602294921875, 0.1395416259765625)

# an impulse at gradient position (y, x) lands on output rows y - 4 .. y + 3 and columns x - 3 .. x + 4
TABLE = np.array([
    [1, 2, 4, 8, 8, 4, 2, 1],
    [1, 2, 4, 8, 8, 4, 2, 1],
    [0, 1, 2, 4, 4, 2, 1, 0],
    [0, 0, 1, 2, 2, 1, 0, 0],
    [0, 0, 0, 1, 1, 0, 0, 0],
    [0, 0, 0, 1, 1, 0, 0, 0],
    [0, 0, 1, 2, 2, 1, 0, 0],
    [0, 1, 2, 4, 4, 2, 1, 0],
], np.int64)
assert int(TABLE.sum()) == 104

# every plane of every case satisfies tool_reads_inside (name, content, w, h, 4:4:4, depth, frames, seed)
CASES = [
    ("natural_420_8", "natural", 64, 32, False, 8, 2, 11),
    ("texture_420_10", "texture", 96, 64, False, 10, 2, 12),
    ("min_444_8", "noise", 16, 16, True, 8, 1, 13),             # level 3 is 1 x 1
    ("natural_444_10_odd", "natural", 31, 47, True, 10, 2, 14),  # level 0 clamps the last row and column
    ("texture_444_8", "texture", 48, 80, True, 8, 1, 15),
]


def level_size(w, h, level):
    """(w_l, h_l): the size of level `level` of a w x h plane."""
    for _ in range(level + 1):
        w, h = (w + 1) >> 1, (h + 1) >> 1
    return w, h


def tool_reads_inside(w, h):
    """True where the tool's fs_downsample_level reads stay inside the level it reads: levels 0, 1 and 2 even in both
    directions."""
    return all(v % 2 == 0 for l in range(LEVELS - 1) for v in level_size(w, h, l))


def down(a):
    """The 2x2 sums at the rounded-up size, a missing neighbour replaced by the last row / column."""
    h, w = a.shape
    j0 = 2 * np.arange((h + 1) >> 1)
    i0 = 2 * np.arange((w + 1) >> 1)
    j1 = np.minimum(j0 + 1, h - 1)
    i1 = np.minimum(i0 + 1, w - 1)
    return a[j0][:, i0] + a[j0][:, i1] + a[j1][:, i0] + a[j1][:, i1]


def pyramid(plane):
    """[level] int64 planes, level 0 the 2x2 sum of the plane."""
    out = [down(np.asarray(plane).astype(np.int64))]
    for _ in range(1, LEVELS):
        out.append(down(out[-1]))
    return out


def gradient(s):
    """int64 [h][w]: g on the (h - 1) x (w - 1) interior, zero in the last row and column."""
    g = np.zeros(s.shape, np.int64)
    g1 = np.abs(s[1:, 1:] - s[:-1, :-1])
    g2 = np.abs(s[1:, :-1] - s[:-1, 1:])
    g[:-1, :-1] = 4 * np.maximum(g1, g2) + np.minimum(g1, g2)
    return g


def window(p):
    """int64 [h][w]: out(r, c) = sum TABLE[a][b] * p(r + 4 - a, c + 3 - b), p zero outside [h][w]."""
    h, w = p.shape
    pad = np.zeros((h + 7, w + 7), np.int64)
    pad[3:3 + h, 4:4 + w] = p
    out = np.zeros((h, w), np.int64)
    for a in range(8):
        for b in range(8):
            if TABLE[a, b]:
                out += TABLE[a, b] * pad[7 - a:7 - a + h, 7 - b:7 - b + w]
    return out


def table_window(gx, gy):
    """(mugx2, mugy2, mugxgy) float64 [h][w] by the table."""
    return tuple(window(p).astype(np.float64) for p in (gx * gx, gy * gy, gx * gy))


def loops_window(gx, gy):
    """(mugx2, mugy2, mugxgy) float64 [h][w]: a literal port of fs_calc_structure's loops (:347-417) over given
    gradients (int [h][w], the last row and column ignored, as the tool never computes them).  Slow: small sizes."""
    h, w = gx.shape
    stride = w + 8
    buf = [np.zeros((8, stride), np.float64), np.zeros((8, stride), np.float64)]
    out = [np.zeros((h, w), np.float64) for _ in range(3)]
    col = np.zeros((3, 8), np.float64)

    def prod(j, joffs, i, ioffs):
        x = buf[0][(j + joffs) & 7, i + ioffs]
        y = buf[1][(j + joffs) & 7, i + ioffs]
        return np.array([x * x, y * y, x * y])

    for j in range(h + 4):
        if j < h - 1:
            for i in range(w - 1):
                buf[0][j & 7, i + 4] = float(gx[j, i])
                buf[1][j & 7, i + 4] = float(gy[j, i])
        else:
            buf[0][j & 7, :] = 0
            buf[1][j & 7, :] = 0
        if j >= 4:
            col[:, 0:4] = 0
            for i in range(4, 8):
                col[:, i] = prod(j, -1, i, 0)
                col[:, i] += prod(j, 0, i, 0)
                for k in range(1, 8 - i):
                    col[:, i] = col[:, i] * 2
                    col[:, i] += prod(j, -k - 1, i, 0)
                    col[:, i] += prod(j, k, i, 0)
            for i in range(w):
                for m in range(3):
                    s = col[m, 0]
                    for k in range(1, 8):
                        s += col[m, k]
                    out[m][j - 4, i] = s
                if i + 1 < w:
                    col[:, 0] = prod(j, -1, i, 1)
                    col[:, 0] += prod(j, 0, i, 1)
                    col[:, 2] -= prod(j, -3, i, 2)
                    col[:, 2] -= prod(j, 2, i, 2)
                    col[:, 1] = col[:, 2] * 0.5
                    col[:, 3] -= prod(j, -4, i, 3)
                    col[:, 3] -= prod(j, 3, i, 3)
                    col[:, 2] = col[:, 3] * 0.5
                    col[:, 3] = col[:, 4]
                    col[:, 4] = col[:, 5] * 2
                    col[:, 4] += prod(j, -4, i, 5)
                    col[:, 4] += prod(j, 3, i, 5)
                    col[:, 5] = col[:, 6] * 2
                    col[:, 5] += prod(j, -3, i, 6)
                    col[:, 5] += prod(j, 2, i, 6)
                    col[:, 6] = col[:, 7] * 2
                    col[:, 6] += prod(j, -2, i, 7)
                    col[:, 6] += prod(j, 1, i, 7)
                    col[:, 7] = prod(j, -1, i, 8)
                    col[:, 7] += prod(j, 0, i, 8)
    return tuple(out)


def c1(depth, level):
    smax = (1 << depth) - 1
    return float(smax * smax * K1 * 4096 * (1 << 4 * level))


def c2(depth, level):
    smax = (1 << depth) - 1
    return smax * smax * K2 * (1 << 4 * level) * 16 * 104


def structure(sx, sy, depth, level):
    """float64 [h][w]: (2*mugxgy + c2)/(mugx2 + mugy2 + c2), each bit for bit the tool's."""
    mugx2, mugy2, mugxgy = table_window(gradient(sx), gradient(sy))
    k = np.float64(c2(depth, level))
    return (2 * mugxgy + k) / (mugx2 + mugy2 + k)


def box(s):
    """int64 [h][w]: the sums over rows j - 4 .. j + 3 and columns i - 4 .. i + 3, coordinates clamped to the level."""
    h, w = s.shape
    out = np.zeros((h, w), np.int64)
    jj = np.arange(h)
    ii = np.arange(w)
    for dj in range(-4, 4):
        rows = s[np.clip(jj + dj, 0, h - 1)]
        for di in range(-4, 4):
            out += rows[:, np.clip(ii + di, 0, w - 1)]
    return out


def box_sums(sx, sy):
    """(mux, muy, wrapped): the tool's two `unsigned` per sample as int64 in [0, 2^32), and where muy wrapped."""
    bx, by = box(sx), box(sy)
    true = by[:, :1] + bx - bx[:, :1]
    return bx % (1 << 32), true % (1 << 32), true < 0


def luminance(sx, sy, depth, level):
    """float64 [h][w]: (2*mux*(double)muy + c1)/(mux*(double)mux + muy*(double)muy + c1), 2*mux an unsigned product."""
    mux, muy, _ = box_sums(sx, sy)
    f = np.float64
    k = f(c1(depth, level))
    two = ((2 * mux) % (1 << 32)).astype(f)
    return (two * muy.astype(f) + k) / (mux.astype(f) * mux.astype(f) + muy.astype(f) * muy.astype(f) + k)


def terms(src, rec, depth):
    """[level] float64 [h_l][w_l]: the structure terms of levels 0..2, structure * luminance of level 3."""
    out = []
    for l, (sx, sy) in enumerate(zip(pyramid(src), pyramid(rec))):
        t = structure(sx, sy, depth, l)
        if l == LEVELS - 1:
            t = t * luminance(sx, sy, depth, l)
        out.append(t)
    return out


def wrapped(src, rec):
    """How many samples of level 3 have a wrapped muy."""
    return int(box_sums(pyramid(src)[-1], pyramid(rec)[-1])[2].sum())


def wrap_pair(w=64, h=48, depth=8):
    """(src, rec) whose muy really wraps: x bright on the left and dark on the right, y dark, so that mux falls along
    a row by more than muy(j, 0)."""
    top = (1 << depth) - 1
    src = np.zeros((h, w), np.int32)
    src[:, :w // 2] = top
    return src, np.full((h, w), 3, np.int32)


def checkerboard(w, h, depth, block=32):
    """(src, rec): 0 / max in blocks of `block` samples and its inverse.  A block is still two samples wide at level 3,
    so along the block edges both diagonal differences are max * 256: the largest gradients there are (where four
    blocks meet both are zero)."""
    top = (1 << depth) - 1
    yy, xx = np.mgrid[0:h, 0:w]
    src = (((yy // block + xx // block) & 1) * top).astype(np.int32)
    return src, top - src


def _pow(a, b):
    try:
        return math.pow(a, b)
    except ValueError:              # a negative base: C's pow gives NAN
        return math.nan


def score(sums, w, h):
    """calc_ssim's product from the four sums."""
    ret = 1.0
    for l in range(LEVELS):
        wl, hl = level_size(w, h, l)
        ret *= _pow(float(sums[l]) / (wl * hl), WEIGHTS[l])
    return ret


def tool_sums(src, rec, depth):
    """The four running doubles of fs_average: the terms of a level added in raster order."""
    return [float(np.cumsum(t.ravel())[-1]) for t in terms(src, rec, depth)]


def tool_value(src, rec, depth):
    """calc_ssim's return value."""
    h, w = np.asarray(src).shape
    return score(tool_sums(src, rec, depth), w, h)


def bits(v):
    """The bit pattern of a double as an int."""
    return struct.unpack("<Q", struct.pack("<d", v))[0]


def convert(v, wt, raw=False):
    """The tool's two conversions: raw, or 10*(log10(weight) - log10(weight - value))."""
    if raw:
        return v / wt
    return 10 * (math.log10(wt) - (math.log10(wt - v) if wt - v > 0 else -math.inf))


def tool_lines(frames, c444, raw=False):
    """dump_fastssim -c's lines (with -r: raw) for per-frame plane values [(y, cb, cr)] (calc_ssim's return values)."""
    cw = 1.0 if c444 else 0.25          # the tool's cweight
    out = []
    g = [0.0, 0.0, 0.0]
    for f, s in enumerate(frames):
        out.append("%08i: %-8G  (Y': %-8G  Cb: %-8G  Cr: %-8G)" % (
            f, convert(s[0] + cw * (s[1] + s[2]), 1 + 2 * cw, raw), convert(s[0], 1, raw), convert(s[1], 1, raw),
            convert(s[2], 1, raw)))
        for i in range(3):
            g[i] += s[i]
    n = len(frames)
    out.append("Total: %-8G  (Y': %-8G  Cb: %-8G  Cr: %-8G)" % (
        convert(g[0] + cw * (g[1] + g[2]), (1 + 2 * cw) * n, raw), convert(g[0], n, raw), convert(g[1], n, raw),
        convert(g[2], n, raw)))
    return out


def case_values(case):
    """[frame][plane] calc_ssim's return values of a CASES entry, restated."""
    name, kind, w, h, c444, depth, nframes, seed = case
    src, dst = M.make_case(case)
    return [[tool_value(a, b, depth) for a, b in zip(fs, fd)] for fs, fd in zip(src, dst)]


def restated_lines(case, raw=False):
    """dump_fastssim -c's lines of a CASES entry, restated."""
    return tool_lines(case_values(case), case[4], raw)
