"""CPU restatement of MS-SSIM as the reference's RD tool computes it (calc_msssim and calc_ssim, tools/dump_msssim.c),
written from its formulas.

A plane pair of w x h samples at depth 8, 10 or 12 gives five scales: scale 0 is the pair itself, scale i > 0 the 2x2
SUM (no division) of scale i - 1 at (w >> 1) x (h >> 1), an odd last row or column dropped, and `max` - (1 << depth) - 1
at scale 0 - times 4.  At every scale an integer Gaussian of weight 1024 (gaussian_filter_init(1.5, 5): nine taps, by
the host libm, which Python's math module calls) runs along the rows, then down the columns, over the six moments mux,
muy, x2, xy, y2, w; taps that fall outside the plane are dropped, which is why the weight w is a moment too.  All
moments are the mathematical integers (numpy int64: below 2^61 at 12 bits and scale 4; above 2^53 they enter the term
through an int64 -> double conversion, which rounds to nearest, as numpy's astype does).  Every sample gives two double
terms, cs and ssim, evaluated operation by operation in the C expressions' association (numpy float64 element
operations are single IEEE operations, never fused).  The tool adds the terms of a scale into running doubles in raster
order (np.cumsum reproduces it), divides by the sum of the weights and multiplies the powers of cs of scales 0..3 and of
ssim of scale 4.

The reference's Y4M reader takes 8 and 10 bits only: depth 12 has this restatement as its only yardstick.

Also: the seeded clip pairs of tests/golden/msssim.npz and the tool's printed lines.
"""
import math

import numpy as np

import _metrics_ref as M

K1 = 0.01
K2 = 0.03
SCALES = 5
MIN_SIZE = 16                       # scale 4 of 16 x 16 is 1 x 1; below it the tool divides 0 by 0
EXPONENT = (0.0448, 0.2856, 0.3001, 0.2363, 0.1333)

# the seven clips of _metrics_ref.CASES and two at the size floor (name, content, w, h, 4:4:4, depth, frames, seed)
FLOOR_CASES = [
    ("min_444_8", "natural", 16, 16, True, 8, 1, 42),           # scale 4 is 1 x 1
    ("min_420_8", "texture", 32, 34, False, 8, 1, 44),          # chroma 16 x 17
]
CASES = list(M.CASES) + FLOOR_CASES


def taps():
    """gaussian_filter_init(1.5, 5) at weight 1024: 8 37 112 218 274 218 112 37 8."""
    sigma, max_len, weight = 1.5, 5, 1024
    scale = 1 / (math.sqrt(2 * math.pi) * sigma)
    nhisigma2 = -0.5 / (sigma * sigma)
    s = math.sqrt(0.5 * math.pi) * sigma * (1.0 / weight)
    ln = 0.0 if s >= 1 else math.floor(sigma * math.sqrt(-2 * math.log(s)))
    n = max_len - 1 if ln >= max_len else int(ln)
    side = [int(weight * scale * math.exp(nhisigma2 * ci * ci) + 0.5) for ci in range(1, n + 1)]
    return side[::-1] + [weight - 2 * sum(side)] + side


TAPS = taps()


def _filter(a, axis):
    """sum_k TAPS[k] * a[.. i - r + k ..] along `axis` over the taps that fall inside the array (int64, exact)."""
    r = len(TAPS) // 2
    a = np.moveaxis(a, axis, -1)
    n = a.shape[-1]
    pad = np.zeros(a.shape[:-1] + (n + 2 * r,), np.int64)
    pad[..., r:r + n] = a
    out = np.zeros(a.shape, np.int64)
    for k, tk in enumerate(TAPS):
        out += int(tk) * pad[..., k:k + n]
    return np.moveaxis(out, -1, axis)


def down(a):
    """downsample_2x: the 2x2 sums, an odd last row or column dropped."""
    h, w = a.shape
    a = a[:2 * (h >> 1), :2 * (w >> 1)]
    return a[0::2, 0::2] + a[0::2, 1::2] + a[1::2, 0::2] + a[1::2, 1::2]


def pyramid(plane):
    """[scale] int64 planes, scale 0 the plane itself."""
    out = [np.asarray(plane).astype(np.int64)]
    for _ in range(1, SCALES):
        out.append(down(out[-1]))
    return out


def moments(s, d):
    """int64 [6][h][w] of one scale: mux, muy, x2, xy, y2, w after both passes."""
    m = np.stack([s, d, s * s, s * d, d * d, np.ones_like(s)])
    return _filter(_filter(m, 2), 1)


def scale_terms(s, d, smax):
    """(cs, ssim) float64 [h][w] of one scale: the tool's per-sample terms, each bit for bit."""
    mux, muy, x2, xy, y2, mw = moments(s, d)
    f = np.float64
    w = mw.astype(f)
    c1 = f(K1 * K1) * f(smax) * f(smax) * w * w
    c2 = f(K2 * K2) * f(smax) * f(smax) * w * w
    mx2 = mux.astype(f) * mux.astype(f)
    mxy = mux.astype(f) * muy.astype(f)
    my2 = muy.astype(f) * muy.astype(f)
    cs = mw.astype(f) * (c2 + 2 * (xy.astype(f) * w - mxy)) / (x2.astype(f) * w - mx2 + y2.astype(f) * w - my2 + c2)
    ssim = cs * (2 * mxy + c1) / (mx2 + my2 + c1)
    return cs, ssim


def terms(src, rec, depth):
    """[(cs, ssim)] of the five scales."""
    smax = (1 << depth) - 1
    return [scale_terms(s, d, smax * 4 ** i) for i, (s, d) in enumerate(zip(pyramid(src), pyramid(rec)))]


def weights(w, h):
    """The sum of the weight moment of every scale: exact integers of the size alone."""
    out = []
    for i in range(SCALES):
        ws, hs = w >> i, h >> i
        col = _filter(np.ones((1, ws), np.int64), 1)
        row = _filter(np.ones((hs, 1), np.int64), 0)
        out.append(int(col.sum()) * int(row.sum()))
    return out


def _pow(a, b):
    try:
        return math.pow(a, b)
    except ValueError:              # a negative base: C's pow gives NAN
        return math.nan


def score(sums, wts):
    """calc_msssim's product from the five sums (cs of scales 0..3, ssim of scale 4) and their weights."""
    v = [float(s) / float(w) for s, w in zip(sums, wts)]
    return _pow(v[0], EXPONENT[0]) * _pow(v[1], EXPONENT[1]) * _pow(v[2], EXPONENT[2]) * _pow(v[3], EXPONENT[3]) \
        * _pow(v[4], EXPONENT[4])


def tool_sums(src, rec, depth):
    """The five running doubles the tool's product uses: cs of scales 0..3 and ssim of scale 4, terms added in raster
    order."""
    t = terms(src, rec, depth)
    return [float(np.cumsum(t[i][0 if i < 4 else 1].ravel())[-1]) for i in range(SCALES)]


def tool_value(src, rec, depth):
    """calc_msssim's return value."""
    h, w = np.asarray(src).shape
    return score(tool_sums(src, rec, depth), weights(w, h))


def convert(v, wt, raw=False):
    """The tool's two conversions: raw, or 10*(log10(weight) - log10(weight - value))."""
    if raw:
        return v / wt
    return 10 * (math.log10(wt) - (math.log10(wt - v) if wt - v > 0 else -math.inf))


def tool_lines(frames, c444, raw=False):
    """dump_msssim's lines (with -r: raw) for per-frame plane values [(y, cb, cr)] (calc_msssim's return values)."""
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


def restated_lines(case, raw=False):
    """dump_msssim's lines of a CASES entry, restated."""
    name, kind, w, h, c444, depth, nframes, seed = case
    src, dst = M.make_case(case)
    return tool_lines([[tool_value(a, b, depth) for a, b in zip(fs, fd)] for fs, fd in zip(src, dst)], c444, raw)
