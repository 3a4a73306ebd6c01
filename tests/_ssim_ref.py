"""CPU restatement of SSIM as the reference's RD tool computes it (calc_ssim, tools/dump_ssim.c), written from its
formulas.

A plane pair of w x h samples: an integer Gaussian (weight 256, taps(sigma, max_len) - the host libm's exp / log,
which Python's math module calls) runs along the rows, then down the columns, over the six moments mux, muy, x2, xy,
y2, w; taps that fall outside the plane are dropped, which is why the weight w is a moment too.  All moments are the
mathematical integers (numpy int64: a horizontal one is below 2^32, a vertical one below 2^41; the tool's own
`signed` products overflow at 12 bits, so depth 12 has no tool yardstick).  Every sample then gives one double term,
evaluated operation by operation in the C expression's association (numpy float64 element operations are single IEEE
operations, never fused).  The tool adds the terms of a plane into one running double in raster order
(np.cumsum reproduces it) and divides by the sum of the weights.

Also: the seeded clip pairs of tests/golden/ssim.npz and the tool's printed lines.
"""
import math

import numpy as np

import _metrics_ref as M

K1 = 0.01 * 0.01
K2 = 0.03 * 0.03

# the seven clips of _metrics_ref.CASES (radius 0 or 1) and tall, narrow ones: the smallest shapes that reach a real
# radius and both truncations at once (name, content, w, h, 4:4:4, depth, frames, seed)
TALL_CASES = [
    ("tall_420_8", "natural", 24, 544, False, 8, 2, 31),        # luma radius 9; chroma 12x272: 4
    ("narrow_420_8", "texture", 8, 544, False, 8, 1, 32),       # luma radius capped to 7; chroma 4x272: capped to 3
    ("tall_444_10", "noise", 40, 256, True, 10, 2, 33),         # radius 4
]
CASES = list(M.CASES) + TALL_CASES


def taps(sigma, max_len):
    """The tap table of gaussian_filter_init: 2*len + 1 unsigned values, len capped to max_len - 1."""
    scale = 1 / (math.sqrt(2 * math.pi) * sigma)
    nhisigma2 = -0.5 / (sigma * sigma)
    s = math.sqrt(0.5 * math.pi) * sigma * (1.0 / 256)
    ln = 0.0 if s >= 1 else math.floor(sigma * math.sqrt(-2 * math.log(s)))
    n = max_len - 1 if ln >= max_len else int(ln)
    side = [int(256 * scale * math.exp(nhisigma2 * ci * ci) + 0.5) for ci in range(1, n + 1)]
    return side[::-1] + [(256 - 2 * sum(side)) & 0xffffffff] + side


def plane_taps(w, h, par=1.0):
    """(vertical, horizontal) tap tables of a w x h plane: both from the plane's own height."""
    return taps(h * (1.5 / 256), min(w, h)), taps(h * (1.5 / 256) / par, min(w, h))


def _filter(a, t, axis):
    """sum_k t[k] * a[.. i - r + k ..] along `axis` over the taps that fall inside the array (int64, exact)."""
    r = len(t) // 2
    a = np.moveaxis(a, axis, -1)
    n = a.shape[-1]
    pad = np.zeros(a.shape[:-1] + (n + 2 * r,), np.int64)
    pad[..., r:r + n] = a
    out = np.zeros(a.shape, np.int64)
    for k, tk in enumerate(t):
        out += int(tk) * pad[..., k:k + n]
    return np.moveaxis(out, -1, axis)


def moments(src, rec, par=1.0):
    """int64 [6][h][w]: mux, muy, x2, xy, y2, w after both passes."""
    s = np.asarray(src).astype(np.int64)
    d = np.asarray(rec).astype(np.int64)
    h, w = s.shape
    vt, ht = plane_taps(w, h, par)
    m = np.stack([s, d, s * s, s * d, d * d, np.ones_like(s)])
    return _filter(_filter(m, ht, 2), vt, 1)


def terms(src, rec, depth, par=1.0):
    """float64 [h][w]: the tool's per-sample term, each bit for bit."""
    mux, muy, x2, xy, y2, mw = moments(src, rec, par)
    smax = (1 << depth) - 1
    f = np.float64
    w = mw.astype(f)
    c1 = f(smax * smax) * f(K1) * w * w
    c2 = f(smax * smax) * f(K2) * w * w
    mx2 = mux.astype(f) * mux.astype(f)
    mxy = mux.astype(f) * muy.astype(f)
    my2 = muy.astype(f) * muy.astype(f)
    num = mw.astype(f) * (2 * mxy + c1) * (c2 + 2 * (xy.astype(f) * w - mxy))
    den = (mx2 + my2 + c1) * (x2.astype(f) * w - mx2 + y2.astype(f) * w - my2 + c2)
    return num / den


def weight(w, h, par=1.0):
    """The sum of the weight moment over a w x h plane: (sum over columns) x (sum over rows), an exact integer."""
    vt, ht = plane_taps(w, h, par)
    col = _filter(np.ones((1, w), np.int64), ht, 1)
    row = _filter(np.ones((h, 1), np.int64), vt, 0)
    return int(col.sum()) * int(row.sum())


def tool_value(src, rec, depth, par=1.0):
    """calc_ssim's return value: the running double over the terms in raster order / the sum of the weights."""
    t = terms(src, rec, depth, par)
    return float(np.cumsum(t.ravel())[-1]) / float(weight(t.shape[1], t.shape[0], par))


def score(ssim, wt, raw=False):
    """The tool's two conversions of a sum and its weight: raw, or 10*(log10(weight) - log10(weight - ssim))."""
    if raw:
        return ssim / wt
    return 10 * (math.log10(wt) - (math.log10(wt - ssim) if wt - ssim > 0 else -math.inf))


def tool_lines(frames, c444, raw=False):
    """dump_ssim's lines (with -r: raw) for per-frame plane values [(y, cb, cr)] (calc_ssim's return values)."""
    cw = 1.0 if c444 else 0.25
    out = []
    g = [0.0, 0.0, 0.0]
    for f, s in enumerate(frames):
        out.append("%08i: %-8G  (Y': %-8G  Cb: %-8G  Cr: %-8G)" % (
            f, score(s[0] + cw * (s[1] + s[2]), 1 + 2 * cw, raw), score(s[0], 1, raw), score(s[1], 1, raw),
            score(s[2], 1, raw)))
        for i in range(3):
            g[i] += s[i]
    n = len(frames)
    out.append("Total: %-8G  (Y': %-8G  Cb: %-8G  Cr: %-8G)" % (
        score(g[0] + cw * (g[1] + g[2]), (1 + 2 * cw) * n, raw), score(g[0], n, raw), score(g[1], n, raw),
        score(g[2], n, raw)))
    return out


def restated_lines(case, raw=False):
    """dump_ssim's lines of a CASES entry, restated."""
    name, kind, w, h, c444, depth, nframes, seed = case
    src, dst = M.make_case(case)
    return tool_lines([[tool_value(a, b, depth) for a, b in zip(fs, fd)] for fs, fd in zip(src, dst)], c444, raw)
