"""CPU restatement of the two quality metrics of the reference's RD tools, written from their formulas.

PSNR (tools/dump_psnr.c): the int64 sum of squared differences over the picture region;
10*(log10(max^2) + log10(npixels) - log10(sse)).  PSNR-HVS-M (calc_psnrhvs, tools/dump_psnrhvs.c): 8x8
windows at step 7; per window single-precision means and variances (whole window and its four 4x4
quarters), od_bin_fdct8x8 of both windows (the oracle's), the contrast-masking thresholds, and 64 float
terms (err*csf)^2.  The tool keeps one running float over a plane (np.cumsum(..., dtype=np.float32)
reproduces it); the device sums the same float terms in double.  Every float operation here is done in
numpy float32 in the tool's order, so each term is the tool's value bit for bit.

Also: the seeded clip pairs of tests/golden/metrics.npz (make_case) and the tools' printed lines.
"""
import ctypes
import math
import os
import re

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
F32 = np.float32


def csf_tables():
    """OD_CSF[3][8][8] of daala_amd/csrc/gen/od_csf_tables.h (luma, Cb, Cr) as float32."""
    text = open(os.path.join(ROOT, "daala_amd", "csrc", "gen", "od_csf_tables.h")).read()
    body = text[text.index("OD_CSF[3][8][8]"):]
    vals = [float.fromhex(v) for v in re.findall(r"(-?0x[0-9a-fA-F.]+p[-+]?\d+)f", body)]
    assert len(vals) == 192
    return np.array(vals, np.float32).reshape(3, 8, 8)


def mask_tables(csf):
    """(float)((csf*k)*(csf*k)) evaluated in double, k = 0.3885746225901003."""
    c = csf.astype(np.float64) * 0.3885746225901003
    return (c * c).astype(np.float32)


def to_depth(s12, depth):
    """The reference's output conversion of int16 samples at 12 bits: OD_CLAMPI(0, (s + (1 << sh >> 1)) >> sh,
    (1 << depth) - 1), sh = 12 - depth."""
    sh = 12 - depth
    v = (np.asarray(s12).astype(np.int32) + ((1 << sh) >> 1)) >> sh
    return np.clip(v, 0, (1 << depth) - 1)


def sse(src, rec):
    d = np.asarray(src).astype(np.int64) - np.asarray(rec).astype(np.int64)
    return int((d * d).sum())


def window_count(w, h):
    nx = (w - 7 + 6) // 7 if w > 7 else 0
    ny = (h - 7 + 6) // 7 if h > 7 else 0
    return nx, ny


def _windows(p, nx, ny):
    ys = 7 * np.arange(ny)
    xs = 7 * np.arange(nx)
    i = np.arange(8)
    win = np.asarray(p).astype(np.int32)[ys[:, None, None, None] + i[None, None, :, None],
                                         xs[None, :, None, None] + i[None, None, None, :]]
    return np.ascontiguousarray(win.reshape(nx * ny, 64))


def _fdct8x8(win):
    from _libs import P, oracle
    out = np.zeros_like(win)
    if len(win):
        oracle().odo_fdct_2d_batch(1, P(out), P(win), ctypes.c_long(len(win)))
    return out


def hvs_terms(src, rec, csf_index):
    """float32 [windows][64]: the terms of every window (raster order of windows, (i, j) order inside one) of the
    pictures src and rec (2-D integer arrays at the source depth, the picture region only)."""
    src = np.asarray(src)
    h, w = src.shape
    nx, ny = window_count(w, h)
    csf = csf_tables()[csf_index]
    mask = mask_tables(csf_tables())[csf_index]
    S = _windows(src, nx, ny)
    D = _windows(rec, nx, ny)
    n = len(S)
    sub = [((i & 12) >> 2) + ((j & 12) >> 1) for i in range(8) for j in range(8)]
    out = []
    for X in (S, D):
        Xf = X.astype(F32)
        gmean = np.zeros(n, F32)
        means = np.zeros((4, n), F32)
        for k in range(64):
            gmean = gmean + Xf[:, k]
            means[sub[k]] = means[sub[k]] + Xf[:, k]
        gmean = gmean / F32(64)
        means = means / F32(16)
        gvar = np.zeros(n, F32)
        var = np.zeros((4, n), F32)
        for k in range(64):
            a = Xf[:, k] - gmean
            b = Xf[:, k] - means[sub[k]]
            gvar = gvar + a * a
            var[sub[k]] = var[sub[k]] + b * b
        gvar = gvar * (F32(1) / F32(63) * F32(64))
        var = var * (F32(1) / F32(15) * F32(16))
        with np.errstate(divide="ignore", invalid="ignore"):
            gvar = np.where(gvar > 0, (((var[0] + var[1]) + var[2]) + var[3]) / gvar, gvar).astype(F32)
        C = _fdct8x8(X)
        m = np.zeros(n, F32)
        for k in range(1, 64):
            m = m + (C[:, k] * C[:, k]).astype(F32) * mask.flat[k]
        m = (np.sqrt((m * gvar).astype(np.float64)) / 32.0).astype(F32)
        out.append((C, m))
    (CS, smask), (CD, dmask) = out
    smask = np.where(dmask > smask, dmask, smask)
    terms = np.zeros((n, 64), F32)
    for k in range(64):
        err = np.abs(CS[:, k] - CD[:, k]).astype(F32)
        if k:
            t = smask / mask.flat[k]
            err = np.where(err < t, F32(0), err - t).astype(F32)
        e = err * csf.flat[k]
        terms[:, k] = e * e
    return terms


def window_sums(src, rec, csf_index):
    """float32 [nwy][nwx]: each window's terms summed in float in (i, j) order (odhip_psnrhvs_windows)."""
    h, w = np.asarray(src).shape
    nx, ny = window_count(w, h)
    t = hvs_terms(src, rec, csf_index)
    return (np.cumsum(t, axis=1, dtype=F32)[:, -1] if len(t) else np.zeros(0, F32)).reshape(ny, nx)


def hvs_sum(src, rec, csf_index):
    """The plane's terms summed exactly (the double sum the device approximates to ~1e-15)."""
    return math.fsum(hvs_terms(src, rec, csf_index).astype(np.float64).ravel().tolist())


def hvs_tool(src, rec, csf_index, depth):
    """calc_psnrhvs's return value: the running float sum / pixels / samplemax^2, all in float."""
    t = hvs_terms(src, rec, csf_index)
    ret = np.cumsum(t.ravel(), dtype=F32)[-1]
    ret = F32(ret / F32(t.size))
    m = (1 << depth) - 1
    return float(F32(ret / F32(m * m)))


# ---- the tools' printed lines ----------------------------------------------------------
def _db(score, weight):
    return 10 * (-1 * math.log10(weight * score))


def psnr_lines(frames, depth):
    """dump_psnr's lines for a clip pair given as [(pl_sse[3], pl_npix[3])] per frame."""
    smax = (1 << depth) - 1
    out = []
    g = [0, 0, 0]
    gn = [0, 0, 0]
    for f, (pse, pnp) in enumerate(frames):
        pl = [10 * (math.log10(smax * smax) + math.log10(pnp[i]) - math.log10(pse[i])) for i in range(3)]
        tot = 10 * (math.log10(smax * smax) + math.log10(sum(pnp)) - math.log10(sum(pse)))
        out.append("%08i: %-7G  (Y': %-7G  Cb: %-7G  Cr: %-7G)" % (f, tot, pl[0], pl[1], pl[2]))
        for i in range(3):
            g[i] += pse[i]
            gn[i] += pnp[i]
    pl = [10 * (math.log10(smax * smax) + math.log10(gn[i]) - math.log10(g[i])) for i in range(3)]
    tot = 10 * (math.log10(smax * smax) + math.log10(sum(gn)) - math.log10(sum(g)))
    out.append("Total: %-7G  (Y': %-7G  Cb: %-7G  Cr: %-7G)" % (tot, pl[0], pl[1], pl[2]))
    return out


def psnrhvs_lines(frames, c444):
    """dump_psnrhvs's lines for per-frame plane scores [(y, cb, cr)] (calc_psnrhvs's values, as doubles)."""
    cw = 1.0 if c444 else 0.25
    out = []
    g = [0.0, 0.0, 0.0]
    for f, s in enumerate(frames):
        out.append("%08i: %-8G  (Y': %-8G  Cb: %-8G  Cr: %-8G)" % (
            f, _db(s[0] + cw * (s[1] + s[2]), 1 + 2 * cw), _db(s[0], 1), _db(s[1], 1), _db(s[2], 1)))
        for i in range(3):
            g[i] += s[i]
    n = len(frames)
    out.append("Total: %-8G  (Y': %-8G  Cb: %-8G  Cr: %-8G)" % (
        _db(g[0] + cw * (g[1] + g[2]), (1 + 2 * cw) * 1. / n), _db(g[0], 1. / n), _db(g[1], 1. / n),
        _db(g[2], 1. / n)))
    return out


# ---- seeded clip pairs (tools/make_golden_metrics.py, tests/test_metrics_host.py, test_gpu_metrics.py) ----
# (name, content, w, h, 4:4:4, depth, frames, seed)
CASES = [
    ("natural_420_8", "natural", 96, 64, False, 8, 2, 1),
    ("texture_420_8_odd", "texture", 77, 53, False, 8, 2, 2),
    ("noise_444_8", "noise", 64, 48, True, 8, 2, 3),
    ("natural_444_8_odd", "natural", 57, 41, True, 8, 1, 4),
    ("texture_420_10", "texture", 80, 56, False, 10, 2, 5),
    ("natural_444_10_odd", "natural", 45, 39, True, 10, 2, 6),
    ("noise_420_10_odd", "noise", 70, 46, False, 10, 1, 7),
]


def _content(kind, rng, w, h, depth):
    top = (1 << depth) - 1
    yy, xx = np.mgrid[0:h, 0:w].astype(np.float64)
    if kind == "natural":
        v = (0.5 + 0.25 * np.cos(xx / (5 + 7 * rng.rand())) * np.cos(yy / (4 + 9 * rng.rand()))
             + 0.15 * np.sin((xx + yy) / 11.0) + 0.03 * rng.randn(h, w))
    elif kind == "texture":
        v = 0.5 + 0.4 * np.sign(np.sin(xx * (0.7 + rng.rand())) * np.sin(yy * (0.5 + rng.rand()))) \
            * (0.5 + 0.5 * rng.rand(h, w))
    else:
        v = rng.rand(h, w)
    return np.clip(np.rint(v * top), 0, top).astype(np.int32)


def make_case(case):
    """([frame][plane] source, [frame][plane] distorted) int32 planes of a CASES entry."""
    name, kind, w, h, c444, depth, nframes, seed = case
    rng = np.random.RandomState(seed)
    top = (1 << depth) - 1
    cw, ch = (w, h) if c444 else ((w + 1) // 2, (h + 1) // 2)
    src, dst = [], []
    for _ in range(nframes):
        fs, fd = [], []
        for pw, ph in ((w, h), (cw, ch), (cw, ch)):
            p = _content(kind, rng, pw, ph, depth)
            amp = max(1, int(top * 0.04 * (0.5 + rng.rand())))
            d = p + rng.randint(-amp, amp + 1, size=p.shape)
            keep = rng.rand(ph, pw) < 0.3
            d[keep] = p[keep]
            fs.append(p)
            fd.append(np.clip(d, 0, top).astype(np.int32))
        src.append(fs)
        dst.append(fd)
    return src, dst


def y4m_bytes(frames, w, h, c444, depth):
    """A YUV4MPEG2 file of [frame][plane] int planes (8 bits: uint8 samples; 10: little-endian uint16)."""
    tag = ("444" if c444 else "420jpeg") if depth == 8 else ("444p10" if c444 else "420p10")
    out = [b"YUV4MPEG2 W%d H%d F30:1 Ip A1:1 C%s\n" % (w, h, tag.encode())]
    dt = np.uint8 if depth == 8 else np.dtype("<u2")
    for f in frames:
        out.append(b"FRAME\n")
        for p in f:
            out.append(np.ascontiguousarray(p.astype(dt)).tobytes())
    return b"".join(out)


def restated_lines(case):
    """(dump_psnr lines, dump_psnrhvs lines) of a CASES entry, restated."""
    name, kind, w, h, c444, depth, nframes, seed = case
    src, dst = make_case(case)
    pf, hf = [], []
    for fs, fd in zip(src, dst):
        pf.append(([sse(a, b) for a, b in zip(fs, fd)], [a.size for a in fs]))
        hf.append([hvs_tool(a, b, i, depth) for i, (a, b) in enumerate(zip(fs, fd))])
    return psnr_lines(pf, depth), psnrhvs_lines(hf, c444)
