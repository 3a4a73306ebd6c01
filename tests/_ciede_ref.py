"""CIEDE2000 of picture pairs restated in numpy, operation by operation as include/daala_hip.h defines it (the yardstick of
tests/test_ciede_host.py, tests/test_gpu_ciede.py and tests/test_gpu_pipe_ciede.py).

Written from the definition, not from the reference tool's text.  Every value is float64 and every line below is one
IEEE operation per operation of the definition, in its order, so that only numpy's pow, cbrt, arctan2, sin, cos, exp and
sqrt can differ from the device's.  Seventh powers are products, hues are degrees (arctan2 times 180/pi, brought into
[0, 360)), and an angle enters sin or cos times pi/180.

dE00 is discontinuous where |h1' - h2'| = 180 degrees.  de00(..., flip=mask) evaluates the OTHER side of the two branches
that compare against 180 (the wrap of dh' and the choice of the mean hue) for the pixels of `mask`; near(stats) says which
pixels are within 1e-9 degrees of the jump, where a device may take either side."""
import numpy as np

DEG = 57.29577951308232            # 180/pi
RAD = 0.017453292519943295         # pi/180
P25_7 = 6103515625.0               # 25^7
KL, KC, KH = 0.65, 1.0, 4.0        # the tool's weights
SAMPLE_U8, SAMPLE_U16, SAMPLE_I16_12 = 0, 1, 2

# L1 a1 b1 | L2 a2 b2 | dE00: the published test data of Sharma, Wu, Dalal 2005 (kL = kC = kH = 1)
TABLE = np.array([
    [50, 2.6772, -79.7751, 50, 0, -82.7485, 2.0425],
    [50, 3.1571, -77.2803, 50, 0, -82.7485, 2.8615],
    [50, 2.8361, -74.0200, 50, 0, -82.7485, 3.4412],
    [50, -1.3802, -84.2814, 50, 0, -82.7485, 1.0000],
    [50, -1.1848, -84.8006, 50, 0, -82.7485, 1.0000],
    [50, -0.9009, -85.5211, 50, 0, -82.7485, 1.0000],
    [50, 0, 0, 50, -1, 2, 2.3669],
    [50, -1, 2, 50, 0, 0, 2.3669],
    [50, 2.49, -0.001, 50, -2.49, 0.0009, 7.1792],
    [50, 2.49, -0.001, 50, -2.49, 0.0010, 7.1792],
    [50, 2.49, -0.001, 50, -2.49, 0.0011, 7.2195],
    [50, 2.49, -0.001, 50, -2.49, 0.0012, 7.2195],
    [50, -0.001, 2.49, 50, 0.0009, -2.49, 4.8045],
    [50, -0.001, 2.49, 50, 0.0010, -2.49, 4.8045],
    [50, -0.001, 2.49, 50, 0.0011, -2.49, 4.7461],
    [50, 2.5, 0, 50, 0, -2.5, 4.3065],
    [50, 2.5, 0, 73, 25, -18, 27.1492],
    [50, 2.5, 0, 61, -5, 29, 22.8977],
    [50, 2.5, 0, 56, -27, -3, 31.9030],
    [50, 2.5, 0, 58, 24, 15, 19.4535],
    [50, 2.5, 0, 50, 3.1736, 0.5854, 1.0000],
    [50, 2.5, 0, 50, 3.2972, 0, 1.0000],
    [50, 2.5, 0, 50, 1.8634, 0.5757, 1.0000],
    [50, 2.5, 0, 50, 3.2592, 0.3350, 1.0000],
    [60.2574, -34.0099, 36.2677, 60.4626, -34.1751, 39.4387, 1.2644],
    [63.0109, -31.0961, -5.8663, 62.8187, -29.7946, -4.0864, 1.2630],
    [61.2901, 3.7196, -5.3901, 61.4292, 2.2480, -4.9620, 1.8731],
    [35.0831, -44.1164, 3.7933, 35.0232, -40.0716, 1.5901, 1.8645],
    [22.7233, 20.0904, -46.6940, 23.0331, 14.9730, -42.5619, 2.0373],
    [36.4612, 47.8580, 18.3852, 36.2715, 50.5065, 21.2231, 1.4146],
    [90.8027, -2.0831, 1.4410, 91.1528, -1.6435, 0.0447, 1.4441],
    [90.9257, -0.5406, -0.9208, 88.6381, -0.8985, -0.7239, 1.5381],
    [6.7747, -0.2908, -2.4247, 5.8714, -0.0985, -2.2286, 0.6377],
    [2.0776, 0.0795, -1.1350, 0.9033, -0.0636, -0.5514, 0.9082],
], np.float64)
assert TABLE.shape == (34, 7)


def samples(plane, fmt, depth):
    """The samples of a plane at the depth as int64: SAMPLE_I16_12 through the reference's output conversion."""
    a = np.asarray(plane)
    if fmt == SAMPLE_I16_12:
        sh = 12 - depth
        return np.clip((a.astype(np.int64) + (1 << sh >> 1)) >> sh, 0, (1 << depth) - 1)
    if fmt == SAMPLE_U16:
        return a.astype(np.int64) & 0xffff
    return a.astype(np.int64)


def ycc_rgb(y, cb, cr, depth):
    """Steps 1 and 2: BT.709 Y'CbCr samples -> unclipped R, G, B."""
    s = float(1 << (depth - 8))
    yp = (np.asarray(y, np.float64) - 16 * s) / (219 * s)
    pb = (np.asarray(cb, np.float64) - 128 * s) / (224 * s)
    pr = (np.asarray(cr, np.float64) - 128 * s) / (224 * s)
    return yp + 1.28033 * pr, (yp - 0.21482 * pb) - 0.38059 * pr, yp + 2.12798 * pb


def _linear(c, stats):
    up = c > 0.04045
    with np.errstate(invalid="ignore"):
        v = np.where(up, np.power((np.where(up, c, 1.0) + 0.055) / 1.055, 2.4), c / 12.92)
    if stats is not None:
        stats.setdefault("srgb_pow", 0), stats.setdefault("srgb_linear", 0), stats.setdefault("rgb_negative", 0)
        stats["srgb_pow"] += int(up.sum())
        stats["srgb_linear"] += int((~up).sum())
        stats["rgb_negative"] += int((c < 0).sum())
    return v


def _f(t, stats):
    up = t > 0.008856
    v = np.where(up, np.cbrt(np.where(up, t, 1.0)), 7.787 * t + 16.0 / 116.0)
    if stats is not None:
        for k in ("f_cbrt", "f_linear", "xyz_negative"):
            stats.setdefault(k, 0)
        stats["f_cbrt"] += int(up.sum())
        stats["f_linear"] += int((~up).sum())
        stats["xyz_negative"] += int((t < 0).sum())
        with np.errstate(divide="ignore", invalid="ignore"):
            rel = np.abs(t - 0.008856) / 0.008856
        stats["f_knee"] = min(stats.get("f_knee", np.inf), float(rel.min()))
    return v


def rgb_lab(r, g, b, stats=None):
    """Steps 3 to 5: R, G, B -> L, a, b."""
    r, g, b = (_linear(np.asarray(c, np.float64), stats) for c in (r, g, b))
    x = ((0.412453 * r + 0.357580 * g) + 0.180423 * b) / 0.95047
    y = ((0.212671 * r + 0.715160 * g) + 0.072169 * b) / 1.0
    z = ((0.019334 * r + 0.119193 * g) + 0.950227 * b) / 1.08883
    fx, fy, fz = _f(x, stats), _f(y, stats), _f(z, stats)
    return 116 * fy - 16, 500 * (fx - fy), 200 * (fy - fz)


def _pow7(c):
    c2 = c * c
    c4 = c2 * c2
    return (c4 * c2) * c


def _hue(b, a):
    h = np.arctan2(b, a) * DEG
    return np.where(h < 0, h + 360, h)


def de00(lab1, lab2, kl=KL, kc=KC, kh=KH, flip=None, stats=None):
    """Step 6: dE00 of source (L1, a1, b1) and reconstruction (L2, a2, b2), arrays of any one shape."""
    L1, A1, B1 = (np.asarray(v, np.float64) for v in lab1)
    L2, A2, B2 = (np.asarray(v, np.float64) for v in lab2)
    c1 = np.sqrt(A1 * A1 + B1 * B1)
    c2 = np.sqrt(A2 * A2 + B2 * B2)
    cb7 = _pow7((c1 + c2) / 2)
    g = 0.5 * (1 - np.sqrt(cb7 / (cb7 + P25_7)))
    a1 = (1 + g) * A1
    a2 = (1 + g) * A2
    cp1 = np.sqrt(a1 * a1 + B1 * B1)
    cp2 = np.sqrt(a2 * a2 + B2 * B2)
    h1 = _hue(B1, a1)
    h2 = _hue(B2, a2)
    dl = L2 - L1
    dc = cp2 - cp1
    cc = cp1 * cp2
    d = h2 - h1
    over, under = d > 180, d < -180
    apart = np.abs(h1 - h2) <= 180
    if flip is not None:
        # the other side of the jump: |h1' - h2'| > 180 where it was not, and the reverse
        f = np.asarray(flip, bool)
        was = over | under
        over = np.where(f, ~was & (d > 0), over)
        under = np.where(f, ~was & (d <= 0), under)
        apart = np.where(f, ~apart, apart)
    dh = np.where(over, d - 360, np.where(under, d + 360, d))
    hs = h1 + h2
    hb = np.where(apart, hs / 2, np.where(hs < 360, (hs + 360) / 2, (hs - 360) / 2))
    zero = cc == 0
    dh = np.where(zero, 0.0, dh)
    hb = np.where(zero, hs, hb)
    dH = (2 * np.sqrt(cc)) * np.sin((dh / 2) * RAD)
    lb = (L1 + L2) / 2
    cpb = (cp1 + cp2) / 2
    t = (((1 - 0.17 * np.cos((hb - 30) * RAD)) + 0.24 * np.cos((2 * hb) * RAD)) + 0.32 * np.cos((3 * hb + 6) * RAD)) \
        - 0.20 * np.cos((4 * hb - 63) * RAD)
    u = (hb - 275) / 25
    dtheta = 30 * np.exp(-(u * u))
    cpb7 = _pow7(cpb)
    rc = 2 * np.sqrt(cpb7 / (cpb7 + P25_7))
    l2 = (lb - 50) * (lb - 50)
    sl = 1 + (0.015 * l2) / np.sqrt(20 + l2)
    sc = 1 + 0.045 * cpb
    sh = 1 + (0.015 * cpb) * t
    rt = -np.sin((2 * dtheta) * RAD) * rc
    x = dl / (kl * sl)
    y = dc / (kc * sc)
    w = dH / (kh * sh)
    r = ((x * x + y * y) + w * w) + (rt * y) * w
    if stats is not None:
        live = ~zero
        stats["hbar_mean"] = stats.get("hbar_mean", 0) + int((live & apart).sum())
        stats["hbar_plus"] = stats.get("hbar_plus", 0) + int((live & ~apart & (hs < 360)).sum())
        stats["hbar_minus"] = stats.get("hbar_minus", 0) + int((live & ~apart & ~(hs < 360)).sum())
        stats["dh_over"] = stats.get("dh_over", 0) + int((live & over).sum())
        stats["dh_under"] = stats.get("dh_under", 0) + int((live & under).sum())
        stats["cc_zero"] = stats.get("cc_zero", 0) + int(zero.sum())
        stats["identical"] = stats.get("identical", 0) + int(((L1 == L2) & (A1 == A2) & (B1 == B2)).sum())
        stats["gap"] = np.abs(np.abs(h1 - h2) - 180)
    return np.sqrt(np.where(r < 0, 0.0, r))


def near(gap):
    """Pixels whose hues are within 1e-9 degrees of 180 apart: either side of the jump is the device's to take."""
    return gap < 1e-9


def picture_lab(planes, fmt, depth, cdec, w, h, stats=None):
    """Steps 1 to 5 of a picture (Y, Cb, Cr) at the picture region w x h: 4:2:0 chroma sample (x >> 1, y >> 1) serves
    pixel (x, y)."""
    y, cb, cr = (samples(p, fmt, depth) for p in planes)
    y = y[:h, :w]
    if cdec:
        assert w % 2 == 0 and h % 2 == 0
        cb = np.repeat(np.repeat(cb[:h >> 1, :w >> 1], 2, axis=0), 2, axis=1)
        cr = np.repeat(np.repeat(cr[:h >> 1, :w >> 1], 2, axis=0), 2, axis=1)
    else:
        cb, cr = cb[:h, :w], cr[:h, :w]
    return rgb_lab(*ycc_rgb(y, cb, cr, depth), stats=stats)


def terms(src, rec, w, h, depth=8, cdec=1, src_fmt=SAMPLE_U8, rec_fmt=SAMPLE_U8, stats=None):
    """dE00 of every pixel of a picture pair, [h][w], and the same with the pixels near the jump on its other side."""
    st = {} if stats is None else stats
    lab1 = picture_lab(src, src_fmt, depth, cdec, w, h, st)
    lab2 = picture_lab(rec, rec_fmt, depth, cdec, w, h, st)
    one = de00(lab1, lab2, stats=st)
    mask = near(st["gap"])
    st["near"] = st.get("near", 0) + int(mask.sum())
    other = de00(lab1, lab2, flip=mask) if mask.any() else one
    return one, other


def score(total, w, h):
    """45 - 20 log10(sum/(w h)); +inf for identical pictures."""
    with np.errstate(divide="ignore"):
        return 45 - 20 * np.log10(np.float64(total) / (float(w) * float(h)))
