"""The fixed picture pairs of the CIEDE2000 tests: tests/test_gpu_ciede.py runs them on the device, and
tests/test_ciede_host.py shows without one that together they reach every branch the device could get wrong.

A case is a dict: name, src and rec ((Y, Cb, Cr) numpy arrays [rows][stride], possibly views with a wider stride and an
unaligned first sample), w, h, depth, cdec, src_fmt, rec_fmt.  uint8 arrays hold SAMPLE_U8, int16 arrays SAMPLE_U16
samples at the depth or SAMPLE_I16_12 samples at 12 bits.  Nothing is larger than 66 x 50."""
import numpy as np

import _ciede_ref as R

U8, U16, I12 = R.SAMPLE_U8, R.SAMPLE_U16, R.SAMPLE_I16_12


def _noisy(rng, a, amp, top):
    return np.clip(a.astype(np.int64) + rng.randint(-amp, amp + 1, size=a.shape), 0, top)


def _random(name, seed, w, h, cdec, depth=8, src_fmt=U8, rec_fmt=U8, pad=0, amp=6):
    """A random picture and a noisy copy; chroma near grey and far from it, a few pixels left identical.  pad > 0: planes
    with `pad` more samples per row than the picture and a first sample `pad` rows and 1 + 2 pad samples into the buffer."""
    rng = np.random.RandomState(seed)
    top = (1 << depth) - 1
    cw, ch = w >> cdec, h >> cdec
    src = [rng.randint(0, top + 1, size=(h, w)), rng.randint(0, top + 1, size=(ch, cw)), rng.randint(0, top + 1, size=(ch, cw))]
    # a band of near-grey chroma: small C', every hue
    src[1][: max(1, ch // 3)] = (top + 1) // 2 + rng.randint(-3, 4, size=src[1][: max(1, ch // 3)].shape)
    src[2][: max(1, ch // 3)] = (top + 1) // 2 + rng.randint(-3, 4, size=src[2][: max(1, ch // 3)].shape)
    rec = [_noisy(rng, p, amp << (depth - 8), top) for p in src]
    # the last rows come back exactly
    for s, r in zip(src, rec):
        r[-1:] = s[-1:]

    def store(p, fmt):
        if fmt == I12:
            # 12-bit samples that round to p at the depth, some beyond the range so that the clamp works
            sh = 12 - depth
            v = (p << sh) + (rng.randint(-(1 << sh >> 1), (1 << sh >> 1), size=p.shape) if sh else 0)
            v = np.where(p == 0, v - rng.randint(0, 40, size=p.shape), v)
            v = np.where(p == top, v + rng.randint(0, 40, size=p.shape), v)
            a = v.astype(np.int16)
            assert (R.samples(a, I12, depth) == p).all()
        else:
            a = p.astype(np.uint8 if fmt == U8 else np.int16)
        if not pad:
            return np.ascontiguousarray(a)
        buf = rng.randint(0, 100, size=(a.shape[0] + 2 * pad, a.shape[1] + 1 + 3 * pad)).astype(a.dtype)
        view = buf[pad:pad + a.shape[0], 1 + 2 * pad:1 + 2 * pad + a.shape[1]]
        view[...] = a
        return view

    return dict(name=name, w=w, h=h, depth=depth, cdec=cdec, src_fmt=src_fmt, rec_fmt=rec_fmt,
                src=[store(p, src_fmt) for p in src], rec=[store(p, rec_fmt) for p in rec])


def _corners():
    """Every combination of 0 / 16 / 128 / 235 / 255 in Y, Cb and Cr, against five other ones each (625 pixels, 25 x 25):
    out of gamut, negative R, G, B and X, Y, Z; the first 125 pixels come back exactly."""
    v = np.array([0, 16, 128, 235, 255])
    p = np.arange(625)
    idx, r = p % 125, p // 125
    to = (idx * np.array([1, 7, 13, 32, 57])[r] + np.array([0, 1, 31, 3, 77])[r]) % 125
    planes = lambda i: [a.reshape(25, 25).astype(np.uint8) for a in (v[i // 25], v[(i // 5) % 5], v[i % 5])]
    return dict(name="corners-444-25x25", w=25, h=25, depth=8, cdec=0, src_fmt=U8, rec_fmt=U8, src=planes(idx),
                rec=planes(to))


def _grey():
    """Grey pictures (Cb = Cr = 128) whose source luma is the column and whose reconstruction's is the row, 0..24: pairs on
    either side of Y = 16 have opposite hues, Y = 16 itself has no chroma at all, the diagonal is identical.
    Up to Y = 24 every channel takes the linear branch of step 3 and every X, Y, Z the linear branch of f, so Lab is plain
    arithmetic and a device's hues differ from the restatement's by the last bits of atan2 alone (~1e-13 degrees): a
    pixel is on the same side of the 1e-9 degree window around the jump for both (tests/test_ciede_host.py shows that
    none lies within 1e-12 of the window's edge).  From Y = 25 on pow enters; one ulp of it moves a chroma of 1e-4 by
    parts in 1e10 and the hue by several 1e-9 degrees, more than that window."""
    y = np.arange(25)
    g = np.full((25, 25), 128, np.uint8)
    src = [np.tile(y, (25, 1)).astype(np.uint8), g, g.copy()]
    rec = [np.tile(y[:, None], (1, 25)).astype(np.uint8), g.copy(), g.copy()]
    return dict(name="grey-444-25x25", w=25, h=25, depth=8, cdec=0, src_fmt=U8, rec_fmt=U8, src=src, rec=rec)


def cases():
    return [
        _random("420-u8-64x48", 1, 64, 48, 1),
        _random("420-u8-2x2", 2, 2, 2, 1),
        _random("444-u8-1x1", 3, 1, 1, 0),
        _random("444-u8-37x23", 4, 37, 23, 0),
        _random("420-u8-66x50", 5, 66, 50, 1),
        _random("420-u16-10bit-34x18", 6, 34, 18, 1, depth=10, src_fmt=U16, rec_fmt=U16),
        _random("420-u8-vs-i12-8bit-34x18", 7, 34, 18, 1, depth=8, src_fmt=U8, rec_fmt=I12),
        _random("444-u16-vs-i12-10bit-19x34", 8, 19, 34, 0, depth=10, src_fmt=U16, rec_fmt=I12),
        _random("420-i12-vs-u16-12bit-34x18", 9, 34, 18, 1, depth=12, src_fmt=I12, rec_fmt=U16),
        _random("420-u8-strided-38x34", 10, 38, 34, 1, pad=3),
        _random("444-u16-strided-12bit-33x9", 11, 33, 9, 0, depth=12, src_fmt=U16, rec_fmt=U16, pad=2),
        _corners(),
        _grey(),
    ]


def restated(case, stats=None):
    """(terms, terms on the other side of the jump where near it) of a case."""
    return R.terms(case["src"], case["rec"], case["w"], case["h"], case["depth"], case["cdec"], case["src_fmt"],
                   case["rec_fmt"], stats=stats)
