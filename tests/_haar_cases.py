"""The fixed inputs of the Haar-wavelet tests and what tests/_haar_ref.py makes of them, computed once per process.

tests/test_gpu_haar.py runs the device on these; tests/test_haar_ref.py checks, without a GPU, that they reach what
they are there to reach (rounding ties, every DC-predictor case, the dead zone from both sides, both clamps ...), so
that the GPU comparison cannot pass on inputs that decide nothing.

Frames are 3 x 2 superblocks (luma 192x128, 4:2:0 chroma 96x64): the smallest grid with all five DC-predictor cases
and interior blocks both ways; one family has a single superblock.  A luma set holds two frames' planes, a chroma set
Cb, Cb, Cr, Cr with one dc_quant per half."""
import collections
import functools

import numpy as np

import _haar_ref as R
from _libs import synth_frame

NSBX, NSBY = 3, 2
PIC = {0: (160, 106), 1: (80, 53)}            # inter picture sizes, in plane samples
QUANT_ALL_ZERO = 1 << 19                      # above twice any coefficient of 8-bit content: every AC rounds to 0

# name: fpr (int16 samples at 12 bits), depth, quant (0 = lossless), inter, superblocks across / down
Case = collections.namedtuple("Case", "name fpr depth quant inter nsbx nsby")
CASES = [
    Case("key-u8-lossless", False, 8, 0, False, NSBX, NSBY),
    Case("key-fpr8-lossless", True, 8, 0, False, NSBX, NSBY),
    Case("key-fpr10-lossless", True, 10, 0, False, NSBX, NSBY),
    Case("key-fpr12-lossless", True, 12, 0, False, NSBX, NSBY),
    Case("key-u8-q16", False, 8, 16, False, NSBX, NSBY),
    Case("key-u8-q183", False, 8, 183, False, NSBX, NSBY),
    Case("key-u8-qzero", False, 8, QUANT_ALL_ZERO, False, NSBX, NSBY),
    Case("key-fpr12-q16", True, 12, 16, False, NSBX, NSBY),
    Case("key-u8-q16-1x1", False, 8, 16, False, 1, 1),
    Case("inter-u8-lossless", False, 8, 0, True, NSBX, NSBY),
    Case("inter-u8-q16", False, 8, 16, True, NSBX, NSBY),
    Case("inter-u8-q183", False, 8, 183, True, NSBX, NSBY),
    Case("inter-fpr10-lossless", True, 10, 0, True, NSBX, NSBY),
    Case("inter-fpr12-q16", True, 12, 16, True, NSBX, NSBY),
]
BY_NAME = {c.name: c for c in CASES}
CASE_IDS = [c.name for c in CASES]


def dc_quants(case, dec):
    """What the caller hands over (src/encode.c:1555-1559, :1330-1335 compute it from the quantiser and a matrix that
    is not this path's business): 1 when lossless; otherwise steps that put the inter DCs of these inputs on both sides
    of the dead zone, Cb and Cr apart."""
    if case.quant == 0:
        return (1, 1)
    if case.quant == QUANT_ALL_ZERO:
        return (3, 3)
    return ((500, 500), (300, 200))[dec]


def plane_split(dec):
    return 2 if dec else 1


def _plane(dec, fpr, nsbx, nsby, variant):
    """One plane of noisy pixels with saturated patches at both ends of the range, as tests/test_gpu_forward_partition.py
    builds them."""
    h, w = (nsby * 64) >> dec, (nsbx * 64) >> dec
    rng = np.random.RandomState(4000 * dec + 100 * variant + 7 * int(fpr) + nsbx)
    base = synth_frame(max(w << dec, 64), max(h << dec, 64), seed=83 + variant)[1 if dec else 0].astype(np.int32)
    base = base[:h, :w]
    if variant & 1:
        base = base[::-1, ::-1]
    px = np.clip(base + rng.randint(-60, 61, size=base.shape), 0, 255)
    px[:8, :8] = 255
    px[8:16, :8] = 0
    px[h - 8:, w - 16:w - 8] = 0
    px[h - 8:, w - 8:] = 255
    if fpr:
        px = np.clip((px << 4) + rng.randint(0, 16, size=px.shape), 0, 4095)
        px[:8, :8] = 4095
        px[h - 8:, w - 8:] = 4095
    return px.astype(np.int16 if fpr else np.uint8)


@functools.lru_cache(maxsize=None)
def source(name, dec):
    """[2 or 4][h][w]: two frames' luma planes, or Cb, Cb, Cr, Cr."""
    c = BY_NAME[name]
    px = np.stack([_plane(dec, c.fpr, c.nsbx, c.nsby, v) for v in range(4 if dec else 2)])
    px.setflags(write=False)
    return px


@functools.lru_cache(maxsize=None)
def prediction(name, dec):
    """The source plus a smooth offset field of -1 .. 2 sample steps (whole steps of 16 at 12 bits): superblock means
    between the integers, so that |DC difference| lands on both sides of dc_quant*141/256."""
    c = BY_NAME[name]
    if not c.inter:
        return None
    px = source(name, dec).astype(np.int32)
    _, h, w = px.shape
    yy, xx = np.mgrid[0:h, 0:w]
    off = (5 * xx // w + 3 * yy // h) // 2 - 1
    pred = np.clip(px + off[None] * (16 if c.fpr else 1), 0, 4095 if c.fpr else 255).astype(source(name, dec).dtype)
    pred.setflags(write=False)
    return pred


def picture(name, dec):
    c = BY_NAME[name]
    _, h, w = source(name, dec).shape
    return PIC[dec] if c.inter else (w, h)


Want = collections.namedtuple("Want", "q tree dc_rec rec stats")


@functools.lru_cache(maxsize=None)
def want(name, dec):
    """tests/_haar_ref.py::encode_planes of the case's plane set, with the statistics of what it met."""
    c = BY_NAME[name]
    stats = R.new_stats()
    pw, ph = picture(name, dec)
    out = R.encode_planes(source(name, dec), prediction(name, dec), dec, pw, ph, c.depth, c.quant, dc_quants(c, dec),
                          plane_split(dec), stats)
    for a in out:
        a.setflags(write=False)
    return Want(*out, stats)


def transform_inputs(ln, seed=5):
    """int32 [3][4n][4n] for the bare transforms: random values of either sign up to 2^17 in magnitude, +-2^17 themselves
    and odd values among them."""
    n = 1 << ln
    rng = np.random.RandomState(seed + ln)
    x = rng.randint(-(1 << 17), (1 << 17) + 1, size=(3, 4 * n, 4 * n)).astype(np.int32)
    x[0, :2, :2] = [[1 << 17, -(1 << 17)], [-(1 << 17), 1 << 17]]
    x[1, :n, :n] = 1 << 17
    x[1, n:2 * n, :n] = -(1 << 17)
    x[2] |= 1
    x.setflags(write=False)
    return x


def tree_violations(q, tree, ln):
    """Entries of `tree` that are not what od_compute_max_tree makes of its neighbours: a parent its own magnitude plus
    its four children, a finest-level entry its magnitude, a DC slot the three roots' sum (src/encode.c:899-919, :1033)."""
    n = 1 << ln
    half = n // 2
    nplanes, h, w = q.shape

    def blocks(a):
        return a.astype(np.int64).reshape(nplanes, h // n, n, w // n, n).transpose(0, 1, 3, 2, 4)

    t = blocks(tree)
    expect = np.abs(blocks(q))
    expect[..., :half, :half] += t[..., 0::2, 0::2] + t[..., 0::2, 1::2] + t[..., 1::2, 0::2] + t[..., 1::2, 1::2]
    expect[..., 0, 0] = t[..., 0, 1] + t[..., 1, 0] + t[..., 1, 1]
    return int((expect != t).sum())
