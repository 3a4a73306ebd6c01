"""Shared inputs of the block-size decision tests (test_bsize_host.py, test_bsize_ref.py, test_gpu_bsize.py):
the named cases, the compiled reference called cell by cell, and the recorded fixture tests/golden/bsize.npz
(tools/gen_bsize_golden.py writes it from the compiled reference)."""
import ctypes
import os

import numpy as np

from _libs import GOLDEN, P, synth_frame

FIXTURE = os.path.join(GOLDEN, "bsize.npz")
BORDER = 6          # OD_BLOCK_OFFSET: samples before and after a cell on each axis
NOISE, PSY = 90, 85  # what od_block_size_comp keeps per cell: noise4_4 .. noise8_32, psy4 .. psy32
# od_block_size_comp (src/block_size_enc.h:86-113): two od_superblock_stats of 3056 int32 each, res[44][44]
NOISE_AT = 2 * 3056 * 4 + 44 * 44
PSY_AT = NOISE_AT + NOISE * 4
TEX_Q = (0, 160, 800, 4000)


def tex():
    """128 x 96: flat ramp on the left, +-60 noise on the right - all four sizes as a keyframe."""
    rng = np.random.RandomState(7)
    yy, xx = np.mgrid[0:96, 0:128]
    return np.clip(128 + rng.randint(-60, 61, (96, 128)) * (xx > 64) + yy // 2, 0, 255).astype(np.uint8)


def _checker(h, w):
    yy, xx = np.mgrid[0:h, 0:w]
    return (((yy + xx) & 1) * 255).astype(np.uint8)


def cases():
    """{name: (px, pred or None, (quantisers))}, px and pred uint8 [h, w]."""
    t = tex()
    s0 = synth_frame(128, 96)[0]
    s3 = synth_frame(128, 96, phase=3)[0]
    rng = np.random.RandomState(19)
    cell = np.clip(128 + rng.randint(-90, 91, (32, 32)) * (np.mgrid[0:32, 0:32][0] > 13), 0, 255).astype(np.uint8)
    wide = np.ascontiguousarray(t[40:72, 40:104])
    return {
        "tex": (t, None, TEX_Q),
        "tex_inter": (t, s0, (800, 4000)),
        "synth_inter": (s0, s3, (160, 800, 4000)),
        "cell": (cell, None, (0, 800)),
        "cell_inter": (cell, np.ascontiguousarray(cell[::-1]), (800,)),
        "wide": (wide, None, (800,)),
        "zeros": (np.zeros((32, 64), np.uint8), None, (800,)),
        "full": (np.full((32, 64), 255, np.uint8), None, (800,)),
        "checker": (_checker(32, 64), None, (800,)),
        "same_pred": (wide, wide.copy(), (800,)),
        "hi_lo": (np.full((32, 32), 255, np.uint8), np.zeros((32, 32), np.uint8), (800,)),
        "lo_hi": (np.zeros((32, 32), np.uint8), np.full((32, 32), 255, np.uint8), (800,)),
    }


def case_ids():
    return [(name, q) for name, (_, _, qs) in cases().items() for q in qs]


def ref_decide(R, px, pred, q):
    """od_split_superblock (src/block_size_enc.c:331-456) of every 32x32 cell of px on the edge-padded picture:
    (map uint8 [h/8, w/8], noise int32 [h/32, w/32, 90], psy float32 [h/32, w/32, 85])."""
    h, w = px.shape
    ppx = np.ascontiguousarray(np.pad(px, BORDER, mode="edge"))
    ppred = None if pred is None else np.ascontiguousarray(np.pad(pred, BORDER, mode="edge"))
    stride = w + 2 * BORDER
    bmap = np.zeros((h // 8, w // 8), np.uint8)
    noise = np.zeros((h // 32, w // 32, NOISE), np.int32)
    psy = np.zeros((h // 32, w // 32, PSY), np.float32)
    scratch = np.zeros(65536, np.uint8)
    fn = R.od_split_superblock
    fn.restype = None
    fn.argtypes = [ctypes.c_void_p, ctypes.c_void_p, ctypes.c_int, ctypes.c_void_p, ctypes.c_int, ctypes.c_void_p,
                   ctypes.c_int]
    for cy in range(h // 32):
        for cx in range(w // 32):
            at = (cy * 32 + BORDER) * stride + cx * 32 + BORDER
            dec = np.full((8, 8), -1, np.int32)          # int bsize[OD_BSIZE_GRID][OD_BSIZE_GRID]
            scratch[:] = 0
            fn(P(scratch), ppx.ctypes.data + at, stride, None if ppred is None else ppred.ctypes.data + at, stride,
               P(dec), int(q))
            bmap[cy * 4:cy * 4 + 4, cx * 4:cx * 4 + 4] = dec[:4, :4]
            noise[cy, cx] = scratch[NOISE_AT:NOISE_AT + NOISE * 4].view(np.int32)
            psy[cy, cx] = scratch[PSY_AT:PSY_AT + PSY * 4].view(np.float32)
    return bmap, noise, psy


_fixture = {}


def expected(name, q):
    """(map, noise [.., 90], psy [.., 85]) of a case as recorded from the compiled reference."""
    if not _fixture:
        with np.load(FIXTURE) as z:
            _fixture.update({k: z[k] for k in z.files})
    key = "%s_q%d" % (name, q)
    return _fixture[key + "_map"], _fixture[key + "_noise"], _fixture[key + "_psy"]


def same_bits(a, b):
    """Bit-for-bit equality of two float32 arrays (a NaN or a signed zero would not hide)."""
    return np.array_equal(np.ascontiguousarray(a, np.float32).view(np.uint32),
                          np.ascontiguousarray(b, np.float32).view(np.uint32))
