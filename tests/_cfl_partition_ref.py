"""Chroma-from-luma reference planes at a block-size map, from the oracle: od_resample_luma_coeffs
(odo_resample_luma_coeffs, pinned to the compiled reference by tests/test_oracle_golden.py) of every chroma leaf of
the encoder's walk (tests/_partition_ref.py::_walk), as od_block_encode calls it (src/encode.c:1681-1686): the chroma
leaf of size lv at chroma (y, x) is predicted from the luma area at (2y, 2x), and the luma MAP VALUE there chooses
between od_tf_up_hv_lp of four 4x4 blocks (0) and the upper-left quarter of one block (>= 1).

The case set serves tests/test_cfl_partition_host.py and tests/test_gpu_cfl_partition.py; every expected plane is
computed once and never written again.
"""
import ctypes
import functools

import numpy as np

import _partition_ref as R
from _libs import P, oracle

POISON = 0x5a5a5a5a
# (luma superblocks per row, the maps of the call's two frames)
CASES = [(nsbx, pair) for nsbx in (2, 3) for pair in (("mixed", "all4"), ("all64", "corners"), ("extremes", "units01"))]
CASE_IDS = ["%d-%s+%s" % (64 * nsbx, pair[0], pair[1]) for nsbx, pair in CASES]
NSBY = 2


@functools.lru_cache(maxsize=None)
def maps(nsbx):
    """Frame maps of nsbx x 2 superblocks: all five sizes mixed, 4x4 everywhere (the TF branch everywhere), 64x64
    everywhere, the deep corners, 4x4 against 64x64, and values 0 and 1 interleaved (the two kinds of 4x4 chroma leaf
    side by side)."""
    rng = np.random.RandomState(11 + nsbx)
    for _ in range(200):
        mixed = R.random_map(rng, nsbx, NSBY, 0.6)
        if R.leaf_sizes(mixed) == [0, 1, 2, 3, 4]:
            break
    assert R.leaf_sizes(mixed) == [0, 1, 2, 3, 4]
    out = {"mixed": mixed, "all4": R.uniform(0, nsbx, NSBY), "all64": R.uniform(4, nsbx, NSBY),
           "corners": R.corners(nsbx, NSBY), "extremes": R.extremes(nsbx, NSBY), "units01": R.units01(nsbx, NSBY)}
    for m in out.values():
        assert R.is_quadtree(m)
        m.setflags(write=False)
    return out


def leaves(bmap, dec, h, w):
    """[(y, x, lv, luma map value)] of the chroma (dec = 1) or luma (dec = 0) leaves of a plane of h x w."""
    found = []

    def leaf(y, x, lv):
        found.append((y, x, lv, int(bmap[(y << dec) >> 3, (x << dec) >> 3])))

    nothing = lambda *_: None  # noqa: E731
    R._walk(bmap, dec, w, h, w << dec, h << dec, leaf, nothing, nothing)
    return found


def expected(luma, bmap, dec):
    """The reference plane int32 [h >> dec][w >> dec] of one dequantised luma plane [h][w] at its map.  dec = 1:
    odo_resample_luma_coeffs per leaf.  dec = 0: od_resample_luma_coeffs copies the block (src/intra.c:97-108 with
    xdec = ydec = 0), leaf by leaf over a poisoned plane, so that the leaves must tile it."""
    o = oracle()
    luma = np.ascontiguousarray(luma, np.int32)
    h, w = luma.shape
    ch, cw = h >> dec, w >> dec
    out = np.full((ch, cw), POISON, np.int32)
    for y, x, lv, value in leaves(bmap, dec, ch, cw):
        n = 4 << lv
        if dec:
            pred = np.zeros((n, n), np.int32)
            area = ctypes.c_void_p(luma.ctypes.data + 4 * ((2 * y) * w + 2 * x))
            o.odo_resample_luma_coeffs(P(pred), n, area, w, lv, value)
            out[y:y + n, x:x + n] = pred
        else:
            out[y:y + n, x:x + n] = luma[y:y + n, x:x + n]
    return out


@functools.lru_cache(maxsize=None)
def case(index):
    """(luma int32 [2][128][64*nsbx], maps uint8 [2][16][8*nsbx], {dec: expected planes [2][..][..]}) of CASES[index].
    Luma: random in +-2^20, so that both arithmetic shifts of the TF branch see negative values and the products with
    OD_CFL_SCALING4 (<= 128 = 2^7, on sums of four inputs) stay below 2^30."""
    nsbx, pair = CASES[index]
    rng = np.random.RandomState(1000 + index)
    h, w = 64 * NSBY, 64 * nsbx
    luma = rng.randint(-(1 << 20), 1 << 20, size=(2, h, w)).astype(np.int32)
    bmaps = np.stack([maps(nsbx)[name] for name in pair])
    want = {dec: np.stack([expected(luma[f], bmaps[f], dec) for f in range(2)]) for dec in (0, 1)}
    for a in (luma, bmaps, want[0], want[1]):
        a.setflags(write=False)
    return luma, bmaps, want


def coverage():
    """What the case set reaches at dec = 1: {"tf": TF leaves, "copy4": quarter-copy 4x4 leaves, 8 / 16 / 32: leaves
    of that chroma size, "odd_negative": TF Haar groups whose ll - hh (after ll += lh, hh -= hl) is odd and
    negative - the case in which an arithmetic and a truncating shift differ}."""
    stats = {"tf": 0, "copy4": 0, 8: 0, 16: 0, 32: 0, "odd_negative": 0}
    for index in range(len(CASES)):
        luma, bmaps, _ = case(index)
        for f in range(2):
            h, w = luma[f].shape
            for y, x, lv, value in leaves(bmaps[f], 1, h // 2, w // 2):
                if lv:
                    stats[4 << lv] += 1
                elif value:
                    stats["copy4"] += 1
                else:
                    stats["tf"] += 1
                    a = luma[f, 2 * y:2 * y + 8, 2 * x:2 * x + 8].astype(np.int64)
                    ll = a[0:2, 0:2] + a[0:2, 4:6]
                    hh = a[4:6, 4:6] - a[4:6, 0:2]
                    d = ll - hh
                    stats["odd_negative"] += int(((d < 0) & ((d & 1) == 1)).sum())
    return stats
