"""ctypes types and helpers for the two host caches the drop-in encoder talks to (the frame cache,
daala_amd/csrc/frame_cache.hip, and the deringing cache, daala_amd/csrc/dering_cache.hip),
for tests that call their entry points directly (on daala_amd.lib(), whose prototypes come
from the header, so raw host addresses pass as plain ints).

Both caches key on HOST ADDRESSES: an array handed to them must stay alive, and at the same
address, for the life of the cache.  `Pinned` keeps such arrays (nothing here reallocates or
copies them); tests write new contents into them in place."""
import ctypes
import os
import sys

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))  # run as a script: tests/ alone is on it
from daala_amd import _abi  # noqa: E402

EINVAL = -10          # ODHIP_EINVAL, include/daala_hip.h
NBSIZES = 5

vp = ctypes.c_void_p
ci = ctypes.c_int
cd = ctypes.c_double

DCT_FN = ctypes.CFUNCTYPE(None, vp, ci, vp, ci)   # odhip_dct_func_2d(out, out_stride, in, in_stride)
DCT_TABLE = DCT_FN * NBSIZES


BandCands = _abi.structs()["odhip_band_cands"]


def pulses(cands, slot, n):
    """The first n pulses of candidate `slot` of a BandCands: its y[slot] is an address into the cache."""
    return tuple(ctypes.cast(cands.y[slot], ctypes.POINTER(ctypes.c_int16))[:n])


def addr(a, *index):
    """The address of element a[index] of a numpy array (index may be shorter than a.ndim), as an
    int: pointer arithmetic in elements, never a copy."""
    off = sum(i * s for i, s in zip(index, a.strides))
    return a.ctypes.data + off


def pair(fn, c):
    """The two long counters of a *_stats entry point."""
    a, b = ctypes.c_long(-1), ctypes.c_long(-1)
    fn(c, ctypes.byref(a), ctypes.byref(b))
    return a.value, b.value


class Pinned:
    """Arrays whose addresses a cache keys on: created once, never reallocated, kept alive with
    the cache; new contents are written in place."""

    def __init__(self):
        self._keep = []

    def array(self, shape, dtype, fill=0):
        a = np.full(shape, fill, dtype)
        self._keep.append(a)
        return a

    def like(self, src):
        a = np.ascontiguousarray(src).copy()
        self._keep.append(a)
        return a
