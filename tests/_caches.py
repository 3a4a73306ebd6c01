"""ctypes prototypes of the two host caches the drop-in encoder talks to (the frame cache,
daala_amd/csrc/frame_cache.hip, and the deringing cache, daala_amd/csrc/dering_cache.hip),
for tests that call their entry points directly.

Both caches key on HOST ADDRESSES: an array handed to them must stay alive, and at the same
address, for the life of the cache.  `Pinned` keeps such arrays (nothing here reallocates or
copies them); tests write new contents into them in place."""
import ctypes

import numpy as np

EINVAL = -10          # ODHIP_EINVAL, include/daala_hip.h
NBSIZES = 5

vp = ctypes.c_void_p
ci = ctypes.c_int
cl = ctypes.c_long
cd = ctypes.c_double
plong = ctypes.POINTER(ctypes.c_long)

DCT_FN = ctypes.CFUNCTYPE(None, vp, ci, vp, ci)   # odhip_dct_func_2d(out, out_stride, in, in_stride)
DCT_TABLE = DCT_FN * NBSIZES


class BandCands(ctypes.Structure):
    """odhip_band_cands."""
    _fields_ = [("n", ci), ("q", ctypes.c_int32), ("beta", ctypes.c_int32), ("cg", ctypes.c_int32),
                ("gain", ctypes.c_int32 * 2), ("k", ctypes.c_int32 * 2), ("flags", ctypes.c_int32 * 2),
                ("dist0", cd), ("dist", cd * 2), ("y", ctypes.POINTER(ctypes.c_int16) * 2)]


_PROTOS = {
    # frame cache
    "odhip_cache_create": (vp, []),
    "odhip_cache_destroy": (None, [vp]),
    "odhip_cache_set_picture": (None, [vp, ci, ci]),
    "odhip_cache_make_current": (None, [vp]),
    "odhip_cache_plane_pixels": (ci, [vp, ci, ctypes.POINTER(vp), ctypes.POINTER(vp), ctypes.POINTER(ci),
                                      ctypes.POINTER(ci)]),
    "odhip_cache_load_plane": (ci, [vp, ci, vp, ci, ci, ci, ci]),
    "odhip_cache_lookup": (ci, [vp, vp, ci, ci, vp, ci]),
    "odhip_cache_stats": (None, [vp, plong, plong]),
    "odhip_install_cached_dct_vtbl": (None, [DCT_TABLE, DCT_TABLE]),
    "odhip_cache_load_bands": (ci, [vp, ci, vp, cd]),
    "odhip_cache_band": (ci, [vp, ci, ci, ci, ci, ci, vp, ctypes.POINTER(BandCands)]),
    "odhip_cache_band_stats": (None, [vp, plong, plong]),
    # deringing cache
    "odhip_dering_cache_create": (vp, []),
    "odhip_dering_cache_destroy": (None, [vp]),
    "odhip_dering_cache_begin": (None, [vp]),
    "odhip_dering_cache_call": (ci, [vp, vp, ci, vp, ci, ci, ci, ci, ci, ci, ci, ci, vp, ci, vp, ci, ci, ci, ci]),
    "odhip_dering_cache_stats": (None, [vp, plong, plong]),
    "odhip_dering_cache_set_source": (ci, [vp, vp, vp, ci, ci, ci]),
    "odhip_dering_cache_dist": (ci, [vp, vp, vp, ci, ci, ci, ci, ci, ci, ci, ctypes.POINTER(cd)]),
    "odhip_dering_cache_dist_served": (cl, [vp]),
}


def bind(L):
    """Set restype / argtypes of every cache entry point on the loaded library L; returns L."""
    for name, (res, args) in _PROTOS.items():
        fn = getattr(L, name)
        fn.restype = res
        fn.argtypes = args
    return L


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
