"""Plane sets in a strided, sentinel-surrounded layout, for tests that hand the C entry points
something else than packed planes on a fresh allocation.

A PlaneSet is ONE flat buffer (a CUDA tensor, or a numpy array with device=None for host code such
as the oracle) filled with a sentinel, longer than the planes need at both ends.  Sample (x, y) of
plane p is element  LEAD + base + p*plane_stride + y*stride + x;  everything that is not such an
element for x < w, y < h must still hold the sentinel after a call that only writes the windows.
Strides, the base offset and the plane pitch count samples of the set's type; the allocation itself
is 256-byte aligned and LEAD keeps that alignment, so `base` is the offset from a 256-byte boundary.
"""
import ctypes

import numpy as np

SENTINEL = {np.dtype(np.uint8): 0xA5, np.dtype(np.int16): 0x5AA5, np.dtype(np.int32): 0x5AA55AA5}
LEAD = 256       # elements in front of the base (a multiple of 256 bytes for every type)
TAIL = 256

# name -> (stride - w, base offset, plane_stride - stride*h), see the table of layouts in
# test_gpu_plane_layouts.py
LAYOUTS = {"packed": (0, 0, 0), "gap16": (16, 16, 16), "min4": (4, 4, 4), "pitch4": (16, 0, 4)}


class PlaneSet:
    def __init__(self, nplanes, h, w, dtype, stride=None, base=0, plane_stride=None, device="cuda"):
        self.nplanes, self.h, self.w = int(nplanes), int(h), int(w)
        self.dtype = np.dtype(dtype)
        self.stride = self.w if stride is None else int(stride)
        self.base = int(base)
        self.plane_stride = self.stride * self.h if plane_stride is None else int(plane_stride)
        self.sentinel = SENTINEL[self.dtype]
        self.size = LEAD + self.base + (self.nplanes - 1) * self.plane_stride + self.stride * self.h + TAIL
        self.device = device
        host = np.full(self.size, self.sentinel, self.dtype)
        if device is None:
            self.buf = host
        else:
            import torch
            self.buf = torch.from_numpy(host).to(device)
            assert self.buf.data_ptr() % 256 == 0

    @classmethod
    def in_layout(cls, name, nplanes, h, w, dtype, device="cuda"):
        ds, base, dp = LAYOUTS[name]
        return cls(nplanes, h, w, dtype, w + ds, base, (w + ds) * h + dp, device)

    @property
    def ptr(self):
        """The base pointer: sample (0, 0) of plane 0."""
        addr = self.buf.ctypes.data if self.device is None else self.buf.data_ptr()
        return ctypes.c_void_p(addr + (LEAD + self.base) * self.dtype.itemsize)

    @property
    def pitch(self):
        return ctypes.c_long(self.plane_stride)

    def _index(self, w=None, h=None):
        w = self.w if w is None else w
        h = self.h if h is None else h
        p, y, x = np.ogrid[0:self.nplanes, 0:h, 0:w]
        return LEAD + self.base + p * self.plane_stride + y * self.stride + x

    def _host(self):
        return self.buf if self.device is None else self.buf.cpu().numpy()

    def write(self, data):
        """[nplanes][h][w] samples into the windows; the rest of the buffer keeps what it holds."""
        data = np.asarray(data)
        assert data.shape == (self.nplanes, self.h, self.w) and data.dtype == self.dtype, (data.shape, data.dtype)
        host = self._host().copy()
        host[self._index()] = data
        if self.device is None:
            self.buf[:] = host
        else:
            import torch
            self.buf.copy_(torch.from_numpy(host))
        return self

    def read(self):
        """The windows as [nplanes][h][w]."""
        return np.ascontiguousarray(self._host()[self._index()])

    def intact(self, w=None, h=None):
        """True when every element outside the [p][y < h][x < w] windows still holds the sentinel
        (w, h: windows other than the set's own, for the helper's self-test)."""
        host = self._host()
        outside = np.ones(self.size, bool)
        outside[self._index(w, h).ravel()] = False
        return bool((host[outside] == self.dtype.type(self.sentinel)).all())
