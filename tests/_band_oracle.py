"""The oracle's pvq_theta trace of ONE band coded without a reference vector (the path the
no-reference band stage restates): the ctypes class of odo_pvq_band_trace and the call that
fills it.  Shared by tests/test_gpu_pvq_bands.py (the band stage itself) and
tests/test_gpu_frame_cache.py (the band stage behind the frame cache)."""
import ctypes
import os
import sys

import numpy as np

from _libs import P, ROOT, oracle

sys.path.insert(0, ROOT)         # a test module run as a script has tests/ on its path, not the root
from daala_amd import _abi  # noqa: E402

cd = ctypes.c_double


# odo_pvq_cand and odo_pvq_band_trace, as oracle/od_oracle.h lays them out
_ODO_H = os.path.join(ROOT, "oracle", "od_oracle.h")
Cand, Trace = _abi.structs(_ODO_H)["odo_pvq_cand"], _abi.structs(_ODO_H)["odo_pvq_band_trace"]
MAXN = _abi.constants(_ODO_H)["ODO_MAX_PVQ_SIZE"]


def block_vector(coef, n, bx, by):
    """Block (bx, by) of side n of the int32 plane `coef`, in coding order."""
    w = coef.shape[1]
    vec = np.zeros(n * n, np.int32)
    oracle().odo_raster_to_coding_order(P(vec), n, ctypes.c_void_p(
        coef.ctypes.data + 4 * (by * n * w + bx * n)), w)
    return vec


def band_trace(x0, q, beta, qm, qmi, lam):
    """odo_pvq_theta on the band x0 (int32, coding order) with a null reference vector, step q,
    beta (Q12), the band's slices of the quantisation matrix and its inverse, and lambda:
    (the Trace, its no-reference candidates in the order pvq_theta tried them)."""
    m = len(x0)
    x0 = np.ascontiguousarray(x0, np.int32)
    r0 = np.zeros(m, np.int32)
    out = np.zeros(m, np.int32)
    y = np.zeros(m, np.int32)
    i1, i2, i3 = ctypes.c_int(), ctypes.c_int(), ctypes.c_int()
    sd = cd(0)
    tr = Trace()
    qq = np.ascontiguousarray(qm)
    qi = np.ascontiguousarray(qmi)
    oracle().odo_pvq_theta(P(out), P(x0), P(r0), m, int(q), P(y), ctypes.byref(i1),
                           ctypes.byref(i2), ctypes.byref(i3), int(beta),
                           ctypes.byref(sd), 1, 1, 0, P(qq), P(qi), cd(lam), 1,
                           ctypes.byref(tr))
    nr = [tr.cands[i] for i in range(tr.ncands) if not tr.cands[i].with_ref]
    assert len(nr) in (1, 2)
    return tr, nr
