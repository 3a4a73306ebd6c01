"""The oracle's pvq_theta trace of ONE band coded without a reference vector (the path the
no-reference band stage restates): the ctypes mirror of odo_pvq_band_trace and the call that
fills it.  Shared by tests/test_gpu_pvq_bands.py (the band stage itself) and
tests/test_gpu_frame_cache.py (the band stage behind the frame cache)."""
import ctypes

import numpy as np

from _libs import P, oracle

cd = ctypes.c_double
MAXN = 128


class Cand(ctypes.Structure):
    _fields_ = [("with_ref", ctypes.c_int32), ("gain", ctypes.c_int32),
                ("theta", ctypes.c_int32), ("ts", ctypes.c_int32), ("k", ctypes.c_int32),
                ("qcg", ctypes.c_int32), ("qtheta", ctypes.c_int32),
                ("searched", ctypes.c_int32), ("cos_dist", ctypes.c_double),
                ("dist", ctypes.c_double), ("y", ctypes.c_int32 * MAXN)]


class Trace(ctypes.Structure):
    _fields_ = [("xshift", ctypes.c_int32), ("rshift", ctypes.c_int32),
                ("g", ctypes.c_int32), ("gr", ctypes.c_int32), ("cg", ctypes.c_int32),
                ("cgr", ctypes.c_int32), ("icgr", ctypes.c_int32),
                ("gain_offset", ctypes.c_int32), ("m", ctypes.c_int32), ("s", ctypes.c_int32),
                ("theta", ctypes.c_int32), ("corr", ctypes.c_double),
                ("dist0", ctypes.c_double), ("skip_dist", ctypes.c_double),
                ("x16", ctypes.c_int16 * MAXN), ("r16", ctypes.c_int16 * MAXN),
                ("ncands", ctypes.c_int32), ("cands", Cand * 24)]


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
