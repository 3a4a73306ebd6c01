"""The directed corpus (tests/_pvq_corpus.py) through pvq_theta band by band: the table sets, the
(matrix, mode, band size, case, quantiser) runs in a fixed order, and the call itself for the
oracle (with its trace) or the compiled reference.  Shared by tests/test_pvq_corpus_host.py,
tests/test_gpu_pvq_corpus.py and tools/make_golden_pvq_corpus.py."""
import ctypes
import os
import zlib

import numpy as np

import _pvq_corpus as C
from _band_oracle import Trace
from _libs import GOLDEN, P

cd = ctypes.c_double
LAMBDA = 0.147
MODES = [(1, 1), (0, 0), (0, 1), (1, 0)]      # (is_keyframe, pli), as tests/test_gpu_pvq_refbands.py
# the flat matrix runs in the two modes that differ most: chroma from luma and inter luma
MATRIX_MODES = {"hvs": MODES, "flat": [(1, 1), (0, 0)]}
BS = 2                                        # the 16x16 block: it has a band of every size
BAND_INDEX = {15: 0, 8: 1, 32: 3, 128: 6}

_tables = {}


def tables():
    if not _tables:
        g = np.load(os.path.join(GOLDEN, "quant_v20.npz"))
        for k in ("qm", "qm_inv", "qm_flat", "qm_inv_flat", "qm_offset", "beta"):
            _tables[k] = g[k]
    return _tables


_slices = {}


def band_setup(matrix, pli, n):
    """(qm, qm_inv, beta, cases) of the band of n coefficients of a 16x16 block of plane pli."""
    key = (matrix, 1 if pli else 0, n)
    if key not in _slices:
        t = tables()
        a = int(t["qm_offset"][BS, key[1]]) + C.BAND_START[n]
        sfx = "_flat" if matrix == "flat" else ""
        qm = np.ascontiguousarray(t["qm" + sfx][a:a + n])
        qmi = np.ascontiguousarray(t["qm_inv" + sfx][a:a + n])
        _slices[key] = (qm, qmi, C.cases(n, qm))
    qm, qmi, cs = _slices[key]
    return qm, qmi, int(tables()["beta"][1, pli, BS, BAND_INDEX[n]]), cs


def runs():
    """Every comparison of the corpus, in the fixture's order:
    (matrix, is_keyframe, pli, n, name, x0, r0, q0, beta, qm, qm_inv)."""
    for matrix in ("hvs", "flat"):
        for kf, pli in MATRIX_MODES[matrix]:
            for n in C.SIZES:
                qm, qmi, beta, cs = band_setup(matrix, pli, n)
                for name, _, x0, r0 in cs:
                    for q0 in C.quantizers_for(n, x0):
                        yield matrix, kf, pli, n, name, x0, r0, q0, beta, qm, qmi


def inputs_digest():
    c = 0
    for matrix in ("hvs", "flat"):
        for dec in (0, 1):
            for n in C.SIZES:
                c = zlib.crc32(np.uint32(C.digest(band_setup(matrix, dec, n)[3])).tobytes(), c)
    return c


def theta(fn, x0, r0, n, q0, beta, kf, pli, qm, qmi, trace=None):
    """pvq_theta through fn (odo_pvq_theta with trace = a Trace or None passed on; ref_pvq_theta with
    trace = False).  Returns dict(ret, itheta, max_theta, k, skip_diff, out, y)."""
    out = np.zeros(n, np.int32)
    y = np.zeros(n, np.int32)
    i1, i2, i3 = ctypes.c_int(), ctypes.c_int(), ctypes.c_int()
    sd = cd(0)
    x0 = np.ascontiguousarray(x0, np.int32)
    r0 = np.ascontiguousarray(r0, np.int32)
    args = [P(out), P(x0), P(r0), n, int(q0), P(y), ctypes.byref(i1), ctypes.byref(i2), ctypes.byref(i3),
            int(beta), ctypes.byref(sd), 1, kf, pli, P(qm), P(qmi), cd(LAMBDA), 1]
    if trace is not False:
        args.append(ctypes.byref(trace) if trace is not None else None)
    ret = fn(*args)
    return dict(ret=ret, itheta=i1.value, max_theta=i2.value, k=i3.value, skip_diff=sd.value, out=out, y=y)


def new_trace():
    return Trace()


FIELDS = ("ret", "itheta", "max_theta", "k", "crc_out", "crc_y")


def record(res):
    return (res["ret"], res["itheta"], res["max_theta"], res["k"],
            zlib.crc32(res["out"].astype("<i4").tobytes()), zlib.crc32(res["y"].astype("<i4").tobytes()))
