"""MS-SSIM without a GPU: the restatement (tests/_msssim_ref.py) against what the reference's dump_msssim printed
(tests/golden/msssim.npz, tools/make_golden_msssim.py), and the host-only entry points against the restatement.

- every printed line of every golden clip, dB and raw (-r), is reproduced as a string;
- odhip_msssim_taps, built by the host libm, equals the restatement's table and (it compares them itself) the nine
  values the kernels compile in;
- odhip_msssim_weights equals the restatement's sums of the weight moment (16 x 16, where scale 4 is one sample; odd
  sizes; 1920 x 1080);
- odhip_msssim_score equals the restatement's product; a negative sum gives NaN, as the tool prints.  A sum of exactly
  zero gives 0, not NaN: the tool's pow(0, positive) is 0 and the score is not special-cased (the issue's "a sum <= 0
  gives NaN" holds for every negative sum; at exactly 0 the tool's own value wins);
- sizes below 16 or above 65535 and NULL arrays are refused;
- the C ABI carries the new symbols and the Python mirror the new flag."""
import ctypes
import math
import os
import sys

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))

import _msssim_ref as S  # noqa: E402


@pytest.fixture(scope="module")
def D():
    import daala_amd
    return daala_amd


@pytest.mark.parametrize("idx", range(len(S.CASES)), ids=[c[0] for c in S.CASES])
def test_restatement_prints_the_tool_lines(idx):
    g = np.load(os.path.join(ROOT, "tests", "golden", "msssim.npz"))
    case = S.CASES[idx]
    assert str(g["names"][idx]) == case[0]
    assert S.restated_lines(case) == str(g["msssim"][idx]).splitlines()
    assert S.restated_lines(case, raw=True) == str(g["msssim_raw"][idx]).splitlines()


def test_taps(D):
    assert S.TAPS == [8, 37, 112, 218, 274, 218, 112, 37, 8] and sum(S.TAPS) == 1024
    # the library builds them with the host libm and compares them with its compile-time table itself: 0, not ODHIP_EIMPL
    buf = (ctypes.c_uint32 * 9)()
    assert D.lib().odhip_msssim_taps(buf) == 0 and list(buf) == S.TAPS
    assert D.msssim_taps() == S.TAPS
    assert D.lib().odhip_msssim_taps(None) == -10


def test_weights(D):
    for w, h in ((16, 16), (17, 31), (77, 53), (45, 39), (49, 35), (33, 65), (130, 70), (1920, 1080), (65535, 16)):
        assert D.msssim_weights(w, h) == S.weights(w, h), (w, h)
    # the weight really is the sum of the weight moment of every sample of every scale
    z = np.zeros((39, 45), np.int64)
    assert S.weights(45, 39) == [int(S.moments(a, a)[5].sum()) for a in S.pyramid(z)]
    assert S.weights(16, 16)[4] == 274 * 274                                # one sample: the centre taps
    L = D.lib()
    wt = (ctypes.c_int64 * 5)()
    for w, h in ((15, 64), (64, 15), (65536, 64), (64, 65536), (0, 0)):
        assert L.odhip_msssim_weights(w, h, wt) == -10
    assert L.odhip_msssim_weights(64, 64, None) == -10


def test_score(D):
    L = D.lib()
    wt = np.array(S.weights(77, 53), np.int64)
    rng = np.random.RandomState(5)
    for _ in range(8):
        sums = wt * (0.8 + 0.2 * rng.rand(5))
        assert D.msssim_score(sums, wt, raw=True) == S.score(sums, wt)
        assert D.msssim_score(sums, wt) == pytest.approx(S.convert(S.score(sums, wt), 1), rel=1e-14)
    sums = wt * 0.9
    for sc in range(5):
        neg = sums.copy()
        neg[sc] = -neg[sc]
        assert math.isnan(D.msssim_score(neg, wt, raw=True)) and math.isnan(S.score(neg, wt))
        zero = sums.copy()
        zero[sc] = 0.0
        assert D.msssim_score(zero, wt, raw=True) == S.score(zero, wt) == 0.0
    many = D.msssim_score(np.stack([sums, sums * 0.5]), wt, raw=True)
    assert many.shape == (2,) and many[0] == S.score(sums, wt) and many[1] == S.score(sums * 0.5, wt)
    out = ctypes.c_double()
    p = lambda a: a.ctypes.data_as(ctypes.c_void_p)
    assert L.odhip_msssim_score(None, p(wt), ctypes.byref(out)) == -10
    assert L.odhip_msssim_score(p(sums), None, ctypes.byref(out)) == -10
    assert L.odhip_msssim_score(p(sums), p(wt), None) == -10
    assert L.odhip_msssim_score(p(sums), p(np.zeros(5, np.int64)), ctypes.byref(out)) == -10


def test_refusals_before_any_device_work(D):
    """Arguments are checked before a context or a device is looked for: these answer without a GPU."""
    from daala_amd.api import _MetricsPair
    L = D.lib()
    buf = np.zeros(64 * 64, np.uint8)
    out = np.zeros(10, np.float64)
    po = out.ctypes.data_as(ctypes.c_void_p)

    def pair(w, h, depth=8, fmt=0):
        return _MetricsPair(buf.ctypes.data, buf.ctypes.data, fmt, fmt, 64, 64, w, h, depth, 0)

    for bad in (pair(15, 64), pair(64, 15), pair(64, 64, 9), pair(64, 64, 10, 0), pair(65536, 64)):
        arr = (_MetricsPair * 2)(pair(64, 64), bad)
        assert L.odhip_msssim_planes(arr, 2, po, None, None) == -10
        assert L.odhip_msssim_terms(ctypes.byref(bad), 0, po, po, None) == -10
    arr = (_MetricsPair * 1)(pair(64, 64))
    assert L.odhip_msssim_planes(arr, -1, po, None, None) == -10
    assert L.odhip_msssim_planes(None, 1, po, None, None) == -10
    assert L.odhip_msssim_planes(arr, 1, None, None, None) == -10
    assert L.odhip_msssim_terms(ctypes.byref(arr[0]), 5, po, po, None) == -10
    assert L.odhip_msssim_terms(ctypes.byref(arr[0]), -1, po, po, None) == -10
    assert L.odhip_msssim_terms(ctypes.byref(arr[0]), 0, None, po, None) == -10
    assert L.odhip_msssim_terms(None, 0, po, po, None) == -10
    assert L.odhip_msssim_planes(arr, 0, po, None, None) == 0                 # nothing to do
    assert not out.any()
    assert L.odhip_msssim_prepare(15, 64, 1) == -10 and L.odhip_msssim_prepare(64, 64, 0) == -10


def test_abi_and_mirror(D):
    L = D.lib()
    for name in ("odhip_msssim_taps", "odhip_msssim_weights", "odhip_msssim_planes", "odhip_msssim_prepare",
                 "odhip_msssim_score", "odhip_msssim_terms", "odhip_pipe_set_metrics3", "odhip_pipe_metrics_take3",
                 "odhip_pipe_metrics_msssim_weights"):
        assert hasattr(L, name), name
    header = open(os.path.join(ROOT, "include", "daala_hip.h")).read()
    assert "#define ODHIP_METRIC_MSSSIM (1 << 3)" in header and "#define ODHIP_MSSSIM_MIN_SIZE 16" in header
    assert D.METRIC_MSSSIM == 8 and D.MSSSIM_SCALES == 5 and D.MSSSIM_MIN_SIZE == S.MIN_SIZE == 16
