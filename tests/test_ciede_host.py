"""CIEDE2000 without a GPU: the restatement (tests/_ciede_ref.py) against the published numbers, the host-only entry
points, and the fixed inputs of the GPU tests (tests/_ciede_cases.py).

- step 6 with kL = kC = kH = 1 reproduces all 34 rows of the test data of Sharma, Wu, Dalal 2005 after rounding to four
  decimals;
- steps 3 to 5 give the Lab values of the sRGB primaries and of mid grey to four decimals (they guard the transcription
  of the constants; they come from the same arithmetic, not from an independent source);
- odhip_ciede_pictures, odhip_ciede_terms, odhip_ciede_lab_terms, odhip_ciede_prepare and odhip_ciede_score refuse a NULL
  pointer, n < 1, an empty or odd-sized 4:2:0 picture, a depth other than 8 / 10 / 12, an unknown format, SAMPLE_U8 at
  another depth and cdec outside 0..1 with ODHIP_EINVAL before they touch a device;
- odhip_ciede_score is 45 - 20 log10(sum/(w h)) and +inf at 0;
- the fixed inputs of the GPU tests meet, in the restatement, both sRGB branches and negative R, G, B, both branches of f
  and negative X, Y, Z, all three branches of the mean hue and both wraps of the hue difference, C1'C2' = 0, identical
  pixels and pixels on the jump at 180 degrees - and no X, Y or Z within 1e-6 relative of f's knee, where a last-bit
  difference of the device's pow could change the branch."""
import ctypes
import math
import os
import sys

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))

import _ciede_cases as C  # noqa: E402
import _ciede_ref as R  # noqa: E402

EINVAL = -10


@pytest.fixture(scope="module")
def D():
    import daala_amd
    return daala_amd


def test_restatement_reproduces_the_published_table():
    t = R.TABLE
    got = R.de00(t[:, 0:3].T, t[:, 3:6].T, 1.0, 1.0, 1.0)
    assert got.shape == (34,)
    assert np.array_equal(np.round(got, 4), t[:, 6]), np.stack([got, t[:, 6]], 1)
    # the measure is symmetric
    back = R.de00(t[:, 3:6].T, t[:, 0:3].T, 1.0, 1.0, 1.0)
    assert np.abs(back - got).max() < 1e-12


def test_lab_of_the_primaries_and_grey():
    rgb = np.array([[1, 0, 0], [0, 1, 0], [0, 0, 1], [.5, .5, .5]], np.float64)
    want = np.array([[53.2406, 80.0923, 67.2028], [87.7351, -86.1830, 83.1797], [32.2957, 79.1856, -107.8573],
                     [53.3890, -0.0015, 0.0028]])
    got = np.stack(R.rgb_lab(rgb[:, 0], rgb[:, 1], rgb[:, 2]), 1)
    assert np.array_equal(np.round(got, 4), want), got


def _pair(D, **kw):
    from daala_amd.api import _CiedePair
    q = _CiedePair()
    for i in range(3):
        q.src[i] = 0x1000
        q.rec[i] = 0x2000
    q.src_fmt = q.rec_fmt = D.SAMPLE_U8
    q.src_stride = q.rec_stride = 64
    q.src_cstride = q.rec_cstride = 32
    q.w, q.h, q.depth, q.cdec = 64, 48, 8, 1
    for k, v in kw.items():
        if k in ("src", "rec"):
            getattr(q, k)[v[0]] = v[1]
        else:
            setattr(q, k, v)
    return q


BAD = [dict(w=0), dict(h=0), dict(w=-2), dict(w=63), dict(h=47), dict(depth=9), dict(depth=16), dict(src_fmt=3),
       dict(rec_fmt=-1), dict(depth=10), dict(depth=12, rec_fmt=2), dict(cdec=2), dict(cdec=-1), dict(src=(1, None)),
       dict(rec=(0, None)), dict(src_stride=63), dict(rec_cstride=31), dict(w=65536, src_stride=65536, rec_stride=65536)]


def test_arguments_are_refused_before_any_device_work(D):
    L = D.lib()
    out = ctypes.c_void_p(0x3000)                        # never written: every call below returns first
    good = _pair(D)
    assert L.odhip_ciede_pictures(None, 1, out, None) == EINVAL
    assert L.odhip_ciede_pictures(ctypes.byref(good), 1, None, None) == EINVAL
    assert L.odhip_ciede_pictures(ctypes.byref(good), 0, out, None) == EINVAL
    assert L.odhip_ciede_pictures(ctypes.byref(good), -1, out, None) == EINVAL
    assert L.odhip_ciede_terms(None, out, None) == EINVAL
    assert L.odhip_ciede_terms(ctypes.byref(good), None, None) == EINVAL
    for kw in BAD:
        q = _pair(D, **kw)
        assert L.odhip_ciede_pictures(ctypes.byref(q), 1, out, None) == EINVAL, kw
        assert L.odhip_ciede_terms(ctypes.byref(q), out, None) == EINVAL, kw
    # a bad pair behind a good one
    from daala_amd.api import _CiedePair
    two = (_CiedePair * 2)(good, _pair(D, h=47))
    assert L.odhip_ciede_pictures(two, 2, out, None) == EINVAL
    # odd sizes are a 4:2:0 restriction
    assert _pair(D, w=63, h=47, cdec=0, src_cstride=64, rec_cstride=64).cdec == 0
    for args in ((0, 8, 1), (8, 0, 1), (8, 8, 0), (65536, 8, 1)):
        assert L.odhip_ciede_prepare(*args) == EINVAL, args
    a = ctypes.c_void_p(0x1000)
    for args in ((None, a, 4, 1., 1., 1., out), (a, None, 4, 1., 1., 1., out), (a, a, 4, 1., 1., 1., None),
                 (a, a, 0, 1., 1., 1., out), (a, a, 4, 0., 1., 1., out), (a, a, 4, 1., -1., 1., out),
                 (a, a, 4, 1., 1., float("nan"), out)):
        assert L.odhip_ciede_lab_terms(*args, None) == EINVAL, args
    v = ctypes.c_double()
    assert L.odhip_ciede_score(1., 8, 8, None) == EINVAL
    assert L.odhip_ciede_score(1., 0, 8, ctypes.byref(v)) == EINVAL
    assert L.odhip_ciede_score(1., 8, -1, ctypes.byref(v)) == EINVAL


def test_score(D):
    for total, w, h in ((1234.5, 64, 48), (3e6, 1920, 1080), (1e-3, 2, 2)):
        want = 45 - 20 * math.log10(total / (w * h))
        assert D.ciede_score(total, w, h) == want == float(R.score(total, w, h))
    assert D.ciede_score(0.0, 64, 48) == math.inf
    got = D.ciede_score(np.array([[1., 2.], [0., 4.]]), 4, 4)
    assert got.shape == (2, 2) and got[1, 0] == math.inf and got[0, 1] == 45 - 20 * math.log10(2. / 16)


def test_symbols_and_flag(D):
    L = D.lib()
    for name in ("odhip_ciede_pictures", "odhip_ciede_prepare", "odhip_ciede_score", "odhip_ciede_terms",
                 "odhip_ciede_lab_terms", "odhip_pipe_set_metrics5", "odhip_pipe_metrics_take5",
                 "odhip_pipe_metrics_ciede_values"):
        assert hasattr(L, name), name
    assert D.METRIC_CIEDE == 32
    from daala_amd.api import _CiedePair
    assert ctypes.sizeof(_CiedePair) == 6 * 8 + 10 * 4


def test_fixed_inputs_reach_every_branch():
    total = {}
    knee = np.inf
    for case in C.cases():
        st = {}
        one, other = C.restated(case, st)
        assert one.shape == (case["h"], case["w"]) and not np.isnan(one).any() and not np.isnan(other).any()
        assert max(case["w"], case["h"]) <= 66 and min(case["w"], case["h"]) <= 50
        knee = min(knee, st.pop("f_knee"))
        st.pop("gap")
        for k, v in st.items():
            total[k] = total.get(k, 0) + v
        # off the jump both sides are one value; on it they differ, by far less than any bound on a term
        m = one != other
        assert int(m.sum()) <= st["near"]
        if m.any():
            assert np.abs(one - other)[m].max() < 1e-4
    print(total, "knee", knee)
    for k in ("srgb_pow", "srgb_linear", "rgb_negative", "f_cbrt", "f_linear", "xyz_negative", "hbar_mean", "hbar_plus",
              "hbar_minus", "dh_over", "dh_under", "cc_zero", "identical", "near"):
        assert total[k] > 0, k
    assert knee > 1e-6


def test_grey_pairs_across_black_sit_on_the_jump():
    case = [c for c in C.cases() if c["name"].startswith("grey")][0]
    st = {}
    one, other = C.restated(case, st)
    # plain arithmetic up to atan2: no pow, no cbrt
    assert st["srgb_pow"] == 0 and st["f_cbrt"] == 0
    y1, y2 = np.meshgrid(np.arange(25), np.arange(25))
    across = ((y1 < 16) & (y2 > 16)) | ((y1 > 16) & (y2 < 16))
    gap = st["gap"]
    assert across.sum() == 2 * 16 * 8 and (gap[across] < 1e-7).all() and (gap[~across] > 1).all()
    inside = R.near(gap)
    assert inside[across].sum() > 50 and (~inside)[across].sum() > 50
    assert (np.abs(gap - 1e-9) > 1e-12).all()
    # the jump itself, at a chroma of 1e-4: orders of magnitude below any bound on a term
    m = one != other
    assert m.sum() > 50 and 0 < np.abs(one - other)[m].max() < 1e-12
    assert (one[y1 == y2] == 0).all()
