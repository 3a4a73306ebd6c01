"""CIEDE2000 on the device (k_ciede, k_ciede_lab) against the numpy restatement (tests/_ciede_ref.py) on the fixed inputs
of tests/_ciede_cases.py, which tests/test_ciede_host.py shows to reach every branch.

- odhip_ciede_lab_terms on the published table of Sharma, Wu, Dalal 2005: every row within 1e-4 of the printed value
  and within BOUND of the restatement.  Rows 9 and 13 are pairs of EXACTLY opposite hues, (a, b) against (-a, -b): the
  print is the value of "not above 180", which the device reaches because it takes the side of the jump from a cross
  product that is exactly 0 there; the rounded difference of two atan2 results is 180 give or take a last bit;
- odhip_ciede_terms of every case - 4:2:0 at 64 x 48, 2 x 2 and 66 x 50 (a tile crossed in both directions), 4:4:4 at
  1 x 1 and 37 x 23, uint16 at 10 bits, int16 at 12 bits (ODHIP_SAMPLE_I16_12) against uint8 at 8 bits and against
  uint16 at 10 and 12 (uint8 samples exist at 8 bits only), planes with wider strides and unaligned first samples, the
  0 / 16 / 128 / 235 / 255 corner combinations, and grey pictures on either side of Y = 16 - within BOUND of the
  restatement, pixel by pixel.  dE00 jumps where the two hues are 180 degrees apart; a pixel whose restated hues are
  within 1e-9 degrees of that may match the value on either side of the jump, every other pixel matches the one value.
  Nothing is left out;
- odhip_ciede_pictures: a sum equals the sum of the call's own terms within N 2^-53 sum|term|, two runs give the same
  bits, identical pictures give exactly 0.0, and three pairs of different sizes and formats in one call give the bits of
  three single calls - and so do five pairs of one source picture, which the kernel walks as one run;
- ciede_score is the Python expression.

BOUND is 8 times the largest |device - restatement| measured over these cases on an MI355X, 1.47e-13 in the 64 x 48 case
(profiles/ciede.txt): margin for other math-library builds, still orders of magnitude below a single-precision slip
(~1e-5) and below the ceiling the arithmetic gives (2-ulp functions, the factor 500 on a: ~1e-9)."""
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

pytestmark = pytest.mark.gpu

BOUND = 8 * 1.47e-13
CASES = C.cases()


@pytest.fixture(scope="module")
def D():
    import daala_amd
    daala_amd.init(0)
    return daala_amd


@pytest.fixture(scope="module")
def restated():
    """The restatement of every case, computed once."""
    return {c["name"]: C.restated(c) for c in CASES}


def _device_planes(planes):
    """The planes on the device with their strides and first-sample offsets: a view of the uploaded parent buffer."""
    import torch
    out = []
    for a in planes:
        base = a.base if a.base is not None else a
        t = torch.from_numpy(np.ascontiguousarray(base)).cuda()
        if a.base is not None:
            off = (a.__array_interface__["data"][0] - base.__array_interface__["data"][0]) // a.itemsize
            r0, c0 = divmod(off, base.shape[1])
            t = t[r0:r0 + a.shape[0], c0:c0 + a.shape[1]]
            assert c0 > 0 and t.stride(0) > a.shape[1]
        assert np.array_equal(t.cpu().numpy(), a)
        out.append(t)
    return out


def _upload(case):
    return _device_planes(case["src"]), _device_planes(case["rec"])


def _opts(case):
    return dict(w=case["w"], h=case["h"], depth=case["depth"], src_fmt=case["src_fmt"], rec_fmt=case["rec_fmt"])


def _table(D, kl, kc, kh):
    """(device, restatement, restatement on the other side of the jump for the rows on it) of the table's 34 pairs."""
    t = R.TABLE
    got = D.ciede_lab_terms(t[:, 0:3], t[:, 3:6], kl, kc, kh)
    st = {}
    one = R.de00(t[:, 0:3].T, t[:, 3:6].T, kl, kc, kh, stats=st)
    other = R.de00(t[:, 0:3].T, t[:, 3:6].T, kl, kc, kh, flip=R.near(st["gap"]))
    return got, one, other


def test_published_table_within_the_bound_of_the_restatement(D):
    for weights in ((1.0, 1.0, 1.0), (R.KL, R.KC, R.KH)):
        got, one, other = _table(D, *weights)
        on_jump = np.nonzero(one != other)[0]
        assert list(on_jump) == [9, 13]                    # (2.49, -0.001) / (-2.49, 0.001) and its transpose: exactly opposite
        err = np.minimum(np.abs(got - one), np.abs(got - other))
        side = ["other" if abs(got[i] - one[i]) > abs(got[i] - other[i]) else "same" for i in on_jump]
        print("table at kL %g kC %g kH %g: max |device - restatement| %.3g; rows 9 and 13 on the %s side as the restatement"
              % (weights + (err.max(), " / ".join(side))))
        assert err.max() <= BOUND


def test_published_table_printed_values(D):
    """Every row within 1e-4 of the printed value, the two rows of exactly opposite hues (9 and 13, counted from 0)
    included: 7.1792 and 4.8045 are the values of 'not above 180'; the other side is 0.0403 and 0.0585 away."""
    got, _, _ = _table(D, 1.0, 1.0, 1.0)
    diff = np.abs(got - R.TABLE[:, 6])
    print("table: max |device - printed| %.3g; rows beyond 1e-4: %s" % (diff.max(), list(np.nonzero(diff >= 1e-4)[0])))
    assert diff.max() < 1e-4


@pytest.mark.parametrize("idx", range(len(CASES)), ids=[c["name"] for c in CASES])
def test_terms_equal_the_restatement(D, restated, idx):
    case = CASES[idx]
    src, rec = _upload(case)
    got = D.ciede_terms(src, rec, **_opts(case))
    one, other = restated[case["name"]]
    assert got.shape == one.shape and not np.isnan(got).any()
    err = np.minimum(np.abs(got - one), np.abs(got - other))
    print("%s: max |device - restatement| %.3g over %d pixels, %d on the jump, largest term %.3g"
          % (case["name"], err.max(), err.size, int((one != other).sum()), one.max()))
    assert err.max() <= BOUND
    # identical pixels: exactly zero
    assert (got[one == 0] == 0).all()


def test_sums_are_the_sums_of_the_terms_and_repeat(D):
    for case in (CASES[0], CASES[3], CASES[4]):
        src, rec = _upload(case)
        pic = (src, rec, _opts(case))
        terms = D.ciede_terms(src, rec, **_opts(case))
        a = D.ciede_pictures([pic])
        b = D.ciede_pictures([pic])
        assert a.shape == (1,) and a.view(np.int64)[0] == b.view(np.int64)[0]
        n = terms.size
        assert abs(a[0] - math.fsum(terms.ravel())) <= n * 2.0 ** -53 * math.fsum(np.abs(terms).ravel())
        assert a[0] > 0
        same = D.ciede_pictures([(src, src, dict(_opts(case), rec_fmt=case["src_fmt"]))])
        assert same[0] == 0.0


def test_pairs_of_one_call_equal_single_calls(D):
    picked = [CASES[0], CASES[7], CASES[9]]                    # 4:2:0 uint8, 4:4:4 10 bits uint16 / int16, strided
    assert len({(c["w"], c["h"]) for c in picked}) == 3
    pics = []
    for case in picked:
        src, rec = _upload(case)
        pics.append((src, rec, _opts(case)))
    together = D.ciede_pictures(pics)
    alone = np.array([D.ciede_pictures([p])[0] for p in pics])
    assert together.shape == (3,) and np.array_equal(together.view(np.int64), alone.view(np.int64)), (together, alone)
    assert len(set(together)) == 3
    # five reconstructions of one source picture, with another picture between them: the source's Lab is computed once
    # for the run of five, and every sum is still that of a single call
    import torch
    case = CASES[4]
    src, rec = _upload(case)
    rng = np.random.RandomState(9)
    recs = [rec] + [[torch.from_numpy(np.clip(p.astype(np.int64) + rng.randint(-k, k + 1, size=p.shape), 0, 255)
                                      .astype(np.uint8)).cuda() for p in case["rec"]] for k in (1, 2, 3, 9)]
    pics = [(src, r, _opts(case)) for r in recs]
    pics.insert(2, _upload(CASES[0]) + (_opts(CASES[0]),))
    together = D.ciede_pictures(pics)
    alone = np.array([D.ciede_pictures([p])[0] for p in pics])
    assert np.array_equal(together.view(np.int64), alone.view(np.int64)), (together, alone)
    assert len(set(together)) == 6


def test_score_is_the_expression(D):
    case = CASES[0]
    src, rec = _upload(case)
    total = D.ciede_pictures([(src, rec, _opts(case))])[0]
    assert D.ciede_score(total, case["w"], case["h"]) == 45 - 20 * math.log10(total / (case["w"] * case["h"]))
    assert D.ciede_score(0.0, 2, 2) == math.inf
