"""The tile sums of SSIM, MS-SSIM and FastSSIM (k_metric_tile_sum, od_metric_launch.cuh: lane i adds the partials i,
i + 256, ... of a (pair, column), then a tree) where a lane adds MORE than one partial: 544x512 is 17 x 16 = 272 tiles of
32x32 for SSIM and scale 0 of MS-SSIM, and 1088x1024 has that level 0 in FastSSIM; the other GPU tests stay at 15 tiles or
fewer.  For that one 8-bit pair per metric (tests/_metric_sums_cases.py):

- every column of the sums of odhip_*_planes is within N * 2^-53 * sum|term| of math.fsum over the DEVICE's own term map
  of that column from odhip_*_terms (MS-SSIM: cs at scales 0..3, ssim at scale 4) - the bound of N doubles added in any
  order; the term maps themselves are pinned bit for bit to the restatements at small sizes by
  test_gpu_ssim.py, test_gpu_msssim.py and test_gpu_fastssim.py;
- the sums, and those of one call of 40 mixed small pairs with shared sources (two launch groups), equal as int64 bit
  patterns what tests/golden/metric_sums.npz recorded (tools/make_golden_metric_sums.py) from the library as it was
  before the three metrics shared one sum kernel and one launch-group scaffold.  The sums repeat bit for bit by design:
  equality, no tolerance."""
import math
import os
import sys

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))

import _metric_sums_cases as C  # noqa: E402

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def D():
    import daala_amd
    daala_amd.init(0)
    return daala_amd


@pytest.fixture(scope="module")
def golden():
    return np.load(os.path.join(ROOT, "tests", "golden", "metric_sums.npz"))


@pytest.mark.parametrize("metric", C.METRICS)
def test_more_than_one_partial_per_lane(D, golden, metric):
    dev = C.Device(D, C.big_pair(metric))
    got = C.planes(D, metric, dev)
    assert got.shape == (1, C.COLUMNS[metric])
    maps = C.term_maps(D, metric, dev)
    w, h = C.BIG[metric]
    w0, h0 = ((w + 1) // 2, (h + 1) // 2) if metric == "fastssim" else (w, h)
    assert maps[0].size == w0 * h0 and -(-w0 // 32) * -(-h0 // 32) > 256           # the tiles of the largest level
    for col, t in enumerate(maps):
        exact = math.fsum(t.tolist())
        bound = t.size * 2.0 ** -53 * math.fsum(np.abs(t).tolist())
        print("%s %dx%d column %d: sum %.17g, off the exact sum of the device's %d terms by %.3g (bound %.3g)"
              % (metric, w, h, col, got[0][col], t.size, got[0][col] - exact, bound))
        assert abs(got[0][col] - exact) <= bound, (metric, col, got[0][col], exact, bound)
    want = golden[metric + "_big"]
    assert np.array_equal(got.view(np.int64), want.view(np.int64)), (metric, got, want)


@pytest.mark.parametrize("metric", C.METRICS)
def test_forty_mixed_pairs_equal_the_recorded_bits(D, golden, metric):
    got = C.planes(D, metric, C.Device(D, C.mixed_pairs(metric)))
    want = golden[metric + "_mixed"]
    assert got.shape == want.shape == (C.MIXED, C.COLUMNS[metric])
    bad = np.argwhere(got.view(np.int64) != want.view(np.int64))
    assert len(bad) == 0, (metric, len(bad), bad[:4], got[tuple(bad[0])], want[tuple(bad[0])])
