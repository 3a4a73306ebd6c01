#!/usr/bin/env python3
"""Record the tile sums of SSIM, MS-SSIM and FastSSIM that the library gives for the seeded pairs of
tests/_metric_sums_cases.py.

Dev-time tool, needs a GPU: `python tools/make_golden_metric_sums.py [OUT]`.  It was run once with a build of the
commit BEFORE the three metrics were given one tile-sum kernel and one launch-group scaffold (ODHIP_LIB selects a
library): the sums are repeatable bit for bit by design, so tests/test_gpu_metric_sums.py asks every later library for
the same bit patterns.  tests/golden/metric_sums.npz keeps, per metric, `<metric>_big` [1][columns] - the one pair with
more than 256 tiles in a level - and `<metric>_mixed` [40][columns], as float64: this project's own results, nothing else.
"""
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
import _metric_sums_cases as C  # noqa: E402

OUT = os.path.join(ROOT, "tests", "golden", "metric_sums.npz")


def main():
    import daala_amd as D
    D.init(0)
    out = {}
    for metric in C.METRICS:
        for name, host in (("big", C.big_pair(metric)), ("mixed", C.mixed_pairs(metric))):
            dev = C.Device(D, host)
            a = C.planes(D, metric, dev)
            b = C.planes(D, metric, dev)
            assert np.array_equal(a.view(np.int64), b.view(np.int64)), (metric, name)
            out["%s_%s" % (metric, name)] = a
            print(metric, name, a.shape, a[0])
    path = sys.argv[1] if len(sys.argv) > 1 else OUT
    np.savez_compressed(path, **out)
    print("wrote", path, os.path.getsize(path), "bytes")


if __name__ == "__main__":
    main()
