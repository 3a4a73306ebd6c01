#!/usr/bin/env python
"""Writes tests/golden/bsize.npz: the maps, noise averages and psy values of the compiled reference's
od_split_superblock (oracle/_ref/libdaalaref.so) for the named cases of tests/_bsize_cases.py, cell by cell on the
edge-padded pictures.  tests/test_bsize_ref.py pins the file to the compiled reference wherever that is built.

  python tools/gen_bsize_golden.py
"""
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tests"))
import _bsize_cases as B  # noqa: E402
from _libs import ref  # noqa: E402


def main():
    R = ref()
    if R is None:
        sys.exit("oracle/_ref/libdaalaref.so is not built (make -C oracle ref)")
    out = {}
    for name, (px, pred, qs) in B.cases().items():
        for q in qs:
            bmap, noise, psy = B.ref_decide(R, px, pred, q)
            key = "%s_q%d" % (name, q)
            out[key + "_map"], out[key + "_noise"], out[key + "_psy"] = bmap, noise, psy
            print("%-18s sizes 0..3: %s" % (key, np.bincount(bmap.ravel(), minlength=4).tolist()))
    np.savez_compressed(B.FIXTURE, **out)
    print("%s: %d bytes" % (B.FIXTURE, os.path.getsize(B.FIXTURE)))


if __name__ == "__main__":
    main()
