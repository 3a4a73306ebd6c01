#!/usr/bin/env python3
"""Record what the reference's dump_msssim prints for the seeded clip pairs of tests/_msssim_ref.CASES.

Dev-time tool: `python tools/make_golden_msssim.py DUMP_MSSSIM`.  Every case - the seven clips of
tests/_metrics_ref.CASES and the two clips at the size floor of tests/_msssim_ref.FLOOR_CASES (a 16 x 16 plane,
whose scale 4 is one sample, and 4:2:0 chroma of 16 x 17) - is generated in memory from its seed, written as
two temporary YUV4MPEG2 files and given to the unmodified reference binary, once as it stands (dB) and once
with -r (raw).  tests/golden/msssim.npz keeps the case list and the printed lines only - no clip and nothing
compiled from the reference.

The binary was built in a scratch directory outside this repository from the reference tree's
tools/dump_msssim.c by the command documented in tools/make_golden_metrics.py.
"""
import os
import subprocess
import sys
import tempfile

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tests"))
import _metrics_ref as M  # noqa: E402
import _msssim_ref as S  # noqa: E402

OUT = os.path.join(ROOT, "tests", "golden", "msssim.npz")


def run(tool, args, a, b):
    r = subprocess.run([tool] + args + [a, b], capture_output=True, text=True, check=True)
    return [ln for ln in r.stdout.splitlines() if ln.strip()]


def main():
    if len(sys.argv) != 2:
        raise SystemExit(__doc__)
    tool = os.path.abspath(sys.argv[1])
    names, db, raw = [], [], []
    with tempfile.TemporaryDirectory() as d:
        for case in S.CASES:
            name, _, w, h, c444, depth, _, _ = case
            src, dst = M.make_case(case)
            a, b = os.path.join(d, "a.y4m"), os.path.join(d, "b.y4m")
            open(a, "wb").write(M.y4m_bytes(src, w, h, c444, depth))
            open(b, "wb").write(M.y4m_bytes(dst, w, h, c444, depth))
            names.append(name)
            db.append("\n".join(run(tool, [], a, b)))
            raw.append("\n".join(run(tool, ["-r"], a, b)))
            print(name, "\n ", db[-1].splitlines()[-1], "\n ", raw[-1].splitlines()[-1])
    np.savez_compressed(OUT, names=np.array(names), msssim=np.array(db), msssim_raw=np.array(raw))
    print("wrote", OUT, os.path.getsize(OUT), "bytes")


if __name__ == "__main__":
    main()
