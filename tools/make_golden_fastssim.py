#!/usr/bin/env python3
"""Record what the reference's dump_fastssim prints for the seeded clip pairs of tests/_fastssim_ref.CASES.

Dev-time tool: `python tools/make_golden_fastssim.py DUMP_FASTSSIM [FASTSSIM_BITS]`.  Every case - 8 and 10 bits,
4:2:0 and 4:4:4, every plane of a size where the tool's downsampling reads stay inside the level it reads
(tests/_fastssim_ref.tool_reads_inside) - is generated in memory from its seed, written as two temporary YUV4MPEG2
files and given to the unmodified reference binary with -c (dB) and with -c -r (raw).  tests/golden/fastssim.npz
keeps the case list and the printed lines only - no clip and nothing compiled from the reference.

The binary was built in a scratch directory outside this repository from the reference tree's tools/dump_fastssim.c
by the command documented in tools/make_golden_metrics.py.

FASTSSIM_BITS (optional) is a throw-away wrapper, built in the same scratch directory: a C file that includes
tools/dump_fastssim.c with `main` renamed by the preprocessor and has a main of its own,
`fastssim_bits W H DEPTH A.raw B.raw`, which reads two raw planes (uint8, or little-endian uint16 above 8 bits),
calls calc_ssim(a, stride, b, stride, depth, w, h) and prints the returned double's bit pattern as 16 hex digits.
With it the file also keeps `bits`: per case the [frame][plane] return values of calc_ssim as uint64.
"""
import os
import subprocess
import sys
import tempfile

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tests"))
import _metrics_ref as M  # noqa: E402
import _fastssim_ref as S  # noqa: E402

OUT = os.path.join(ROOT, "tests", "golden", "fastssim.npz")


def run(tool, args, a, b):
    r = subprocess.run([tool] + args + [a, b], capture_output=True, text=True, check=True)
    return [ln for ln in r.stdout.splitlines() if ln.strip()]


def plane_bits(tool, d, a, b, depth):
    dt = np.uint8 if depth == 8 else np.dtype("<u2")
    fa, fb = os.path.join(d, "a.raw"), os.path.join(d, "b.raw")
    open(fa, "wb").write(np.ascontiguousarray(a.astype(dt)).tobytes())
    open(fb, "wb").write(np.ascontiguousarray(b.astype(dt)).tobytes())
    h, w = a.shape
    r = subprocess.run([tool, str(w), str(h), str(depth), fa, fb], capture_output=True, text=True, check=True)
    return int(r.stdout.strip(), 16)


def main():
    if len(sys.argv) not in (2, 3):
        raise SystemExit(__doc__)
    tool = os.path.abspath(sys.argv[1])
    wrapper = os.path.abspath(sys.argv[2]) if len(sys.argv) == 3 else None
    names, db, raw, bits = [], [], [], {}
    with tempfile.TemporaryDirectory() as d:
        for case in S.CASES:
            name, _, w, h, c444, depth, _, _ = case
            src, dst = M.make_case(case)
            for fs in src:
                for p in fs:
                    assert S.tool_reads_inside(p.shape[1], p.shape[0]), (name, p.shape)
            a, b = os.path.join(d, "a.y4m"), os.path.join(d, "b.y4m")
            open(a, "wb").write(M.y4m_bytes(src, w, h, c444, depth))
            open(b, "wb").write(M.y4m_bytes(dst, w, h, c444, depth))
            names.append(name)
            db.append("\n".join(run(tool, ["-c"], a, b)))
            raw.append("\n".join(run(tool, ["-c", "-r"], a, b)))
            if wrapper:
                bits["bits_" + name] = np.array([[plane_bits(wrapper, d, pa, pb, depth) for pa, pb in zip(fs, fd)]
                                                 for fs, fd in zip(src, dst)], np.uint64)
            print(name, "\n ", db[-1].splitlines()[-1], "\n ", raw[-1].splitlines()[-1])
    np.savez_compressed(OUT, names=np.array(names), fastssim=np.array(db), fastssim_raw=np.array(raw), **bits)
    print("wrote", OUT, os.path.getsize(OUT), "bytes")


if __name__ == "__main__":
    main()
