#!/usr/bin/env python3
"""Record what the reference's RD tools print for the seeded clip pairs of tests/_metrics_ref.CASES.

Dev-time tool: `python tools/make_golden_metrics.py DUMP_PSNR DUMP_PSNRHVS`.  Every case (natural-like,
texture and noise content; odd sizes; 4:2:0 and 4:4:4; 8 and 10 bits - the tools' Y4M reader takes no
12-bit tag) is generated in memory from its seed, written as two temporary YUV4MPEG2 files and given to
the two unmodified reference binaries.  tests/golden/metrics.npz keeps the case list and their printed
lines only - no clip and nothing compiled from the reference.

The binaries were built in a scratch directory outside this repository, each from the reference tree's
tools/<tool>.c linked with tools/vidinput.c, tools/y4m_input.c, src/dct.c and src/internal.c:

    touch config.h                      # an empty config.h, compiled with -DHAVE_CONFIG_H
    mkdir ogg                           # ogg/os_types.h: the ogg_int*_t typedefs over <stdint.h> and
                                        # _ogg_malloc / _ogg_free defined as malloc / free (libogg's own)
    gcc -O2 -DHAVE_CONFIG_H -I. -IREF/include -IREF/src -include stdlib.h -o dump_psnr \\
        REF/tools/dump_psnr.c REF/tools/vidinput.c REF/tools/y4m_input.c REF/src/dct.c REF/src/internal.c -lm

and the same command for dump_psnrhvs.
"""
import os
import subprocess
import sys
import tempfile

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tests"))
import _metrics_ref as M  # noqa: E402

OUT = os.path.join(ROOT, "tests", "golden", "metrics.npz")


def run(tool, a, b):
    r = subprocess.run([tool, a, b], capture_output=True, text=True, check=True)
    return [ln for ln in r.stdout.splitlines() if ln.strip()]


def main():
    if len(sys.argv) != 3:
        raise SystemExit(__doc__)
    psnr_tool, hvs_tool = (os.path.abspath(p) for p in sys.argv[1:])
    names, psnr, hvs = [], [], []
    with tempfile.TemporaryDirectory() as d:
        for case in M.CASES:
            name, _, w, h, c444, depth, _, _ = case
            src, dst = M.make_case(case)
            a, b = os.path.join(d, "a.y4m"), os.path.join(d, "b.y4m")
            open(a, "wb").write(M.y4m_bytes(src, w, h, c444, depth))
            open(b, "wb").write(M.y4m_bytes(dst, w, h, c444, depth))
            names.append(name)
            psnr.append("\n".join(run(psnr_tool, a, b)))
            hvs.append("\n".join(run(hvs_tool, a, b)))
            print(name, "\n ", psnr[-1].splitlines()[-1], "\n ", hvs[-1].splitlines()[-1])
    np.savez_compressed(OUT, names=np.array(names), psnr=np.array(psnr), psnrhvs=np.array(hvs))
    print("wrote", OUT, os.path.getsize(OUT), "bytes")


if __name__ == "__main__":
    main()
