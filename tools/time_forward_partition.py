#!/usr/bin/env python3
"""The forward lapped transform at a block-size map (odhip_forward_partition, k_forward_part<64/32>) beside the calls
it stands between: F = 16 pictures of 1080p (coded 1920 x 1088), luma and 4:2:0 chroma, in one process on one device.
Writes profiles/forward_partition.txt.

    python tools/time_forward_partition.py [--resources FILE]

  forward   odhip_forward_partition at three maps: every superblock one 64x64 block (uniform 4), every block 4x4
            (uniform 0), and a random quadtree per frame (tests/_partition_ref.py::random_map, p_split 0.5).
  pyramid   odhip_forward_pyramid of the same planes storing all of its levels (five luma, four chroma): the only
            forward call there was.  Its code is the parent commit's, untouched.
  inverse   odhip_inverse_partition of the forward call's coefficients at the same maps.
  Device events round `--calls` back-to-back calls, median of `--rounds` such windows after a warm-up window, all
  cases alternating.  The expectation checked at the end: the new call is no slower than the pyramid, with the
  pyramid's own run-to-run spread (max - min of its windows) as the margin.
  --resources: the output of `tools/kres.py lapped_kernels.hip 'k_forward_part|k_inverse_part|k_forward_pyramid'`,
  copied into the record (the compiler runs wherever the sources are; the timing needs the device)."""
import argparse
import ctypes
import os
import subprocess
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
OUT = os.path.join(ROOT, "profiles", "forward_partition.txt")
F, W, H = 16, 1920, 1088
KERNELS = "k_forward_part|k_inverse_part|k_forward_pyramid"


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--calls", type=int, default=10)
    ap.add_argument("--rounds", type=int, default=9)
    ap.add_argument("--resources", default=None)
    ap.add_argument("--out", default=OUT)
    args = ap.parse_args()
    import torch
    import daala_amd as D
    import _partition_ref as R
    D.init(0)
    L = D.lib()
    lines = ["Forward lapped transform at a block-size map - tools/time_forward_partition.py on one MI355X.", ""]

    def say(s):
        print(s, flush=True)
        lines.append(s)

    say("F = %d pictures of 1080p (coded %d x %d): %d luma planes, %d planes of 4:2:0 chroma (%d x %d, Cb and Cr of a "
        "frame share its map)." % (F, W, H, F, 2*F, W//2, H//2))
    if args.resources:
        res = open(args.resources).read()
    else:
        res = subprocess.run([sys.executable, os.path.join(ROOT, "tools", "kres.py"), "lapped_kernels.hip", KERNELS],
                             capture_output=True, text=True, check=True).stdout
    say("")
    say("Compiler resources (tools/kres.py; occ = waves per SIMD):")
    for ln in res.rstrip().splitlines():
        say("  " + ln)
    nsbx, nsby = W//64, H//64
    rng = np.random.RandomState(5)
    maps = {"uniform 4": np.stack([R.uniform(4, nsbx, nsby)]*F), "uniform 0": np.stack([R.uniform(0, nsbx, nsby)]*F),
            "random .5": np.stack([R.random_map(rng, nsbx, nsby, 0.5) for _ in range(F)])}
    leaves = 100.0*np.bincount(maps["random .5"].ravel(), minlength=5)/maps["random .5"].size
    say("")
    say("random .5: luma samples by leaf size 4x4 .. 64x64: %s %%" % ", ".join("%.1f" % v for v in leaves))
    stream = lambda: ctypes.c_void_p(torch.cuda.current_stream().cuda_stream)      # noqa: E731
    work, keep = {}, []
    for dec, kind in ((0, "luma"), (1, "chroma")):
        w, h, ppf = W >> dec, H >> dec, 1 + dec
        n = F*ppf
        px = torch.randint(0, 256, (n, h, w), dtype=torch.uint8, device="cuda")
        back = torch.empty_like(px)
        keep.append((px, back))
        pyr = [None]

        def pyramid(px=px, dec=dec, pyr=pyr):
            pyr[0] = D.forward_pyramid(px, dec, W, H, levels=pyr[0])
            return 0

        work["pyramid   %-6s all levels" % kind] = pyramid
        for name, m in maps.items():
            bm = torch.from_numpy(m).cuda()
            coef = torch.empty((n, h, w), dtype=torch.int32, device="cuda")
            keep.append((bm, coef))
            rows, cols = m.shape[1:]

            def forward(px=px, bm=bm, coef=coef, dec=dec, ppf=ppf):
                D.forward_partition(px, bm, dec, W, H, ppf, out=coef)
                return 0

            def inverse(back=back, bm=bm, coef=coef, dec=dec, ppf=ppf, n=n, w=w, h=h, rows=rows, cols=cols):
                return L.odhip_inverse_partition(ctypes.c_void_p(back.data_ptr()), w, ctypes.c_long(h*w),
                                                 ctypes.c_void_p(coef.data_ptr()), n, w, h, dec,
                                                 ctypes.c_void_p(bm.data_ptr()), cols, ctypes.c_long(rows*cols), ppf, W, H,
                                                 stream())

            work["forward   %-6s %s" % (kind, name)] = forward
            work["inverse   %-6s %s" % (kind, name)] = inverse
            # the record is of calls that compute the right thing: the round trip gives the pixels back
            forward()
            assert inverse() == 0
            torch.cuda.synchronize()
            assert torch.equal(back, px), (kind, name)

    def window(fn, calls):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        for _ in range(calls):
            rc = fn()
            assert rc == 0, rc
        b.record()
        b.synchronize()
        return 1000*a.elapsed_time(b)/calls

    us = {k: [] for k in work}
    for k, fn in work.items():
        window(fn, args.calls)
    for _ in range(args.rounds):
        for k, fn in work.items():
            us[k].append(window(fn, args.calls))
    med = {k: float(np.median(v)) for k, v in us.items()}
    say("")
    say("us per call: median of %d windows of %d calls, min, max; all cases alternating; inverse(forward(px)) == px "
        "checked for every map before the timing:" % (args.rounds, args.calls))
    for k, v in us.items():
        say("  %-28s %8.1f us (min %.1f, max %.1f)" % (k, med[k], min(v), max(v)))
    say("")
    say("The new call against the pyramid (margin: the pyramid's own max - min):")
    ok = True
    for kind in ("luma", "chroma"):
        p = "pyramid   %-6s all levels" % kind
        spread = max(us[p]) - min(us[p])
        for name in maps:
            t = med["forward   %-6s %s" % (kind, name)]
            fine = t <= med[p] + spread
            ok = ok and fine
            say("  %-6s %s: %.1f us against %.1f + %.1f: %s (%.2f of the pyramid)"
                % (kind, name, t, med[p], spread, "no slower" if fine else "SLOWER", t/med[p]))
    say("")
    say("expectation (no slower than the pyramid on the same planes): %s" % ("holds" if ok else "DOES NOT HOLD"))
    with open(args.out, "w") as f:
        f.write("\n".join(lines) + "\n")
    return 0 if ok else 1


if __name__ == "__main__":
    sys.exit(main())
