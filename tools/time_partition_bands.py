#!/usr/bin/env python3
"""The copies that put the leaves of a block-size map into planes of one block size and back (odhip_partition_gather /
odhip_partition_scatter, k_part_copy) beside the library's own copy ceiling: F = 16 luma planes of 1080p (coded
1920 x 1088) under one random quadtree per frame (tests/_partition_ref.py::random_map, p_split 0.5), in one process on
one device.  Writes profiles/partition_bands.txt.

    python tools/time_partition_bands.py

  Bytes are counted from the shapes: a gather reads every leaf of its size and writes the whole dense set (padding
  included), a scatter reads and writes every leaf.  Device events round `--calls` back-to-back calls, median of
  `--rounds` windows after a warm-up window, all cases and odhip_copy_ceiling (a plain 16-byte-vector copy of one plane
  set's bytes, best of its three variants) alternating.  The round trip is checked before the timing."""
import argparse
import ctypes
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
OUT = os.path.join(ROOT, "profiles", "partition_bands.txt")
F, W, H = 16, 1920, 1088


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--calls", type=int, default=10)
    ap.add_argument("--rounds", type=int, default=9)
    ap.add_argument("--out", default=OUT)
    args = ap.parse_args()
    import torch
    import daala_amd as D
    import _partition_ref as R
    D.init(0)
    lines = ["Gather and scatter of the leaves of a block-size map - tools/time_partition_bands.py on one MI355X.", ""]

    def say(s):
        print(s, flush=True)
        lines.append(s)

    rng = np.random.RandomState(5)
    maps = torch.from_numpy(np.stack([R.random_map(rng, W//64, H//64, 0.5) for _ in range(F)])).cuda()
    t0 = time.perf_counter()
    lv = D.partition_leaves(maps, F, H, W, 0)
    t1 = time.perf_counter()
    lv = D.partition_leaves(maps, F, H, W, 0)
    t2 = time.perf_counter()
    sizes = lv.sizes()
    plane_bytes = 4*F*W*H
    leaf_bytes = {s: 4*int(lv.counts[s].sum())*(4 << s)**2 for s in sizes}
    dense_bytes = {s: 4*F*W*lv.dense_rows(s) for s in sizes}
    assert sum(leaf_bytes.values()) == plane_bytes
    say("F = %d luma planes of %d x %d, %.1f MB; one random quadtree per frame." % (F, W, H, plane_bytes/1e6))
    say("samples by leaf size 4x4 .. 64x64: %s %%; dense sets (padding included): %s MB"
        % (", ".join("%.1f" % (100.*leaf_bytes.get(s, 0)/plane_bytes) for s in range(5)),
           ", ".join("%.1f" % (dense_bytes.get(s, 0)/1e6) for s in range(5))))
    say("odhip_partition_leaves (three launches, the counts back to the host, a stream synchronise): %.0f us the first "
        "call, %.0f us the second, host clock" % (1e6*(t1 - t0), 1e6*(t2 - t1)))
    src = torch.randint(-(1 << 20), 1 << 20, (F, H, W), dtype=torch.int32, device="cuda")
    back = torch.full_like(src, 0x5a5a5a5a)
    dense = {s: torch.empty((F, lv.dense_rows(s), W), dtype=torch.int32, device="cuda") for s in sizes}

    def gather(s):
        D.partition_gather(src, lv, s, out=dense[s])

    def scatter(s):
        D.partition_scatter(back, dense[s], lv, s)

    def both():
        for s in sizes:
            gather(s)
        for s in sizes:
            scatter(s)

    both()
    torch.cuda.synchronize()
    assert torch.equal(back, src)
    work = {"gather + scatter, all sizes": (both, sum(leaf_bytes[s] + dense_bytes[s] + 2*leaf_bytes[s] for s in sizes))}
    for s in sizes:
        n = 4 << s
        work["gather  %2dx%-2d" % (n, n)] = (lambda s=s: gather(s), leaf_bytes[s] + dense_bytes[s])
        work["scatter %2dx%-2d" % (n, n)] = (lambda s=s: scatter(s), 2*leaf_bytes[s])

    def window(fn, calls):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        for _ in range(calls):
            fn()
        b.record()
        b.synchronize()
        return 1000*a.elapsed_time(b)/calls

    def ceiling():
        best = 0.0
        for variant in range(3):
            g = ctypes.c_double()
            rc = D.lib().odhip_copy_ceiling(plane_bytes, args.calls, variant, ctypes.byref(g),
                                            ctypes.c_void_p(torch.cuda.current_stream().cuda_stream))
            assert rc == 0, rc
            best = max(best, g.value)
        return best

    us = {k: [] for k in work}
    ceil = []
    for k, (fn, _) in work.items():
        window(fn, args.calls)
    ceiling()
    for _ in range(args.rounds):
        for k, (fn, _) in work.items():
            us[k].append(window(fn, args.calls))
        ceil.append(ceiling())
    top = float(np.median(ceil))
    say("")
    say("odhip_copy_ceiling of %.1f MB: %.0f GB/s read + written (median of %d, min %.0f, max %.0f)"
        % (plane_bytes/1e6, top, args.rounds, min(ceil), max(ceil)))
    say("us per call: median of %d windows of %d calls (min, max); bytes read + written; GB/s; share of the ceiling:"
        % (args.rounds, args.calls))
    for k, v in us.items():
        med = float(np.median(v))
        gbs = work[k][1]/med/1e3
        say("  %-28s %8.1f us (%.1f, %.1f)  %7.1f MB  %6.0f GB/s  %.2f" % (k, med, min(v), max(v), work[k][1]/1e6, gbs,
                                                                      gbs/top))
    with open(args.out, "w") as f:
        f.write("\n".join(lines) + "\n")
    return 0


if __name__ == "__main__":
    sys.exit(main())
