#!/usr/bin/env python3
"""What building the chroma-from-luma reference planes at a block-size map costs: odhip_cfl_refs_partition (k_cfl_part)
on F = 16 frames of the benchmark's 1080p natural content, edge-padded to 1920 x 1088 (whole superblocks), at the map
odhip_bsize_decide gives them, on the dequantised luma planes of the no-reference band stage.  Writes
profiles/cfl_partition.txt.

    python tools/time_cfl_partition.py

  the kernel        between two events on the stream: one call (median of `--calls` after a warm-up; a call this short
                    carries the launch with it) and `--burst` calls back to back over the burst (the launches overlap
                    the kernels: the kernel's own time)
  its bytes         what the algorithm needs: one chroma plane's worth of luma per frame (the quarter of every block of
                    8x8 and more, the 2x2 corners of four 4x4 blocks), planes_per_frame chroma planes written, the map
  the ceiling       odhip_copy_ceiling of as many bytes, and k_part_copy (odhip_partition_gather of every size) on the
                    reference planes themselves
  beside it         the with-reference band stage on the Cb and Cr planes of the same frames against these references
                    (pvq_partition_ref, is_keyframe = 1, distortion-only choice; wall clock, stream drained)"""
import argparse
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
OUT = os.path.join(ROOT, "profiles", "cfl_partition.txt")
F, W, H, CW, CH = 16, 1920, 1080, 1920, 1088
Q = 800
PPF = 2


def content():
    """(luma [F][CH][CW], chroma [2F][CH/2][CW/2] with Cb and Cr of a frame adjacent), edge-padded."""
    import bench
    frames = [bench.CONTENT["natural"](i, 1) for i in range(F)]
    luma = np.stack([f[0][:H, :W] for f in frames])
    chroma = np.stack([f[p][:H // 2, :W // 2] for f in frames for p in (1, 2)])
    luma = np.pad(luma, ((0, 0), (0, CH - H), (0, CW - W)), mode="edge")
    chroma = np.pad(chroma, ((0, 0), (0, (CH - H) // 2), (0, (CW - W) // 2)), mode="edge")
    return np.ascontiguousarray(luma), np.ascontiguousarray(chroma)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--calls", type=int, default=20)
    ap.add_argument("--burst", type=int, default=50)
    ap.add_argument("--out", default=OUT)
    args = ap.parse_args()
    import torch
    import daala_amd as D
    D.init(0)
    lines = []

    def say(s):
        print(s, flush=True)
        lines.append(s)

    def events(fn, reps):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        torch.cuda.synchronize()
        e0.record()
        for _ in range(reps):
            fn()
        e1.record()
        torch.cuda.synchronize()
        return e0.elapsed_time(e1) / reps

    def wall(fn):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        fn()
        torch.cuda.synchronize()
        return (time.perf_counter() - t0) * 1e3

    luma, chroma = content()
    qt = D.QuantTables.load()
    lam = D.OD_PVQ_LAMBDA
    px = torch.from_numpy(luma).cuda()
    bmap, _ = D.bsize_decide(px, Q)
    hist = np.bincount(bmap.cpu().numpy().ravel(), minlength=5)
    coef = D.forward_partition(px, bmap, 0, W, H)
    dq = D.pvq_partition_noref(coef, bmap, 0, qt.size_tables(0, 0), lam).dq
    del coef, px
    ref = torch.empty((F * PPF, CH // 2, CW // 2), dtype=torch.int32, device="cuda")
    call = lambda: D.cfl_refs_partition(dq, bmap, 1, planes_per_frame=PPF, out=ref)  # noqa: E731
    call()
    say("Chroma-from-luma references at a block-size map - tools/time_cfl_partition.py on one MI355X.")
    say("odhip_cfl_refs_partition (k_cfl_part), F = %d frames of %d x %d (coded %d x %d: %d superblocks), benchmark natural "
        "content, the map of odhip_bsize_decide at quantiser %d, planes_per_frame = %d, dec = 1."
        % (F, W, H, CW, CH, F * (CW // 64) * (CH // 64), Q, PPF))
    say("  map entries 4x4 / 8x8 / 16x16 / 32x32 / 64x64: %s" % " / ".join(
        "%d (%.1f%%)" % (n, 100. * n / hist.sum()) for n in hist[:5]))
    single = float(np.median([events(call, 1) for _ in range(args.calls)]))
    burst = float(np.median([events(call, args.burst) for _ in range(5)]))
    plane = F * (CH // 2) * (CW // 2) * 4
    nbytes = plane * (1 + PPF) + bmap.numel()
    ceiling = D.copy_ceiling((nbytes // 2) & ~15, n=10)
    say("  k_cfl_part, one call between two events (median of %d):        %8.1f us" % (args.calls, single * 1e3))
    say("  k_cfl_part, %d calls back to back, per call (median of 5):      %8.1f us = %.2f us per frame"
        % (args.burst, burst * 1e3, burst * 1e3 / F))
    say("  algorithmic bytes: luma read %.1f MB + %d chroma planes written %.1f MB + map %.2f MB = %.1f MB -> %.0f GB/s "
        "(back to back), %.0f GB/s (one call)" % (plane / 1e6, PPF, PPF * plane / 1e6, bmap.numel() / 1e6, nbytes / 1e6,
                                                  nbytes / burst / 1e6, nbytes / single / 1e6))
    say("  odhip_copy_ceiling of as many bytes: %.0f GB/s, i.e. %.1f us; k_cfl_part reaches %.0f%% of it back to back, "
        "%.0f%% in one call" % (ceiling, nbytes / ceiling / 1e3, 100. * nbytes / burst / 1e6 / ceiling,
                                100. * nbytes / single / 1e6 / ceiling))
    # the other branch: the decided map of this content holds few 4x4 areas, so the same planes at a map of 4x4 alone
    # (od_tf_up_hv_lp everywhere: four 8-byte loads per group instead of one 16-byte load, the same bytes)
    zeros = torch.zeros_like(bmap)
    tf_call = lambda: D.cfl_refs_partition(dq, zeros, 1, planes_per_frame=PPF, out=ref)  # noqa: E731
    tf_call()
    tf = float(np.median([events(tf_call, args.burst) for _ in range(5)]))
    say("  the same at a map of 4x4 alone (the TF branch everywhere), %d calls back to back, per call: %8.1f us -> %.0f GB/s "
        "= %.0f%% of the ceiling" % (args.burst, tf * 1e3, nbytes / tf / 1e6, 100. * nbytes / tf / 1e6 / ceiling))
    call()
    # k_part_copy on the same planes: the gather of every size present reads each leaf once and writes the dense sets
    leaves = D.partition_leaves(bmap, F * PPF, CH // 2, CW // 2, 1, planes_per_frame=PPF)
    sizes = leaves.sizes()
    dense = {s: torch.empty((F * PPF, leaves.dense_rows(s), CW // 2), dtype=torch.int32, device="cuda") for s in sizes}

    def gathers():
        for s in sizes:
            D.partition_gather(ref, leaves, s, out=dense[s])

    gathers()
    gms = float(np.median([events(gathers, args.burst) for _ in range(5)]))
    gbytes = PPF * plane + sum(d.numel() * 4 for d in dense.values())
    say("  k_part_copy on the same planes (odhip_partition_gather of the %d sizes present, %d calls back to back): %.1f us "
        "for %.1f MB read + written -> %.0f GB/s = %.0f%% of the ceiling" % (len(sizes), args.burst, gms * 1e3,
                                                                            gbytes / 1e6, gbytes / gms / 1e6,
                                                                            100. * gbytes / gms / 1e6 / ceiling))
    # the stage these planes feed
    cpx = torch.from_numpy(chroma).cuda()
    ccoef = D.forward_partition(cpx, bmap, 1, W, H, planes_per_frame=PPF)
    tables = qt.size_tables(1, 1)
    stage = lambda: D.pvq_partition_ref(ccoef, ref, bmap, 1, tables, lam, 1, 1, planes_per_frame=PPF)  # noqa: E731
    stage()
    sms = float(np.median([wall(stage) for _ in range(max(args.calls // 4, 3))]))
    say("Beside it: pvq_partition_ref on the %d Cb and Cr planes of the same frames against these references (leaf lists, "
        "gathers, band stage, resolve, choice on distortion, synthesis, scatters; Cb's quantisers for both; wall clock, "
        "stream drained): %.2f ms - the references are %.2f%% of it." % (F * PPF, sms, 100. * burst / sms))
    with open(args.out, "w") as f:
        f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
