#!/usr/bin/env python3
"""What deciding a frame's block sizes on the device costs: odhip_bsize_decide + odhip_bsize_resolve on F = 16 luma
planes of the benchmark's 1080p natural content, edge-padded to 1920 x 1088 (multiples of 32).  Writes
profiles/bsize.txt.

    python tools/time_bsize.py

  keyframe   no prediction, quantiser 800 (50 << OD_COEFF_SHIFT)
  inter      the next picture of the sequence as the prediction, quantiser 800: (800 >> 4) > 40, the coding-gain
             adjustment is on

Per configuration: the kernel alone (k_bsize_cell between two events on the stream, median of `--calls` calls after a
warm-up), decide + resolve as a caller sees it (wall clock around both, stream drained), the relisted cells and the
histogram of the map.  Beside them, in the same process: odhip_copy_ceiling of the bytes the decision touches (the
planes read once, the map written once - the copy reads and writes each byte once) and one step of the frame-batch
pipe on the same pictures, so that a reader sees the share."""
import argparse
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
OUT = os.path.join(ROOT, "profiles", "bsize.txt")
F, W, H, CW, CH = 16, 1920, 1080, 1920, 1088
Q = 800


def content():
    """(luma [F + 1][CH][CW] edge-padded, luma [F][H][W], chroma [2F][H/2][W/2]) of the benchmark's natural content."""
    import bench
    frames = [bench.CONTENT["natural"](i, 1) for i in range(F + 1)]
    luma = np.stack([f[0][:H, :W] for f in frames])
    chroma = np.concatenate([np.stack([f[p][:H // 2, :W // 2] for f in frames[:F]]) for p in (1, 2)])
    padded = np.pad(luma, ((0, 0), (0, CH - H), (0, CW - W)), mode="edge")
    return np.ascontiguousarray(padded), np.ascontiguousarray(luma[:F]), np.ascontiguousarray(chroma)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--calls", type=int, default=10)
    ap.add_argument("--out", default=OUT)
    args = ap.parse_args()
    import torch
    import daala_amd as D
    D.init(0)
    lines = []

    def say(s):
        print(s, flush=True)
        lines.append(s)

    padded, luma, chroma = content()
    px = torch.from_numpy(padded[:F]).cuda()
    pred = torch.from_numpy(padded[1:]).cuda()
    cells = F * (CW // 32) * (CH // 32)
    say("Block sizes by activity masking - tools/time_bsize.py on one MI355X.")
    say("odhip_bsize_decide + odhip_bsize_resolve, F = %d luma planes of %d x %d (coded %d x %d: %d cells of 32 x 32), "
        "benchmark natural content, quantiser %d; median of %d calls after a warm-up call." % (F, W, H, CW, CH, cells, Q,
                                                                                                args.calls))
    for label, p in (("keyframe", None), ("inter", pred)):
        out = torch.empty((F, CH // 8, CW // 8), dtype=torch.uint8, device="cuda")
        kernel_ms, both_ms = [], []
        relisted = 0
        for i in range(args.calls + 1):
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record()
            D.bsize_decide(px, Q, p, out=out, resolve=False)
            e1.record()
            torch.cuda.synchronize()
            if i:
                kernel_ms.append(e0.elapsed_time(e1))
            t0 = time.perf_counter()
            _, relisted = D.bsize_decide(px, Q, p, out=out)
            torch.cuda.synchronize()
            if i:
                both_ms.append((time.perf_counter() - t0) * 1e3)
        hist = np.bincount(out.cpu().numpy().ravel(), minlength=4)
        nbytes = px.numel() * (2 if p is not None else 1) + out.numel()
        ceiling = D.copy_ceiling((nbytes // 2) & ~15, n=10)
        k = float(np.median(kernel_ms))
        say("  %-8s k_bsize_cell (events) %8.3f ms = %6.1f us per frame; decide + resolve (wall) %8.3f ms; relisted "
            "%d of %d cells = %.2e" % (label, k, k * 1e3 / F, float(np.median(both_ms)), relisted, cells,
                                       relisted / cells))
        say("           map entries 4x4 / 8x8 / 16x16 / 32x32: %s" % " / ".join(
            "%d (%.1f%%)" % (n, 100. * n / hist.sum()) for n in hist[:4]))
        say("           bytes touched %.1f MB -> %.0f GB/s; odhip_copy_ceiling of as many bytes: %.0f GB/s, i.e. %.3f ms"
            % (nbytes / 1e6, nbytes / k / 1e6, ceiling, nbytes / ceiling / 1e6))
    del px, pred
    pipe = D.Pipe(D.QuantTables.load(), F, W, H, chroma_cfl=True, price=True)
    pipe.set_pictures(luma, chroma)
    ms = []
    for i in range(args.calls + 1):
        pipe.sync()
        t0 = time.perf_counter()
        pipe.step()
        pipe.sync()
        if i:
            ms.append((time.perf_counter() - t0) * 1e3)
    pipe.destroy()
    say("One keyframe step of the frame-batch pipe on the same %d pictures (4:2:0, device-priced choice; wall clock, "
        "stream drained): %.2f ms." % (F, float(np.median(ms))))
    with open(args.out, "w") as f:
        f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
