#!/usr/bin/env python3
"""What FastSSIM costs a pipe step: F = 16 pictures of 1080p 4:2:0, chroma from luma, priced on the device.

    python tools/time_pipe_fastssim.py                  # every configuration, one child process each
    python tools/time_pipe_fastssim.py --config fast    # one of them

  off      metrics off (flags 0)
  alone    FastSSIM alone (flags 16): against `off`, the column by itself
  three    SSE + PSNR-HVS-M + SSIM (flags 7)
  msssim   ... + MS-SSIM (flags 15): against `three`, what MS-SSIM costs - the figure of profiles/pipe_msssim.txt again,
           in this session
  fast     ... + FastSSIM (flags 31): against `msssim`, the same pipe with the bit clear
  kernel   odhip_fastssim_planes alone over 16 luma pairs of 1080p (pair array, sums and scratch made ahead: events
           round the launches only, on the null stream as the events are), against odhip_copy_ceiling (k_copy16): its
           algorithmic bytes are both sample planes read once plus both pyramids (int32, levels 0..3) written once and
           read once; and odhip_msssim_planes over the same pairs, for the comparison

A timed window is `--steps` back-to-back steps ending in flush + sync, wall clock; median over `--rounds` windows after
a warm-up window.  Every configuration runs as a child process under its own time limit, one after the other, and the
run stops at the first that fails.  Output: profiles/pipe_fastssim.txt keeps a run of this tool."""
import argparse
import os
import subprocess
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

FLAGS = {"off": 0, "alone": 16, "three": 7, "msssim": 15, "fast": 31}


def pictures(F, W, H):
    import bench
    frames = [bench.CONTENT["natural"](i, 1) for i in range(F)]
    luma = np.ascontiguousarray(np.stack([f[0][:H, :W] for f in frames]))
    chroma = np.ascontiguousarray(np.concatenate([np.stack([f[p][:H // 2, :W // 2] for f in frames]) for p in (1, 2)]))
    return luma, chroma


def kernel(args, D, luma, W, H):
    import ctypes
    import torch
    from daala_amd.api import _metric_pairs
    F = args.frames
    s = torch.from_numpy(luma).cuda()
    r = torch.roll(s, 1, 2).contiguous()
    # only the launches lie between the events: the pair array, the sums and the scratch exist before
    pairs, n = _metric_pairs(s, r, W, H, 8, D.CSF_Y, None, None)
    # one buffer for both calls: MS-SSIM writes [n][5], FastSSIM the first [n][4] doubles of it; nothing reads it
    d_sums = torch.zeros((n, 5), dtype=torch.float64, device="cuda")
    L = D.lib()
    assert L.odhip_fastssim_prepare(W, H, n) == 0 and L.odhip_msssim_prepare(W, H, n) == 0
    out = ctypes.c_void_p(d_sums.data_ptr())

    def fast():
        assert L.odhip_fastssim_planes(pairs, n, out, None) == 0

    def ms5():
        assert L.odhip_msssim_planes(pairs, n, out, None, None) == 0

    ceiling = D.copy_ceiling()
    for name, call, nbytes in (
            ("odhip_fastssim_planes", fast,
             F * (2 * W * H + 2 * 2 * 4 * sum(a * b for a, b in (D.fastssim_level_size(W, H, l) for l in range(4))))),
            ("odhip_msssim_planes", ms5, F * (2 * W * H + 2 * 2 * 4 * sum((W >> i) * (H >> i) for i in range(1, 5))))):
        call()
        torch.cuda.synchronize()
        ms = []
        for _ in range(args.rounds):
            a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            a.record()
            call()
            b.record()
            torch.cuda.synchronize()
            ms.append(a.elapsed_time(b))
        t = float(np.median(ms))
        gbs = nbytes / t / 1e6
        print("config kernel: %s over %d pairs of %dx%d: median %.3f ms (the launches alone, min %.3f, max %.3f); "
              "%.1f MB algorithmic = %.1f GB/s = %.1f %% of k_copy16 (%.1f GB/s)"
              % (name, F, W, H, t, min(ms), max(ms), nbytes / 1e6, gbs, 100 * gbs / ceiling, ceiling), flush=True)


def one(args):
    import daala_amd as D
    D.init(0)
    F, W, H = args.frames, 1920, 1080
    luma, chroma = pictures(F, W, H)
    cfg = args.config
    if cfg == "kernel":
        return kernel(args, D, luma, W, H)
    pipe = D.Pipe(D.QuantTables.load(), F, W, H, chroma_cfl=True, price=True)
    pipe.set_pictures(luma, chroma)
    flags = FLAGS[cfg]
    if flags:
        on = lambda bit: bool(flags & bit)
        pipe.set_metrics(sse=on(D.METRIC_SSE), psnrhvs=on(D.METRIC_PSNRHVS), depth=2, ssim=on(D.METRIC_SSIM),
                         msssim=on(D.METRIC_MSSSIM), fastssim=on(D.METRIC_FASTSSIM))
        assert pipe.metrics_layout().flags == flags

    def window(n):
        for _ in range(n):
            while True:
                try:
                    pipe.step()
                    break
                except D.ExportRingBusyError:           # both ring slots hold untaken steps: take the oldest
                    pipe.metrics_take(wait=True)
            if flags:
                pipe.metrics_take(wait=False)
        pipe.flush()
        pipe.sync()
        if flags:
            while pipe.metrics_take(wait=True) is not None:
                pass

    window(3)
    ms = []
    for _ in range(args.rounds):
        t0 = time.perf_counter()
        window(args.steps)
        ms.append((time.perf_counter() - t0) * 1e3 / args.steps)
    print("config %s (flags %d): median %.3f ms/step over %d windows of %d steps (min %.3f, max %.3f)"
          % (cfg, flags, float(np.median(ms)), args.rounds, args.steps, min(ms), max(ms)), flush=True)
    pipe.destroy()


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--config", choices=sorted(FLAGS) + ["kernel"])
    ap.add_argument("--frames", type=int, default=16)
    ap.add_argument("--steps", type=int, default=20)
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--limit", type=int, default=120, help="seconds per configuration")
    args = ap.parse_args()
    if args.config:
        return one(args)
    for cfg in ("off", "alone", "three", "msssim", "fast", "kernel"):
        r = subprocess.run(["timeout", "-k", "10", str(args.limit), sys.executable, os.path.abspath(__file__),
                            "--config", cfg, "--frames", str(args.frames), "--steps", str(args.steps),
                            "--rounds", str(args.rounds)])
        if r.returncode:
            raise SystemExit("configuration %s failed with status %d: stopping" % (cfg, r.returncode))


if __name__ == "__main__":
    main()
