#!/usr/bin/env python3
"""What SSIM costs a pipe step: F = 16 pictures of 1080p 4:2:0, chroma from luma, priced on the device.

    python tools/time_pipe_ssim.py [--parent-lib PATH]     # every configuration, one child process each
    python tools/time_pipe_ssim.py --config ssim            # one of them

  parent   the parent commit's library (--parent-lib: a build of the parent's sources, daala_amd.build.build_variant
           style, selected with ODHIP_LIB), metrics off, run TWICE: its own run-to-run range
  off      this library, metrics off - must lie inside the parent's range
  both     SSE + PSNR-HVS-M
  ssim     SSE + PSNR-HVS-M + SSIM
  kernel   k_ssim alone over the 16 luma and 32 chroma plane pairs of a step (odhip_ssim_planes, events round the
           call), against odhip_copy_ceiling (k_copy16): its algorithmic bytes are the two sample planes read once

A timed window is `--steps` back-to-back steps ending in flush + sync, wall clock; median over `--rounds` windows after
a warm-up window.  Every configuration runs as a child process under its own time limit, one after the other, and the
run stops at the first that fails.  Output: profiles/pipe_ssim.txt keeps a run of this tool."""
import argparse
import os
import subprocess
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def pictures(F, W, H):
    import bench
    frames = [bench.CONTENT["natural"](i, 1) for i in range(F)]
    luma = np.ascontiguousarray(np.stack([f[0][:H, :W] for f in frames]))
    chroma = np.ascontiguousarray(np.concatenate([np.stack([f[p][:H // 2, :W // 2] for f in frames]) for p in (1, 2)]))
    return luma, chroma


def one(args):
    import torch
    import daala_amd as D
    D.init(0)
    F, W, H = args.frames, 1920, 1080
    luma, chroma = pictures(F, W, H)
    cfg = args.config
    if cfg == "kernel":
        planes = [(torch.from_numpy(luma).cuda(), W, H), (torch.from_numpy(chroma).cuda(), W // 2, H // 2)]
        rec = [(torch.roll(p, 1, 2).contiguous(), w, h) for p, w, h in planes]
        total, nbytes = 0.0, 0
        for (s, w, h), (r, _, _) in zip(planes, rec):
            D.ssim_planes(s, r, w, h)
            ms = []
            for _ in range(args.rounds):
                a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                a.record()
                D.ssim_planes(s, r, w, h)
                b.record()
                torch.cuda.synchronize()
                ms.append(a.elapsed_time(b))
            total += float(np.median(ms))
            nbytes += 2 * s.shape[0] * w * h
            print("  k_ssim over %d pairs of %dx%d: median %.3f ms (call + readback included)"
                  % (s.shape[0], w, h, float(np.median(ms))), flush=True)
        print("config kernel: %.3f ms for one level of a step's planes, %.1f MB algorithmic = %.1f GB/s"
              % (total, nbytes / 1e6, nbytes / total / 1e6), flush=True)
        return
    pipe = D.Pipe(D.QuantTables.load(), F, W, H, chroma_cfl=True, price=True)
    pipe.set_pictures(luma, chroma)
    if cfg == "both":
        pipe.set_metrics(depth=2)
    elif cfg == "ssim":
        pipe.set_metrics(depth=2, ssim=True)

    def window(n):
        for _ in range(n):
            while True:
                try:
                    pipe.step()
                    break
                except D.ExportRingBusyError:           # both ring slots hold untaken steps: take the oldest
                    pipe.metrics_take(wait=True)
            if cfg in ("both", "ssim"):
                pipe.metrics_take(wait=False)
        pipe.flush()
        pipe.sync()
        if cfg in ("both", "ssim"):
            while pipe.metrics_take(wait=True) is not None:
                pass

    window(3)
    ms = []
    for _ in range(args.rounds):
        t0 = time.perf_counter()
        window(args.steps)
        ms.append((time.perf_counter() - t0) * 1e3 / args.steps)
    print("config %s%s: median %.3f ms/step over %d windows of %d steps (min %.3f, max %.3f)"
          % (cfg, " (parent library)" if os.environ.get("ODHIP_LIB") else "", float(np.median(ms)), args.rounds,
             args.steps, min(ms), max(ms)), flush=True)
    pipe.destroy()


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--config", choices=["off", "both", "ssim", "kernel"])
    ap.add_argument("--parent-lib")
    ap.add_argument("--frames", type=int, default=16)
    ap.add_argument("--steps", type=int, default=20)
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--limit", type=int, default=120, help="seconds per configuration")
    args = ap.parse_args()
    if args.config:
        return one(args)
    runs = [("off", args.parent_lib)] * 2 if args.parent_lib else []
    runs += [("off", None), ("both", None), ("ssim", None), ("kernel", None)]
    for cfg, lib in runs:
        env = dict(os.environ)
        if lib:
            env["ODHIP_LIB"] = os.path.abspath(lib)
        r = subprocess.run(["timeout", "-k", "10", str(args.limit), sys.executable, os.path.abspath(__file__),
                            "--config", cfg, "--frames", str(args.frames), "--steps", str(args.steps),
                            "--rounds", str(args.rounds)], env=env)
        if r.returncode:
            raise SystemExit("configuration %s failed with status %d: stopping" % (cfg, r.returncode))


if __name__ == "__main__":
    main()
