#!/usr/bin/env python3
"""What CIEDE2000 costs: k_ciede alone and as a column of a pipe step, F = 16 pictures of 1080p.

    python tools/time_ciede.py                  # every configuration, one child process each
    python tools/time_ciede.py --config kernel  # one of them

  kernel   odhip_ciede_pictures alone (pair array, sums and scratch made ahead: events round the launches only):
           16 pairs of 1080p at 4:2:0 and at 4:4:4, every pair its own source; then the 80 pairs of a pipe step - 16
           source pictures with five reconstructions each - once as the library runs them, the source's Lab computed
           once per tile for the run of five, and once with every pair computing it again
           (ODHIP_CIEDE_NO_RUNS=1, which only the experiments build reads: the child is started with it)
  off      a pipe, metrics off (flags 0)
  fast     SSE + PSNR-HVS-M + SSIM + MS-SSIM + FastSSIM (flags 31)
  all      ... + CIEDE2000 (flags 63): against `fast`, the same pipe with the bit clear
  alone    CIEDE2000 alone (flags 32): against `off`, the column by itself, which includes the luma chain of a step no
           longer overlapping the chroma chain of the step before

A pipe window is `--steps` back-to-back steps ending in flush + sync, wall clock; median over `--rounds` windows after a
warm-up window.  Every configuration runs as a child process under its own time limit, one after the other, and the run
stops at the first that fails.  profiles/ciede.txt keeps a run of this tool."""
import argparse
import os
import subprocess
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

FLAGS = {"off": 0, "fast": 31, "all": 63, "alone": 32}


def pictures(F, W, H):
    import bench
    frames = [bench.CONTENT["natural"](i, 1) for i in range(F)]
    luma = np.ascontiguousarray(np.stack([f[0][:H, :W] for f in frames]))
    chroma = np.ascontiguousarray(np.concatenate([np.stack([f[p][:H // 2, :W // 2] for f in frames]) for p in (1, 2)]))
    return luma, chroma


def kernel(args, D, luma, chroma, W, H):
    import ctypes
    import torch
    from daala_amd.api import _CiedePair, _ciede_pair
    F = args.frames
    L = D.lib()
    y = torch.from_numpy(luma).cuda()
    c = torch.from_numpy(chroma).cuda()
    c4 = torch.repeat_interleave(torch.repeat_interleave(c, 2, 1), 2, 2).contiguous()

    def noisy(t, k):
        g = torch.Generator(device="cuda").manual_seed(k)
        n = torch.randint(-3, 4, t.shape, generator=g, device="cuda", dtype=torch.int16)
        return (t.to(torch.int16) + n).clamp(0, 255).to(torch.uint8)

    def pairs_of(cp, nrec):
        recs = [(noisy(y, 10 + k), noisy(cp, 20 + k)) for k in range(nrec)]
        out = (_CiedePair * (F * nrec))()
        for k, (ry, rc) in enumerate(recs):
            for f in range(F):
                out[k * F + f] = _ciede_pair((y[f], cp[f], cp[F + f]), (ry[f], rc[f], rc[F + f]), W, H, 8, None, None)
        return out, recs

    runs = os.environ.get("ODHIP_CIEDE_NO_RUNS", "0") in ("", "0")
    for name, cp, nrec in (("4:2:0", c, 1), ("4:4:4", c4, 1), ("4:2:0, five reconstructions per source", c, 5)):
        pairs, keep = pairs_of(cp, nrec)
        n = F * nrec
        d = torch.zeros(n, dtype=torch.float64, device="cuda")
        assert L.odhip_ciede_prepare(W, H, n) == 0
        call = lambda: L.odhip_ciede_pictures(pairs, n, ctypes.c_void_p(d.data_ptr()), None)
        assert call() == 0
        torch.cuda.synchronize()
        ms = []
        for _ in range(args.rounds):
            a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            a.record()
            assert call() == 0
            b.record()
            torch.cuda.synchronize()
            ms.append(a.elapsed_time(b))
        t = float(np.median(ms))
        print("config kernel (%s): odhip_ciede_pictures over %d pairs of %dx%d %s: median %.3f ms (min %.3f, max %.3f) "
              "= %.2f ns per pixel pair" % ("runs share the source's Lab" if runs else "every pair computes its source's Lab",
                                           n, W, H, name, t, min(ms), max(ms), t * 1e6 / (n * W * H)), flush=True)
        del keep


def one(args):
    import daala_amd as D
    D.init(0)
    F, W, H = args.frames, 1920, 1080
    luma, chroma = pictures(F, W, H)
    cfg = args.config
    if cfg == "kernel":
        return kernel(args, D, luma, chroma, W, H)
    pipe = D.Pipe(D.QuantTables.load(), F, W, H, chroma_cfl=True, price=True)
    pipe.set_pictures(luma, chroma)
    flags = FLAGS[cfg]
    if flags:
        on = lambda bit: bool(flags & bit)
        pipe.set_metrics(sse=on(D.METRIC_SSE), psnrhvs=on(D.METRIC_PSNRHVS), depth=2, ssim=on(D.METRIC_SSIM),
                         msssim=on(D.METRIC_MSSSIM), fastssim=on(D.METRIC_FASTSSIM), ciede=on(D.METRIC_CIEDE))
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
    import daala_amd
    for cfg, env in (("kernel", {}), ("kernel", {"ODHIP_CIEDE_NO_RUNS": "1", "ODHIP_LIB": daala_amd.EXPERIMENTS_LIB}),
                     ("off", {}), ("fast", {}), ("all", {}), ("alone", {})):
        r = subprocess.run(["timeout", "-k", "10", str(args.limit), sys.executable, os.path.abspath(__file__),
                            "--config", cfg, "--frames", str(args.frames), "--steps", str(args.steps),
                            "--rounds", str(args.rounds)], env=dict(os.environ, **env))
        if r.returncode:
            raise SystemExit("configuration %s failed with status %d: stopping" % (cfg, r.returncode))


if __name__ == "__main__":
    main()
