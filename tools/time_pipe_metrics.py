#!/usr/bin/env python3
"""What measuring every step costs: a 16-frame 1080p 4:2:0 step (bench.py's configuration: chroma from luma, priced
on the device) timed with metrics off, with SSE alone and with SSE + PSNR-HVS-M, alternating the three pipes.

    python tools/time_pipe_metrics.py [--frames 16] [--steps 20] [--rounds 3]

Each timed window is `steps` back-to-back steps of one pipe ending in flush + sync, the metrics of every step taken
as soon as the next step has been enqueued (a streaming consumer); ms per step is printed per round and as the
median over the rounds.
"""
import argparse
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--frames", type=int, default=16)
    ap.add_argument("--steps", type=int, default=20)
    ap.add_argument("--rounds", type=int, default=3)
    ap.add_argument("--width", type=int, default=1920)
    ap.add_argument("--height", type=int, default=1080)
    args = ap.parse_args()
    import bench
    import daala_amd as D
    D.init(0)
    F, W, H = args.frames, args.width, args.height
    frames = [bench.CONTENT["natural"](i, 1) for i in range(F)]
    luma = np.stack([f[0][:H, :W] for f in frames])
    chroma = np.concatenate([np.stack([f[p][:H // 2, :W // 2] for f in frames]) for p in (1, 2)])
    qt = D.QuantTables.load()
    configs = (("off", None), ("sse", (True, False)), ("sse+psnrhvs", (True, True)))
    pipes = {}
    for name, m in configs:
        p = D.Pipe(qt, F, W, H, chroma_cfl=True, price=True)
        p.set_pictures(np.ascontiguousarray(luma), np.ascontiguousarray(chroma))
        if m:
            p.set_metrics(sse=m[0], psnrhvs=m[1], depth=3)
        pipes[name] = p

    def run(p, n):
        taken = 0
        for _ in range(n):
            p.step()
            while p.metrics_layout().flags and p.metrics_take(wait=False) is not None:
                taken += 1
        p.flush()
        p.sync()
        while p.metrics_layout().flags and p.metrics_take(wait=False) is not None:
            taken += 1
        return taken

    for p in pipes.values():
        run(p, 3)                                   # warm-up
    res = {name: [] for name, _ in configs}
    for r in range(args.rounds):
        for name, _ in configs:
            p = pipes[name]
            t0 = time.perf_counter()
            taken = run(p, args.steps)
            ms = (time.perf_counter() - t0) * 1e3 / args.steps
            res[name].append(ms)
            print("round %d %-12s %.3f ms/step (%d steps measured)" % (r, name, ms, taken), flush=True)
    base = float(np.median(res["off"]))
    for name, _ in configs:
        med = float(np.median(res[name]))
        print("median %-12s %.3f ms/step  (%+.3f ms, %+.1f%% vs off)" % (name, med, med - base,
                                                                       100 * (med / base - 1)))
    m = None
    p = pipes["sse+psnrhvs"]
    p.step()
    p.flush()
    while True:
        t = p.metrics_take()
        if t is None:
            break
        m = t
    if m is not None:
        ps, hv = m.psnr(), m.psnrhvs()
        print("last step, picture 0, level 0: luma PSNR %.4f dB, PSNR-HVS-M %.4f dB" % (ps[0][0, 0], hv[0][0, 0]))
    for p in pipes.values():
        p.destroy()


if __name__ == "__main__":
    main()
