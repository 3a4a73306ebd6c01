#!/usr/bin/env python3
"""What it costs an inter step to build its own prediction: F = 16 pictures of 1080p 4:2:0, priced on the device.

    python tools/time_pipe_mc.py                 # the four configurations, one child process each
    python tools/time_pipe_mc.py --config b      # one of them

  a  the prediction pictures resident (odhip_pipe_set_reference_pictures once): the floor - what the band stages
     cost when the prediction is free.  This path is the parent commit's, unchanged.
  b  reference frames and grids resident (odhip_pipe_set_reference_frames + odhip_pipe_set_mvs once): every step
     builds its prediction on its two chains.  b - a is the cost of the feature.
  c  as b, but the frames (two slots) and the grids of every step are fed from pinned memory
     (odhip_pipe_feed_reference_frames + odhip_pipe_feed_mvs) while the previous step computes.
  d  the only way to change predictions per step without this feature: odhip_pipe_set_reference_pictures before
     every step (syncs the pipe, copies synchronously).  The host-side motion compensation that would have to
     produce those pictures is NOT included: d is a lower bound for that way.

A timed window is `--steps` back-to-back steps ending in flush + sync, wall clock (the pipe runs two streams and a
copy stream; the window's end is the only common point); median over `--rounds` windows after a warm-up window.
Without --config every configuration runs as a child process under its own time limit, one after the other, and
the run stops at the first that fails."""
import argparse
import os
import subprocess
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def one(args):
    import torch
    import bench
    import daala_amd as D
    D.init(0)
    F, W, H = args.frames, 1920, 1080
    CW, CH = 1920, 1088
    frames = [bench.CONTENT["natural"](i, 1) for i in range(F)]
    luma = np.ascontiguousarray(np.stack([f[0][:H, :W] for f in frames]))
    chroma = np.ascontiguousarray(np.concatenate([np.stack([f[p][:H // 2, :W // 2] for f in frames]) for p in (1, 2)]))
    # two reference slots: the pictures themselves, edge-extended to the coded size, and a shifted copy
    rl = np.pad(luma, ((0, 0), (0, CH - H), (0, CW - W)), mode="edge")
    rc = np.pad(chroma, ((0, 0), (0, (CH - H) // 2), (0, (CW - W) // 2)), mode="edge")
    rl = [rl, np.ascontiguousarray(np.roll(rl, 3, 2))]
    rc = [rc, np.ascontiguousarray(np.roll(rc, 1, 2))]
    rng = np.random.RandomState(2)
    nh, nv = CW // 8, CH // 8
    grid = np.zeros((F, nv + 1, nh + 1), D.MV_POINT)
    valid = (rng.rand(nv + 1, nh + 1) < 0.3).astype(np.uint8)
    valid[::8, ::8] = 1
    grid["valid"] = valid
    grid["ref"] = rng.randint(0, 2, size=grid.shape)
    grid["mvx"] = rng.randint(-16*8, 16*8 + 1, size=grid.shape)
    grid["mvy"] = rng.randint(-16*8, 16*8 + 1, size=grid.shape)
    pipe = D.Pipe(D.QuantTables.load(), F, W, H, chroma_cfl=True, price=True, inter=True)
    pipe.set_pictures(luma, chroma)
    cfg = args.config
    if cfg in "ad":
        pl = D.mc_predict([torch.from_numpy(x).cuda() for x in rl], grid, dec=0).cpu().numpy()[:, :H, :W]
        pc = D.mc_predict([torch.from_numpy(x).cuda() for x in rc], grid, dec=1).cpu().numpy()[:, :H // 2, :W // 2]
        pl, pc = np.ascontiguousarray(pl), np.ascontiguousarray(pc)
        pipe.set_reference_pictures(pl, pc)
    else:
        pipe.set_reference_frames(rl, rc)
        pipe.set_mvs(grid)
    if cfg == "c":
        hl = [torch.from_numpy(x).pin_memory() for x in rl]
        hc = [torch.from_numpy(x).pin_memory() for x in rc]
        hg = torch.from_numpy(np.frombuffer(grid.tobytes(), np.uint8).copy()).pin_memory()
        g = hg.numpy().view(D.MV_POINT).reshape(grid.shape)

    def window(n):
        for _ in range(n):
            if cfg == "c":
                pipe.feed_reference_frames(hl, hc)
                pipe.feed_mvs(g)
            elif cfg == "d":
                pipe.set_reference_pictures(pl, pc)
            pipe.step()
        pipe.flush()
        pipe.sync()

    window(3)
    ms = []
    for _ in range(args.rounds):
        t0 = time.perf_counter()
        window(args.steps)
        ms.append((time.perf_counter() - t0)*1e3/args.steps)
    print("config %s: median %.3f ms/step over %d windows of %d steps (min %.3f, max %.3f)"
          % (cfg, float(np.median(ms)), args.rounds, args.steps, min(ms), max(ms)), flush=True)
    if cfg == "b":
        pipe.record(True)
        window(args.steps)
        t = pipe.timings()
        print("  exclusive stage averages (ms per launch group; the pad stages are the prediction here): "
              + ", ".join("%s %.3f" % (k, v[0]) for k, v in t.items()), flush=True)
    pipe.destroy()


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--config", choices=list("abcd"))
    ap.add_argument("--frames", type=int, default=16)
    ap.add_argument("--steps", type=int, default=20)
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--limit", type=int, default=240, help="seconds per configuration")
    args = ap.parse_args()
    if args.config:
        return one(args)
    for cfg in "abcd":
        r = subprocess.run(["timeout", "-k", "10", str(args.limit), sys.executable, os.path.abspath(__file__),
                            "--config", cfg, "--frames", str(args.frames), "--steps", str(args.steps),
                            "--rounds", str(args.rounds)])
        if r.returncode:
            raise SystemExit("configuration %s failed with status %d: stopping" % (cfg, r.returncode))


if __name__ == "__main__":
    main()
