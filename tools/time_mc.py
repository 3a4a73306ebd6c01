#!/usr/bin/env python3
"""Time odhip_mc_predict_planes at the bench shape: F = 16 pictures of 1080p 4:2:0 (coded 1920x1088), one
luma plane set and one chroma plane set (2F planes), 8-bit and full-precision samples, two reference slots.

`python tools/time_mc.py [--runs N]`: HIP events round each call (classification and the four prediction
launches; the grid is resident on the device, no copy is timed), median over the runs after a warm-up, for
three kinds of grid: every 64x64 cell unsplit, a mixed quadtree, every cell split down to 8x8.  Bytes are the algorithmic ones: every destination sample
written once, every reference sample read once per distinct corner vector is NOT counted (windows overlap and
hit the caches), so the rate printed is destination + one reference read: a LOWER bound of the
traffic the kernels cause (a 16x16 tile stages (16 + 5)^2 = 1.7 tile areas per distinct corner vector)."""
import argparse
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--runs", type=int, default=15)
    args = ap.parse_args()
    import torch
    import daala_amd as D
    import _mc_ref as R
    D.init(0)
    F, W, H = 16, 1920, 1088
    nh, nv = W // 8, H // 8
    rng = np.random.RandomState(1)
    kinds = {}
    for name, p in (("unsplit", 0.0), ("mixed", 0.5), ("all 8x8", 1.0)):
        valid = (rng.rand(nv + 1, nh + 1) < p).astype(np.uint8)
        valid[::8, ::8] = 1
        g = np.zeros((F, nv + 1, nh + 1), D.MV_POINT)
        g["valid"] = valid
        g["ref"] = rng.randint(0, 2, size=g.shape)
        g["mvx"] = rng.randint(-24*8, 24*8 + 1, size=g.shape)
        g["mvy"] = rng.randint(-24*8, 24*8 + 1, size=g.shape)
        assert D.mc_check_grid(g, W, H, 0, 2) == 0 and D.mc_check_grid(g, W, H, 1, 2) == 0
        kinds[name] = (g, len(R.leaves(valid)))
    print("odhip_mc_predict_planes, F = %d, %dx%d coded, median of %d runs" % (F, W, H, args.runs))
    for dt, label, nbytes in ((torch.uint8, "8-bit", 1), (torch.int16, "12-bit int16", 2)):
        for dec, nplanes, what in ((0, F, "luma"), (1, 2*F, "chroma 4:2:0")):
            h, w = H >> dec, W >> dec
            refs = [torch.randint(0, 256 if nbytes == 1 else 4096, (nplanes, h, w), device="cuda").to(dt)
                    for _ in range(2)]
            out = torch.empty_like(refs[0])
            for name, (g, nleaves) in kinds.items():
                dgrid = torch.from_numpy(np.frombuffer(g.tobytes(), np.uint8).copy()).cuda()
                times = []
                for run in range(args.runs + 3):
                    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                    a.record()
                    D.mc_predict(refs, dgrid, dec=dec, out=out)
                    b.record()
                    torch.cuda.synchronize()
                    if run >= 3:
                        times.append(a.elapsed_time(b)*1e3)
                us = float(np.median(times))
                moved = 2.0*nplanes*h*w*nbytes
                print("  %-13s %-13s %-8s %6d leaves/picture  %8.1f us  %6.1f MB  %5.2f TB/s"
                      % (label, what, name, nleaves, us, moved/1e6, moved/us/1e6))


if __name__ == "__main__":
    main()
