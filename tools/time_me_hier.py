#!/usr/bin/env python3
"""What the coarse-to-fine motion search costs and finds against the exhaustive one: F = 16 pictures of 1080p, 16 x 16
blocks, two slots, 1/8 pel, in one process on one device.  Writes profiles/me_hier.txt.

    python tools/time_me_hier.py

  (a) odhip_me_search2 at range 16          (b) odhip_me_search2 at range 32
  (c) odhip_me_search3, levels 2, range 8, refine 2: the reach of (b)
  (d) odhip_me_search3, levels 2, range 32, refine 2: +-128 pixels

  search   the stand-alone call (for (c) and (d) the pyramids, the coarse levels, level 0 and stage 2): device events
           round `--calls` back-to-back calls, median of `--rounds` such windows after a warm-up window, the cases
           alternating.  The same call with res = 3 leaves stage 2 out: everything in front of k_me_subpel.
  agree    on the bench content: the share of points where (c) returns the vector and slot of (b), and the cost of
           (c) over the cost of (b) - the ratio of the sums and the mean of the per-point ratios where (b) is not 0.
  pipe     the inter step with each search on, one pipe per case, the windows alternating: wall clock over `--steps`
           back-to-back steps ending in flush + sync."""
import argparse
import ctypes
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tools"))
OUT = os.path.join(ROOT, "profiles", "me_hier.txt")
LG, RES, LAM = 1, 0, 4
CASES = [("(a) exhaustive, range 16", 16, 0, 1), ("(b) exhaustive, range 32", 32, 0, 1),
         ("(c) levels 2, range 8, refine 2", 8, 2, 2), ("(d) levels 2, range 32, refine 2", 32, 2, 2)]


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--calls", type=int, default=5)
    ap.add_argument("--steps", type=int, default=10)
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--flags", type=int, default=0, help="ODHIP_ME_CHROMA | ODHIP_ME_SATD")
    ap.add_argument("--out", default=OUT)
    args = ap.parse_args()
    import torch
    import daala_amd as D
    from time_me import content, F, W, H, CW, CH
    D.init(0)
    luma, chroma, rl, rc = content()
    d_src, d_csrc = torch.from_numpy(luma).cuda(), torch.from_numpy(chroma).cuda()
    d_refs, d_crefs = [torch.from_numpy(x).cuda() for x in rl], [torch.from_numpy(x).cuda() for x in rc]
    lines = ["Coarse-to-fine motion search - tools/time_me_hier.py on one MI355X.", ""]

    def say(s):
        print(s, flush=True)
        lines.append(s)

    say("F = %d pictures of %d x %d (coded %d x %d), 16 x 16 blocks, two slots, res 0, lambda %d, flags %d."
        % (F, W, H, CW, CH, LAM, args.flags))
    L = D.lib()
    shape = (F, CH // 8 + 1, CW // 8 + 1)
    jobs, keep, keep3, found = {}, [], [], {}
    for name, rng, levels, refine in CASES:
        job, scratch = D.api._me_job3(d_src, d_refs, W, H, LG, rng, RES, LAM, LAM, args.flags, d_csrc, d_crefs, 1, levels,
                                      refine)
        grid = torch.empty(shape + (D.MV_POINT.itemsize,), dtype=torch.uint8, device="cuda")
        cost = torch.empty(shape, dtype=torch.int32, device="cuda")
        job.base.luma.grid, job.base.luma.cost = grid.data_ptr(), cost.data_ptr()
        keep.append((scratch, grid, cost))
        jobs[name] = job
        # the same job without stage 2, into buffers of its own
        job3, scratch3 = D.api._me_job3(d_src, d_refs, W, H, LG, rng, 3, LAM, LAM, args.flags, d_csrc, d_crefs, 1, levels,
                                        refine)
        grid3 = torch.empty_like(grid)
        job3.base.luma.grid = grid3.data_ptr()
        keep3.append((scratch3, grid3))
        jobs[name + " res 3"] = job3

    def window(job):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        for _ in range(args.calls):
            rc_ = L.odhip_me_search3(ctypes.byref(job), ctypes.c_void_p(torch.cuda.current_stream().cuda_stream))
            assert rc_ == 0, rc_
        b.record()
        b.synchronize()
        return a.elapsed_time(b)/args.calls

    ms = {k: [] for k in jobs}
    for job in jobs.values():
        window(job)
    for _ in range(args.rounds):
        for k, job in jobs.items():
            ms[k].append(window(job))
    say("")
    say("The stand-alone search, ms per call (median of %d windows of %d calls, min, max), the same without stage 2, "
        "scratch:" % (args.rounds, args.calls))
    for (name, _, _, _), (scratch, grid, cost) in zip(CASES, keep):
        v = ms[name]
        say("  %-34s %8.3f ms (min %.3f, max %.3f)  res 3: %7.3f ms  scratch %.1f MiB"
            % (name, float(np.median(v)), min(v), max(v), float(np.median(ms[name + " res 3"])),
               (scratch.numel() if scratch is not None else 0)/2.0**20))
        found[name] = (grid.cpu().numpy().view(D.MV_POINT).reshape(shape), cost.cpu().numpy().view(np.uint32))

    s = 1 << LG
    say("")
    say("Agreement on this content (the slots are the pictures moved by 5 and 3 pixels), valid points only:")
    gb, cb = (x[:, ::s, ::s] for x in found[CASES[1][0]])
    for name in (CASES[0][0], CASES[2][0], CASES[3][0]):
        g, c = (x[:, ::s, ::s] for x in found[name])
        same = (g["mvx"] == gb["mvx"]) & (g["mvy"] == gb["mvy"]) & (g["ref"] == gb["ref"])
        nz = cb > 0
        say("  %-34s same vector and slot as (b) at %.2f %% of %d points; cost sum / (b)'s %.4f, mean ratio %.4f; "
            "longest component %d"
            % (name, 100*same.mean(), same.size, c.sum(dtype=np.float64)/cb.sum(dtype=np.float64),
               float((c[nz]/cb[nz].astype(np.float64)).mean()), max(np.abs(g["mvx"]).max(), np.abs(g["mvy"]).max())))

    qt = D.QuantTables.load()
    pipes = {}
    for name, rng, levels, refine in CASES:
        p = D.Pipe(qt, F, W, H, chroma_cfl=True, price=True, inter=True)
        p.set_pictures(luma, chroma)
        p.set_reference_frames(rl, rc)
        p.set_motion_search3(LG, rng, RES, LAM, LAM, args.flags, levels, refine)
        pipes[name] = p

    def steps(p, n):
        t0 = time.perf_counter()
        for _ in range(n):
            p.step()
        p.flush()
        p.sync()
        return (time.perf_counter() - t0)*1e3/n

    for p in pipes.values():
        steps(p, 3)
    pms = {k: [] for k in pipes}
    for _ in range(args.rounds):
        for k, p in pipes.items():
            pms[k].append(steps(p, args.steps))
    say("")
    say("Inter step with the search on, F = %d 1080p 4:2:0, priced on the device; wall clock per step, median of %d "
        "windows of %d steps, the pipes alternating:" % (F, args.rounds, args.steps))
    for k, v in pms.items():
        say("  %-34s %8.3f ms/step (min %.3f, max %.3f)" % (k, float(np.median(v)), min(v), max(v)))
    for p in pipes.values():
        p.destroy()
    with open(args.out, "w") as f:
        f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
