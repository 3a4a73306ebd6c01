#!/usr/bin/env python3
"""What the motion search at variable block sizes costs beyond the uniform searches it is made of: F = 16 pictures of
1080p, two slots, range 16, 1/8 pel, sizes (1, 3) and (0, 3), in one process on one device.  Writes
profiles/me_vbs.txt.

    python tools/time_me_vbs.py

  call      odhip_me_search_vbs: device events round `--calls` back-to-back calls, median of `--rounds` such windows
            after a warm-up window, all cases alternating.
  searches  odhip_me_search3 at each size on its own, the uniform search's code path and legality, levels cut to
            log_size + 1 as the call cuts them.
  predicts  odhip_mc_predict_planes of each of those grids: luma, 8-bit, dec 0.
  new       call - searches - predicts of its sizes: what k_me_cell_dist, k_me_vbs_decide and k_me_vbs_grid cost (the
            call's searches run under another legality predicate, which moves a few vectors at the frame's edges).
  cell_dist odhip_me_cell_dist alone on the call's number of predictions: (nsizes + 1) bytes per picture sample read,
            over its time, beside odhip_copy_ceiling (bytes read + written) on the same device.  "warm" repeats the
            call on one set of predictions, which the device's last-level cache holds, as it holds what the call's own
            predictions have just written; "cold" goes round `--sets` sets, more than that cache holds."""
import argparse
import ctypes
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tools"))
OUT = os.path.join(ROOT, "profiles", "me_vbs.txt")
RNG, RES, LAM, PENALTY = 16, 0, 4, 64
SIZES = [(1, 3), (0, 3)]


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--calls", type=int, default=3)
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--flags", type=int, default=0, help="ODHIP_ME_CHROMA | ODHIP_ME_SATD")
    ap.add_argument("--levels", type=int, default=0)
    ap.add_argument("--refine", type=int, default=2)
    ap.add_argument("--sets", type=int, default=5)
    ap.add_argument("--out", default=OUT)
    args = ap.parse_args()
    import torch
    import daala_amd as D
    from time_me import content, F, W, H, CW, CH
    D.init(0)
    luma, chroma, rl, rc = content()
    d_src, d_csrc = torch.from_numpy(luma).cuda(), torch.from_numpy(chroma).cuda()
    d_refs, d_crefs = [torch.from_numpy(x).cuda() for x in rl], [torch.from_numpy(x).cuda() for x in rc]
    lines = ["Motion search at variable block sizes - tools/time_me_vbs.py on one MI355X.", ""]

    def say(s):
        print(s, flush=True)
        lines.append(s)

    say("F = %d pictures of %d x %d (coded %d x %d), two slots, range %d, res %d, lambda %d, flags %d, levels %d, "
        "split_penalty %d." % (F, W, H, CW, CH, RNG, RES, LAM, args.flags, args.levels, PENALTY))
    L = D.lib()
    stream = lambda: ctypes.c_void_p(torch.cuda.current_stream().cuda_stream)      # noqa: E731
    shape = (F, CH // 8 + 1, CW // 8 + 1)
    work, keep = {}, []

    def buffers():
        grid = torch.empty(shape + (D.MV_POINT.itemsize,), dtype=torch.uint8, device="cuda")
        cost = torch.empty(shape, dtype=torch.int32, device="cuda")
        return grid, cost

    # the uniform searches and the predictions of their grids
    grids = {}
    for lg in range(4):
        job, scratch = D.api._me_job3(d_src, d_refs, W, H, lg, RNG, RES, LAM, LAM, args.flags, d_csrc, d_crefs, 1,
                                      min(args.levels, lg + 1), args.refine)
        grid, cost = buffers()
        job.base.luma.grid, job.base.luma.cost = grid.data_ptr(), cost.data_ptr()
        keep.append((job, scratch, grid, cost))
        grids[lg] = grid
        work["search %d" % lg] = lambda job=job: L.odhip_me_search3(ctypes.byref(job), stream())
        pred = torch.empty_like(d_refs[0])
        keep.append(pred)
        work["predict %d" % lg] = lambda lg=lg, pred=pred: (D.mc_predict(d_refs, grids[lg].view(-1), 0, pred), 0)[1]
    # the calls
    found = {}
    for lo, hi in SIZES:
        job, scratch = D.api._me_job4(d_src, d_refs, W, H, lo, hi, RNG, RES, LAM, LAM, args.flags, d_csrc, d_crefs, 1,
                                      args.levels, args.refine, PENALTY)
        grid, cost = buffers()
        job.base.base.luma.grid, job.base.base.luma.cost = grid.data_ptr(), cost.data_ptr()
        keep.append((job, scratch, grid, cost))
        found[lo, hi] = (grid, scratch)
        work["call %d %d" % (lo, hi)] = lambda job=job: L.odhip_me_search_vbs(ctypes.byref(job), stream())
        # step 3 alone on as many predictions (their content does not change its time)
        n = hi - lo + 1
        sets = []
        for _ in range(args.sets):
            preds = [torch.empty_like(d_refs[0]).copy_(d_refs[k & 1]) for k in range(n)]
            sets.append((preds, (ctypes.c_void_p * n)(*[t.data_ptr() for t in preds])))
        dist = torch.empty((n, F, CH // 8, CW // 8), dtype=torch.int32, device="cuda")
        cjob = D.api._me_job(d_src, d_refs, W, H, 0, 0, 0, 0)
        turn = [0]
        keep.append((sets, dist, cjob))

        def cell_dist(step, cjob=cjob, sets=sets, n=n, dist=dist, turn=turn):
            turn[0] = (turn[0] + step) % len(sets)
            return L.odhip_me_cell_dist(ctypes.byref(cjob), sets[turn[0]][1], n, ctypes.c_void_p(dist.data_ptr()),
                                        stream())

        work["cell_dist %d warm" % n] = lambda f=cell_dist: f(0)
        work["cell_dist %d cold" % n] = lambda f=cell_dist: f(1)

    def window(fn, calls):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        for _ in range(calls):
            rc_ = fn()
            assert rc_ == 0, rc_
        b.record()
        b.synchronize()
        return a.elapsed_time(b)/calls

    calls = {k: args.calls*(20 if k.startswith("cell_dist") else 1) for k in work}
    ms = {k: [] for k in work}
    for k, fn in work.items():
        window(fn, calls[k])
    for _ in range(args.rounds):
        for k, fn in work.items():
            ms[k].append(window(fn, calls[k]))
    med = {k: float(np.median(v)) for k, v in ms.items()}
    say("")
    say("ms per call: median of %d windows of %d calls (cell_dist: %d), min, max; all cases alternating:"
        % (args.rounds, args.calls, 20*args.calls))
    for k, v in ms.items():
        say("  %-18s %9.3f ms (min %.3f, max %.3f)" % (k, med[k], min(v), max(v)))
    say("")
    say("The call against its parts:")
    for lo, hi in SIZES:
        searches = sum(med["search %d" % lg] for lg in range(lo, hi + 1))
        predicts = sum(med["predict %d" % lg] for lg in range(lo, hi + 1))
        call = med["call %d %d" % (lo, hi)]
        leaves = D.mc_leaves(found[lo, hi][0].cpu().numpy().view(D.MV_POINT).reshape(shape)[:1], CW, CH)[0]
        sizes = np.bincount(leaves >> 24 & 3, minlength=4)
        say("  sizes %d..%d: call %.3f ms = searches %.3f + predictions %.3f + new kernels %.3f ms (%.1f %% of the call); "
            "scratch %.1f MiB; leaves of picture 0 by size: %s"
            % (lo, hi, call, searches, predicts, call - searches - predicts, 100*(call - searches - predicts)/call,
               found[lo, hi][1].numel()/2.0**20, sizes.tolist()))
    ceiling = D.copy_ceiling(1 << 30, 10)
    say("")
    say("k_me_cell_dist alone against the copy kernels (odhip_copy_ceiling: %.0f GB/s read + written):" % ceiling)
    for lo, hi in SIZES:
        n = hi - lo + 1
        moved = (n + 1)*F*W*H + 4*n*F*(CH // 8)*(CW // 8)
        for how in ("warm", "cold"):
            t = med["cell_dist %d %s" % (n, how)]
            say("  %d predictions, %s: %.3f ms for %.1f MB read and written: %.0f GB/s, %.0f %% of the copy rate"
                % (n, how, t, moved/1e6, moved/t/1e6, 100*moved/t/1e6/ceiling))
    with open(args.out, "w") as f:
        f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
