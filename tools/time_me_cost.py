#!/usr/bin/env python3
"""What chroma in the cost and SATD as the sub-pel metric cost the motion search: F = 16 pictures of 1080p 4:2:0.
Writes profiles/me_cost.txt.

    python tools/time_me_cost.py                 # resources, kernels, pipe: one child process per part
    python tools/time_me_cost.py --part noflags  # one of them (resources needs hipcc and no GPU)

  resources  the compiler's figures of the instantiations of me_kernels.hip that serve the flags: k_me_fullpel<LG, CH>
             with chroma (CH = 1: 4:4:4, 2: 4:2:0; 0 is luma alone), k_me_subpel<LG, true>, and k_me_costs<LG>
  kernels    odhip_me_search2 stand-alone, log_size 1 and 2, range 16, two slots, flags 0 / CHROMA / SATD / both,
             lambda 4, lambda_subpel 3.  A call with res = 3 is stage 1 (and two memsets), the same call with res = 0
             adds stage 2, so the difference is the sub-pel kernel.  Device events round `--calls` back-to-back calls,
             median of `--rounds` such windows after a warm-up window.
  pipe       the inter step of tools/time_me.py with the search on and both flags set against the same step with
             flags 0, two pipes in one process, the windows alternating.
  noflags    odhip_me_search (no flags) alone, with min and max of the windows: run once per library
             (ODHIP_LIB=another build) to compare two builds in one session on one device; not part of the default run."""
import argparse
import os
import subprocess
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tools"))
import time_me as T  # noqa: E402

OUT = os.path.join(ROOT, "profiles", "me_cost.txt")
F, W, H, CW, CH = T.F, T.W, T.H, T.CW, T.CH
NAMES = {0: "none", 1: "CHROMA", 2: "SATD", 3: "CHROMA | SATD"}


def resources(args):
    r = subprocess.run([sys.executable, os.path.join(ROOT, "tools", "time_me.py"), "--part", "resources"],
                       capture_output=True, text=True, check=True)
    # the chroma instantiations of stage 1, the flagged one of stage 2, the test surface
    plain = (", 0>", "false>")
    print("\n".join(line for line in r.stdout.splitlines() if "k_me" not in line or not any(p in line for p in plain)))


def windows(fn, calls, rounds):
    import torch

    def window():
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        for _ in range(calls):
            rc = fn()
            assert rc == 0, rc
        b.record()
        b.synchronize()
        return a.elapsed_time(b)/calls
    window()
    return [window() for _ in range(rounds)]


def kernels(args):
    import ctypes
    import torch
    import daala_amd as D
    D.init(0)
    luma, chroma, rl, rc = T.content()
    d_src, d_csrc = torch.from_numpy(luma).cuda(), torch.from_numpy(chroma).cuda()
    d_refs = [torch.from_numpy(x).cuda() for x in rl]
    d_crefs = [torch.from_numpy(x).cuda() for x in rc]
    grid = torch.empty((F, CH // 8 + 1, CW // 8 + 1, D.MV_POINT.itemsize), dtype=torch.uint8, device="cuda")
    L = D.lib()
    stream = ctypes.c_void_p(torch.cuda.current_stream().cuda_stream)
    print("odhip_me_search2, F = %d pictures of %d x %d 4:2:0 (coded %d x %d), range 16, two slots, lambda 4, "
          "lambda_subpel 3; ms per call, median of %d windows of %d calls:" % (F, W, H, CW, CH, args.rounds, args.calls))
    print("  log_size flags          | stage 1 (res 3) | stage 2 (res 0 - res 3)")
    for lg in (1, 2):
        for flags in (0, 1, 2, 3):
            ms = []
            for res in (3, 0):
                job = D.api._me_job2(d_src, d_refs, W, H, lg, 16, res, 4, 3, flags, d_csrc, d_crefs, 1)
                job.luma.grid = grid.data_ptr()
                ms.append(float(np.median(windows(lambda: L.odhip_me_search2(ctypes.byref(job), stream), args.calls,
                                                  args.rounds))))
            print("  %8d %-14s | %12.3f ms | %12.3f ms" % (lg, NAMES[flags], ms[0], ms[1] - ms[0]), flush=True)


def noflags(args):
    import ctypes
    import torch
    import daala_amd as D
    D.init(0)
    luma, _, rl, _ = T.content()
    d_src = torch.from_numpy(luma).cuda()
    d_refs = [torch.from_numpy(x).cuda() for x in rl]
    grid = torch.empty((F, CH // 8 + 1, CW // 8 + 1, D.MV_POINT.itemsize), dtype=torch.uint8, device="cuda")
    L = D.lib()
    stream = ctypes.c_void_p(torch.cuda.current_stream().cuda_stream)
    print("odhip_me_search of %s, range 16, two slots, lambda 4; ms per call over %d windows of %d calls:"
          % (os.environ.get("ODHIP_LIB") or "this tree", args.rounds, args.calls))
    for lg in (1, 2):
        for res in (3, 0):
            job = D.api._me_job(d_src, d_refs, W, H, lg, 16, res, 4)
            job.grid = grid.data_ptr()
            v = windows(lambda: L.odhip_me_search(ctypes.byref(job), stream), args.calls, args.rounds)
            print("  log_size %d res %d: median %.3f ms (min %.3f, max %.3f)"
                  % (lg, res, float(np.median(v)), min(v), max(v)), flush=True)


def pipe(args):
    import daala_amd as D
    D.init(0)
    luma, chroma, rl, rc = T.content()
    qt = D.QuantTables.load()
    pipes = {}
    for name, flags in (("flags 0", 0), ("CHROMA | SATD", 3)):
        p = D.Pipe(qt, F, W, H, chroma_cfl=True, price=True, inter=True)
        p.set_pictures(luma, chroma)
        p.set_reference_frames(rl, rc)
        p.set_motion_search2(1, 16, 0, 4, 3, flags)
        pipes[name] = p

    def window(p, n):
        t0 = time.perf_counter()
        for _ in range(n):
            p.step()
        p.flush()
        p.sync()
        return (time.perf_counter() - t0)*1e3/n

    for p in pipes.values():
        window(p, 3)
    ms = {k: [] for k in pipes}
    for _ in range(args.rounds):
        for k, p in pipes.items():
            ms[k].append(window(p, args.steps))
    print("Inter step, F = %d 1080p 4:2:0, priced on the device, two slots, the search on (log_size 1, range 16, res 0, "
          "lambda 4, lambda_subpel 3); wall clock per step, median of %d windows of %d steps, the pipes alternating "
          "in one process:" % (F, args.rounds, args.steps))
    for k, v in ms.items():
        print("  %-16s %.3f ms/step (min %.3f, max %.3f)" % (k, float(np.median(v)), min(v), max(v)), flush=True)
    for p in pipes.values():
        p.destroy()


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--part", choices=["resources", "kernels", "pipe", "noflags"])
    ap.add_argument("--calls", type=int, default=5)
    ap.add_argument("--steps", type=int, default=20)
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--limit", type=int, default=280, help="seconds per part")
    ap.add_argument("--out", default=OUT)
    args = ap.parse_args()
    if args.part:
        return {"resources": resources, "kernels": kernels, "pipe": pipe, "noflags": noflags}[args.part](args)
    text = []
    for part in ("resources", "kernels", "pipe"):
        r = subprocess.run(["timeout", "-k", "10", str(args.limit), sys.executable, os.path.abspath(__file__), "--part",
                            part, "--calls", str(args.calls), "--steps", str(args.steps), "--rounds", str(args.rounds)],
                           capture_output=True, text=True)
        sys.stdout.write(r.stdout)
        if r.returncode:
            sys.stderr.write(r.stderr[-2000:])
            raise SystemExit("part %s failed with status %d: stopping" % (part, r.returncode))
        text.append(r.stdout)
    with open(args.out, "w") as f:
        f.write("Motion search with chroma in the cost and SATD - tools/time_me_cost.py on one MI355X.\n\n"
                + "\n".join(text))


if __name__ == "__main__":
    main()
