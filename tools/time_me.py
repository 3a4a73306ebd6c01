#!/usr/bin/env python3
"""What the block-matching motion search costs: F = 16 pictures of 1080p, 8-bit luma.  Writes profiles/me.txt.

    python tools/time_me.py                  # resources, the kernels, the pipe: one child process per part
    python tools/time_me.py --part kernels   # one of them (resources needs hipcc and no GPU)

  resources  the compiler's figures of every kernel of me_kernels.hip (-Rpass-analysis=kernel-resource-usage)
  kernels    odhip_me_search stand-alone, log_size 1 and 2, range 8 / 16 / 32, one and two slots, res 3 and 0.
             A call with res = 3 is k_me_fullpel<LG, kNoChroma> (and two memsets); the same call with res = 0 adds
             k_me_subpel<LG, false>, so the difference of the two is that kernel.  Device events round `--calls` back-to-back calls, median of
             `--rounds` such windows after a warm-up window.  For k_me_fullpel the byte differences the search
             needs, (2 range + 1)^2 x slots x B^2 per point, over its time, against the VALU issue peak of DESIGN.md
             section 4 (614 G wave-instructions/s) at four bytes per lane-instruction.
  pipe       the inter step of tools/time_pipe_mc.py, case (b) (reference frames and grids resident), against the
             same step with the search on (log_size 1, range 16, res 0, two slots), two pipes in one process, the
             windows alternating: wall clock over `--steps` back-to-back steps ending in flush + sync."""
import argparse
import os
import re
import subprocess
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
OUT = os.path.join(ROOT, "profiles", "me.txt")
ISSUE_PEAK = 614e9          # wave-instructions/s, DESIGN.md section 4
F, W, H, CW, CH = 16, 1920, 1080, 1920, 1088


def resources(args):
    from daala_amd import build as b
    src = os.path.join(b.CSRC, "me_kernels.hip")
    r = subprocess.run([b.HIPCC] + b.FLAGS + ["-Rpass-analysis=kernel-resource-usage", "-c", src, "-o", os.devnull],
                       capture_output=True, text=True, check=True)
    rows = {}
    name = None
    for line in r.stderr.splitlines():
        m = re.search(r"Function Name: (\S+)", line)
        if m:
            name = subprocess.run(["c++filt", m.group(1)], capture_output=True, text=True).stdout.strip()
            name = re.sub(r"\(anonymous namespace\)::|void |\(.*", "", name)
            rows[name] = {}
        for key in ("VGPRs", "AGPRs", "ScratchSize [bytes/lane]", "Occupancy [waves/SIMD]", "LDS Size [bytes/block]"):
            m = re.search(re.escape(key) + r": (\d+)", line)
            if m and name:
                rows[name][key] = int(m.group(1))
    print("Compiler resources (gfx950, 256 lanes per block):")
    for name, v in rows.items():
        print("  %-21s VGPRs %3d  scratch %d  LDS %5d B/block  occupancy %d waves/SIMD"
              % (name, v["VGPRs"], v["ScratchSize [bytes/lane]"], v["LDS Size [bytes/block]"],
                 v["Occupancy [waves/SIMD]"]))


def content():
    import bench
    frames = [bench.CONTENT["natural"](i, 1) for i in range(F)]
    luma = np.ascontiguousarray(np.stack([f[0][:H, :W] for f in frames]))
    chroma = np.ascontiguousarray(np.concatenate([np.stack([f[p][:H // 2, :W // 2] for f in frames]) for p in (1, 2)]))
    rl = np.pad(luma, ((0, 0), (0, CH - H), (0, CW - W)), mode="edge")
    rc = np.pad(chroma, ((0, 0), (0, (CH - H) // 2), (0, (CW - W) // 2)), mode="edge")
    rl = [np.ascontiguousarray(np.roll(rl, -5, 2)), np.ascontiguousarray(np.roll(rl, 3, 1))]
    rc = [np.ascontiguousarray(np.roll(rc, -2, 2)), np.ascontiguousarray(np.roll(rc, 1, 1))]
    return luma, chroma, rl, rc


def kernels(args):
    import ctypes
    import torch
    import daala_amd as D
    D.init(0)
    luma, _, rl, _ = content()
    d_src = torch.from_numpy(luma).cuda()
    d_refs = [torch.from_numpy(x).cuda() for x in rl]
    shape = (F, CH // 8 + 1, CW // 8 + 1)
    grid = torch.empty(shape + (D.MV_POINT.itemsize,), dtype=torch.uint8, device="cuda")
    L = D.lib()

    def timed(job):
        def window():
            a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            a.record()
            for _ in range(args.calls):
                rc = L.odhip_me_search(ctypes.byref(job), ctypes.c_void_p(torch.cuda.current_stream().cuda_stream))
                assert rc == 0, rc
            b.record()
            b.synchronize()
            return a.elapsed_time(b)/args.calls
        window()
        return float(np.median([window() for _ in range(args.rounds)]))

    print("odhip_me_search, F = %d pictures of %d x %d (coded %d x %d), lambda 4; ms per call, median of %d windows of "
          "%d calls:" % (F, W, H, CW, CH, args.rounds, args.calls))
    print("  log_size range slots | k_me_fullpel   G byte differences/s  of issue peak | k_me_subpel (res 0)")
    for lg in (1, 2):
        for rng in (8, 16, 32):
            for slots in (1, 2):
                ms = []
                for res in (3, 0):
                    job = D.api._me_job(d_src, d_refs[:slots], W, H, lg, rng, res, 4)
                    job.grid = grid.data_ptr()
                    ms.append(timed(job))
                blk = 8 << lg
                points = F*((CW >> 3 >> lg) + 1)*((CH >> 3 >> lg) + 1)
                diffs = points*(2*rng + 1)**2*slots*blk*blk
                rate = diffs/(ms[0]*1e-3)
                print("  %8d %5d %5d | %9.3f ms %18.1f %13.1f %% | %9.3f ms"
                      % (lg, rng, slots, ms[0], rate/1e9, 100*rate/(ISSUE_PEAK*64*4), ms[1] - ms[0]), flush=True)


def pipe(args):
    import torch
    import daala_amd as D
    D.init(0)
    luma, chroma, rl, rc = content()
    rng = np.random.RandomState(2)
    nh, nv = CW // 8, CH // 8
    grid = np.zeros((F, nv + 1, nh + 1), D.MV_POINT)
    valid = (rng.rand(nv + 1, nh + 1) < 0.3).astype(np.uint8)
    valid[::8, ::8] = 1
    grid["valid"] = valid
    grid["ref"] = rng.randint(0, 2, size=grid.shape)
    grid["mvx"] = rng.randint(-16*8, 16*8 + 1, size=grid.shape)
    grid["mvy"] = rng.randint(-16*8, 16*8 + 1, size=grid.shape)
    qt = D.QuantTables.load()
    pipes = {}
    for name in ("resident grids (b)", "uniform resident grid", "search on"):
        p = D.Pipe(qt, F, W, H, chroma_cfl=True, price=True, inter=True)
        p.set_pictures(luma, chroma)
        p.set_reference_frames(rl, rc)
        pipes[name] = p
    pipes["resident grids (b)"].set_mvs(grid)
    pipes["search on"].set_motion_search(1, 16, 0, 4)
    pipes["search on"].step()
    pipes["search on"].flush()
    # the searched grid itself, resident: the same prediction work without the search
    pipes["uniform resident grid"].set_mvs(pipes["search on"].read_mvs())

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
    print("Inter step, F = %d 1080p 4:2:0, priced on the device, two slots; wall clock per step, median of %d windows "
          "of %d steps, the pipes alternating in one process:" % (F, args.rounds, args.steps))
    for k, v in ms.items():
        print("  %-24s %.3f ms/step (min %.3f, max %.3f)" % (k, float(np.median(v)), min(v), max(v)))
    p = pipes["search on"]
    p.record(True)
    window(p, args.steps)
    print("  search on, exclusive stage averages (ms per launch group; the luma pad stage holds the search and the "
          "prediction): " + ", ".join("%s %.3f" % (k, v[0]) for k, v in p.timings().items()), flush=True)
    for p in pipes.values():
        p.destroy()


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--part", choices=["resources", "kernels", "pipe"])
    ap.add_argument("--calls", type=int, default=5)
    ap.add_argument("--steps", type=int, default=20)
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--limit", type=int, default=280, help="seconds per part")
    ap.add_argument("--out", default=OUT)
    args = ap.parse_args()
    if args.part:
        return {"resources": resources, "kernels": kernels, "pipe": pipe}[args.part](args)
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
        f.write("Motion search by block matching - tools/time_me.py on one MI355X.\n\n" + "\n".join(text))


if __name__ == "__main__":
    main()
