#!/usr/bin/env python3
"""What the Haar-wavelet / lossless path costs: F = 16 pictures of 1080p 4:2:0.  Writes profiles/haar.txt.

    python tools/time_haar.py                  # resources, then the kernels: one child process per part
    python tools/time_haar.py --part resources # the compiler's figures only (needs hipcc and no GPU)

  resources  the compiler's figures of every kernel of haar_kernels.hip (tools/kres.py)
  kernels    odhip_haar_encode_planes with a reconstruction, keyframe and inter, lossless and quant = 16, the luma set
             (16 planes of 1920 x 1088) and the chroma set (32 planes of 960 x 544), `--calls` calls each after a
             warm-up call, in a child under `rocprofv3 --kernel-trace`: per kernel the median duration of its
             dispatches, and the algorithmic bytes (8-bit samples: forward 1 in + 4 + 4 out, inverse 4 in + 1 out, one
             more read each when inter) over it, beside odhip_copy_ceiling of as many bytes - the keyframe's or the
             inter job's, each measured - in the same process.  k_haar_dc against the encode (k_haar_forward +
             k_haar_dc) of its set."""
import argparse
import csv
import glob
import json
import os
import re
import subprocess
import sys
import tempfile

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
OUT = os.path.join(ROOT, "profiles", "haar.txt")
F, W, H, CW, CH = 16, 1920, 1080, 1920, 1088
CONFIGS = [("keyframe lossless", False, 0), ("keyframe quant 16", False, 16), ("inter lossless", True, 0),
           ("inter quant 16", True, 16)]
SETS = [("luma", 0), ("chroma", 1)]


def resources(args):
    os.makedirs("/tmp/kres", exist_ok=True)         # where tools/kres.py puts its object file
    r = subprocess.run([sys.executable, os.path.join(ROOT, "tools", "kres.py"), "haar_kernels.hip"], capture_output=True,
                       text=True, check=True)
    print("Compiler resources (gfx950; tools/kres.py haar_kernels.hip):")
    print(r.stdout)


def content():
    """(luma [F][CH][CW], chroma [2F][CH/2][CW/2]) uint8: the benchmark's natural content, edge-padded to the coded
    size; Cb planes first, then Cr."""
    import bench
    frames = [bench.CONTENT["natural"](i, 1) for i in range(F)]
    luma = np.stack([f[0][:H, :W] for f in frames])
    chroma = np.concatenate([np.stack([f[p][:H // 2, :W // 2] for f in frames]) for p in (1, 2)])
    luma = np.pad(luma, ((0, 0), (0, CH - H), (0, CW - W)), mode="edge")
    chroma = np.pad(chroma, ((0, 0), (0, (CH - H) // 2), (0, (CW - W) // 2)), mode="edge")
    return np.ascontiguousarray(luma), np.ascontiguousarray(chroma)


def run(args):
    """The traced child: the calls in a fixed order, then the plan of that order and the copy ceilings as one JSON line."""
    import torch
    import daala_amd as D
    D.init(0)
    planes = [torch.from_numpy(x).cuda() for x in content()]
    preds = [torch.roll(x, shifts=(1, -2), dims=(1, 2)).contiguous() for x in planes]
    plan = []
    for label, inter, quant in CONFIGS:
        for (sname, dec), px, pred in zip(SETS, planes, preds):
            nplanes = px.shape[0]
            dcq = 1 if quant == 0 else (21, 27)
            for _ in range(args.calls + 1):
                D.haar_encode(px, pred if inter else None, dec=dec, pic_w=W >> dec, pic_h=H >> dec, depth=8, quant=quant,
                              dc_quant=dcq, plane_split=nplanes // (1 + dec))
            torch.cuda.synchronize()
            plan.append({"config": label, "set": sname, "inter": inter, "samples": px.numel(),
                         "kernels": ["k_haar_forward", "k_haar_inverse"] if inter
                         else ["k_haar_forward", "k_haar_dc", "k_haar_inverse"]})
    ceil = {}
    for (sname, _), px in zip(SETS, planes):
        for what, per_sample in (("forward", 9), ("inverse", 5)):
            for inter in (0, 1):                                   # one more byte read per sample when inter
                nbytes = (px.numel() * (per_sample + inter) // 2) & ~15      # the copy reads and writes each byte once
                ceil["%s %s %d" % (sname, what, inter)] = D.copy_ceiling(nbytes, n=10)
    print("PLAN " + json.dumps({"plan": plan, "ceiling": ceil, "calls": args.calls}), flush=True)


def short(name):
    name = name.replace("(anonymous namespace)::", "")
    return re.sub(r"\(.*$", "", re.sub(r"^void ", "", name))


def kernels(args):
    with tempfile.TemporaryDirectory() as tmp:
        r = subprocess.run(["rocprofv3", "--kernel-trace", "--output-format", "csv", "-d", tmp, "-o", "t", "--",
                            sys.executable, os.path.abspath(__file__), "--part", "run", "--calls", str(args.calls)],
                           capture_output=True, text=True)
        if r.returncode:
            sys.stderr.write(r.stderr[-2000:])
            raise SystemExit("the traced run failed with status %d" % r.returncode)
        info = json.loads([ln for ln in r.stdout.splitlines() if ln.startswith("PLAN ")][-1][5:])
        files = glob.glob(os.path.join(tmp, "**", "*kernel_trace.csv"), recursive=True)
        assert len(files) == 1, files
        with open(files[0]) as f:
            rows = [(int(x["Start_Timestamp"]), short(x["Kernel_Name"]), int(x["End_Timestamp"]) - int(x["Start_Timestamp"]))
                    for x in csv.DictReader(f)]
    rows = sorted(x for x in rows if x[1].startswith("k_haar"))
    calls = info["calls"]
    assert len(rows) == sum(len(p["kernels"]) for p in info["plan"]) * (calls + 1), len(rows)
    print("odhip_haar_encode_planes with a reconstruction, F = %d pictures of %d x %d 4:2:0 (coded %d x %d), 8-bit; "
          "median kernel duration of %d calls (rocprofv3 --kernel-trace), algorithmic bytes over it, and "
          "odhip_copy_ceiling of as many bytes in the same process:" % (F, W, H, CW, CH, calls))
    print("  %-18s %-6s %-24s %9s %9s %9s %7s" % ("config", "set", "kernel", "us", "GB/s", "ceiling", "share"))
    at = 0
    for p in info["plan"]:
        per = len(p["kernels"])
        block = rows[at + per:at + per*(calls + 1)]            # the first call warms up
        at += per*(calls + 1)
        med = {}
        for i, want in enumerate(p["kernels"]):
            got = block[i::per]
            assert all(g[1].startswith(want) for g in got), (want, got[0][1])
            med[want] = (float(np.median([g[2] for g in got]))/1e3, got[0][1])
        for want in p["kernels"]:
            us, name = med[want]
            if want == "k_haar_dc":
                print("  %-18s %-6s %-24s %9.1f %9s %9s %6.1f%% of k_haar_forward + k_haar_dc"
                      % (p["config"], p["set"], name, us, "-", "-", 100*us/(us + med["k_haar_forward"][0])))
                continue
            what = "forward" if want == "k_haar_forward" else "inverse"
            nbytes = p["samples"]*((9 if what == "forward" else 5) + (1 if p["inter"] else 0))
            gbs = nbytes/(us*1e-6)/1e9
            ceil = info["ceiling"]["%s %s %d" % (p["set"], what, int(p["inter"]))]
            print("  %-18s %-6s %-24s %9.1f %9.0f %9.0f %6.1f%%" % (p["config"], p["set"], name, us, gbs, ceil, 100*gbs/ceil))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--part", choices=["resources", "kernels", "run"])
    ap.add_argument("--calls", type=int, default=10)
    ap.add_argument("--limit", type=int, default=280, help="seconds per part")
    ap.add_argument("--out", default=OUT)
    args = ap.parse_args()
    if args.part:
        return {"resources": resources, "kernels": kernels, "run": run}[args.part](args)
    text = []
    for part in ("resources", "kernels"):
        r = subprocess.run(["timeout", "-k", "10", str(args.limit), sys.executable, os.path.abspath(__file__), "--part",
                            part, "--calls", str(args.calls)], capture_output=True, text=True)
        sys.stdout.write(r.stdout)
        if r.returncode:
            sys.stderr.write(r.stderr[-2000:])
            raise SystemExit("part %s failed with status %d: stopping" % (part, r.returncode))
        text.append(r.stdout)
    with open(args.out, "w") as f:
        f.write("Lossless and Haar-wavelet frames - tools/time_haar.py on one MI355X.\n\n" + "\n".join(text))


if __name__ == "__main__":
    main()
