"""Times the 4:4:4 frame-batch step (odhip_pipe with chroma_444 = 1) the way bench.py times the
4:2:0 one: F resident 1080p pictures, device pricing, chroma from luma; warm-up steps, then
`repeats` timed runs of `steps` steps + flush + sync, median milliseconds per step.  The 4:2:0
step of the same pictures is timed beside it, and one recorded run of each gives the per-stage
times of both chains (odhip_pipe_record / odhip_pipe_timings).  Prints one JSON line.

    python tools/time_pipe444.py [--frames 16] [--steps 10] [--warmup 2] [--repeats 5]"""
import argparse
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))

import numpy as np  # noqa: E402

import bench  # noqa: E402
import daala_amd as D  # noqa: E402
import _pipe444_check as C  # noqa: E402

PW, PH = 1920, 1080


def blocks_per_frame(dec_chroma):
    W, H = (PW + 63) & ~63, (PH + 63) & ~63
    luma = sum((W >> (2 + bs)) * (H >> (2 + bs)) for bs in range(5))
    chroma = sum((W >> (2 + bs + dec_chroma)) * (H >> (2 + bs + dec_chroma)) for bs in range(5 - dec_chroma))
    return luma + 2 * chroma


def measure(qt, luma, chroma, F, chroma_444, a):
    pipe = D.Pipe(qt, F, PW, PH, chroma_cfl=True, price=True, chroma_444=chroma_444)
    try:
        pipe.set_pictures(luma, chroma)
        ms = C.time_steps(D, pipe, a.steps, a.warmup, a.repeats)
        pipe.record(True)
        for _ in range(a.steps):
            pipe.step()
        pipe.flush()
        stages = {k: round(v[0], 4) for k, v in pipe.timings().items()}
        pipe.record(False)
    finally:
        pipe.destroy()
    blocks = blocks_per_frame(0 if chroma_444 else 1) * F
    return {"ms_per_step": round(ms, 4), "blocks_per_step": blocks, "blocks_per_s": round(blocks / ms * 1e3),
            "stage_ms": stages}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--frames", type=int, default=16)
    ap.add_argument("--steps", type=int, default=10)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--repeats", type=int, default=5)
    a = ap.parse_args()
    D.init(0)
    qt = D.QuantTables.load()
    F = a.frames
    fr444 = [C.pictures444("checker", i, 4321, PW, PH) for i in range(F)]
    l444, c444 = C.stack444(fr444)
    l420, c420 = bench.synth_pictures(F, 4321)
    r420 = measure(qt, l420, c420, F, False, a)
    r444 = measure(qt, l444, c444, F, True, a)
    out = {"frames": F, "steps": a.steps, "warmup": a.warmup, "repeats": a.repeats,
           "420": r420, "444": r444, "ratio_ms": round(r444["ms_per_step"] / r420["ms_per_step"], 3),
           "ratio_blocks": round(r444["blocks_per_step"] / r420["blocks_per_step"], 3)}
    print(json.dumps(out))


if __name__ == "__main__":
    np.seterr(all="ignore")
    main()
