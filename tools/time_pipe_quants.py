"""Times a quality ladder in the frame-batch step (odhip_pipe_set_quants): ONE 1080p picture coded at 16
quantisers in one step (the picture replicated F = 16 times, picture f at quantiser f), against the same 16
codings as 16 separate F = 1 pipes (one step each, what a caller without per-picture quantisers runs), and
beside them a 16-frame step of 16 different pictures at the same mix of quantisers and bench.py's uniform
-v 20 step.  Device pricing, chroma from luma; warm-up steps, then `repeats` timed runs of `steps` steps +
flush + sync, median milliseconds per step (tests/_pipe444_check.time_steps).  Prints one JSON line.

The 16 quantisers: the six keyframe pairs of QUALITY_QUANTIZERS from -v 1 to -v 100, and two more between
each neighbouring pair, log-spaced in both quantizer and base_quantizer.

    python tools/time_pipe_quants.py [--steps 10] [--warmup 2] [--repeats 5]"""
import argparse
import json
import math
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))

import numpy as np  # noqa: E402

import bench  # noqa: E402
import daala_amd as D  # noqa: E402
from daala_amd.quant import QUALITY_QUANTIZERS  # noqa: E402
import _pipe444_check as C  # noqa: E402

PW, PH = 1920, 1080
QUALITIES = (1, 5, 10, 20, 40, 100)


def ladder():
    """16 (base_quantizer, quantizer) pairs, finest first."""
    pts = [QUALITY_QUANTIZERS[v] for v in QUALITIES]
    out = []
    for (b0, q0), (b1, q1) in zip(pts, pts[1:]):
        out.append((b0, q0))
        for t in (1 / 3, 2 / 3):
            out.append((round(b0 * math.pow(b1 / b0, t)), round(q0 * math.pow(q1 / q0, t))))
    out.append(pts[-1])
    return out


def measure(quants, luma, chroma, a):
    pipe = D.Pipe(D.QuantTables.load(), luma.shape[0], PW, PH, chroma_cfl=True, price=True)
    try:
        pipe.set_pictures(luma, chroma)
        if quants is not None:
            pipe.set_quants(quants)
        return C.time_steps(D, pipe, a.steps, a.warmup, a.repeats)
    finally:
        pipe.destroy()


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--steps", type=int, default=10)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--repeats", type=int, default=5)
    a = ap.parse_args()
    D.init(0)
    pairs = ladder()
    assert len(pairs) == 16
    quants = [D.QuantTables(b, q) for b, q in pairs]
    F = len(quants)
    l16, c16 = bench.synth_pictures(F, 4321)
    # one picture (frame 0 of the bench batch) replicated: luma [F], chroma [F Cb, F Cr]
    l1 = np.ascontiguousarray(np.repeat(l16[:1], F, axis=0))
    c1 = np.ascontiguousarray(np.concatenate([np.repeat(c16[:1], F, axis=0), np.repeat(c16[F:F + 1], F, axis=0)]))
    ladder_ms = measure(quants, l1, c1, a)
    singles = [measure([q], l16[:1], np.ascontiguousarray(c16[[0, F]]), a) for q in quants]
    mixed_ms = measure(quants, l16, c16, a)
    uniform_ms = measure(None, l16, c16, a)
    out = {"pictures": "1920x1080, bench generator frame 0 (ladder, singles) / frames 0..15 (mixed, uniform)",
           "steps": a.steps, "warmup": a.warmup, "repeats": a.repeats,
           "quantisers": [{"base_quantizer": b, "quantizer": q} for b, q in pairs],
           "ladder_one_step_ms": round(ladder_ms, 4),
           "ladder_16_single_pipes_ms": round(sum(singles), 4),
           "single_pipe_ms": [round(x, 4) for x in singles],
           "speedup_one_step_vs_16_pipes": round(sum(singles) / ladder_ms, 3),
           "mixed_16_pictures_same_quantisers_ms": round(mixed_ms, 4),
           "uniform_v20_16_pictures_ms": round(uniform_ms, 4)}
    print(json.dumps(out))


if __name__ == "__main__":
    np.seterr(all="ignore")
    main()
