"""Times the decision export as a consumer reads it: 1080p, F = 16 pictures fed from pinned host memory every step,
device pricing, chroma from luma (bench.py's configuration).  Median milliseconds per step over `repeats` runs of
`steps` steps, after `warmup` steps:

  no_export       feed, step back to back; flush + sync once at the end (bench.py's streaming_input)
  streaming_io    the same with the single export buffer set (bench.py's streaming_io: nobody can read it)
  drained         the single buffer read exactly: feed, step, flush, sync, decode - every step
  ring            a ring of 3 buffers: the main thread feeds and steps (waiting on a refused step), a consumer
                  thread takes every step as soon as it is complete, decodes it and releases it

`drained` and `ring` are also timed with the consumer only touching the totals of each step instead of decoding
it (`*_nodecode`), and the decode of one step is timed alone (daala_amd.decode_export_sections, numpy).  Prints one
JSON line.

    python tools/time_export_ring.py [--steps 10] [--warmup 2] [--repeats 3]"""
import argparse
import json
import os
import statistics
import sys
import threading
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

import numpy as np  # noqa: E402

import bench  # noqa: E402
import daala_amd as D  # noqa: E402

PW, PH, F = 1920, 1080, 16


def run_plain(pipe, pics, n):
    s0 = time.perf_counter()
    for k in range(n):
        pipe.feed(*pics[k & 1])
        pipe.step()
    pipe.flush()
    pipe.sync()
    return time.perf_counter() - s0


def run_drained(pipe, pics, n, host, decode):
    s0 = time.perf_counter()
    for k in range(n):
        pipe.feed(*pics[k & 1])
        pipe.step()
        pipe.flush()
        pipe.sync()
        h = host.numpy()
        if decode:
            pipe.decode_export(h)
        else:
            int(h[:64].view(np.uint32).sum())
    return time.perf_counter() - s0


def run_ring(pipe, pics, n, decode):
    """The consumer thread takes steps first .. first + n - 1 (numbered from set_export_ring)."""
    first = pipe._ring_steps
    done = []
    err = []

    def consumer():
        try:
            want = first
            while want < first + n:
                t = pipe.export_take(wait=True)
                if t is None:
                    time.sleep(0.0002)
                    continue
                s, buf, ovf = t
                assert s == want and ovf == 0, (s, want, ovf)
                if decode:
                    pipe.decode_export(buf)
                else:
                    int(buf[:64].view(np.uint32).sum())
                pipe.export_release(s)
                want += 1
            done.append(time.perf_counter())
        except BaseException as e:      # surfaced by the main thread
            err.append(e)

    th = threading.Thread(target=consumer)
    s0 = time.perf_counter()
    th.start()
    k = 0
    while k < n and not err:
        pipe.feed(*pics[k & 1])
        while True:
            try:
                pipe.step()
                break
            except D.ExportRingBusyError:
                time.sleep(0.0002)       # the consumer holds every slot
        k += 1
    pipe.flush()
    th.join()
    if err:
        raise err[0]
    pipe._ring_steps += n
    return done[0] - s0


def median_ms(fn, a):
    fn(a.warmup)
    return statistics.median(fn(a.steps) / a.steps * 1e3 for _ in range(a.repeats))


def main():
    import torch
    ap = argparse.ArgumentParser()
    ap.add_argument("--steps", type=int, default=10)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--repeats", type=int, default=3)
    ap.add_argument("--slots", type=int, default=3)
    a = ap.parse_args()
    D.init(0)
    l16, c16 = bench.synth_pictures(F, 4321)
    l2, c2 = bench.synth_pictures(F, 99)
    pics = [(torch.from_numpy(np.ascontiguousarray(l)).pin_memory(), torch.from_numpy(np.ascontiguousarray(c)).pin_memory())
            for l, c in ((l16, c16), (l2, c2))]
    pipe = D.Pipe(D.QuantTables.load(), F, PW, PH, chroma_cfl=True, price=True)
    out = {"pictures": "1920x1080 x %d, bench.synth_pictures, two sets alternating, fed every step" % F,
           "steps": a.steps, "warmup": a.warmup, "repeats": a.repeats, "ring_slots": a.slots}
    try:
        pipe.set_pictures(l16, c16)
        out["no_export_ms"] = median_ms(lambda n: run_plain(pipe, pics, n), a)
        host = torch.zeros(pipe.export_bytes(), dtype=torch.uint8).pin_memory()
        pipe.set_export(host)
        out["streaming_io_ms"] = median_ms(lambda n: run_plain(pipe, pics, n), a)
        out["drained_ms"] = median_ms(lambda n: run_drained(pipe, pics, n, host, True), a)
        out["drained_nodecode_ms"] = median_ms(lambda n: run_drained(pipe, pics, n, host, False), a)
        h = host.numpy()
        t0 = time.perf_counter()
        for _ in range(3):
            pipe.decode_export(h)
        out["decode_one_step_ms"] = (time.perf_counter() - t0) / 3 * 1e3
        out["export_shipped_bytes_per_step"] = int(pipe.export_shipped_bytes(h))
        pipe.set_export(None)
        slots = [torch.zeros(pipe.export_bytes(), dtype=torch.uint8).pin_memory() for _ in range(a.slots)]
        pipe.set_export_ring(slots)
        pipe._ring_steps = 0
        out["ring_ms"] = median_ms(lambda n: run_ring(pipe, pics, n, True), a)
        out["ring_nodecode_ms"] = median_ms(lambda n: run_ring(pipe, pics, n, False), a)
        out["ring_stale"] = pipe.export_stale()
        pipe.set_export_ring(None)
    finally:
        pipe.destroy()
    for k in list(out):
        if k.endswith("_ms"):
            out[k] = round(out[k], 3)
    print(json.dumps(out))


if __name__ == "__main__":
    np.seterr(all="ignore")
    main()
