#!/usr/bin/env python3
"""tests/golden/partition.npz: what the REAL reference decoder reconstructs from, and what it reconstructs,
at its frame-level post-filter - per plane of a few tiny clips the dequantised coefficient plane, the
compact block-size map, the picture size, xdec, whether the frame is a keyframe, and the decoder's own
pixels after od_apply_postfilter_frame_sbs.  Pins tests/_partition_ref.py's inverse() (and through it
odhip_inverse_partition, tests/test_gpu_partition.py) on boxes without the reference.

    python tools/make_golden_partition.py REFERENCE_TREE

Dev-container only, CPU only: needs oracle/_ref/libdaalaref.so (make -C oracle) and the reference's public
headers; compiles tools/partition_recorder.c into a temporary directory.  Nothing is saved unless inverse()
reproduces every recorded plane exactly and the set has the coverage the tests rely on."""
import ctypes
import os
import subprocess
import sys
import tempfile

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tests"))
from _libs import GOLDEN, P  # noqa: E402
import _partition_ref as R  # noqa: E402

# (picture w, h, frames, quality, keyframe interval, content seed)
CLIPS = [(128, 64, 1, 30, 1, 5),        # a multiple of 64: the picture gate sits exactly on node borders
         (120, 72, 2, 45, 4, 6),        # cropped both ways inside a 128x128 frame; frame 1 is an inter frame
         (72, 56, 2, 12, 4, 7)]         # fine quantiser: small blocks; pic_w - 8 == frame_w/2: chroma nodes straddle it
MAX_BYTES = 512 * 1024


def clip_frames(w, h, nframes, seed):
    """Flat, smooth, and noisy regions side by side, with detail at several scales, drifting by two pixels a
    frame: the encoder then picks every block size from 64x64 down to 4x4."""
    rng = np.random.RandomState(seed)
    W, H = w + 2 * nframes, h
    yy, xx = np.mgrid[0:H, 0:W]
    base = np.full((H, W), 96.0)
    right = xx >= W * 0.55
    base += right * (40 * np.sin(xx / 3.1) * np.sin(yy / 2.3) + rng.randint(-45, 46, size=(H, W)))
    band = (yy >= H * 0.5) & ~right
    base += band * ((xx * 0.9 + yy * 0.4) % 64 - 32) * 0.8
    base[(yy // 16 + xx // 16) % 5 == 0] += 25
    luma = np.clip(base, 0, 255)
    out = []
    for f in range(nframes):
        y = luma[:, 2 * f:2 * f + w]
        cw, ch = (w + 1) // 2, (h + 1) // 2
        yp = np.pad(y, ((0, h & 1), (0, w & 1)), mode="edge")
        sub = yp.reshape(ch, 2, cw, 2).mean(axis=(1, 3))
        cb = np.clip(128 + (sub - 96) * 0.5 + rng.randint(-3, 4, size=sub.shape), 0, 255)
        cr = np.clip(128 - (sub - 96) * 0.4 + rng.randint(-3, 4, size=sub.shape), 0, 255)
        out.append(np.concatenate([p.astype(np.uint8).ravel() for p in (y, cb, cr)]))
    return np.concatenate(out)


def build_recorder(ref_tree, outdir):
    refdir = os.path.join(ROOT, "oracle", "_ref")
    so = os.path.join(outdir, "libpartrec.so")
    subprocess.run(["gcc", "-O2", "-fPIC", "-shared", "-std=gnu99", "-Wall", "-I" + os.path.join(ref_tree, "include"),
                    "-o", so, os.path.join(ROOT, "tools", "partition_recorder.c"), "-L" + refdir, "-ldaalaref",
                    "-Wl,-rpath," + refdir, "-ldl"], check=True)
    return so


RECORD_FN = ctypes.CFUNCTYPE(None, ctypes.c_int, ctypes.c_int, ctypes.c_int, ctypes.c_int, ctypes.c_int, ctypes.c_int,
                             ctypes.c_int, ctypes.c_void_p, ctypes.c_void_p, ctypes.c_void_p, ctypes.c_int)


def record(lib):
    """Every plane of every decoded frame of CLIPS, in decoding order."""
    records = []
    state = {"clip": 0, "planes": 0}

    def on_plane(pli, xdec, keyframe, w, h, pic_w, pic_h, d, c, bsize, bstride):
        coef = np.ctypeslib.as_array(ctypes.cast(d, ctypes.POINTER(ctypes.c_int32)), (h, w)).copy()
        rec = np.ctypeslib.as_array(ctypes.cast(c, ctypes.POINTER(ctypes.c_int32)), (h, w))
        rows, cols = (h << xdec) // 8, (w << xdec) // 8
        full = np.ctypeslib.as_array(ctypes.cast(bsize, ctypes.POINTER(ctypes.c_uint8)), (rows, bstride))
        # the pixel conversion of od_coeff_to_ref_buf for 8-bit buffers, as tests/interpose/interpose.c applies it
        px = np.clip(((rec + 8) >> 4) + 128, 0, 255).astype(np.uint8)
        records.append(dict(clip=state["clip"], frame=state["planes"] // 3, pli=pli, dec=xdec, keyframe=keyframe,
                            pic_w=pic_w, pic_h=pic_h, coef=coef, bmap=full[:, :cols].copy(), recon=px))
        state["planes"] += 1

    cb = RECORD_FN(on_plane)
    lib.partrec_set_callback(cb)
    for i, (w, h, nframes, quality, kf_rate, seed) in enumerate(CLIPS):
        state["clip"], state["planes"] = i, 0
        frames = clip_frames(w, h, nframes, seed)
        n = lib.partrec_roundtrip(P(frames), w, h, nframes, quality, 7, kf_rate)
        assert n == nframes and state["planes"] == 3 * nframes, (n, state)
    lib.partrec_set_callback(RECORD_FN())
    return records


def main():
    if len(sys.argv) != 2 or not os.path.isdir(os.path.join(sys.argv[1], "include", "daala")):
        sys.exit(__doc__)
    with tempfile.TemporaryDirectory() as tmp:
        lib = ctypes.CDLL(build_recorder(sys.argv[1], tmp), mode=ctypes.RTLD_GLOBAL)
        records = record(lib)
    for r in records:
        assert R.is_quadtree(r["bmap"]), (r["clip"], r["frame"])
        got = R.inverse(r["coef"], r["bmap"], r["dec"], r["pic_w"], r["pic_h"], False)
        bad = int((got != r["recon"]).sum())
        assert bad == 0, "inverse() differs from the decoder: clip %d frame %d plane %d, %d samples" % (
            r["clip"], r["frame"], r["pli"], bad)
    R.check_golden_coverage(records)
    path = os.path.join(GOLDEN, "partition.npz")
    R.save_cases(path, records)
    size = os.path.getsize(path)
    assert size <= MAX_BYTES, size
    luma = [r for r in records if r["pli"] == 0]
    print("ok: %d planes, %d bytes; luma leaf sizes per frame %s; keyframes %s" % (
        len(records), size, [R.leaf_sizes(r["bmap"]) for r in luma], [r["keyframe"] for r in luma]))


if __name__ == "__main__":
    main()
