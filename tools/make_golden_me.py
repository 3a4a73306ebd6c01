#!/usr/bin/env python3
"""Record what the reference's block-matching cost gives, for tests/golden/me.npz.

Dev-time tool, runs on the CPU: `python tools/make_golden_me.py REFERENCE_TREE` (needs oracle/_ref/libdaalaref.so,
which __graft_entry__.build() compiles from that tree).  The predictor's full-pel branch copies through the state's
function table, so the tool hands it a zeroed od_state filled in by the library's own od_state_opt_vtbl_init_c; the
size of that structure comes from a one-line probe compiled in a temporary directory against the tree's headers and
is doubled, because the library may have been configured with members the bare headers leave out.  Only the function
table is written and read; were the buffer still too small, od_state_opt_vtbl_init_c would write past it and the tool
would crash or record values that its own assertion against tests/_me_ref.py rejects - nothing is saved then.
For every case it calls, through ctypes, what
od_mv_est_bma_sad calls for the luma plane (src/mcenc.c:2224-2264): od_mc_predict1fmv8_c of the vector on the block
centred on a grid point of a reference plane with a replicated border, then - after the clipping of od_enc_sad
(src/mcenc.c:1615-1679), restated here because that function is static - od_mc_compute_sad8_c of the prediction
against the source picture.

The cases share one source picture and one bordered reference plane: all eight sub-pel phases in both
directions, blocks of 8, 16, 32 and 64, and blocks clipped at each edge and corner of the picture, one of them to
nothing.  The script asserts that tests/_me_ref.bma_sad agrees with every recorded value.  tests/golden/me.npz
keeps recorded data only: the picture, the plane, the cases (vx, vy, log_size, mvx, mvy) and the SADs."""
import ctypes
import os
import subprocess
import sys
import tempfile

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tests"))
import _me_ref as M  # noqa: E402

OUT = os.path.join(ROOT, "tests", "golden", "me.npz")
CODED_W = CODED_H = 128
PIC_W, PIC_H = 120, 104
BORDER = 72          # the reference replicates 64 samples; the filter support of the vectors below stays inside


def cases(rng):
    out = []
    # every phase pair once, spread over the block sizes, on points whose block is whole
    inner = {0: (5, 6), 1: (6, 5), 2: (6, 6), 3: (8, 8)}
    for fy in range(8):
        for fx in range(8):
            lg = (fx + 3*fy) % 4
            vx, vy = inner[lg]
            out.append((vx, vy, lg, 8*int(rng.randint(-5, 6)) + fx, 8*int(rng.randint(-5, 6)) + fy))
    # clipped blocks: every edge and corner of the picture, every size; at the right and bottom the picture
    # ends inside the block (120 x 104 in 128 x 128), at 16 / 16 nothing is left
    for lg in range(4):
        s = 1 << lg
        last_x, last_y = (PIC_W//8)//s*s, (PIC_H//8)//s*s
        for vx, vy in ((0, 0), (last_x, 0), (0, last_y), (last_x, last_y), (0, 8), (8, 0), (last_x, 8), (8, last_y),
                       (16, 16), (16, 8), (8, 16)):
            out.append((vx, vy, lg, int(rng.randint(-300, 301)), int(rng.randint(-300, 301))))
    return np.array(out, np.int32)


PROBE = r"""
#include <stdio.h>
#include "state.h"
int main(void) { printf("%lu\n", (unsigned long)sizeof(od_state)); return 0; }
"""


def state_bytes(ref_tree):
    with tempfile.TemporaryDirectory() as d:
        open(os.path.join(d, "probe.c"), "w").write(PROBE)
        exe = os.path.join(d, "probe")
        subprocess.run(["gcc", "-std=gnu99", "-w", "-I" + os.path.join(ref_tree, "include"),
                        "-I" + os.path.join(ref_tree, "src"), "-o", exe, os.path.join(d, "probe.c")], check=True)
        return int(subprocess.run([exe], check=True, capture_output=True, text=True).stdout)


def main():
    lib = ctypes.CDLL(os.path.join(ROOT, "oracle", "_ref", "libdaalaref.so"))
    # twice the probe's figure: the library may have been configured with members the bare headers leave out
    state = np.zeros(2*state_bytes(sys.argv[1]), np.uint8)
    lib.od_state_opt_vtbl_init_c(ctypes.c_void_p(state.ctypes.data))
    u8p = ctypes.POINTER(ctypes.c_uint8)
    lib.od_mc_predict1fmv8_c.argtypes = [ctypes.c_void_p, u8p, ctypes.c_void_p, ctypes.c_int, ctypes.c_int32,
                                         ctypes.c_int32, ctypes.c_int, ctypes.c_int]
    lib.od_mc_predict1fmv8_c.restype = None
    lib.od_mc_compute_sad8_c.argtypes = [ctypes.c_void_p, ctypes.c_int, ctypes.c_void_p, ctypes.c_int, ctypes.c_int,
                                         ctypes.c_int]
    lib.od_mc_compute_sad8_c.restype = ctypes.c_int32
    rng = np.random.RandomState(2264)
    src = M.smooth_noise(rng, PIC_H, PIC_W)
    plane = M.smooth_noise(rng, CODED_H, CODED_W)
    # related content, so that the SADs are not all alike
    plane[:PIC_H, :PIC_W] = np.clip(src.astype(int)//2 + plane[:PIC_H, :PIC_W].astype(int)//2 + 3, 0, 255)
    bordered = np.ascontiguousarray(np.pad(plane, BORDER, mode="edge"))
    stride = bordered.shape[1]
    todo = cases(rng)
    sads = np.zeros(len(todo), np.int32)
    for n, (vx, vy, lg, mvx, mvy) in enumerate(todo.tolist()):
        bx, by, blk = M.block_of(vx, vy, lg)
        pred = np.zeros((blk, blk), np.uint8)
        at = bordered.ctypes.data + (by + BORDER)*stride + bx + BORDER
        lib.od_mc_predict1fmv8_c(state.ctypes.data, pred.ctypes.data_as(u8p), at, stride, mvx, mvy, lg + 3, lg + 3)
        # od_enc_sad for the luma plane: clip the block to the picture, advance the prediction with it
        x, y, w, h, px, py = bx, by, blk, blk, 0, 0
        if -x > 0:
            w, px, x = w + x, -x, 0
        if -y > 0:
            h, py, y = h + y, -y, 0
        w, h = min(w, PIC_W - x), min(h, PIC_H - y)
        if w > 0 and h > 0:
            sads[n] = lib.od_mc_compute_sad8_c(src.ctypes.data + y*PIC_W + x, PIC_W,
                                               pred.ctypes.data + py*blk + px, blk, w, h)
        else:
            # nothing of the block is inside the picture: the loops of the reference's SAD run zero times (the
            # pointers are not formed here)
            sads[n] = lib.od_mc_compute_sad8_c(src.ctypes.data, PIC_W, pred.ctypes.data, blk, w, h)
        mine = M.bma_sad(src, PIC_W, PIC_H, plane, vx, vy, lg, mvx, mvy)
        assert mine == sads[n], (n, vx, vy, lg, mvx, mvy, mine, int(sads[n]))
    assert {(c[3] & 7, c[4] & 7) for c in todo.tolist()} == {(a, b) for a in range(8) for b in range(8)}
    assert (sads == 0).sum() >= 4 and (sads > 0).sum() > 80
    np.savez_compressed(OUT, src=src, bordered=bordered, border=np.int32(BORDER), pic=np.array([PIC_W, PIC_H], np.int32),
                        cases=todo, sad=sads)
    print("%s: %d cases, %d bytes" % (OUT, len(todo), os.path.getsize(OUT)))


if __name__ == "__main__":
    main()
