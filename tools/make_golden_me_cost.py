#!/usr/bin/env python3
"""Record what the reference's block-matching distortions give per plane, for tests/golden/me_cost.npz.

Dev-time tool, runs on the CPU: `python tools/make_golden_me_cost.py REFERENCE_TREE` (needs
oracle/_ref/libdaalaref.so, which __graft_entry__.build() compiles from that tree).  It follows
tools/make_golden_me.py (the zeroed od_state filled in by od_state_opt_vtbl_init_c, its size from a probe compiled
against the tree's headers).  For every case and each of the planes Y, Cb, Cr it calls, through ctypes, what
od_mv_est_bma_sad calls with OD_MC_USE_CHROMA (src/mcenc.c:2224-2264): od_mc_predict1fmv8_c of the plane's vector on
the plane's block of a reference plane with a replicated border, then - after the clipping and the size dispatch of
od_enc_sad / od_enc_satd (src/mcenc.c:1615-1748), restated here because those functions are static -
od_mc_compute_sad8_c and od_mc_compute_satd8_{4x4 .. 64x64}_c (the SAD where od_enc_satd falls back to it).

One 4:2:0 and one 4:4:4 plane set in a 128 x 128 coded frame, each costed at the picture sizes 120 x 104 and
119 x 103 (the odd size makes the 4:2:0 chroma picture size round up).  Cases: all 64 luma phase pairs, every block
size, every edge and corner of the picture.  The script asserts the classes of clipped size it must contain
(_me_cost_ref.assert_classes), that at half-pel multiples the chroma vector is od_mv_est_bma_sad's
mv*(1 << (2 - dec)) of the half-pel vector, and that tests/_me_cost_ref.plane_dist agrees with every recorded
value; it saves nothing otherwise.  tests/golden/me_cost.npz keeps recorded data only: pictures, unpadded planes
(the border is their edge replicated), picture sizes, cases (cdec, picture size index, vx, vy, log_size, mvx, mvy),
sad[n][3] and satd[n][3]."""
import ctypes
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tests"))
sys.path.insert(0, os.path.join(ROOT, "tools"))
import _mc_ref as R  # noqa: E402
import _me_cost_ref as C  # noqa: E402
import _me_ref as M  # noqa: E402
from make_golden_me import state_bytes  # noqa: E402

OUT = os.path.join(ROOT, "tests", "golden", "me_cost.npz")
CODED = 128
PICS = ((120, 104), (119, 103))
BORDER = 80          # luma samples; the filter support of the vectors below stays inside


def cases(rng):
    out = []
    inner = {0: (5, 6), 1: (6, 5), 2: (6, 6), 3: (8, 8)}
    for cdec in (1, 0):
        # every phase pair once, spread over the block sizes, on points whose block is whole
        for fy in range(8):
            for fx in range(8):
                lg = (fx + 3*fy) % 4
                vx, vy = inner[lg]
                out.append((cdec, (fx + fy) & 1, vx, vy, lg, 8*int(rng.randint(-5, 6)) + fx,
                            8*int(rng.randint(-5, 6)) + fy))
        # whole 8 x 8 blocks (4 x 4 in 4:2:0 chroma) at half-pel multiples
        for mv in ((4, -12), (-20, 8), (0, 4), (12, 12)):
            out.append((cdec, 0, 5, 6, 0, mv[0], mv[1]))
        # clipped blocks: every edge and corner of the picture, every size; the picture ends inside the block at
        # the right and at the bottom, at 16 / 16 nothing is left of the small blocks
        for pic, (pw, ph) in enumerate(PICS):
            for lg in range(4):
                s = 1 << lg
                last_x, last_y = (pw//8)//s*s, (ph//8)//s*s
                pts = [(0, 0), (last_x, 0), (0, last_y), (last_x, last_y), (0, 8), (8, 0), (last_x, 8), (8, last_y),
                       (16, 16), (16, 8), (8, 16)]
                if lg == 0:
                    pts += [(15, 3), (3, 13), (15, 13)]
                for k, (vx, vy) in enumerate(pts):
                    half = k % 3 == 0       # some at half-pel multiples
                    mv = [int(rng.randint(-75, 76))*4 if half else int(rng.randint(-300, 301)) for _ in range(2)]
                    out.append((cdec, pic, vx, vy, lg, mv[0], mv[1]))
    return np.array(out, np.int32)


def content(rng):
    src_y = M.smooth_noise(rng, PICS[0][1], PICS[0][0])
    ref_y = M.smooth_noise(rng, CODED, CODED)
    ref_y[:104, :120] = np.clip(src_y.astype(int)//2 + ref_y[:104, :120].astype(int)//2 + 3, 0, 255)
    d = dict(src_y=src_y, ref_y=ref_y)
    for tag, dec in (("444", 0), ("420", 1)):
        for name in ("cb", "cr"):
            h, w = C.plane_sz(PICS[0][1], dec), C.plane_sz(PICS[0][0], dec)
            s = M.smooth_noise(rng, h, w, gain=1.5)
            r = M.smooth_noise(rng, CODED >> dec, CODED >> dec, gain=1.5)
            r[:h, :w] = np.clip(s.astype(int)*2//3 + r[:h, :w].astype(int)//3 - 2, 0, 255)
            d["src_%s_%s" % (name, tag)], d["ref_%s_%s" % (name, tag)] = s, r
    return d


def main():
    lib = ctypes.CDLL(os.path.join(ROOT, "oracle", "_ref", "libdaalaref.so"))
    state = np.zeros(2*state_bytes(sys.argv[1]), np.uint8)
    lib.od_state_opt_vtbl_init_c(ctypes.c_void_p(state.ctypes.data))
    u8p = ctypes.POINTER(ctypes.c_uint8)
    lib.od_mc_predict1fmv8_c.argtypes = [ctypes.c_void_p, u8p, ctypes.c_void_p, ctypes.c_int, ctypes.c_int32,
                                         ctypes.c_int32, ctypes.c_int, ctypes.c_int]
    lib.od_mc_predict1fmv8_c.restype = None
    lib.od_mc_compute_sad8_c.argtypes = [ctypes.c_void_p, ctypes.c_int, ctypes.c_void_p, ctypes.c_int, ctypes.c_int,
                                         ctypes.c_int]
    lib.od_mc_compute_sad8_c.restype = ctypes.c_int32
    satd = {}
    for n in (4, 8, 16, 32, 64):
        fn = getattr(lib, "od_mc_compute_satd8_%dx%d_c" % (n, n))
        fn.argtypes = [ctypes.c_void_p, ctypes.c_int, ctypes.c_void_p, ctypes.c_int]
        fn.restype = ctypes.c_int32
        satd[n] = fn
    rng = np.random.RandomState(1681)
    data = content(rng)
    todo = cases(rng)
    sads = np.zeros((len(todo), 3), np.int32)
    satds = np.zeros((len(todo), 3), np.int32)
    halfpel = 0
    for n, (cdec, pic, vx, vy, lg, mvx, mvy) in enumerate(todo.tolist()):
        pw, ph = PICS[pic]
        srcs, refs = C.golden_planes(data, cdec)
        bx, by, _ = M.block_of(vx, vy, lg)
        for pli in range(3):
            dec = cdec if pli else 0
            pad = BORDER >> dec
            bordered = np.ascontiguousarray(np.pad(refs[pli], pad, mode="edge"))
            stride = bordered.shape[1]
            src = np.ascontiguousarray(srcs[pli])
            blk = 8 << lg >> dec
            smx, smy = R.scale_mv(mvx, dec), R.scale_mv(mvy, dec)
            if mvx % 4 == 0 and mvy % 4 == 0:
                # od_mv_est_bma_sad's own scaling of its half-pel vector
                assert (smx, smy) == ((mvx//4)*(1 << (2 - dec)), (mvy//4)*(1 << (2 - dec)))
                halfpel += 1
            pred = np.zeros((blk, blk), np.uint8)
            at = bordered.ctypes.data + ((by >> dec) + pad)*stride + (bx >> dec) + pad
            lib.od_mc_predict1fmv8_c(state.ctypes.data, pred.ctypes.data_as(u8p), at, stride, smx, smy,
                                     lg + 3 - dec, lg + 3 - dec)
            # od_enc_sad / od_enc_satd: the block in the plane, clipped to the picture, the prediction advanced
            x, y, w, h, px, py = bx >> dec, by >> dec, blk, blk, 0, 0
            if -x > 0:
                w, px, x = w + x, -x, 0
            if -y > 0:
                h, py, y = h + y, -y, 0
            w, h = min(w, C.plane_sz(pw, dec) - x), min(h, C.plane_sz(ph, dec) - y)
            sstride = src.shape[1]
            if w > 0 and h > 0:
                sp, pp = src.ctypes.data + y*sstride + x, pred.ctypes.data + py*blk + px
            else:
                # nothing inside: the loops of the reference's SAD run zero times (the pointers are not formed here)
                sp, pp = src.ctypes.data, pred.ctypes.data
            sads[n, pli] = lib.od_mc_compute_sad8_c(sp, sstride, pp, blk, w, h)
            if w == h and w in satd:
                satds[n, pli] = satd[w](sp, sstride, pp, blk)
            else:
                satds[n, pli] = sads[n, pli]
            for metric, want in ((C.SAD_METRIC, sads), (C.SATD_METRIC, satds)):
                mine = C.plane_dist(srcs[pli], pw, ph, refs[pli], vx, vy, lg, mvx, mvy, dec, metric)
                assert mine == want[n, pli], (n, pli, metric, cdec, pic, vx, vy, lg, mvx, mvy, mine, int(want[n, pli]))
    data.update(pics=np.array(PICS, np.int32), cases=todo, sad=sads, satd=satds)
    for cdec in (0, 1):
        sel = [c for c in todo.tolist() if c[0] == cdec]
        assert {(c[5] & 7, c[6] & 7) for c in sel} == {(a, b) for a in range(8) for b in range(8)}
    C.assert_classes(C.golden_classes(data))
    assert halfpel > 30 and (sads != satds).any(axis=1).sum() > 100
    np.savez_compressed(OUT, **data)
    print("%s: %d cases, %d bytes, classes %s" % (OUT, len(todo), os.path.getsize(OUT), C.golden_classes(data)))


if __name__ == "__main__":
    main()
