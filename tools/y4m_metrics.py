#!/usr/bin/env python3
"""PSNR and PSNR-HVS-M of two 8-bit 4:2:0 / 4:4:4 YUV4MPEG2 clips on the GPU.

    python tools/y4m_metrics.py A.y4m B.y4m [--psnr-only | --psnrhvs-only]

Reads both clips with the library's Y4M reader (odhip_y4m_open2), measures every frame's three plane pairs with
odhip_metrics_planes and prints the per-frame and `Total:` lines of the reference's dump_psnr, then those of
dump_psnrhvs, in their formats.  PSNR lines equal the tool's; PSNR-HVS-M sums the tool's exact per-window terms in
double instead of its running float, so its last digits may differ.
"""
import argparse
import math
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def _db(score, weight):
    return 10 * (-1 * math.log10(weight * score))


def psnr_lines(frames, depth=8):
    """dump_psnr's lines (dump_psnr.c:230-256) from [(plane sse[3], plane pixels[3])] per frame."""
    m2 = ((1 << depth) - 1) ** 2
    out = []
    g, gn = [0, 0, 0], [0, 0, 0]
    for f, (se, npx) in enumerate(frames):
        pl = [10 * (math.log10(m2) + math.log10(npx[i]) - math.log10(se[i])) for i in range(3)]
        tot = 10 * (math.log10(m2) + math.log10(sum(npx)) - math.log10(sum(se)))
        out.append("%08i: %-7G  (Y': %-7G  Cb: %-7G  Cr: %-7G)" % (f, tot, pl[0], pl[1], pl[2]))
        g = [g[i] + se[i] for i in range(3)]
        gn = [gn[i] + npx[i] for i in range(3)]
    pl = [10 * (math.log10(m2) + math.log10(gn[i]) - math.log10(g[i])) for i in range(3)]
    tot = 10 * (math.log10(m2) + math.log10(sum(gn)) - math.log10(sum(g)))
    out.append("Total: %-7G  (Y': %-7G  Cb: %-7G  Cr: %-7G)" % (tot, pl[0], pl[1], pl[2]))
    return out


def psnrhvs_lines(frames, c444):
    """dump_psnrhvs's lines (dump_psnrhvs.c:268, 312-327) from the plane scores [(y, cb, cr)] per frame."""
    cw = 1.0 if c444 else 0.25
    out = []
    g = [0.0, 0.0, 0.0]
    for f, s in enumerate(frames):
        out.append("%08i: %-8G  (Y': %-8G  Cb: %-8G  Cr: %-8G)" % (
            f, _db(s[0] + cw * (s[1] + s[2]), 1 + 2 * cw), _db(s[0], 1), _db(s[1], 1), _db(s[2], 1)))
        g = [g[i] + s[i] for i in range(3)]
    n = len(frames)
    out.append("Total: %-8G  (Y': %-8G  Cb: %-8G  Cr: %-8G)" % (
        _db(g[0] + cw * (g[1] + g[2]), (1 + 2 * cw) * 1. / n), _db(g[0], 1. / n), _db(g[1], 1. / n),
        _db(g[2], 1. / n)))
    return out


def measure(path_a, path_b, sse=True, psnrhvs=True):
    """[(pl_sse[3], pl_npix[3], pl_hvs_score[3])] per frame, and whether the clips are 4:4:4."""
    import numpy as np
    import torch
    import daala_amd as D
    D.init(0)
    a, b = D.Y4M(path_a), D.Y4M(path_b)
    try:
        if (a.w, a.h_px, a.chroma_dec) != (b.w, b.h_px, b.chroma_dec):
            raise SystemExit("the clips differ in size or chroma format")
        frames = []
        while True:
            fa, fb = a.read(), b.read()
            if fa is None or fb is None:
                break
            vals = []
            for pli in range(3):
                s = torch.from_numpy(fa[pli][None]).cuda()
                r = torch.from_numpy(fb[pli][None]).cuda()
                vals.append(D.metrics_planes(s, r, depth=8, csf=pli, sse=sse, psnrhvs=psnrhvs))
            frames.append(([int(v[0][0]) for v in vals], [int(v[2][0]) for v in vals],
                           [float(np.float64(v[1][0]) / (64.0 * v[3][0]) / (255.0 * 255.0)) for v in vals]))
        return frames, a.chroma_dec == 0
    finally:
        a.close()
        b.close()


def main():
    ap = argparse.ArgumentParser(description=__doc__.splitlines()[0])
    ap.add_argument("a")
    ap.add_argument("b")
    ap.add_argument("--psnr-only", action="store_true")
    ap.add_argument("--psnrhvs-only", action="store_true")
    args = ap.parse_args()
    frames, c444 = measure(args.a, args.b, sse=not args.psnrhvs_only, psnrhvs=not args.psnr_only)
    if not frames:
        raise SystemExit("no frames")
    if not args.psnrhvs_only:
        print("\n".join(psnr_lines([(f[0], f[1]) for f in frames], 8)))
    if not args.psnr_only:
        print("\n".join(psnrhvs_lines([f[2] for f in frames], c444)))


if __name__ == "__main__":
    main()
