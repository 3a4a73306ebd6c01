#!/usr/bin/env python3
"""Record what the reference's od_state_mc_predict builds, for tests/golden/mc.npz.

Dev-time tool: `python tools/make_golden_mc.py REFERENCE_TREE` (needs oracle/_ref/libdaalaref.so, which
__graft_entry__.build() compiles from that tree).  A small driver of our own (DRIVER below) is compiled in a
temporary directory against the reference's headers and linked with that library.  For every case it encodes a
short synthetic moving clip with the real encoder and, after every inter frame, writes out the state's reference
planes (coded size, without their border), the motion-vector grid the encoder chose (valid flag, reference slot,
vector) and what od_state_mc_predict makes of them.  A second run of the same (deterministic) encode takes
replacement grids drawn here - the encoder's own `valid` patterns with random slots and random vectors over the
legal range: all 64 fractional phases, reads that reach into the replicated border on all four sides, corners
of one leaf pointing into different slots - and records od_state_mc_predict on those as well.

The cases cover 4:2:0 and 4:4:4, 8-bit and full-precision references and a picture size that is not a multiple
of 64; the script asserts that every leaf size and every (outside corner, split flags) pair occurs, and that its
numpy restatement (tests/_mc_ref.py) agrees with every recorded prediction.  tests/golden/mc.npz keeps recorded
data only: neither the driver's binary nor anything from the reference tree."""
import os
import struct
import subprocess
import sys
import tempfile

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tests"))
import _mc_ref as R  # noqa: E402

OUT = os.path.join(ROOT, "tests", "golden", "mc.npz")

# name, picture w, h, 4:4:4, full-precision references, clip frames, inter frames kept, random grids per frame,
# the encoder's quantiser setting and its deepest motion-vector level (OD_SET_MV_LEVEL_MAX; 6 allows 8x8 blocks)
CASES = [
    ("420_8bit_176x120", 176, 120, 0, 0, 5, (2, 4), 1, 3, 6),
    ("444_8bit_128x128", 128, 128, 1, 0, 4, (3,), 1, 10, 6),
    ("420_fpr_128x128", 128, 128, 0, 1, 4, (3,), 1, 10, 4),
    ("444_fpr_72x56", 72, 56, 1, 1, 4, (2,), 2, 10, 4),
]

DRIVER = r"""
#include <stdio.h>
#include <stdlib.h>
#include <string.h>
#include "daala/daalaenc.h"
#include "encint.h"

static void put(FILE *f, const void *p, size_t n) { if (fwrite(p, 1, n, f) != n) abort(); }
static void put_i(FILE *f, int v) { put(f, &v, 4); }

static void put_grid(FILE *f, od_state *st) {
  int vx, vy;
  for (vy = 0; vy <= st->nvmvbs; vy++) for (vx = 0; vx <= st->nhmvbs; vx++) {
    od_mv_grid_pt *g = &st->mv_grid[vy][vx];
    int next = g->ref == OD_FRAME_NEXT;
    put_i(f, g->valid); put_i(f, g->ref); put_i(f, next ? g->mv1[0] : g->mv[0]);
    put_i(f, next ? g->mv1[1] : g->mv[1]);
  }
}

static void put_plane(FILE *f, daala_image_plane *p, int w, int h) {
  int y;
  for (y = 0; y < h; y++) put(f, p->data + (size_t)y*p->ystride, (size_t)w*p->xstride);
}

int main(int argc, char **argv) {
  int w = atoi(argv[1]), h = atoi(argv[2]), c444 = atoi(argv[3]), fpr = atoi(argv[4]), nframes = atoi(argv[5]);
  FILE *clip = fopen(argv[6], "rb"), *out = fopen(argv[7], "wb"), *over = argc > 10 ? fopen(argv[10], "rb") : NULL;
  int cw = c444 ? w : (w + 1) >> 1, ch = c444 ? h : (h + 1) >> 1, quality = atoi(argv[8]) << 4, mvmax = atoi(argv[9]), f, pli;
  size_t frame_bytes = (size_t)w*h + 2*(size_t)cw*ch;
  unsigned char *buf = malloc(frame_bytes);
  daala_info di; daala_comment dc; daala_enc_ctx *enc; daala_packet dp; daala_image img, pred;
  od_state *st;
  od_mv_grid_pt *saved;
  daala_info_init(&di);
  di.pic_width = w; di.pic_height = h; di.bitdepth_mode = OD_BITDEPTH_MODE_8;
  di.timebase_numerator = 30; di.timebase_denominator = 1; di.frame_duration = 1;
  di.pixel_aspect_numerator = di.pixel_aspect_denominator = 1;
  di.full_precision_references = fpr; di.nplanes = 3;
  for (pli = 0; pli < 3; pli++) di.plane_info[pli].xdec = di.plane_info[pli].ydec = pli > 0 && !c444;
  di.keyframe_rate = 256;
  enc = daala_encode_create(&di);
  if (!enc || !clip || !out) return 2;
  st = &enc->state;
  daala_comment_init(&dc);
  daala_encode_ctl(enc, OD_SET_QUANT, &quality, sizeof(quality));
  /* the encoder stops at 16x16 blocks by default (level 4); level 6 lets it go down to 8x8 */
  if (daala_encode_ctl(enc, OD_SET_MV_LEVEL_MAX, &mvmax, sizeof(mvmax))) return 9;
  while (daala_encode_flush_header(enc, &dc, &dp) > 0);
  memset(&pred, 0, sizeof(pred));
  pred.nplanes = 3; pred.width = st->frame_width; pred.height = st->frame_height;
  for (pli = 0; pli < 3; pli++) {
    daala_image_plane *p = pred.planes + pli, *r = st->ref_imgs[0].planes + pli;
    p->xdec = r->xdec; p->ydec = r->ydec; p->xstride = r->xstride; p->bitdepth = r->bitdepth;
    p->ystride = (st->frame_width >> p->xdec)*p->xstride;
    p->data = calloc((size_t)p->ystride, st->frame_height >> p->ydec);
  }
  put_i(out, st->frame_width); put_i(out, st->frame_height);
  saved = malloc(sizeof(*saved)*(st->nhmvbs + 1)*(st->nvmvbs + 1));
  for (f = 0; f < nframes; f++) {
    int slot, nv, v;
    if (fread(buf, 1, frame_bytes, clip) != frame_bytes) return 3;
    memset(&img, 0, sizeof(img));
    img.nplanes = 3; img.width = w; img.height = h;
    for (pli = 0; pli < 3; pli++) {
      daala_image_plane *p = img.planes + pli;
      p->xdec = p->ydec = pli > 0 && !c444; p->xstride = 1; p->bitdepth = 8;
      p->ystride = pli ? cw : w;
      p->data = buf + (pli ? (size_t)w*h + (pli - 1)*(size_t)cw*ch : 0);
    }
    if (daala_encode_img_in(enc, &img, 0) < 0) return 4;
    while (daala_encode_packet_out(enc, 0, &dp) > 0);
    if (f == 0) continue;
    if (st->frame_type != OD_P_FRAME) return 5;
    put_i(out, f);
    for (slot = 0; slot < 2; slot++) {
      if (st->ref_imgi[slot] < 0) return 6;
      for (pli = 0; pli < 3; pli++) {
        daala_image_plane *p = st->ref_imgs[st->ref_imgi[slot]].planes + pli;
        put_plane(out, p, st->frame_width >> p->xdec, st->frame_height >> p->ydec);
      }
    }
    nv = 0;
    if (over && fread(&nv, 4, 1, over) != 1) return 7;
    put_i(out, nv + 1);
    for (v = 0; v <= st->nvmvbs; v++) {
      memcpy(saved + (size_t)v*(st->nhmvbs + 1), st->mv_grid[v], sizeof(*saved)*(st->nhmvbs + 1));
    }
    for (v = 0; v <= nv; v++) {
      if (v > 0) {
        int vx, vy, rec[3];
        for (vy = 0; vy <= st->nvmvbs; vy++) for (vx = 0; vx <= st->nhmvbs; vx++) {
          od_mv_grid_pt *g = &st->mv_grid[vy][vx];
          if (fread(rec, 4, 3, over) != 3 || rec[0] < 0 || rec[0] > 1) return 8;
          g->ref = rec[0]; g->mv[0] = rec[1]; g->mv[1] = rec[2];
        }
      }
      put_grid(out, st);
      od_state_mc_predict(st, &pred);
      for (pli = 0; pli < 3; pli++) {
        put_plane(out, pred.planes + pli, st->frame_width >> pred.planes[pli].xdec,
         st->frame_height >> pred.planes[pli].ydec);
      }
    }
    /* the next frame's motion search starts from this frame's vectors: put the encoder's own back */
    for (v = 0; v <= st->nvmvbs; v++) {
      memcpy(st->mv_grid[v], saved + (size_t)v*(st->nhmvbs + 1), sizeof(*saved)*(st->nhmvbs + 1));
    }
  }
  fclose(out);
  return 0;
}
"""


def make_clip(w, h, c444, nframes, seed, pan_only=False):
    """Textured content cut into tiles that move independently: zones of 8, 16 and 32 pixel tiles and one
    that only pans (the last case pans as a whole), so the encoder splits its grid to different depths; a little noise per frame."""
    rng = np.random.RandomState(seed)
    big = rng.randint(0, 256, size=(h + 128, w + 128)).astype(np.float64)
    for _ in range(2):
        big = (big + np.roll(big, 1, 0) + np.roll(big, 1, 1) + np.roll(np.roll(big, 1, 0), 1, 1))/4
    big = np.clip((big - 128)*3 + 128, 0, 255)
    vel = {}
    frames = []
    for f in range(nframes):
        y = np.zeros((h, w))
        for ty in range(0, h, 8):
            for tx in range(0, w, 8):
                zone = (tx*4//w + ty*4//h) % 4
                size = 64 if pan_only else (8, 16, 32, 64)[zone]
                key = (tx//size, ty//size, size)
                if key not in vel:
                    vel[key] = (rng.uniform(-2.5, 2.5), rng.uniform(-2.5, 2.5)) if size < 64 else (2.0, 1.0)
                vx, vy = vel[key]
                ox, oy = 64 + int(round(vx*f)), 64 + int(round(vy*f))
                y[ty:ty + 8, tx:tx + 8] = big[ty + oy:ty + oy + 8, tx + ox:tx + ox + 8][:h - ty, :w - tx]
        y = np.clip(y + rng.randint(-2, 3, size=y.shape), 0, 255).astype(np.uint8)
        cw, ch = (w, h) if c444 else ((w + 1) >> 1, (h + 1) >> 1)
        step = 1 if c444 else 2
        cb = (128 + (y[::step, ::step][:ch, :cw].astype(int) - 128)//3).astype(np.uint8)
        cr = (128 - (y[::step, ::step][:ch, :cw].astype(int) - 128)//4).astype(np.uint8)
        frames.append(y.tobytes() + cb.tobytes() + cr.tobytes())
    return b"".join(frames)


def offenders(grid, dec):
    """Grid points whose vector takes some leaf corner's filter window outside the border at this decimation."""
    nv, nh = grid.shape[0] - 1, grid.shape[1] - 1
    w, h, pad = nh << 3 >> dec, nv << 3 >> dec, R.BORDER >> dec
    bad = set()
    for vx, vy, lg, oc, s in R.leaves(grid["valid"]):
        blk = 8 << lg >> dec
        for k in range(4):
            dx, dy = R.vertex(oc, s, k)
            py, px = vy + (dy << lg), vx + (dx << lg)
            pt = grid[py, px]
            x0 = (vx << 3 >> dec) + (R.scale_mv(int(pt["mvx"]), dec) >> 3) - 2
            y0 = (vy << 3 >> dec) + (R.scale_mv(int(pt["mvy"]), dec) >> 3) - 2
            if x0 < -pad or x0 + blk + 5 > w + pad or y0 < -pad or y0 + blk + 5 > h + pad:
                bad.add((py, px))
    return bad


def random_grid(valid, rng, decs):
    """The encoder's valid pattern with random slots and vectors, pulled back into the legal range."""
    g = np.zeros(valid.shape, R.MV_POINT)
    g["valid"] = valid
    g["ref"] = rng.randint(0, 2, size=valid.shape)
    g["mvx"] = rng.randint(-62*8, 62*8 + 1, size=valid.shape)
    g["mvy"] = rng.randint(-62*8, 62*8 + 1, size=valid.shape)
    # a third of the points share their left neighbour's vector and slot: corners that need one prediction
    same = rng.rand(*valid.shape) < 0.33
    same[:, 0] = False
    for name in ("ref", "mvx", "mvy"):
        g[name][same] = np.roll(g[name], 1, 1)[same]
    for _ in range(64):
        bad = set()
        for dec in decs:
            bad |= offenders(g, dec)
        if not bad:
            return g
        for py, px in bad:
            # shrink towards zero by a random amount: keeps the fractional phases spread
            g["mvx"][py, px] = int(g["mvx"][py, px]*rng.uniform(0.6, 0.95))
            g["mvy"][py, px] = int(g["mvy"][py, px]*rng.uniform(0.6, 0.95))
    raise SystemExit("could not legalise a random grid")


def parse(blob, c444, fpr, keep):
    pos = 0

    def ints(n):
        nonlocal pos
        v = np.frombuffer(blob, "<i4", n, pos)
        pos += 4*n
        return v

    def planes(w, h):
        nonlocal pos
        out = []
        for pli in range(3):
            pw, ph = (w, h) if (pli == 0 or c444) else (w >> 1, h >> 1)
            out.append(np.frombuffer(blob, "<i2" if fpr else "u1", pw*ph, pos).reshape(ph, pw).copy())
            pos += pw*ph*(2 if fpr else 1)
        return out

    w, h = ints(2)
    nh, nv = w >> 3, h >> 3
    frames = []
    while pos < len(blob):
        f = int(ints(1)[0])
        refs = [planes(w, h) for _ in range(2)]
        variants = []
        for _ in range(int(ints(1)[0])):
            raw = ints((nv + 1)*(nh + 1)*4).reshape(nv + 1, nh + 1, 4)
            g = np.zeros((nv + 1, nh + 1), R.MV_POINT)
            g["valid"], g["ref"], g["mvx"], g["mvy"] = raw[..., 0], raw[..., 1], raw[..., 2], raw[..., 3]
            variants.append((g, planes(w, h)))
        if f in keep:
            frames.append((f, refs, variants))
    return int(w), int(h), frames


def main():
    if len(sys.argv) != 2:
        raise SystemExit(__doc__)
    ref_tree = os.path.abspath(sys.argv[1])
    libdir = os.path.join(ROOT, "oracle", "_ref")
    data = {}
    names = []
    sizes_seen, ocs_seen, phases, reach, mixed = set(), set(), set(), [0, 0, 0, 0], 0
    with tempfile.TemporaryDirectory() as d:
        open(os.path.join(d, "driver.c"), "w").write(DRIVER)
        exe = os.path.join(d, "driver")
        subprocess.run(["gcc", "-O2", "-std=gnu99", "-w", "-I" + os.path.join(ref_tree, "include"),
                        "-I" + os.path.join(ref_tree, "src"), "-o", exe, os.path.join(d, "driver.c"),
                        "-L" + libdir, "-ldaalaref", "-Wl,-rpath," + libdir, "-lm"], check=True)
        for ci, (name, w, h, c444, fpr, nframes, keep, nrand, quant, mvmax) in enumerate(CASES):
            clip = os.path.join(d, "clip.yuv")
            open(clip, "wb").write(make_clip(w, h, c444, nframes, 100 + ci, pan_only=name.startswith("444_fpr")))
            first, over = os.path.join(d, "a.bin"), os.path.join(d, "over.bin")
            args = [exe, str(w), str(h), str(c444), str(fpr), str(nframes), clip]
            subprocess.run(args + [first, str(quant), str(mvmax)], check=True)
            cw, ch, frames = parse(open(first, "rb").read(), c444, fpr, set(range(1, nframes)))
            rng = np.random.RandomState(7 + ci)
            decs = (0,) if c444 else (0, 1)
            with open(over, "wb") as fo:
                for f, _, variants in frames:
                    n = nrand if f in keep else 0
                    fo.write(struct.pack("<i", n))
                    for _ in range(n):
                        g = random_grid(variants[0][0]["valid"], rng, decs)
                        rec = np.stack([g["ref"].astype("<i4"), g["mvx"], g["mvy"]], -1).astype("<i4")
                        fo.write(rec.tobytes())
            second = os.path.join(d, "b.bin")
            subprocess.run(args + [second, str(quant), str(mvmax), over], check=True)
            cw, ch, frames = parse(open(second, "rb").read(), c444, fpr, set(keep))
            assert [f for f, _, _ in frames] == list(keep)
            for f, refs, variants in frames:
                for vi, (g, want) in enumerate(variants):
                    key = "%s_f%d_v%d" % (name, f, vi)
                    names.append(key)
                    assert all(R.grid_in_range(g, dec) for dec in decs), key
                    for pli in range(3):
                        dec = 0 if (pli == 0 or c444) else 1
                        got = R.mc_predict_plane([refs[0][pli], refs[1][pli]], g, dec, fpr)
                        assert np.array_equal(got, want[pli]), (key, pli)
                        data["%s_pred%d" % (key, pli)] = want[pli]
                    data[key + "_grid"] = g
                    data[key + "_refs"] = np.array("%s_f%d" % (name, f))
                    for vx, vy, lg, oc, s in R.leaves(g["valid"]):
                        sizes_seen.add(lg)
                        ocs_seen.add((oc, s) if lg < 3 else (0, 3))
                        slots = set()
                        for k in range(4):
                            dx, dy = R.vertex(oc, s, k)
                            pt = g[vy + (dy << lg), vx + (dx << lg)]
                            slots.add(int(pt["ref"]))
                            phases.add((int(pt["mvx"]) & 7, int(pt["mvy"]) & 7))
                            x0 = (vx << 3) + (int(pt["mvx"]) >> 3) - 2
                            y0 = (vy << 3) + (int(pt["mvy"]) >> 3) - 2
                            reach[0] = min(reach[0], x0)
                            reach[1] = min(reach[1], y0)
                            reach[2] = max(reach[2], x0 + (8 << lg) + 5 - cw)
                            reach[3] = max(reach[3], y0 + (8 << lg) + 5 - ch)
                        mixed += len(slots) > 1
                    print(key, "ok")
                for slot in range(2):
                    for pli in range(3):
                        data["%s_f%d_ref%d_%d" % (name, f, slot, pli)] = refs[slot][pli]
            data[name + "_info"] = np.array([w, h, cw, ch, c444, fpr], np.int32)
    assert sizes_seen == {0, 1, 2, 3}, sizes_seen
    assert ocs_seen == {(oc, s) for oc in range(4) for s in range(4)}, sorted(ocs_seen)
    assert len(phases) == 64, len(phases)
    assert reach[0] <= -48 and reach[1] <= -48 and reach[2] >= 48 and reach[3] >= 48, reach
    assert mixed > 0
    np.savez_compressed(OUT, names=np.array(names), cases=np.array([c[0] for c in CASES]), **data)
    size = os.path.getsize(OUT)
    print("wrote", OUT, size, "bytes; border reach", reach, "leaves with corners in two slots", mixed)
    assert size < 1000000, size


if __name__ == "__main__":
    main()
