"""The lapped transform at a MIXED block-size map, restated from the oracle's primitives.

odhip_inverse_partition replays the decoder's quadtree recursion (include/daala_hip.h; the level-by-level
form of daala_amd/csrc/lapped_kernels.hip, "inverse at an ARBITRARY partition").  The oracle has every
piece of that recursion - odo_idct_2d, odo_fdct_2d, odo_postfilter_split, odo_prefilter_split, the
superblock-edge filters and the pixel conversions - so the yardstick is a composition of them, written
here as the plain recursion and pinned to the real decoder by tests/golden/partition.npz
(tools/make_golden_partition.py, tests/test_partition_ref.py).

A map is uint8 [rows][cols], one entry per 8x8 LUMA area: 0 = four 4x4 blocks, 1 = 8x8 ... 4 = 64x64.
A plane is [h][w] with dec = 0 (luma, or a 4:4:4 chroma plane) or dec = 1 (4:2:0 chroma: h, w are half
the map's extent, blocks one size down, 4x4 for both 8x8 and 4x4 luma).  pic_w, pic_h are the UNPADDED
LUMA picture size, also for chroma.
"""
import ctypes

import numpy as np

from _libs import P, oracle

TOP = 4          # the superblock's level: 64x64 luma


# ---- maps ----------------------------------------------------------------------------------------

def is_quadtree(bmap):
    """Every block of size L sits aligned on its own grid and all of its units hold L."""
    bmap = np.asarray(bmap)
    rows, cols = bmap.shape
    if rows % 8 or cols % 8 or bmap.max() > TOP:
        return False
    for r in range(rows):
        for c in range(cols):
            u = 1 << max(int(bmap[r, c]) - 1, 0)            # units per side: 1 for 4x4 and 8x8
            r0, c0 = r & ~(u - 1), c & ~(u - 1)
            if not (bmap[r0:r0 + u, c0:c0 + u] == bmap[r, c]).all():
                return False
    return True


def leaf_sizes(bmap):
    """The leaf sizes a map holds, sorted."""
    return sorted(int(v) for v in np.unique(bmap))


def random_map(rng, nsbx, nsby, p_split):
    """A random valid quadtree: every node above 4x4 is split with probability p_split."""
    bmap = np.zeros((nsby * 8, nsbx * 8), np.uint8)

    def node(r, c, bsi):
        if bsi > 0 and rng.random_sample() >= p_split:
            u = 1 << (bsi - 1)
            bmap[r:r + u, c:c + u] = bsi
        elif bsi > 1:
            u = 1 << (bsi - 2)
            for dr in (0, u):
                for dc in (0, u):
                    node(r + dr, c + dc, bsi - 1)
        # else: an 8x8 area split into four 4x4 blocks, 0

    for sy in range(nsby):
        for sx in range(nsbx):
            node(sy * 8, sx * 8, TOP)
    return bmap


def deep_corner(which):
    """One superblock split down to 4x4 along the path into one corner only (which: 0 top-left, 1 top-right,
    2 bottom-left, 3 bottom-right); the three siblings at every depth stay whole."""
    m = np.zeros((8, 8), np.uint8)
    right, bottom = which & 1, which >> 1
    r, c = 0, 0
    for bsi in (4, 3, 2):
        u = 1 << (bsi - 2)                                  # units per child side
        for dr in (0, 1):
            for dc in (0, 1):
                m[r + dr * u:r + (dr + 1) * u, c + dc * u:c + (dc + 1) * u] = bsi - 1
        r, c = r + bottom * u, c + right * u
    m[r, c] = 0
    return m


def tiled(sbs, nsbx, nsby):
    """A frame map of nsbx x nsby superblocks taken round-robin from the 8x8 maps `sbs`."""
    bmap = np.zeros((nsby * 8, nsbx * 8), np.uint8)
    for sy in range(nsby):
        for sx in range(nsbx):
            bmap[sy * 8:sy * 8 + 8, sx * 8:sx * 8 + 8] = sbs[(sy * nsbx + sx) % len(sbs)]
    return bmap


def corners(nsbx, nsby):
    return tiled([deep_corner(k) for k in range(4)], nsbx, nsby)


def extremes(nsbx, nsby):
    """All-4x4 and 64x64 superblocks in a checkerboard: every superblock edge couples the two."""
    r, c = np.ogrid[0:nsby * 8, 0:nsbx * 8]
    return (4 * (((r >> 3) + (c >> 3)) & 1)).astype(np.uint8)


def units01(nsbx, nsby):
    """0 and 1 alternating per unit: every 16x16 node is split into 8x8 blocks and 4x4 quads."""
    r, c = np.ogrid[0:nsby * 8, 0:nsbx * 8]
    return ((r + c) & 1).astype(np.uint8)


def nodes16(rng, nsbx, nsby):
    """Every 16x16 node split, its children 8x8 or 4x4 at random."""
    return rng.randint(0, 2, size=(nsby * 8, nsbx * 8)).astype(np.uint8)


def uniform(level, nsbx, nsby):
    return np.full((nsby * 8, nsbx * 8), level, np.uint8)


# ---- the recursion -------------------------------------------------------------------------------

def _walk(bmap, dec, w, h, pic_w, pic_h, leaf, split_before, split_after):
    """od_decode_recursive / od_encode_recursive's walk of every superblock.  Node (bx, by) of luma size
    bsi: obs is the map at the node's TOP-LEFT unit, bs = max(obs, dec); bs == bsi is a leaf, transformed
    at level bsi - dec.  Otherwise the four children, between split_before and split_after, whose filters
    are gated by  (bx + 1) << (2 + bsi - dec) <= pic_w  (and pic_h): the block is counted in the PLANE's
    samples, the picture in LUMA's - the reference does this, for chroma too."""
    def node(bx, by, bsi):
        obs = int(bmap[(by << bsi) >> 1, (bx << bsi) >> 1])
        bs = max(obs, dec)
        assert bs <= bsi, "not a quadtree at (%d, %d) size %d" % (bx, by, bsi)
        lv = bsi - dec
        n = 4 << lv
        if bs == bsi:
            leaf(by * n, bx * n, lv)
            return
        hf = int((bx + 1) << (2 + lv) <= pic_w)
        vf = int((by + 1) << (2 + lv) <= pic_h)
        split_before(by * n, bx * n, lv, hf, vf)
        for cy in (0, 1):
            for cx in (0, 1):
                node(2 * bx + cx, 2 * by + cy, bsi - 1)
        split_after(by * n, bx * n, lv, hf, vf)

    sb = 64 >> dec
    for sby in range(h // sb):
        for sbx in range(w // sb):
            node(sbx, sby, TOP)


def _check(plane, bmap, dec):
    h, w = plane.shape
    sb = 64 >> dec
    assert h % sb == 0 and w % sb == 0 and bmap.shape == ((h // sb) * 8, (w // sb) * 8), (plane.shape, bmap.shape)
    return h, w


def _nothing(*_):
    pass


def inverse(coef, bmap, dec, pic_w, pic_h, fpr):
    """Pixels (uint8, or int16 at 12 bits for fpr) of one dequantised coefficient plane at the map."""
    o = oracle()
    coef = np.ascontiguousarray(coef, np.int32)
    bmap = np.asarray(bmap)
    h, w = _check(coef, bmap, dec)
    c = np.zeros((h, w), np.int32)
    at = lambda a, y, x: ctypes.c_void_p(a.ctypes.data + 4 * (y * w + x))          # noqa: E731

    def leaf(y, x, lv):
        o.odo_idct_2d(lv, at(c, y, x), w, at(coef, y, x), w)

    def post(y, x, lv, hf, vf):
        o.odo_postfilter_split(at(c, y, x), w, lv, hf, vf)

    _walk(bmap, dec, w, h, pic_w, pic_h, leaf, _nothing, post)
    o.odo_apply_postfilter_frame_sbs(P(c), w, w >> (6 - dec), h >> (6 - dec), dec, dec)
    if fpr:
        px = np.zeros((h, w), np.uint16)
        o.odo_coeff_to_px16(P(px), w, P(c), w, w, h)
        return px.view(np.int16)
    px = np.zeros((h, w), np.uint8)
    o.odo_coeff_to_px(P(px), w, P(c), w, w, h)
    return px


def forward(px, bmap, dec, pic_w, pic_h, fpr):
    """The coefficient plane of one pixel plane at the map: every leaf's forward DCT where it lies."""
    o = oracle()
    bmap = np.asarray(bmap)
    h, w = _check(px, bmap, dec)
    c = np.zeros((h, w), np.int32)
    if fpr:
        o.odo_px16_to_coeff(P(c), w, P(np.ascontiguousarray(px, np.int16).view(np.uint16)), w, w, h)
    else:
        o.odo_px_to_coeff(P(c), w, P(np.ascontiguousarray(px, np.uint8)), w, w, h)
    o.odo_apply_prefilter_frame_sbs(P(c), w, w >> (6 - dec), h >> (6 - dec), dec, dec)
    out = np.zeros((h, w), np.int32)
    at = lambda a, y, x: ctypes.c_void_p(a.ctypes.data + 4 * (y * w + x))          # noqa: E731

    def leaf(y, x, lv):
        o.odo_fdct_2d(lv, at(out, y, x), w, at(c, y, x), w)

    def pre(y, x, lv, hf, vf):
        o.odo_prefilter_split(at(c, y, x), w, lv, hf, vf)

    _walk(bmap, dec, w, h, pic_w, pic_h, leaf, pre, _nothing)
    return out


# ---- tests/golden/partition.npz ------------------------------------------------------------------

_META = ("clip", "frame", "pli", "dec", "keyframe", "pic_w", "pic_h")


def save_cases(path, records):
    """Recorded planes of the real decoder (tools/make_golden_partition.py): data only."""
    d = {"meta": np.array([[r[k] for k in _META] for r in records], np.int32)}
    for i, r in enumerate(records):
        d["coef%d" % i] = r["coef"].astype(np.int32)
        d["bmap%d" % i] = r["bmap"].astype(np.uint8)
        d["recon%d" % i] = r["recon"].astype(np.uint8)
    np.savez_compressed(path, **d)


def load_cases(path):
    z = np.load(path)
    out = []
    for i, row in enumerate(z["meta"]):
        r = {k: int(v) for k, v in zip(_META, row)}
        r.update(coef=z["coef%d" % i], bmap=z["bmap%d" % i], recon=z["recon%d" % i])
        out.append(r)
    return out


def check_golden_coverage(records):
    """What the recorder promises and the tests rely on: luma maps that hold all five leaf sizes, some of them
    mixed inside one superblock, an inter frame, and a picture size that is no multiple of 64."""
    luma = [r for r in records if r["pli"] == 0]
    sizes = set()
    for r in luma:
        sizes.update(leaf_sizes(r["bmap"]))
    assert sizes == {0, 1, 2, 3, 4}, sizes
    assert any(len(np.unique(r["bmap"][y:y + 8, x:x + 8])) >= 3 for r in luma
               for y in range(0, r["bmap"].shape[0], 8) for x in range(0, r["bmap"].shape[1], 8))
    assert any(not r["keyframe"] for r in records)
    assert any(r["pic_w"] % 64 or r["pic_h"] % 64 for r in records)
    assert {r["dec"] for r in records} == {0, 1}
