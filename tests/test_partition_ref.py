"""CPU: tests/_partition_ref.py - the lapped transform at a mixed block-size map, composed from the oracle's
primitives - against the oracle's own uniform-level plane functions, against itself (forward then inverse is
the identity), and against planes recorded inside the real reference decoder (tests/golden/partition.npz,
tools/make_golden_partition.py).  It is the yardstick of tests/test_gpu_partition.py."""
import ctypes
import functools

import numpy as np
import pytest

import _partition_ref as R
from _libs import GOLDEN, P, oracle

NSBX, NSBY = 2, 2                      # a 128x128 frame: one interior superblock edge each way
# luma picture sizes: the full frame; cropped by a few samples; one at which the gate flips inside a
# superblock for every node size (100 = 64 + 32 + 4, 44 = 32 + 8 + 4) and lands ON node borders of 8 and 16
# (96, 48); one so small that it flips for 4:2:0 chroma too (17 < 64 = the chroma plane's width)
PICS = [(128, 128), (122, 118), (100, 44), (96, 48), (17, 9)]
PIC_IDS = ["%dx%d" % p for p in PICS]


def _px(rng, h, w, fpr):
    top = 4095 if fpr else 255
    px = rng.randint(0, top + 1, size=(h, w))
    px[:8, :8] = top
    px[8:16, :8] = 0
    return px.astype(np.int16 if fpr else np.uint8)


@functools.lru_cache(maxsize=None)
def _maps():
    rng = np.random.RandomState(77)
    maps = {"corners": R.corners(NSBX, NSBY), "extremes": R.extremes(NSBX, NSBY), "units01": R.units01(NSBX, NSBY),
            "nodes16": R.nodes16(rng, NSBX, NSBY)}
    for k, p in enumerate((0.5, 0.75)):
        maps["random%d" % k] = R.random_map(rng, NSBX, NSBY, p)
    for m in maps.values():
        m.setflags(write=False)
    return maps


MAP_NAMES = ["corners", "extremes", "units01", "nodes16", "random0", "random1"]


def test_map_helpers():
    for name, m in _maps().items():
        assert R.is_quadtree(m), name
    assert R.leaf_sizes(_maps()["corners"]) == [0, 1, 2, 3]
    assert R.leaf_sizes(_maps()["extremes"]) == [0, 4]
    assert R.leaf_sizes(_maps()["units01"]) == [0, 1]
    for which in range(4):
        m = R.deep_corner(which)
        r, c = 7 * (which >> 1), 7 * (which & 1)
        assert m[r, c] == 0 and (m == 0).sum() == 1 and (m == 1).sum() == 3, which
        assert (m == 2).sum() == 3 * 4 and (m == 3).sum() == 3 * 16 and R.is_quadtree(m)
    assert any(R.leaf_sizes(R.random_map(np.random.RandomState(s), 3, 2, 0.6)) == [0, 1, 2, 3, 4] for s in range(4))
    bad = R.uniform(2, 1, 1)
    bad[1, 1] = 1                               # a 16x16 block one of whose units says 8x8
    assert not R.is_quadtree(bad)
    bad = R.uniform(0, 1, 1)
    bad[1:3, 1:3] = 2                           # a 16x16 block off its grid
    assert not R.is_quadtree(bad)
    assert not R.is_quadtree(R.uniform(5, 1, 1))


@pytest.mark.parametrize("pic", PICS, ids=PIC_IDS)
@pytest.mark.parametrize("fpr", [0, 1], ids=["u8", "fpr"])
@pytest.mark.parametrize("dec", [0, 1])
def test_uniform_map_equals_the_oracles_level_functions(dec, fpr, pic):
    """inverse() == odo_inverse_level_plane and forward() == that level of odo_forward_pyramid_plane over the
    whole plane, for every level; a 4:2:0 plane at level L from the luma map L + 1, and level 0 from map 0 too."""
    o = oracle()
    rng = np.random.RandomState(10 * dec + fpr)
    h, w = (NSBY * 64) >> dec, (NSBX * 64) >> dec
    pw, ph = pic
    px = _px(rng, h, w, fpr)
    levels = [np.zeros((h, w), np.int32) for _ in range(5)]
    o.odo_set_fpr(fpr)
    try:
        o.odo_forward_pyramid_plane((ctypes.c_void_p * 5)(*[a.ctypes.data for a in levels]), P(np.zeros((h, w), np.int32)),
                                    P(px), w, w, h, dec, pw, ph)
        for lum in range(5):
            lv = max(lum - dec, 0)
            bmap = R.uniform(lum, NSBX, NSBY)
            assert np.array_equal(R.forward(px, bmap, dec, pw, ph, fpr), levels[lv]), (lum, "forward")
            coef = np.ascontiguousarray(((levels[lv] + 32) // 64) * 64 + rng.randint(-700, 701, size=(h, w)).astype(np.int32))
            want = np.zeros((h, w), np.uint16 if fpr else np.uint8)
            o.odo_inverse_level_plane(P(want), w, P(np.zeros((h, w), np.int32)), P(coef), w, h, dec, lv, pw, ph)
            got = R.inverse(coef, bmap, dec, pw, ph, fpr)
            assert np.array_equal(got, want.view(got.dtype)), (lum, "inverse")
    finally:
        o.odo_set_fpr(0)


@pytest.mark.parametrize("pic", PICS, ids=PIC_IDS)
@pytest.mark.parametrize("name", MAP_NAMES)
@pytest.mark.parametrize("fpr", [0, 1], ids=["u8", "fpr"])
@pytest.mark.parametrize("dec", [0, 1])
def test_forward_then_inverse_is_the_identity(dec, fpr, name, pic):
    rng = np.random.RandomState(3 + dec)
    h, w = (NSBY * 64) >> dec, (NSBX * 64) >> dec
    px = _px(rng, h, w, fpr)
    bmap = _maps()[name]
    coef = R.forward(px, bmap, dec, pic[0], pic[1], fpr)
    assert np.array_equal(R.inverse(coef, bmap, dec, pic[0], pic[1], fpr), px)


def _mixed_from_uniform(bmap, dec, by_level):
    """Every superblock of the map is uniform: take each superblock's samples from that level's plane."""
    out = np.zeros_like(by_level[0])
    sb = 64 >> dec
    for sy in range(bmap.shape[0] // 8):
        for sx in range(bmap.shape[1] // 8):
            lv = max(int(bmap[sy * 8, sx * 8]) - dec, 0)
            out[sy * sb:(sy + 1) * sb, sx * sb:(sx + 1) * sb] = by_level[lv][sy * sb:(sy + 1) * sb, sx * sb:(sx + 1) * sb]
    return out


@pytest.mark.parametrize("pic", PICS, ids=PIC_IDS)
@pytest.mark.parametrize("dec", [0, 1])
def test_picture_gate_of_every_node_size_in_a_mixed_map(dec, pic):
    """`extremes` has uniform superblocks, so its forward() is superblock by superblock the oracle's pyramid at
    the picture sizes where the gate flips inside a superblock (the pre-filters of a split superblock touch
    nothing outside it); a map split to 4x4 everywhere must DIFFER between a picture size and the next one down
    a node border, or the gate would be decoration."""
    o = oracle()
    rng = np.random.RandomState(5)
    h, w = (NSBY * 64) >> dec, (NSBX * 64) >> dec
    pw, ph = pic
    px = _px(rng, h, w, 0)
    levels = [np.zeros((h, w), np.int32) for _ in range(5)]
    o.odo_forward_pyramid_plane((ctypes.c_void_p * 5)(*[a.ctypes.data for a in levels]), P(np.zeros((h, w), np.int32)),
                                P(px), w, w, h, dec, pw, ph)
    bmap = R.extremes(NSBX, NSBY)
    assert np.array_equal(R.forward(px, bmap, dec, pw, ph, 0), _mixed_from_uniform(bmap, dec, levels))
    fine = R.uniform(0, NSBX, NSBY)
    coef = levels[0]
    for n in (8, 16, 32, 64):                       # node sizes in plane samples; a 4:2:0 plane has none of 64
        edge = (min(pw, w) // n) * n                  # the last node border inside the picture and the plane
        if n > (64 >> dec) or edge == 0:
            continue
        cols = slice(edge - n, edge)
        on = R.inverse(coef, fine, dec, edge, ph, 0)  # `<=`: the node that ends ON the picture's edge is filtered,
        off = R.inverse(coef, fine, dec, edge - 1, ph, 0)   # one sample less and it is not
        assert not np.array_equal(on[:, cols], off[:, cols]), n


def test_only_the_top_left_unit_of_a_node_is_read():
    """The recursion reads the map at a node's top-left unit and nowhere else (OD_BLOCK_SIZE4x4 at (bx << bsi,
    by << bsi)): scribbling over the other units of every leaf of 16x16 and more changes nothing."""
    rng = np.random.RandomState(8)
    for name in ("corners", "random0", "extremes"):
        bmap = _maps()[name]
        dirty = bmap.copy()
        for r in range(dirty.shape[0]):
            for c in range(dirty.shape[1]):
                u = 1 << max(int(bmap[r, c]) - 1, 0)
                if r % u or c % u:
                    dirty[r, c] = (int(bmap[r, c]) + 1 + rng.randint(4)) % 5
        assert not np.array_equal(dirty, bmap) and not R.is_quadtree(dirty)
        for dec in (0, 1):
            h, w = (NSBY * 64) >> dec, (NSBX * 64) >> dec
            coef = (rng.randint(-300, 301, size=(h, w)) * 8).astype(np.int32)
            assert np.array_equal(R.inverse(coef, dirty, dec, 122, 118, 0), R.inverse(coef, bmap, dec, 122, 118, 0))


def test_chroma_420_has_no_leaf_below_the_8x8_luma_area():
    """4x4 and 8x8 luma both give a 4x4 chroma leaf: any map of 0s and 1s is, for a 4:2:0 plane, the uniform
    map 1 - the oracle's level 0."""
    o = oracle()
    rng = np.random.RandomState(9)
    h, w = NSBY * 32, NSBX * 32
    coef = (rng.randint(-300, 301, size=(h, w)) * 8).astype(np.int32)
    want = np.zeros((h, w), np.uint8)
    o.odo_inverse_level_plane(P(want), w, P(np.zeros((h, w), np.int32)), P(coef), w, h, 1, 0, 100, 44)
    for name in ("units01", "nodes16"):
        assert np.array_equal(R.inverse(coef, _maps()[name], 1, 100, 44, 0), want), name


# ---- the real decoder ----------------------------------------------------------------------------

CASES = R.load_cases(GOLDEN + "/partition.npz")


def test_golden_has_the_coverage_the_recorder_promised():
    R.check_golden_coverage(CASES)
    for r in CASES:
        assert R.is_quadtree(r["bmap"]), (r["clip"], r["frame"])
        sb = 64 >> r["dec"]
        h, w = r["coef"].shape
        assert r["recon"].shape == (h, w) and r["recon"].dtype == np.uint8 and r["coef"].dtype == np.int32
        assert r["bmap"].shape == (h // sb * 8, w // sb * 8)


@pytest.mark.parametrize("i", range(len(CASES)), ids=["c%df%dp%d" % (r["clip"], r["frame"], r["pli"]) for r in CASES])
def test_inverse_equals_the_real_decoder(i):
    r = CASES[i]
    got = R.inverse(r["coef"], r["bmap"], r["dec"], r["pic_w"], r["pic_h"], False)
    assert np.array_equal(got, r["recon"]), int((got != r["recon"]).sum())
