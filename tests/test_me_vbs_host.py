"""The point rule of the variable-block-size motion search as its kernels compile it (daala_amd/csrc/me_vbs.cuh:
od_vbs_point_valid, od_vbs_point_size, od_vbs_leaf_log; included by k_me_vbs_decide and k_me_vbs_grid) compiled for the
HOST and compared, over whole frames of decision words, with the ordered construction of the pattern
(_mc_patterns.build), the yardstick's point sizes (_me_vbs_ref.point_sizes) and the recursive leaf walk
(_mc_ref.leaves).  Frames of more than one row of 64x64 cells, so that the cell above and the cell below are real, and
of more than one column, so that a row of words is indexed.  No GPU."""
import ctypes
import os
import subprocess

import numpy as np
import pytest

import _mc_patterns as P
import _mc_ref as R
import _me_vbs_ref as V

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

SRC = r"""
#include <stdint.h>
#define __host__
#define __device__
#include "me_vbs.cuh"
/* words [nv/8][nh/8]; valid, size [nv + 1][nh + 1]; leaf [nv][nh] */
extern "C" void vbs_fill(const uint32_t *words, int nh, int nv, uint8_t *valid, uint8_t *size, uint8_t *leaf) {
  const int n64 = nh >> 3;
  auto bits = [&](int bx, int by) { return words[by*n64 + bx]; };
  for (int y = 0; y <= nv; y++) {
    for (int x = 0; x <= nh; x++) {
      valid[y*(nh + 1) + x] = od_vbs_point_valid(bits, x, y, nh, nv);
      size[y*(nh + 1) + x] = (uint8_t)od_vbs_point_size(bits, x, y, nh, nv);
    }
  }
  for (int y = 0; y < nv; y++) {
    for (int x = 0; x < nh; x++) leaf[y*nh + x] = (uint8_t)od_vbs_leaf_log(bits, x, y, nh, nv);
  }
}
extern "C" int vbs_bit(int lg, int x, int y) { return od_vbs_bit(lg, x, y); }
"""

FRAMES = ((1, 1), (2, 1), (1, 3), (3, 2), (2, 3), (3, 3))      # in cells of 64: across, down
ALL = (1 << 21) - 1


@pytest.fixture(scope="module")
def lib(tmp_path_factory):
    d = tmp_path_factory.mktemp("vbs")
    src = d / "vbs.cc"
    src.write_text(SRC)
    so = d / "libvbs.so"
    subprocess.run(["g++", "-O1", "-std=c++17", "-fPIC", "-shared", "-I", os.path.join(ROOT, "daala_amd", "csrc"),
                    "-o", str(so), str(src)], check=True, capture_output=True)
    return ctypes.CDLL(str(so))


def bit(lg, x, y):
    """od_vbs_bit: the bit of the cell of 1 << lg steps that holds the 8x8 cell (x, y) of a 64x64 cell."""
    return 0 if lg == 3 else 1 + 2*(y >> 2) + (x >> 2) if lg == 2 else 5 + 4*(y >> 1) + (x >> 1)


def header(lib, words):
    """(valid, size, leaf) of the frame whose decision words are words [nv/8][nh/8], by the header."""
    words = np.ascontiguousarray(words, np.uint32)
    nv, nh = 8*words.shape[0], 8*words.shape[1]
    valid = np.full((nv + 1, nh + 1), 0xee, np.uint8)
    size = np.full((nv + 1, nh + 1), 0xee, np.uint8)
    leaf = np.full((nv, nh), 0xee, np.uint8)
    lib.vbs_fill(ctypes.c_void_p(words.ctypes.data), nh, nv,
                 *(ctypes.c_void_p(a.ctypes.data) for a in (valid, size, leaf)))
    return valid, size, leaf


def yardstick(words):
    """The same three arrays from build, point_sizes and leaves."""
    nv, nh = 8*words.shape[0], 8*words.shape[1]

    def split(lg, x, y):                        # of the cell of size lg at origin (x, y)
        return bool(int(words[y >> 3, x >> 3]) >> bit(lg, x & 7, y & 7) & 1)

    valid = P.build(8*nh, 8*nv, lambda lg, x, y: split(lg, x - (1 << lg >> 1), y - (1 << lg >> 1)),
                    lambda lg, x, y: True)
    sizes = V.point_sizes(valid)
    size = np.array([[sizes.get((x, y), 4) for x in range(nh + 1)] for y in range(nv + 1)], np.uint8)
    leaf = np.full((nv, nh), 0xff, np.uint8)
    for vx, vy, lg, _, _ in R.leaves(valid):
        leaf[vy:vy + (1 << lg), vx:vx + (1 << lg)] = lg
    return valid, size, leaf


def same(lib, words, what):
    got, want = header(lib, words), yardstick(words)
    for name, g, w in zip(("valid", "size", "leaf"), got, want):
        bad = np.argwhere(g != w)
        assert bad.size == 0, (what, name, bad[:5].tolist(), [hex(int(x)) for x in words.ravel()])
    return want


def test_the_bit_layout(lib):
    seen = set()
    for lg in (3, 2, 1):
        for y in range(0, 8, 1 << lg):
            for x in range(0, 8, 1 << lg):
                assert lib.vbs_bit(lg, x, y) == bit(lg, x, y)
                assert lib.vbs_bit(lg, x + (1 << lg) - 1, y + (1 << lg) - 1) == bit(lg, x, y)
                seen.add(bit(lg, x, y))
    assert seen == set(range(21))


@pytest.mark.parametrize("cols,rows", FRAMES)
def test_random_words(lib, cols, rows):
    rng = np.random.RandomState(17 + 8*cols + rows)
    kinds = set()
    for p in (0.5, 0.8, 1.0):
        for trial in range(1 if p == 1.0 else 12):
            words = np.zeros((rows, cols), np.uint32)
            for b in range(21):
                words |= (rng.rand(rows, cols) < p).astype(np.uint32) << b
            # (bits above the 21 decisions are nobody's: set in every other trial, they change nothing)
            if trial & 1:
                words |= rng.randint(0, 1 << 11, size=(rows, cols)).astype(np.uint32) << 21
            valid, size, leaf = same(lib, words, (cols, rows, p, trial))
            kinds |= set(leaf.ravel().tolist())
            assert p < 1.0 or (valid.all() and not size.any() and not leaf.any())
    assert kinds == {0, 1, 2, 3}


@pytest.mark.parametrize("cols,rows", FRAMES)
def test_all_zero_and_all_one_words(lib, cols, rows):
    valid, size, leaf = same(lib, np.zeros((rows, cols), np.uint32), "zeros")
    assert int(valid.sum()) == (rows + 1)*(cols + 1) and np.all(leaf == 3)
    assert np.all(size[::8, ::8] == 3) and int((size == 4).sum()) == size.size - (rows + 1)*(cols + 1)
    valid, size, leaf = same(lib, np.full((rows, cols), 0xffffffff, np.uint32), "ones")
    assert valid.all() and not size.any() and not leaf.any()


@pytest.mark.parametrize("cols,rows", FRAMES)
def test_one_unsplit_cell_among_fully_split_ones(lib, cols, rows):
    """Exactly one 64x64 cell is a leaf (whatever its other bits say) and every other cell is split down to 8x8: the
    midpoints of the leaf's four edges are invalid, every neighbour keeps the two 32x32 quadrants along the shared edge
    whole and no other - above and below as to the left and right."""
    rng = np.random.RandomState(3)
    for cy in range(rows):
        for cx in range(cols):
            for rest in (ALL & ~1, int(rng.randint(0, 1 << 20)) << 1):
                words = np.full((rows, cols), ALL, np.uint32)
                words[cy, cx] = rest
                valid, size, leaf = same(lib, words, (cols, rows, cx, cy, rest))
                x, y = 8*cx, 8*cy
                assert np.all(leaf[y:y + 8, x:x + 8] == 3) and int((leaf == 3).sum()) == 64
                assert not valid[y + 4, x + 4]
                assert not (valid[y, x + 4] or valid[y + 8, x + 4] or valid[y + 4, x] or valid[y + 4, x + 8])
                # the neighbours' quadrants along the shared edge: leaves of 32, as many as there are neighbours
                sides = [(x, y - 4, 8, 4), (x, y + 8, 8, 4), (x - 4, y, 4, 8), (x + 8, y, 4, 8)]
                inside = [(sx, sy, w, h) for sx, sy, w, h in sides if 0 <= sx < 8*cols and 0 <= sy < 8*rows]
                for sx, sy, w, h in inside:
                    assert np.all(leaf[sy:sy + h, sx:sx + w] == 2), (cx, cy, sx, sy)
                assert int((leaf == 2).sum()) == 32*len(inside)
