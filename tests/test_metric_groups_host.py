"""How a call of a tiled metric is cut into launch groups (daala_amd/csrc/od_metric_groups.h: metric_groups, which
odhip_ssim_planes, odhip_msssim_planes and odhip_fastssim_planes call with 32 pairs and 1 << 22 tiles per group) compiled
for the HOST and driven with 4 pairs and 10 tiles per group, so that every branch is reached - the tile cap too, which no
plane a test can afford reaches in the library.  Compared with a restatement of the rule in Python, and checked against
the rule's own terms: the order is a permutation, stable by source plane when planes are sorted; no group above the pair
cap; none above the tile cap unless it is one run; a run that fits the pair cap is never split.  No GPU."""
import ctypes
import os
import subprocess
import sys

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

SRC = r"""
#include "od_metric_groups.h"
/* idx [n], first [n + 1]; returns the number of groups.  A pair of w x h has ceil(w/2) x ceil(h/2) tiles. */
extern "C" int plan(const odhip_metrics_pair *pairs, int n, int max_pairs, long max_tiles, int by_plane, int *idx,
 int *first) {
  const MetricGroups g = metric_groups(pairs, n,
   [](const odhip_metrics_pair &q) { return (long)((q.w + 1)/2)*((q.h + 1)/2); }, max_pairs, max_tiles, by_plane != 0);
  for (size_t i = 0; i < g.idx.size(); i++) idx[i] = g.idx[i];
  for (size_t i = 0; i < g.first.size(); i++) first[i] = g.first[i];
  return g.count();
}
extern "C" int before(const odhip_metrics_pair *a, const odhip_metrics_pair *b) { return plane_before(*a, *b); }
extern "C" int same(const odhip_metrics_pair *a, const odhip_metrics_pair *b) { return same_plane(*a, *b); }
"""

PAIRS, TILES = 4, 10


@pytest.fixture(scope="module")
def lib(tmp_path_factory):
    d = tmp_path_factory.mktemp("groups")
    src = d / "groups.cc"
    src.write_text(SRC)
    so = d / "libgroups.so"
    subprocess.run(["g++", "-O1", "-std=c++17", "-fPIC", "-shared", "-I", os.path.join(ROOT, "daala_amd", "csrc"),
                    "-o", str(so), str(src)], check=True, capture_output=True)
    L = ctypes.CDLL(str(so))
    L.plan.argtypes = [ctypes.c_void_p, ctypes.c_int, ctypes.c_int, ctypes.c_long, ctypes.c_int, ctypes.c_void_p,
                       ctypes.c_void_p]
    return L


def pair(src, w, h, fmt=0, stride=None, depth=8, rec=0x9000):
    """(src, rec, src_fmt, rec_fmt, src_stride, rec_stride, w, h, depth, csf)"""
    return (src, rec, fmt, 0, w if stride is None else stride, w, w, h, depth, 0)


def key(p):
    """what plane_before orders by and same_plane compares: the source plane, not the reconstruction"""
    return (p[0], p[2], p[4], p[6], p[7], p[8])


def tiles(p):
    return ((p[6] + 1) // 2) * ((p[7] + 1) // 2)


def restated(pairs, by_plane, max_pairs=PAIRS, max_tiles=TILES):
    """The rule again: (order, runs, group boundaries)."""
    n = len(pairs)
    idx = sorted(range(n), key=lambda i: key(pairs[i])) if by_plane else list(range(n))      # sorted() is stable
    runs, a = [], 0
    while a < n:
        b = a + 1
        while by_plane and b < n and b - a < max_pairs and key(pairs[idx[b]]) == key(pairs[idx[a]]):
            b += 1
        runs.append((a, b))
        a = b
    first, m, t = [0], 0, 0
    for a, b in runs:
        rt = sum(tiles(pairs[idx[k]]) for k in range(a, b))
        if m > 0 and (m + b - a > max_pairs or t + rt > max_tiles):
            first.append(a)
            m = t = 0
        m += b - a
        t += rt
    if n:
        first.append(n)
    return idx, runs, first


def plan(lib, pairs, by_plane):
    from daala_amd.api import _MetricsPair
    n = len(pairs)
    arr = (_MetricsPair * max(1, n))(*[_MetricsPair(*p) for p in pairs])
    idx = np.full(n, -1, np.int32)
    first = np.full(n + 1, -1, np.int32)
    g = lib.plan(ctypes.addressof(arr), n, PAIRS, TILES, int(by_plane), idx.ctypes.data, first.ctypes.data)
    return idx.tolist(), first[:g + 1].tolist()


def check(lib, pairs, by_plane):
    """Every property of the plan of `pairs`; returns what closed or filled its groups, for the coverage assertions."""
    n = len(pairs)
    idx, first = plan(lib, pairs, by_plane)
    want_idx, runs, want_first = restated(pairs, by_plane)
    assert sorted(idx) == list(range(n))
    assert idx == want_idx and (by_plane or idx == list(range(n)))
    assert first == want_first, (pairs, by_plane, first, want_first)
    assert first[0] == 0 and first[-1] == n and all(a < b for a, b in zip(first, first[1:]))
    seen = set()
    group_of = {}
    for g, (a, b) in enumerate(zip(first, first[1:])):
        for k in range(a, b):
            group_of[k] = g
        t = sum(tiles(pairs[idx[k]]) for k in range(a, b))
        assert b - a <= PAIRS
        one_run = (a, b) in runs
        assert t <= TILES or one_run, (pairs, by_plane, a, b, t)
        if t > TILES:
            seen.add("alone above the tile cap")
        if b < n:
            # why the next run did not join: one cap or the other (or both)
            nb = next(y for x, y in runs if x == b)
            nt = sum(tiles(pairs[idx[k]]) for k in range(b, nb))
            assert (b - a) + (nb - b) > PAIRS or t + nt > TILES
            seen.add("closed by the pair cap" if (b - a) + (nb - b) > PAIRS else "closed by the tile cap")
    # a stretch of one source plane no longer than the pair cap is in one group
    a = 0
    while by_plane and a < n:
        b = a + 1
        while b < n and key(pairs[idx[b]]) == key(pairs[idx[a]]):
            b += 1
        if b - a <= PAIRS:
            assert len({group_of[k] for k in range(a, b)}) == 1, (pairs, a, b, first)
        else:
            seen.add("a run longer than the pair cap")
        a = b
    return seen


def test_the_key_is_the_source_plane(lib):
    from daala_amd.api import _MetricsPair
    base = pair(0x1000, 4, 6)
    others = [pair(0x2000, 4, 6), pair(0x1000, 4, 6, fmt=1), pair(0x1000, 4, 6, stride=5), pair(0x1000, 5, 6),
              pair(0x1000, 4, 7), pair(0x1000, 4, 6, depth=10)]
    a = _MetricsPair(*base)
    for o in others:
        b = _MetricsPair(*o)
        assert not lib.same(ctypes.byref(a), ctypes.byref(b))
        ab, ba = lib.before(ctypes.byref(a), ctypes.byref(b)), lib.before(ctypes.byref(b), ctypes.byref(a))
        assert ab == (key(base) < key(o)) and ba == (not ab), o
    b = _MetricsPair(*pair(0x1000, 4, 6, rec=0x7000))                   # another reconstruction of the same source
    assert lib.same(ctypes.byref(a), ctypes.byref(b)) and not lib.before(ctypes.byref(a), ctypes.byref(b))
    assert not lib.before(ctypes.byref(b), ctypes.byref(a))


@pytest.mark.parametrize("by_plane", [True, False], ids=["by_plane", "call_order"])
def test_fixed_cases(lib, by_plane):
    assert plan(lib, [], by_plane) == ([], [0])
    # one pair above the tile cap goes alone, and so does a run of them
    assert check(lib, [pair(0x1000, 8, 8)], by_plane) == {"alone above the tile cap"}
    big = [pair(0x1000, 2, 2), pair(0x2000, 8, 8), pair(0x2000, 8, 8, rec=0x7000), pair(0x3000, 2, 2)]
    assert plan(lib, big, by_plane)[1] == ([0, 1, 3, 4] if by_plane else [0, 1, 2, 3, 4])
    check(lib, big, by_plane)
    # a run of one source longer than the pair cap: cut at the cap, the rest is a run of its own
    long_run = [pair(0x1000, 2, 2, rec=0x7000 + i) for i in range(6)] + [pair(0x2000, 2, 2)]
    assert plan(lib, long_run, by_plane)[1] == [0, 4, 7]
    assert ("a run longer than the pair cap" in check(lib, long_run, by_plane)) == by_plane
    # a run that exactly fills a group, behind a pair that it cannot join
    fill = [pair(0x1000, 2, 2)] + [pair(0x2000, 2, 2, rec=0x7000 + i) for i in range(4)] + [pair(0x3000, 2, 2)]
    assert plan(lib, fill, by_plane)[1] == ([0, 1, 5, 6] if by_plane else [0, 4, 6])
    check(lib, fill, by_plane)
    # ... and in tiles: 4 + 6 = 10 fits, one more tile does not
    exact = [pair(0x1000, 4, 4), pair(0x2000, 4, 6), pair(0x3000, 2, 2)]
    assert plan(lib, exact, by_plane)[1] == [0, 2, 3]
    assert check(lib, exact, by_plane) == {"closed by the tile cap"}
    # the order: sources interleaved in the call come together, reconstructions of one source in the call's order
    mixed = [pair(0x2000, 2, 2, rec=1), pair(0x1000, 2, 2, rec=2), pair(0x2000, 2, 2, rec=3), pair(0x1000, 2, 2, rec=4)]
    assert plan(lib, mixed, by_plane)[0] == ([1, 3, 0, 2] if by_plane else [0, 1, 2, 3])


@pytest.mark.parametrize("by_plane", [True, False], ids=["by_plane", "call_order"])
def test_random_calls(lib, by_plane):
    rng = np.random.RandomState(5)
    seen = set()
    sizes = [(2, 2), (2, 4), (4, 4), (3, 6), (6, 6), (8, 8)]             # 1, 2, 4, 6, 9 and 16 tiles
    for trial in range(300):
        n = int(rng.randint(0, 41))
        nsrc = int(rng.randint(1, 7))
        planes = [(0x1000 * (1 + int(rng.randint(0, 4))),) + sizes[int(rng.randint(0, len(sizes) - (trial % 3 > 0)))]
                  for _ in range(nsrc)]
        pairs = []
        for i in range(n):
            src, w, h = planes[int(rng.randint(0, nsrc))]
            pairs.append(pair(src, w, h, rec=0x100000 + i))
        seen |= check(lib, pairs, by_plane)
    want = {"closed by the pair cap", "closed by the tile cap", "alone above the tile cap"}
    assert seen == want | ({"a run longer than the pair cap"} if by_plane else set())
