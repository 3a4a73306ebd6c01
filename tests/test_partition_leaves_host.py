"""CPU: odhip_partition_leaves_host (include/daala_hip.h, "the PVQ band stages on the leaves of a block-size map") -
the lists and counts equal the encoder's top-down walk, restated here with tests/_partition_ref.py::_walk; and every
argument outside the contract of the four odhip_partition_* entry points is answered ODHIP_EINVAL by host-side checks
in front of any HIP call (there is no GPU here; device pointers are fake addresses, as in tests/test_abi_symbols.py).

  the rule          bs = max(map at the node's top-left entry, dec); bs == bsi is a leaf of size bsi - dec
  the order         strictly ascending block index by*(w/N) + bx, whatever order the walk meets the leaves in
  dec = 1           map values 0 and 1 side by side are both one 4x4 chroma leaf per 8x8 luma area
  batch geometry    plane p reads the map of frame p / planes_per_frame; rows and frames may lie wider apart
  not a quadtree    unspecified lists, but no index twice and no count above (w/N)*(h/N)
"""
import ctypes
import subprocess

import numpy as np
import pytest

import _partition_ref as R

EINVAL = -10
NB = 5
GAP = 9                                   # what lies between map rows and frames: no block size
NAMES = ("odhip_partition_leaves_host", "odhip_partition_leaves", "odhip_partition_gather", "odhip_partition_scatter")


@pytest.fixture(scope="module")
def hip():
    import daala_amd
    from daala_amd import build
    build.build()
    return daala_amd


def _walk_lists(bmap, dec, h, w):
    """{s: ascending block indices} of one plane by the reference's recursion."""
    found = {s: [] for s in range(NB - dec)}

    def leaf(y, x, lv):
        n = 4 << lv
        found[lv].append((y // n) * (w // n) + x // n)

    nothing = lambda *_: None  # noqa: E731
    R._walk(bmap, dec, w, h, w << dec, h << dec, leaf, nothing, nothing)
    return {s: np.array(sorted(v), np.uint32) for s, v in found.items()}


def _assert_leaves(got, maps, ppf, dec, h, w):
    nplanes = len(maps) * ppf
    assert got.counts.shape == (NB, nplanes) and got.counts.dtype == np.int32
    covered = np.zeros(nplanes, np.int64)
    for p in range(nplanes):
        want = _walk_lists(maps[p // ppf], dec, h, w)
        for s in range(NB):
            ws = want.get(s, np.zeros(0, np.uint32))
            assert got.counts[s, p] == len(ws), (s, p)
            if s < NB - dec:
                assert np.array_equal(got.list(s)[p, :len(ws)], ws), (s, p)
                covered[p] += len(ws) * (4 << s) ** 2
    assert (covered == h * w).all()                       # the leaves tile every plane


def _frames(maps, extra_cols=0, extra_rows=0):
    """The maps as one [frames, rows, cols] view of a GAP-filled buffer with wider rows and frames."""
    rows, cols = maps[0].shape
    buf = np.full((len(maps), rows + extra_rows, cols + extra_cols), GAP, np.uint8)
    view = buf[:, :rows, :cols]
    for f, m in enumerate(maps):
        view[f] = m
    return view


def _size(nsbx, nsby, dec):
    return (nsby * 64) >> dec, (nsbx * 64) >> dec


@pytest.mark.parametrize("dec", [0, 1])
@pytest.mark.parametrize("level", range(5))
def test_uniform_levels(hip, dec, level):
    h, w = _size(3, 2, dec)
    m = R.uniform(level, 3, 2)
    got = hip.partition_leaves_host(m, 1, h, w, dec)
    _assert_leaves(got, [m], 1, dec, h, w)
    s = max(level, dec) - dec
    assert got.sizes() == [s] and got.counts[s, 0] == got.cap(s)
    assert np.array_equal(got.list(s)[0], np.arange(got.cap(s)))
    assert got.dense_rows(s) == h and all(got.dense_rows(t) == 0 for t in range(NB - dec) if t != s)


@pytest.mark.parametrize("dec", [0, 1])
def test_map_families(hip, dec):
    rng = np.random.RandomState(31 + dec)
    h, w = _size(3, 2, dec)
    lone = R.uniform(4, 3, 2)
    lone[8:16, 16:24] = R.deep_corner(3)                  # the only superblock that is not one 64x64 block
    maps = [R.random_map(rng, 3, 2, 0.5), R.random_map(rng, 3, 2, 0.8), R.corners(3, 2), R.extremes(3, 2), lone,
            R.units01(3, 2)]
    assert all(R.is_quadtree(m) for m in maps)
    got = hip.partition_leaves_host(np.stack(maps), len(maps), h, w, dec)
    _assert_leaves(got, maps, 1, dec, h, w)
    # a deep corner holds three blocks of every size above the smallest, and one more 8x8 quartered
    p = 4
    if dec == 0:
        assert list(got.counts[:, p]) == [4, 3, 3, 3, 5]
    else:
        assert list(got.counts[:, p]) == [4, 3, 3, 5, 0]    # 4x4 and 8x8 luma both code 4x4 chroma


def test_values_0_and_1_side_by_side_at_dec_1(hip):
    h, w = _size(2, 1, 1)
    m = R.units01(2, 1)
    got = hip.partition_leaves_host(m, 1, h, w, 1)
    _assert_leaves(got, [m], 1, 1, h, w)
    assert got.sizes() == [0] and got.counts[0, 0] == (h // 4) * (w // 4)
    # the same map at dec = 0: a 4x4 quad and an 8x8 block alternate
    got = hip.partition_leaves_host(m, 1, 2 * h, 2 * w, 0)
    _assert_leaves(got, [m], 1, 0, 2 * h, 2 * w)
    assert list(got.counts[:, 0]) == [4 * 64, 64, 0, 0, 0]


@pytest.mark.parametrize("dec,ppf", [(0, 1), (1, 2), (0, 2)])
def test_two_frames_with_their_own_maps_and_wide_strides(hip, dec, ppf):
    rng = np.random.RandomState(7 + ppf)
    h, w = _size(2, 2, dec)
    maps = [R.random_map(rng, 2, 2, 0.6), R.corners(2, 2)]
    compact = hip.partition_leaves_host(np.stack(maps), 2 * ppf, h, w, dec, planes_per_frame=ppf)
    _assert_leaves(compact, maps, ppf, dec, h, w)
    view = _frames(maps, extra_cols=5, extra_rows=3)
    assert view.strides == (19 * 21, 21, 1)
    wide = hip.partition_leaves_host(view, 2 * ppf, h, w, dec, planes_per_frame=ppf)
    assert np.array_equal(wide.counts, compact.counts) and np.array_equal(wide.lists, compact.lists)
    # the planes of one frame share its lists; the two frames differ
    if ppf == 2:
        for s in compact.sizes():
            assert np.array_equal(compact.list(s)[0], compact.list(s)[1])
    assert not np.array_equal(compact.counts[:, 0], compact.counts[:, ppf])


@pytest.mark.parametrize("dec", [0, 1])
def test_a_map_that_is_no_quadtree_repeats_no_index(hip, dec):
    rng = np.random.RandomState(99)
    h, w = _size(2, 2, dec)
    for k in range(4):
        m = rng.randint(0, 5 if k < 3 else 256, size=(16, 16)).astype(np.uint8)
        assert not R.is_quadtree(m)
        got = hip.partition_leaves_host(m, 1, h, w, dec)
        for s in range(NB - dec):
            c = int(got.counts[s, 0])
            assert 0 <= c <= got.cap(s)
            ids = got.list(s)[0, :c]
            assert (np.diff(ids.astype(np.int64)) > 0).all() and (c == 0 or ids[-1] < got.cap(s))
        assert (got.counts[NB - dec:] == 0).all()


def test_both_builds_export_the_entry_points_and_the_package_the_wrappers(hip):
    from daala_amd import build
    for path in (build.LIB, hip.EXPERIMENTS_LIB):
        out = subprocess.run(["nm", "-D", "--defined-only", path], capture_output=True, text=True, check=True).stdout
        names = {ln.split()[-1] for ln in out.splitlines() if " T " in ln}
        assert set(NAMES) <= names, path
    for f in ("partition_leaves", "partition_leaves_host", "partition_gather", "partition_scatter", "pvq_partition_noref",
              "pvq_partition_ref", "inverse_partition"):
        assert callable(getattr(hip, f)), f


# ---- refusals: fake addresses, nothing may be dereferenced or launched --------------------------------

W = H = 128
LISTS, COUNT, MAP, DENSE, COEF = 0x100000, 0x200000, 0x300000, 0x400000, 0x500000
P = ctypes.c_void_p


def _leaves(L, device, lists=LISTS, count=COUNT, nplanes=2, w=W, h=H, dec=0, bsize=MAP, bstride=None, frame_stride=1024,
            ppf=1):
    if bstride is None:
        bstride = 8 * (w // (64 >> (dec & 1)))
    args = (P(lists), P(count), nplanes, w, h, dec, P(bsize), bstride, ctypes.c_long(frame_stride), ppf)
    return L.odhip_partition_leaves(*args, None) if device else L.odhip_partition_leaves_host(*args)


@pytest.mark.parametrize("device", [False, True], ids=["host", "device"])
def test_leaves_refuse_bad_arguments_without_gpu(hip, device):
    L = hip.lib()
    call = lambda **kw: _leaves(L, device, **kw)  # noqa: E731
    assert call(lists=0) == EINVAL
    assert call(count=0) == EINVAL
    assert call(bsize=0) == EINVAL
    assert call(ppf=0) == EINVAL
    assert call(ppf=-1) == EINVAL
    assert call(nplanes=0) == EINVAL
    assert call(dec=2) == EINVAL
    assert call(dec=-1) == EINVAL
    assert call(w=W - 32) == EINVAL
    assert call(h=H - 32) == EINVAL
    assert call(w=W - 16, dec=1, bstride=64) == EINVAL
    assert call(h=H - 4, dec=1) == EINVAL
    assert call(w=0) == EINVAL
    assert call(h=-64) == EINVAL
    assert call(bstride=8 * (W // 64) - 1) == EINVAL
    assert call(dec=1, bstride=8 * (W // 32) - 1) == EINVAL


@pytest.mark.parametrize("name", NAMES[2:])
def test_copies_refuse_bad_arguments_without_gpu(hip, name):
    L = hip.lib()
    fn = getattr(L, name)

    def call(dst=DENSE, src=COEF, s=1, lst=LISTS, count=(3, 0), nplanes=2, w=W, h=H, dec=0):
        c = (ctypes.c_int32 * max(len(count), 1))(*count) if count is not None else None
        return fn(P(dst), P(src), s, P(lst), c, nplanes, w, h, dec, None)

    assert call(dst=0) == EINVAL
    assert call(src=0) == EINVAL
    assert call(lst=0) == EINVAL
    assert call(count=None) == EINVAL
    assert call(nplanes=0) == EINVAL
    assert call(dec=2) == EINVAL
    assert call(w=W - 32) == EINVAL
    assert call(h=H - 32) == EINVAL
    assert call(w=W - 16, dec=1) == EINVAL
    assert call(s=-1) == EINVAL
    assert call(s=5) == EINVAL
    assert call(s=4, dec=1) == EINVAL                    # 4:2:0 chroma stops at 32x32
    assert call(dst=DENSE + 4) == EINVAL
    assert call(dst=DENSE + 8) == EINVAL
    assert call(src=COEF + 4) == EINVAL
    assert call(count=(-1, 0)) == EINVAL
    assert call(count=(0, (W // 8) * (H // 8) + 1)) == EINVAL    # above the capacity of 8x8 blocks
    assert call(s=4, count=(5, 0)) == EINVAL                     # 2 x 2 blocks of 64x64
    # no leaf of the size anywhere: there is no dense set, and nothing to launch
    assert call(count=(0, 0)) == 0
