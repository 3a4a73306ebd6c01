"""CPU: odhip_cfl_refs_partition_host (include/daala_hip.h, "Chroma-from-luma reference planes at a block-size map")
against od_resample_luma_coeffs of every leaf (tests/_cfl_partition_ref.py), bit for bit; and the refusals of both
entry points, answered by host-side checks in front of any HIP call (device pointers are fake addresses, as in
tests/test_partition_leaves_host.py).  The host entry point runs the kernel's own per-group code, so what is pinned
here is the arithmetic of k_cfl_part as well.

  coverage          the case set holds TF leaves, quarter-copy 4x4 leaves, every larger chroma size and a TF group
                    whose ll - hh is odd and negative
  every case        two frames with different maps, dec = 1 and dec = 0; at dec = 0 the plane is the luma plane
  every sample      is written: a poison laid first is gone; guard rows around both buffers stay
  not a quadtree    success, and the guards stay
"""
import ctypes
import subprocess

import numpy as np
import pytest

import _cfl_partition_ref as C

EINVAL = -10
GUARD = 3                       # rows before and after each buffer
LUMA_GUARD = 0x7e7e7e7e
P = ctypes.c_void_p
NAMES = ("odhip_cfl_refs_partition", "odhip_cfl_refs_partition_host")


@pytest.fixture(scope="module")
def hip():
    import daala_amd
    from daala_amd import build
    build.build()
    return daala_amd


def _guarded(shape, fill):
    """(the whole buffer, its inner [h][w] view) with GUARD rows of `fill` before and after."""
    h, w = shape
    buf = np.full((h + 2 * GUARD, w), fill, np.int32)
    return buf, buf[GUARD:GUARD + h]


def _host_call(hip, luma, bmap, dec, extra_cols=0):
    """The raw entry point on guarded buffers: the reference plane, after checking the guards, the luma plane and
    the map."""
    h, w = luma.shape
    lbuf, lview = _guarded((h, w), LUMA_GUARD)
    lview[:] = luma
    rbuf, rview = _guarded((h >> dec, w >> dec), C.POISON)
    mbuf = np.full((bmap.shape[0] + 2, bmap.shape[1] + extra_cols), 9, np.uint8)
    mview = mbuf[1:1 + bmap.shape[0], :bmap.shape[1]]
    mview[:] = bmap
    lcopy, mcopy = lbuf.copy(), mbuf.copy()
    rc = hip.lib().odhip_cfl_refs_partition_host(P(rview.ctypes.data), P(lview.ctypes.data), w, h, dec,
                                                 P(mview.ctypes.data), mbuf.strides[0])
    assert rc == 0
    assert (rbuf[:GUARD] == C.POISON).all() and (rbuf[-GUARD:] == C.POISON).all()
    assert np.array_equal(lbuf, lcopy) and np.array_equal(mbuf, mcopy)
    return rview.copy()


def test_the_case_set_reaches_every_branch():
    stats = C.coverage()
    print(stats)
    assert stats["tf"] >= 50 and stats["copy4"] >= 50
    assert stats[8] >= 1 and stats[16] >= 1 and stats[32] >= 1
    assert stats["odd_negative"] >= 1


@pytest.mark.parametrize("dec", [1, 0])
@pytest.mark.parametrize("index", range(len(C.CASES)), ids=C.CASE_IDS)
def test_host_planes_equal_the_oracle_leaf_by_leaf(hip, index, dec):
    luma, bmaps, want = C.case(index)
    for f in range(2):
        got = _host_call(hip, luma[f], bmaps[f], dec, extra_cols=5 * f)
        assert not (got == C.POISON).any()                          # every sample is written
        assert np.array_equal(got, want[dec][f]), (f, np.argwhere(got != want[dec][f])[:4])
        if dec == 0:
            assert np.array_equal(got, luma[f])
        # the numpy wrapper makes the same call
        assert np.array_equal(hip.cfl_refs_partition_host(luma[f], bmaps[f], dec), got)
    assert not np.array_equal(want[1][0], want[1][1])


def test_the_map_value_not_the_chroma_size_chooses_the_branch(hip):
    """One 8x8 luma area, the same coefficients: map value 1 copies the quarter, map value 0 merges four blocks."""
    luma, _, _ = C.case(0)
    plane = luma[0][:64, :64]
    m1 = np.full((8, 8), 1, np.uint8)
    m0 = np.zeros((8, 8), np.uint8)
    copy = _host_call(hip, plane, m1, 1)
    tf = _host_call(hip, plane, m0, 1)
    quarter = plane.reshape(8, 8, 8, 8)[:, :4, :, :4].reshape(32, 32)
    assert np.array_equal(copy, quarter)
    assert np.array_equal(tf, C.expected(plane, m0, 1)) and not np.array_equal(tf, copy)


@pytest.mark.parametrize("dec", [1, 0])
def test_a_map_that_is_no_quadtree_stays_inside_its_buffers(hip, dec):
    rng = np.random.RandomState(77)
    luma, _, _ = C.case(3)
    for k in range(4):
        m = rng.randint(0, 5 if k < 3 else 256, size=(16, 24)).astype(np.uint8)
        assert not C.R.is_quadtree(m)
        got = _host_call(hip, luma[0], m, dec)                      # asserts success and the guards
        assert not (got == C.POISON).any()


def test_both_builds_export_the_entry_points_and_the_package_the_wrappers(hip):
    from daala_amd import build
    for path in (build.LIB, hip.EXPERIMENTS_LIB):
        out = subprocess.run(["nm", "-D", "--defined-only", path], capture_output=True, text=True, check=True).stdout
        names = {ln.split()[-1] for ln in out.splitlines() if " T " in ln}
        assert set(NAMES) <= names, path
    L = hip.lib()
    # the prototypes come from the header (daala_amd/_abi.py): the frame stride passes as a long
    assert L.odhip_cfl_refs_partition.argtypes[8] is ctypes.c_long and len(L.odhip_cfl_refs_partition.argtypes) == 11
    assert len(L.odhip_cfl_refs_partition_host.argtypes) == 7
    for f in ("cfl_refs_partition", "cfl_refs_partition_host", "keyframe_partition_420"):
        assert callable(getattr(hip, f)), f


# ---- refusals: fake addresses, nothing may be dereferenced or launched --------------------------------

W = H = 128
REF, LUMA, MAP = 0x100000, 0x200000, 0x300000


def _device(L, ref=REF, luma=LUMA, nplanes=2, w=W, h=H, dec=1, bsize=MAP, bstride=None, ppf=2):
    if bstride is None:
        bstride = w // 8
    return L.odhip_cfl_refs_partition(P(ref), P(luma), nplanes, w, h, dec, P(bsize), bstride, 1024, ppf, None)


def _host(L, ref=REF, luma=LUMA, w=W, h=H, dec=1, bsize=MAP, bstride=None):
    if bstride is None:
        bstride = w // 8
    return L.odhip_cfl_refs_partition_host(P(ref), P(luma), w, h, dec, P(bsize), bstride)


@pytest.mark.parametrize("call", [_device, _host], ids=["device", "host"])
def test_entry_points_refuse_bad_arguments_without_gpu(hip, call):
    L = hip.lib()
    for dec in (0, 1):
        assert call(L, w=W - 32, dec=dec) == EINVAL
        assert call(L, h=H - 32, dec=dec) == EINVAL
        assert call(L, w=0, dec=dec) == EINVAL
        assert call(L, h=0, dec=dec) == EINVAL
        assert call(L, w=-64, dec=dec) == EINVAL
        assert call(L, h=-64, dec=dec) == EINVAL
        assert call(L, bstride=W // 8 - 1, dec=dec) == EINVAL
        assert call(L, ref=0, dec=dec) == EINVAL
        assert call(L, luma=0, dec=dec) == EINVAL
        assert call(L, bsize=0, dec=dec) == EINVAL
        assert call(L, ref=LUMA, dec=dec) == EINVAL                 # d_ref == d_luma
    assert call(L, dec=2) == EINVAL
    assert call(L, dec=-1) == EINVAL


def test_the_device_entry_point_refuses_its_own_arguments_without_gpu(hip):
    L = hip.lib()
    assert _device(L, nplanes=0) == EINVAL
    assert _device(L, nplanes=-1) == EINVAL
    assert _device(L, ppf=0) == EINVAL
    assert _device(L, ppf=-2) == EINVAL
    for off in (4, 8, 12):
        assert _device(L, ref=REF + off) == EINVAL
        assert _device(L, luma=LUMA + off) == EINVAL
