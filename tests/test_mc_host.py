"""CPU: the numpy motion compensation of tests/_mc_ref.py is pinned to the reference - to every recorded output of
od_state_mc_predict in tests/golden/mc.npz and, where the compiled reference is present, to its leaf functions on
fresh random inputs - and the C ABI of the motion compensation is what the ctypes mirror expects.  All exact."""
import ctypes
import os

import numpy as np
import pytest

import _mc_ref as R
from _libs import GOLDEN, P, ref

CASES = R.load_cases(os.path.join(GOLDEN, "mc.npz"))


def test_fixture_coverage():
    sizes, pairs, kinds = set(), set(), set()
    for c in CASES:
        kinds.add((c["c444"], c["fpr"]))
        for vx, vy, lg, oc, s in R.leaves(c["grid"]["valid"]):
            sizes.add(lg)
            pairs.add((oc, s) if lg < 3 else (0, 3))
    assert sizes == {0, 1, 2, 3}
    assert pairs == {(oc, s) for oc in range(4) for s in range(4)}
    assert {k[0] for k in kinds} == {0, 1} and {k[1] for k in kinds} == {0, 1}
    assert any(c["name"].startswith("420_8bit_176x120") and (c["w"], c["h"]) == (192, 128) for c in CASES)


@pytest.mark.parametrize("case", CASES, ids=[c["name"] for c in CASES])
def test_numpy_equals_recorded_prediction(case):
    for pli in range(3):
        dec = 0 if (pli == 0 or case["c444"]) else 1
        assert R.grid_in_range(case["grid"], dec)
        got = R.mc_predict_plane([case["refs"][0][pli], case["refs"][1][pli]], case["grid"], dec, case["fpr"])
        assert np.array_equal(got, case["pred"][pli]), (case["name"], pli)


def test_vertex_points_stay_inside_the_grid():
    for c in CASES:
        nv, nh = c["grid"].shape[0] - 1, c["grid"].shape[1] - 1
        for vx, vy, lg, oc, s in R.leaves(c["grid"]["valid"]):
            for k in range(4):
                dx, dy = R.vertex(oc, s, k)
                assert 0 <= vx + (dx << lg) <= nh and 0 <= vy + (dy << lg) <= nv


needs_ref = pytest.mark.skipif(ref() is None, reason="oracle/_ref/libdaalaref.so not built")


@needs_ref
@pytest.mark.parametrize("fpr", [0, 1])
def test_numpy_equals_reference_subpel_predictor(fpr):
    L = ref()
    fn = L.od_mc_predict1fmv16_c if fpr else L.od_mc_predict1fmv8_c
    rng = np.random.RandomState(5 + fpr)
    dt = np.int16 if fpr else np.uint8
    for trial in range(200):
        lb = rng.randint(2, 7)
        n = 1 << lb
        # extremes now and then: the clamps and the int16 first pass of the 8-bit variant
        hi = 4096 if fpr else 256
        src = rng.randint(0, hi, size=(n + 16, n + 16))
        if trial % 4 == 0:
            src = np.where(rng.rand(*src.shape) < 0.5, 0, hi - 1)
        src = np.ascontiguousarray(src.astype(dt))
        mvx, mvy = int(rng.randint(-40, 41)), int(rng.randint(-40, 41))
        if not (mvx & 7 or mvy & 7):
            mvx += 1          # the full-pel branch goes through the state: sub-pel vectors only
        want = np.zeros((n, n), dt)
        origin = src.ctypes.data + (8*src.shape[1] + 8)*src.itemsize
        fn(None, P(want), ctypes.c_void_p(origin), src.shape[1]*src.itemsize, mvx, mvy, lb, lb)
        got = R.predict1(src, 8, 8, mvx, mvy, n, fpr)
        assert np.array_equal(got, want), (trial, lb, mvx, mvy)


@needs_ref
@pytest.mark.parametrize("fpr", [0, 1])
def test_numpy_equals_reference_blends(fpr):
    L = ref()
    full = L.od_mc_blend_full16_c if fpr else L.od_mc_blend_full8_c
    split = L.od_mc_blend_full_split16_c if fpr else L.od_mc_blend_full_split8_c
    rng = np.random.RandomState(9 + fpr)
    dt = np.int16 if fpr else np.uint8
    for trial in range(120):
        lb = rng.randint(2, 7)
        n = 1 << lb
        pred = [np.ascontiguousarray(rng.randint(0, 4096 if fpr else 256, size=(n, n)).astype(dt)) for _ in range(4)]
        if trial % 3 == 0:
            pred[2] = pred[0]
        ptrs = (ctypes.c_void_p*4)(*[p.ctypes.data for p in pred])
        want = np.zeros((n, n), dt)
        full(P(want), n*want.itemsize, ptrs, lb, lb)
        assert np.array_equal(R.blend(pred, 0, 3, lb).astype(dt), want), (trial, lb)
        if lb < 6:
            for oc in range(4):
                for s in range(3):
                    split(P(want), n*want.itemsize, ptrs, oc, s, lb, lb)
                    assert np.array_equal(R.blend(pred, oc, s, lb).astype(dt), want), (trial, lb, oc, s)


def test_abi_of_the_motion_compensation():
    import daala_amd
    from daala_amd import api, build
    build.build()
    L = daala_amd.lib()
    for name in ("odhip_mc_predict_planes", "odhip_mc_check_grid", "odhip_mc_leaves", "odhip_mc_sizeof"):
        assert hasattr(L, name), name
    assert L.odhip_mc_sizeof(0) == ctypes.sizeof(api._MvPoint) == api.MV_POINT.itemsize == R.MV_POINT.itemsize == 12
    assert L.odhip_mc_sizeof(1) == ctypes.sizeof(api._McJob)
    assert api.MV_POINT == R.MV_POINT


def test_grid_check_on_the_host():
    """odhip_mc_check_grid never touches the device: the fixtures' grids pass, a vector that takes a window out of
    the border is ODHIP_ERANGE, a slot beyond nrefs ODHIP_EINVAL - in step with the numpy rule."""
    from daala_amd import api, build
    build.build()
    rng = np.random.RandomState(3)
    for c in CASES:
        decs = (0,) if c["c444"] else (0, 1)
        for dec in decs:
            assert api.mc_check_grid(c["grid"], c["w"], c["h"], dec, 2) == 0
        if c["grid"]["ref"].max() > 0:
            assert api.mc_check_grid(c["grid"], c["w"], c["h"], 0, 1) == -10
        for _ in range(20):
            g = c["grid"].copy()
            y, x = rng.randint(0, g.shape[0]), rng.randint(0, g.shape[1])
            g["mvx"][y, x] = int(rng.randint(-80*8, 80*8))
            g["mvy"][y, x] = int(rng.randint(-80*8, 80*8))
            for dec in decs:
                want = 0 if R.grid_in_range(g, dec) else api.ERANGE
                assert api.mc_check_grid(g, c["w"], c["h"], dec, 2) == want
    g = CASES[0]["grid"].copy()
    g["mvx"][0, 0] = -66*8
    assert api.mc_check_grid(g, CASES[0]["w"], CASES[0]["h"], 0, 2) == api.ERANGE
    # a coded size that is no multiple of 64
    assert api.lib().odhip_mc_check_grid(P(g), 100, 64, 1, 0, 2) == -10
