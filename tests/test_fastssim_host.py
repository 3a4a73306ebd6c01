"""FastSSIM without a GPU: the restatement (tests/_fastssim_ref.py) against what the reference's dump_fastssim printed
(tests/golden/fastssim.npz, tools/make_golden_fastssim.py), and the host-only entry points against the restatement.

- every printed line of every golden clip, dB and raw (-c and -c -r, chroma planes included), is reproduced as a
  string, and every plane's calc_ssim return value bit for bit;
- the literal port of the tool's sliding loops equals the 8 x 8 table on random gradients and on impulses at corners,
  edges and in the interior, bit for bit;
- the predicate for "the tool's reads stay inside the level" rejects 1920 x 1080, accepts 1920 x 1088, and holds for
  every plane of every golden clip;
- odhip_fastssim_level_size, odhip_fastssim_tool_exact and odhip_fastssim_score equal the restatement;
- sizes below 16 or above 65535, other depths and NULL arrays are refused before any device work;
- the C ABI carries the new symbols and the Python mirror the new flag."""
import ctypes
import math
import os
import sys

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))

import _fastssim_ref as S  # noqa: E402
import _metrics_ref as M  # noqa: E402

SIZES = ((16, 16), (17, 31), (33, 31), (70, 50), (130, 66), (31, 47), (1920, 1080), (1920, 1088), (65535, 16),
         (16, 65535))


@pytest.fixture(scope="module")
def D():
    import daala_amd
    return daala_amd


@pytest.mark.parametrize("idx", range(len(S.CASES)), ids=[c[0] for c in S.CASES])
def test_restatement_prints_the_tool_lines(idx):
    g = np.load(os.path.join(ROOT, "tests", "golden", "fastssim.npz"))
    case = S.CASES[idx]
    assert str(g["names"][idx]) == case[0]
    values = S.case_values(case)
    assert S.tool_lines(values, case[4]) == str(g["fastssim"][idx]).splitlines()
    assert S.tool_lines(values, case[4], raw=True) == str(g["fastssim_raw"][idx]).splitlines()
    want = g["bits_" + case[0]]
    got = np.array([[S.bits(v) for v in f] for f in values], np.uint64)
    assert want.shape == got.shape and (want == got).all()


def test_golden_cases_stay_inside():
    for case in S.CASES:
        src, _ = M.make_case(case)
        for p in src[0]:
            assert S.tool_reads_inside(p.shape[1], p.shape[0]), (case[0], p.shape)


def test_predicate():
    assert not S.tool_reads_inside(1920, 1080)          # 540 -> 270 -> 135 rows
    assert S.tool_reads_inside(1920, 1088)
    assert S.tool_reads_inside(16, 16) and S.tool_reads_inside(31, 47) and not S.tool_reads_inside(33, 31)
    for w, h in SIZES:
        assert S.tool_reads_inside(w, h) == (((w + 1) // 2) % 8 == 0 and ((h + 1) // 2) % 8 == 0)


def _same(a, b):
    return all((x.view(np.int64) == y.view(np.int64)).all() for x, y in zip(a, b))


@pytest.mark.parametrize("h,w", [(1, 1), (2, 2), (3, 9), (9, 3), (8, 8), (12, 17), (20, 11)])
def test_loops_are_the_table(h, w):
    rng = np.random.RandomState(100 * h + w)
    top = 5 * 4095 * 256                                # the largest gradient: 12 bits, level 3
    for k in range(3):
        gx = rng.randint(0, top + 1, size=(h, w)).astype(np.int64)
        gy = rng.randint(0, top + 1, size=(h, w)).astype(np.int64)
        if k == 2:
            gx[:], gy[:] = top, top
        gx[-1, :] = gx[:, -1] = gy[-1, :] = gy[:, -1] = 0       # outside the gradient domain
        assert _same(S.loops_window(gx, gy), S.table_window(gx, gy))


def test_impulses():
    h, w = 14, 15
    seen = np.zeros((8, 8), np.int64)
    for y, x in ((0, 0), (0, w - 2), (h - 2, 0), (h - 2, w - 2), (0, 7), (6, 0), (h - 2, 5), (5, w - 2), (6, 7)):
        gx = np.zeros((h, w), np.int64)
        gx[y, x] = 1
        gy = 3 * gx
        got = S.loops_window(gx, gy)
        assert _same(got, S.table_window(gx, gy))
        # the impulse's footprint is the table, cut by the level only
        want = np.zeros((h + 8, w + 8), np.int64)
        want[y:y + 8, x + 1:x + 9] = S.TABLE            # rows y - 4 .., columns x - 3 .. of a plane offset by 4
        assert (got[0] == want[4:4 + h, 4:4 + w]).all() and (got[1] == 9 * got[0]).all() and (got[2] == 3 * got[0]).all()
        if (y, x) == (6, 7):
            seen = got[0][y - 4:y + 4, x - 3:x + 5].astype(np.int64)
    assert (seen == S.TABLE).all() and seen.sum() == 104


def test_wrap_and_checkerboard_cases_are_not_void():
    assert S.wrapped(*S.wrap_pair()) > 0
    src, rec = S.checkerboard(96, 80, 12)
    assert int(S.gradient(S.pyramid(src)[3]).max()) == 5 * 4095 * 256     # the bound of the exactness argument
    assert int(S.window(S.gradient(S.pyramid(src)[3]) ** 2).max()) < 1 << 52


def test_level_size_and_tool_exact(D):
    L = D.lib()
    wl, hl = ctypes.c_int(), ctypes.c_int()
    for w, h in SIZES:
        for l in range(4):
            assert L.odhip_fastssim_level_size(w, h, l, ctypes.byref(wl), ctypes.byref(hl)) == 0
            assert (wl.value, hl.value) == S.level_size(w, h, l), (w, h, l)
        assert L.odhip_fastssim_tool_exact(w, h) == int(S.tool_reads_inside(w, h)), (w, h)
    assert L.odhip_fastssim_level_size(64, 64, 4, ctypes.byref(wl), ctypes.byref(hl)) == -10
    assert L.odhip_fastssim_level_size(64, 64, -1, ctypes.byref(wl), ctypes.byref(hl)) == -10
    assert L.odhip_fastssim_level_size(15, 64, 0, ctypes.byref(wl), ctypes.byref(hl)) == -10
    assert L.odhip_fastssim_level_size(64, 65536, 0, ctypes.byref(wl), ctypes.byref(hl)) == -10
    assert L.odhip_fastssim_level_size(64, 64, 0, None, ctypes.byref(hl)) == -10
    for w, h in ((15, 64), (64, 15), (65536, 64), (0, 0)):
        assert L.odhip_fastssim_tool_exact(w, h) == -10


def test_score(D):
    L = D.lib()
    rng = np.random.RandomState(5)
    for w, h in ((77, 53), (16, 16), (1920, 1080)):
        n = np.array([a * b for a, b in (S.level_size(w, h, l) for l in range(4))], np.float64)
        for _ in range(4):
            sums = n * (0.8 + 0.2 * rng.rand(4))
            assert D.fastssim_score(sums, w, h, raw=True) == S.score(sums, w, h)
            assert D.fastssim_score(sums, w, h) == pytest.approx(S.convert(S.score(sums, w, h), 1), rel=1e-14)
        assert D.fastssim_score(n, w, h, raw=True) == 1.0           # identical planes
        neg = n * 0.9
        neg[2] = -neg[2]
        assert math.isnan(D.fastssim_score(neg, w, h, raw=True)) and math.isnan(S.score(neg, w, h))
    many = D.fastssim_score(np.stack([n, n * 0.5]), 1920, 1080, raw=True)
    assert many.shape == (2,) and many[0] == 1.0 and many[1] == S.score(n * 0.5, 1920, 1080)
    out = ctypes.c_double()
    p = n.ctypes.data_as(ctypes.c_void_p)
    assert L.odhip_fastssim_score(None, 64, 64, ctypes.byref(out)) == -10
    assert L.odhip_fastssim_score(p, 64, 64, None) == -10
    assert L.odhip_fastssim_score(p, 15, 64, ctypes.byref(out)) == -10
    assert L.odhip_fastssim_score(p, 64, 65536, ctypes.byref(out)) == -10


def test_refusals_before_any_device_work(D):
    """Arguments are checked before a context or a device is looked for: these answer without a GPU."""
    from daala_amd.api import _MetricsPair
    L = D.lib()
    buf = np.zeros(64 * 64, np.uint8)
    out = np.zeros(8, np.float64)
    po = out.ctypes.data_as(ctypes.c_void_p)

    def pair(w, h, depth=8, fmt=0):
        return _MetricsPair(buf.ctypes.data, buf.ctypes.data, fmt, fmt, 64, 64, w, h, depth, 0)

    for bad in (pair(15, 64), pair(64, 15), pair(64, 64, 9), pair(64, 64, 10, 0), pair(65536, 64)):
        arr = (_MetricsPair * 2)(pair(64, 64), bad)
        assert L.odhip_fastssim_planes(arr, 2, po, None) == -10
        assert L.odhip_fastssim_terms(ctypes.byref(bad), 0, po, None) == -10
    arr = (_MetricsPair * 1)(pair(64, 64))
    assert L.odhip_fastssim_planes(arr, -1, po, None) == -10
    assert L.odhip_fastssim_planes(None, 1, po, None) == -10
    assert L.odhip_fastssim_planes(arr, 1, None, None) == -10
    assert L.odhip_fastssim_terms(ctypes.byref(arr[0]), 4, po, None) == -10
    assert L.odhip_fastssim_terms(ctypes.byref(arr[0]), -1, po, None) == -10
    assert L.odhip_fastssim_terms(ctypes.byref(arr[0]), 0, None, None) == -10
    assert L.odhip_fastssim_terms(None, 0, po, None) == -10
    assert L.odhip_fastssim_planes(arr, 0, po, None) == 0                     # nothing to do
    assert not out.any()
    assert L.odhip_fastssim_prepare(15, 64, 1) == -10 and L.odhip_fastssim_prepare(64, 64, 0) == -10


def test_abi_and_mirror(D):
    L = D.lib()
    for name in ("odhip_fastssim_level_size", "odhip_fastssim_tool_exact", "odhip_fastssim_planes",
                 "odhip_fastssim_prepare", "odhip_fastssim_score", "odhip_fastssim_terms", "odhip_pipe_set_metrics4",
                 "odhip_pipe_metrics_take4"):
        assert hasattr(L, name), name
    header = open(os.path.join(ROOT, "include", "daala_hip.h")).read()
    assert "#define ODHIP_METRIC_FASTSSIM (1 << 4)" in header and "#define ODHIP_FASTSSIM_LEVELS 4" in header
    assert D.METRIC_FASTSSIM == 16 and D.FASTSSIM_LEVELS == S.LEVELS == 4
