"""SSIM without a GPU: the restatement (tests/_ssim_ref.py) against what the reference's dump_ssim printed
(tests/golden/ssim.npz, tools/make_golden_ssim.py), and the host-only entry points against the restatement.

- every printed line of every golden clip, dB and raw (-r), is reproduced as a string;
- odhip_ssim_taps equals the restatement's table entry for entry (heights 16 .. 2160, capped and uncapped), and
  refuses bad arguments;
- odhip_ssim_weight equals the restatement's sum of the weight moment;
- the C ABI carries the new symbols and the Python mirror the new flag."""
import ctypes
import os
import sys

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))

import _ssim_ref as S  # noqa: E402

HEIGHTS = (16, 64, 256, 544, 1088, 2160)


@pytest.fixture(scope="module")
def D():
    import daala_amd
    return daala_amd


@pytest.mark.parametrize("idx", range(len(S.CASES)), ids=[c[0] for c in S.CASES])
def test_restatement_prints_the_tool_lines(idx):
    g = np.load(os.path.join(ROOT, "tests", "golden", "ssim.npz"))
    case = S.CASES[idx]
    assert str(g["names"][idx]) == case[0]
    assert S.restated_lines(case) == str(g["ssim"][idx]).splitlines()
    assert S.restated_lines(case, raw=True) == str(g["ssim_raw"][idx]).splitlines()


def test_radii_of_the_cases():
    """The shapes the golden clips were chosen for."""
    r = lambda w, h: tuple(len(t) // 2 for t in S.plane_taps(w, h))
    assert r(24, 544) == (9, 9) and r(12, 272) == (4, 4)
    assert r(8, 544) == (7, 7) and r(4, 272) == (3, 3)
    assert r(40, 256) == (4, 4)
    assert r(1920, 1080) == (16, 16) and r(96, 64) == (1, 1)
    assert max(r(c[2], c[3])[0] for c in S.CASES[:7]) <= 1


@pytest.mark.parametrize("h", HEIGHTS)
def test_taps(D, h):
    for par in (1.0, 4 / 3):
        sigma = h * (1.5 / 256) / par
        full = S.taps(sigma, 1 << 20)
        for max_len in (1 << 20, len(full) // 2 + 1, max(1, len(full) // 2), 2, 1):
            want = S.taps(sigma, max_len)
            assert len(want) == 2 * min(len(full) // 2, max_len - 1) + 1
            assert D.ssim_taps(sigma, max_len) == want, (h, par, max_len)
            assert sum(want) == 256


def test_taps_errors(D):
    L = D.lib()
    buf = (ctypes.c_uint32 * 64)()
    d = ctypes.c_double
    assert L.odhip_ssim_taps(d(0.0), 100, buf, 64) == -10
    assert L.odhip_ssim_taps(d(-1.0), 100, buf, 64) == -10
    assert L.odhip_ssim_taps(d(float("nan")), 100, buf, 64) == -10
    assert L.odhip_ssim_taps(d(3.1875), 0, buf, 64) == -10
    assert L.odhip_ssim_taps(d(3.1875), 100, None, 64) == -10
    assert L.odhip_ssim_taps(d(3.1875), 100, buf, 18) == -10           # 19 taps
    assert L.odhip_ssim_taps(d(3.1875), 100, buf, 19) == 19
    assert list(buf[:19]) == S.taps(3.1875, 100)


def test_weight(D):
    for w, h, par in ((96, 64, 1.0), (24, 544, 1.0), (12, 272, 1.0), (8, 544, 1.0), (4, 272, 1.0), (40, 256, 1.0),
                      (77, 53, 4 / 3), (77, 53, 1.0), (24, 544, 4 / 3), (24, 544, 0.5), (1920, 1080, 1.0), (1, 1, 1.0),
                      (300, 2160, 1.0)):
        assert D.ssim_weight(w, h, par) == S.weight(w, h, par), (w, h, par)
    # the weight really is the sum of the weight moment of every sample
    assert S.weight(24, 544) == int(S.moments(np.zeros((544, 24)), np.zeros((544, 24)))[5].sum())
    L = D.lib()
    wt = ctypes.c_int64()
    d = ctypes.c_double
    assert L.odhip_ssim_weight(0, 10, d(1.0), ctypes.byref(wt)) == -10
    assert L.odhip_ssim_weight(10, 10, d(0.0), ctypes.byref(wt)) == -10
    assert L.odhip_ssim_weight(10, 10, d(1.0), None) == -10


def test_abi_and_mirror(D):
    L = D.lib()
    for name in ("odhip_ssim_taps", "odhip_ssim_weight", "odhip_ssim_planes", "odhip_ssim_terms", "odhip_ssim_prepare",
                 "odhip_ssim_tile_count", "odhip_pipe_set_metrics2", "odhip_pipe_metrics_take2", "odhip_pipe_metrics_ssim_weights"):
        assert hasattr(L, name), name
    header = open(os.path.join(ROOT, "include", "daala_hip.h")).read()
    assert "#define ODHIP_METRIC_SSIM (1 << 2)" in header and "#define ODHIP_SSIM_MAX_RADIUS 64" in header
    assert D.METRIC_SSIM == 4 and D.SSIM_MAX_RADIUS == 64
    # the tool's two scores
    assert D.ssim_score(3.0, 4.0, raw=True) == 0.75
    assert float(D.ssim_score(3.0, 4.0)) == S.score(3.0, 4.0)
