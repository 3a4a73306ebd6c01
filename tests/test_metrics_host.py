"""CPU: the restatement of PSNR and PSNR-HVS-M (tests/_metrics_ref.py) reproduces every line the reference's
dump_psnr and dump_psnrhvs printed for the seeded clip pairs of tests/golden/metrics.npz - PSNR as the identical
%-7G string, PSNR-HVS-M as the identical %-8G string with the tool's running float sum - and the Python mirror of
the metrics section of include/daala_hip.h matches the header."""
import ctypes
import os
import re
import sys

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))


def _golden():
    return np.load(os.path.join(ROOT, "tests", "golden", "metrics.npz"))


@pytest.mark.parametrize("index", range(7))
def test_restatement_reproduces_the_tools(index):
    import _metrics_ref as M
    g = _golden()
    case = M.CASES[index]
    assert str(g["names"][index]) == case[0]
    psnr, hvs = M.restated_lines(case)
    assert psnr == str(g["psnr"][index]).splitlines()
    assert hvs == str(g["psnrhvs"][index]).splitlines()


def test_golden_covers_the_formats():
    import _metrics_ref as M
    assert len(M.CASES) == len(_golden()["names"])
    assert {c[4] for c in M.CASES} == {False, True}                 # 4:2:0 and 4:4:4
    assert {c[5] for c in M.CASES} == {8, 10}
    assert any(c[2] % 2 for c in M.CASES) and {c[1] for c in M.CASES} == {"natural", "texture", "noise"}


def test_python_mirror_matches_the_header():
    from daala_amd import _abi, api
    hdr = open(os.path.join(ROOT, "include", "daala_hip.h")).read()
    consts = dict((k, int(v)) for k, v in re.findall(r"#define (ODHIP_(?:METRIC|SAMPLE|CSF)_[A-Z0-9_]+) (\d+)", hdr))
    assert consts == {"ODHIP_METRIC_SSE": api.METRIC_SSE, "ODHIP_METRIC_PSNRHVS": api.METRIC_PSNRHVS,
                      "ODHIP_SAMPLE_U8": api.SAMPLE_U8, "ODHIP_SAMPLE_U16": api.SAMPLE_U16,
                      "ODHIP_SAMPLE_I16_12": api.SAMPLE_I16_12, "ODHIP_CSF_Y": api.CSF_Y, "ODHIP_CSF_CB": api.CSF_CB,
                      "ODHIP_CSF_CR": api.CSF_CR}
    # the classes are the header's own structs (tests/test_abi_structs.py checks every layout against the compiler)
    structs = _abi.structs()
    assert api._MetricsPair is structs["odhip_metrics_pair"] and api._PipeMetricsInfo is structs["odhip_pipe_metrics_info"]
    assert ctypes.sizeof(api._MetricsPair) == 48 and ctypes.sizeof(api._PipeMetricsInfo) == 32


def test_argument_validation_without_gpu():
    import daala_amd
    from daala_amd import api
    L = daala_amd.lib()
    EINVAL = -10
    pair = api._MetricsPair(1, 2, api.SAMPLE_U8, api.SAMPLE_U8, 64, 64, 64, 64, 8, api.CSF_Y)
    # flags, depth / format, csf, region and stride are checked before any HIP call
    assert L.odhip_metrics_planes(ctypes.byref(pair), 1, 0, ctypes.c_void_p(8), ctypes.c_void_p(8), None, None,
                                  None) == EINVAL
    for field, bad in (("depth", 9), ("csf", 3), ("w", 0), ("src_stride", 10), ("rec_fmt", 7)):
        q = api._MetricsPair.from_buffer_copy(pair)
        setattr(q, field, bad)
        assert L.odhip_metrics_planes(ctypes.byref(q), 1, 3, ctypes.c_void_p(8), ctypes.c_void_p(8), None, None,
                                      None) == EINVAL, field
    q = api._MetricsPair.from_buffer_copy(pair)
    q.depth = 10                                # uint8 samples are 8-bit only
    assert L.odhip_metrics_planes(ctypes.byref(q), 1, 1, ctypes.c_void_p(8), None, None, None, None) == EINVAL
    assert L.odhip_metrics_planes(ctypes.byref(pair), 1, 2, ctypes.c_void_p(8), None, None, None, None) == EINVAL
    npix = (ctypes.c_long * 1)()
    assert L.odhip_metrics_planes(None, 0, 3, ctypes.c_void_p(8), ctypes.c_void_p(8), npix, None, None) == 0
    nx, ny = ctypes.c_int(), ctypes.c_int()
    assert L.odhip_psnrhvs_window_count(77, 53, ctypes.byref(nx), ctypes.byref(ny)) == 10 * 7
    assert (nx.value, ny.value) == (10, 7)
    assert L.odhip_psnrhvs_window_count(7, 100, None, None) == 0
    assert L.odhip_psnrhvs_windows(ctypes.byref(pair), None, None) == EINVAL
    assert L.odhip_pipe_set_metrics(None, 3, 2) == EINVAL
    assert L.odhip_pipe_metrics_take(None, 1, None, None, None) == EINVAL
