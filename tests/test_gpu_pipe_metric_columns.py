"""The columns of a pipe's metrics slot at every flag set (odhip_pipe_set_metrics5, odhip_pipe_metrics_take .. take5).

One keyframe pipe: F = 2 pictures of 64x64 at 4:2:0, chroma from luma, priced - the smallest shape every metric takes
(chroma is 32x32; MS-SSIM and FastSSIM need 16).  The resident pictures stay, so every step is the same step and the
metrics, which are repeatable, are the same bits.  The reference columns are those of flags 63.
- every other non-empty flag set, 1 .. 62, on the same pipe: take5 into arrays filled with a sentinel returns every
  column whose bit is set equal to the reference column bit for bit, and leaves every optional column whose bit is clear
  at the sentinel;
- sse with ODHIP_METRIC_SSE clear and hvs with ODHIP_METRIC_PSNRHVS clear are copied out all the same and read zero:
  set_metrics zeroes the ring and nothing writes the column;
- odhip_pipe_metrics_layout reports the flags in force and the same `values` every time;
- with flags 63, take, take2, take3 and take4 each return exactly the reference's leading columns, the steps numbered
  from the set_metrics call, and leave nothing else written."""
import ctypes
import os
import sys

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))

pytestmark = pytest.mark.gpu

F, PW, PH = 2, 64, 64
VALUES = 5 * F + 4 * 2 * F
SENTINEL = -7
# name, bit, entries, dtype: the arrays of take5 in its argument order
COLUMNS = (("sse", 1, VALUES, np.int64), ("hvs", 2, VALUES, np.float64), ("ssim", 4, VALUES, np.float64),
           ("msssim", 8, VALUES * 5, np.float64), ("fastssim", 16, VALUES * 4, np.float64),
           ("ciede", 32, 5 * F, np.float64))
TAKES = ("odhip_pipe_metrics_take", "odhip_pipe_metrics_take2", "odhip_pipe_metrics_take3",
         "odhip_pipe_metrics_take4", "odhip_pipe_metrics_take5")


def _ptr(a):
    return a.ctypes.data_as(ctypes.c_void_p)


def _bits(a):
    return a.view(np.int64)


def _set(D, pipe, flags):
    assert D.lib().odhip_pipe_set_metrics5(pipe._p(), flags, 2) == 0
    info = pipe.metrics_layout()
    assert info.flags == flags and info.values == VALUES and info.slots == 2 and info.depth == 8
    assert (info.luma_levels, info.chroma_levels, info.luma_planes, info.chroma_planes) == (5, 4, F, 2 * F)


def _step_and_take(D, pipe, name="odhip_pipe_metrics_take5"):
    """One step, complete; its columns through the named take into sentinel-filled arrays: (step, {name: array})."""
    pipe.step()
    pipe.flush()
    got = {c[0]: np.full(c[2], SENTINEL, c[3]) for c in COLUMNS}
    step = ctypes.c_long(-1)
    narrays = 2 + TAKES.index(name)
    args = [_ptr(got[c[0]]) for c in COLUMNS[:narrays]]
    assert getattr(D.lib(), name)(pipe._p(), 1, ctypes.byref(step), *args) == 1
    pipe.sync()
    return step.value, got


@pytest.fixture(scope="module")
def rig():
    """The pipe and the reference columns (flags 63), computed once and left unchanged."""
    import daala_amd as D
    import _export_check as X
    D.init(0)
    pipe = D.Pipe(D.QuantTables.for_quality(40), F, PW, PH, chroma_cfl=True, price=True)
    try:
        pipe.set_pictures(*X.stack([X.pictures(("natural", "checker")[i % 2], i, 21, PW, PH, False) for i in range(F)]))
        _set(D, pipe, 63)
        step, ref = _step_and_take(D, pipe)
        assert step == 0
        for name, _, n, _ in COLUMNS:
            # every entry written, and with something: a clear column cannot pass for a set one
            assert (ref[name] != SENTINEL).all() and (ref[name] != 0).all(), name
            ref[name].setflags(write=False)
        yield D, pipe, ref
    finally:
        pipe.destroy()


@pytest.mark.parametrize("flags", range(1, 63))
def test_every_flag_set_places_its_columns(rig, flags):
    D, pipe, ref = rig
    _set(D, pipe, flags)
    step, got = _step_and_take(D, pipe)
    assert step == 0                                                       # numbered from set_metrics
    for name, bit, n, dtype in COLUMNS:
        if flags & bit:
            assert np.array_equal(_bits(got[name]), _bits(ref[name])), (flags, name, got[name], ref[name])
        elif bit <= 2:
            assert not got[name].any(), (flags, name, got[name])           # copied out of the zeroed slot
        else:
            assert (got[name] == SENTINEL).all(), (flags, name, got[name])
    assert pipe.metrics_layout().flags == flags and pipe.metrics_layout().values == VALUES


def test_numbered_takes_return_the_leading_columns(rig):
    D, pipe, ref = rig
    _set(D, pipe, 63)
    for k, name in enumerate(TAKES[:4]):
        step, got = _step_and_take(D, pipe, name)
        assert step == k, name
        for i, (col, _, _, _) in enumerate(COLUMNS):
            if i < 2 + k:
                assert np.array_equal(_bits(got[col]), _bits(ref[col])), (name, col)
            else:
                assert (got[col] == SENTINEL).all(), (name, col)
    # NULL skips an array, the others arrive
    pipe.step()
    pipe.flush()
    ssim = np.full(VALUES, SENTINEL, np.float64)
    step = ctypes.c_long(-1)
    assert D.lib().odhip_pipe_metrics_take5(pipe._p(), 1, ctypes.byref(step), None, None, _ptr(ssim), None, None, None) == 1
    pipe.sync()
    assert step.value == 4 and np.array_equal(_bits(ssim), _bits(ref["ssim"]))
