"""CPU: the strided, sentinel-surrounded plane sets of tests/_strided.py, exercised with the oracle writing
into a host-side set - the sentinel check must notice a single column written outside the windows."""
import ctypes

import numpy as np
import pytest

from _libs import P, oracle
from _strided import LAYOUTS, LEAD, PlaneSet


@pytest.mark.parametrize("layout", list(LAYOUTS))
@pytest.mark.parametrize("dtype", [np.uint8, np.int16])
def test_write_read_and_sentinel(layout, dtype):
    rng = np.random.RandomState(1)
    data = rng.randint(0, 200, size=(2, 6, 12)).astype(dtype)
    ps = PlaneSet.in_layout(layout, 2, 6, 12, dtype, device=None)
    ds, base, dp = LAYOUTS[layout]
    assert (ps.stride, ps.base, ps.plane_stride) == (12 + ds, base, (12 + ds) * 6 + dp)
    assert ps.ptr.value == ps.buf.ctypes.data + (LEAD + base) * np.dtype(dtype).itemsize
    assert ps.intact(0, 0)
    ps.write(data)
    assert np.array_equal(ps.read(), data) and ps.intact() and not ps.intact(0, 0)
    # plane 1, row 2, sample 3 is where the layout says
    assert ps.buf[LEAD + base + ps.plane_stride + 2 * ps.stride + 3] == data[1, 2, 3]
    for at in (0, LEAD + base - 1, LEAD + base + 12 if ds else None, ps.size - 1):
        if at is not None:
            keep = ps.buf[at]
            ps.buf[at] = 1
            assert not ps.intact(), at
            ps.buf[at] = keep
    assert ps.intact()


def test_sentinel_check_notices_a_window_one_column_too_narrow():
    """The oracle's input padding writes a 64x64 plane into each window of a gapped set: intact for the
    windows it wrote, not intact when the helper is told the windows are one column narrower (or one row
    shorter)."""
    o = oracle()
    rng = np.random.RandomState(2)
    pic = rng.randint(0, 256, size=(2, 17, 33)).astype(np.uint8)
    ps = PlaneSet.in_layout("gap16", 2, 64, 64, np.uint8, device=None)
    for p in range(2):
        o.odo_img_plane_copy_pad(ctypes.c_void_p(ps.ptr.value + p * ps.plane_stride), ps.stride, 64, 64,
                                 P(np.ascontiguousarray(pic[p])), 33, 33, 17)
    want = np.zeros((64, 64), np.uint8)
    o.odo_img_plane_copy_pad(P(want), 64, 64, 64, P(np.ascontiguousarray(pic[1])), 33, 33, 17)
    assert np.array_equal(ps.read()[1], want)
    assert ps.intact()
    assert not ps.intact(w=63)
    assert not ps.intact(h=63)
