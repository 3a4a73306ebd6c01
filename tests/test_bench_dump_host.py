"""bench.py --dump-outputs on the host: a stand-in pipe whose buffers are as large as the 16-frame step's
reconstructions; the files must be float32, within 64 MB, and identical from one call to the next."""
import os

import numpy as np

import bench


class _D:
    BUF_RECON = 3


class _Pipe:
    def read(self, what, set_, level):
        assert what == _D.BUF_RECON
        n = 16 * bench.H * bench.W if set_ == 0 else 32 * (bench.H // 2) * (bench.W // 2)
        n >>= 2 * level
        return np.random.RandomState(10 * set_ + level).randint(0, 256, size=n).astype(np.uint8)


def _dump(path):
    bench.dump_outputs(_D, _Pipe(), str(path), decisions=False)
    return {f: np.load(os.path.join(path, f)) for f in sorted(os.listdir(path))}


def test_dump_outputs_is_bounded_float32_and_repeatable(tmp_path):
    a = _dump(tmp_path / "a")
    b = _dump(tmp_path / "b")
    assert sorted(a) == ["recon_%s_l%d.npy" % (s, l) for s in ("chroma", "luma") for l in range(5 - (s == "chroma"))]
    assert sum(v.nbytes for v in a.values()) <= 64 << 20
    for name, v in a.items():
        assert v.dtype == np.float32 and v.size <= bench.DUMP_CAP
        assert np.array_equal(v, b[name]), name
    # a buffer under the cap is written whole
    whole = _Pipe().read(_D.BUF_RECON, 0, 4)
    assert whole.size <= bench.DUMP_CAP and np.array_equal(a["recon_luma_l4.npy"], whole)
