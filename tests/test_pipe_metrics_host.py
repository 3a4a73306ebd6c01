"""PipeMetrics without a GPU: what Pipe.metrics_take hands over - the flat arrays of odhip_pipe_metrics_take5 and a
hand-filled odhip_pipe_metrics_info - laid out as documented.  F = 2 pictures, chroma_levels 4 (4:2:0) and 5 (4:4:4).

- every attribute has the documented shape: sse / hvs / ssim (luma [5][F], chroma [nlev][2F]), msssim and fastssim the
  same with a trailing 5 and 4, ciede [5][F];
- entry [set][level][plane] is the flat entry at level*planes + plane, chroma behind the 5F luma entries, for every
  column, the trailing 5 and 4 of MS-SSIM and FastSSIM and the [5][F] of CIEDE2000 included;
- every *_scores() (psnr, psnrhvs) equals the stand-alone score function applied to the same slice;
- a column that was not set reads None."""
import os
import sys

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

F = 2
NPIX, NWIN = (64 * 64, 32 * 32), (15 * 15, 7 * 7)
SSIM_WEIGHTS = (4096 * 1000, 1024 * 1000)
SIZES = ((64, 64), (32, 32))


@pytest.fixture(scope="module")
def A():
    from daala_amd import api
    return api


def _info(A, nlev, depth=8, flags=63):
    info = A._PipeMetricsInfo()
    info.luma_levels, info.chroma_levels, info.luma_planes, info.chroma_planes = 5, nlev, F, 2 * F
    info.values = 5 * F + nlev * 2 * F
    info.depth, info.flags, info.slots = depth, flags, 2
    return info


def _flat(A, nlev, seed):
    """Distinct positive values everywhere, small enough against the weights and sizes for finite scores."""
    rng = np.random.RandomState(seed)
    v = 5 * F + nlev * 2 * F
    return dict(sse=rng.permutation(v * 7)[:v].astype(np.int64) + 1,
                hvs=rng.permutation(v * 7)[:v] + rng.uniform(.25, .75, v),
                ssim=rng.permutation(v * 7)[:v] + rng.uniform(.25, .75, v),
                msssim=(rng.permutation(v * A.MSSSIM_SCALES * 3)[:v * A.MSSSIM_SCALES]
                        + rng.uniform(.25, .75, v * A.MSSSIM_SCALES)).reshape(v, A.MSSSIM_SCALES),
                fastssim=(rng.permutation(v * A.FASTSSIM_LEVELS * 3)[:v * A.FASTSSIM_LEVELS]
                          + rng.uniform(.25, .75, v * A.FASTSSIM_LEVELS)).reshape(v, A.FASTSSIM_LEVELS),
                ciede=rng.permutation(5 * F * 9)[:5 * F] + rng.uniform(.25, .75, 5 * F))


def _msssim_weights(A, seed):
    return np.random.RandomState(seed).randint(1 << 20, 1 << 24, size=(2, A.MSSSIM_SCALES)).astype(np.int64)


def _full(A, nlev, seed, depth=8):
    flat = _flat(A, nlev, seed)
    m = A.PipeMetrics(7, flat["sse"], flat["hvs"], _info(A, nlev, depth), list(NPIX), list(NWIN))
    m.set_ssim(flat["ssim"], SSIM_WEIGHTS)
    m.set_msssim(flat["msssim"], _msssim_weights(A, seed))
    m.set_fastssim(flat["fastssim"], SIZES)
    m.set_ciede(flat["ciede"], SIZES[0])
    return m, flat


def _same(a, b):
    a, b = np.asarray(a), np.asarray(b)
    return a.shape == b.shape and np.array_equal(a, b, equal_nan=True)


@pytest.mark.parametrize("nlev", (4, 5))
def test_shapes_and_places(A, nlev):
    m, flat = _full(A, nlev, 100 + nlev)
    assert m.step == 7 and m.depth == 8 and m.npixels == NPIX and m.nwindows == NWIN
    planes = (F, 2 * F)
    levels = (5, nlev)
    for name, tail in (("sse", ()), ("hvs", ()), ("ssim", ()), ("msssim", (A.MSSSIM_SCALES,)),
                       ("fastssim", (A.FASTSSIM_LEVELS,))):
        got = getattr(m, name)
        assert isinstance(got, tuple) and len(got) == 2
        for si in (0, 1):
            assert got[si].shape == (levels[si], planes[si]) + tail, (name, si)
            assert got[si].dtype == (np.int64 if name == "sse" else np.float64)
            for bs in range(levels[si]):
                for pl in range(planes[si]):
                    at = (5 * F if si else 0) + bs * planes[si] + pl
                    assert _same(got[si][bs, pl], flat[name][at]), (name, si, bs, pl)
    assert m.ciede.shape == (5, F) and m.ciede.dtype == np.float64
    for l in range(5):
        for f in range(F):
            assert m.ciede[l, f] == flat["ciede"][l * F + f]
    assert m.ssim_weights == SSIM_WEIGHTS and m.fastssim_sizes == SIZES and m.ciede_size == SIZES[0]
    assert m.msssim_weights.shape == (2, A.MSSSIM_SCALES) and m.msssim_weights.dtype == np.int64
    assert np.array_equal(m.msssim_weights, _msssim_weights(A, 100 + nlev))


@pytest.mark.parametrize("nlev,depth", ((4, 8), (5, 10)))
def test_scores_are_the_stand_alone_functions(A, nlev, depth):
    m, flat = _full(A, nlev, 200 + nlev, depth)
    wt = _msssim_weights(A, 200 + nlev)
    n = 5 * F
    shape = ((5, F), (nlev, 2 * F))
    cut = lambda a, si: (a[:n] if si == 0 else a[n:]).reshape(shape[si] + a.shape[1:])
    for name, got in (("psnr", m.psnr()), ("psnrhvs", m.psnrhvs()), ("ssim", m.ssim_scores()),
                      ("ssim_raw", m.ssim_scores(raw=True)), ("msssim", m.msssim_scores()),
                      ("msssim_raw", m.msssim_scores(raw=True)), ("fastssim", m.fastssim_scores()),
                      ("fastssim_raw", m.fastssim_scores(raw=True))):
        assert isinstance(got, tuple) and len(got) == 2
        for si in (0, 1):
            raw = name.endswith("_raw")
            want = {"psnr": lambda: A.psnr_db(cut(flat["sse"], si), NPIX[si], depth),
                    "psnrhvs": lambda: A.psnrhvs_db(cut(flat["hvs"], si), NWIN[si], depth),
                    "ssim": lambda: A.ssim_score(cut(flat["ssim"], si), SSIM_WEIGHTS[si], raw),
                    "msssim": lambda: A.msssim_score(cut(flat["msssim"], si), wt[si], raw),
                    "fastssim": lambda: A.fastssim_score(cut(flat["fastssim"], si), *SIZES[si], raw=raw),
                    }[name.replace("_raw", "")]()
            assert got[si].shape == shape[si] and _same(got[si], want), (name, si)
            assert np.isfinite(got[si]).any(), (name, si)
    want = A.ciede_score(flat["ciede"].reshape(5, F), *SIZES[0])
    assert m.ciede_scores().shape == (5, F) and _same(m.ciede_scores(), want) and np.isfinite(want).all()


@pytest.mark.parametrize("nlev", (4, 5))
def test_a_column_that_was_not_set_reads_none(A, nlev):
    flat = _flat(A, nlev, 300 + nlev)
    m = A.PipeMetrics(0, flat["sse"], flat["hvs"], _info(A, nlev, flags=3), list(NPIX), list(NWIN))
    names = ("ssim", "ssim_weights", "msssim", "msssim_weights", "fastssim", "fastssim_sizes", "ciede", "ciede_size")
    for name in names:
        assert getattr(m, name) is None, name
    # each one alone leaves the others unset
    for col, args in (("ssim", (flat["ssim"], SSIM_WEIGHTS)), ("msssim", (flat["msssim"], _msssim_weights(A, 1))),
                      ("fastssim", (flat["fastssim"], SIZES)), ("ciede", (flat["ciede"], SIZES[0]))):
        m = A.PipeMetrics(0, flat["sse"], flat["hvs"], _info(A, nlev), list(NPIX), list(NWIN))
        getattr(m, "set_" + col)(*args)
        for name in names:
            assert (getattr(m, name) is None) == (not name.startswith(col)), (col, name)
        assert m.sse[1].shape == (nlev, 2 * F)
