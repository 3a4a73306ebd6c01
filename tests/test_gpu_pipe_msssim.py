"""MS-SSIM of every pipe step (ODHIP_METRIC_MSSSIM in odhip_pipe_set_metrics3, odhip_pipe_metrics_take3).

F = 2 pictures of 128x64, 4:2:0 and 4:4:4, 8-bit planes and full-precision references at 10 bits; one keyframe step with
chroma from luma and one inter step:
- every (set, level, plane) five sums of take3 equal odhip_msssim_planes on the pipe's own ODHIP_PIPE_BUF_PX /
  ODHIP_PIPE_BUF_RECON buffers, bit for bit, and the weights are odhip_msssim_weights of the plane sizes;
- the SSE, HVS and SSIM columns equal those of a twin pipe with the bit clear, whose layout does not report it;
- the older odhip_pipe_metrics_take and odhip_pipe_metrics_take2 still work on the same pipe.
MS-SSIM alone (flags = 8); the older entry points refuse the bit, a ring of one slot and a 64x24 4:2:0 pipe (chroma
32x12) are refused and leave the metrics as they were.  With the margins forced wide (odhip_pipe_set_test_hooks) the
step re-measured inside the next step equals a drained twin's."""
import ctypes
import os
import sys

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))

pytestmark = pytest.mark.gpu

F, PW, PH = 2, 128, 64


@pytest.fixture(scope="module")
def D():
    import daala_amd
    daala_amd.init(0)
    return daala_amd


def _pictures(pw, ph, c444, depth, seed, k=0, frames=F):
    import _export_check as X
    luma, chroma = X.stack([X.pictures(("natural", "checker")[(i + k) % 2], 10 * k + i, seed, pw, ph, c444)
                            for i in range(frames)])
    if depth > 8:
        rng = np.random.RandomState(seed + k)
        up = lambda a: ((a.astype(np.int32) << (depth - 8))
                        + rng.randint(0, 1 << (depth - 8), size=a.shape)).astype(np.int16)
        return up(luma), up(chroma)
    return luma, chroma


def _own_buffers(D, pipe, depth):
    """odhip_msssim_planes over the pipe's padded source planes and reconstruction levels: (luma [5][F][5], chroma
    [nlev][2F][5]) sums."""
    import torch
    from daala_amd.api import _MetricsPair
    fpr = pipe.fpr_bits != 0
    fmt = D.SAMPLE_I16_12 if fpr else D.SAMPLE_U8
    out = []
    for si in (0, 1):
        dec = 1 if si and not pipe.chroma_444 else 0
        W, H = pipe.W >> dec, pipe.H >> dec
        pw, ph = (pipe.pic_w + dec) >> dec, (pipe.pic_h + dec) >> dec
        nlev = 5 if si == 0 else pipe.chroma_levels
        planes = pipe.frames * (2 if si else 1)
        px, _ = pipe.buffer(D.BUF_PX, si, 0, -1)
        pairs = (_MetricsPair * (nlev * planes))()
        for bs in range(nlev):
            rec, _ = pipe.buffer(D.BUF_RECON, si, bs, -1)
            for pl in range(planes):
                off = pl * W * H * (2 if fpr else 1)
                pairs[bs * planes + pl] = _MetricsPair(px + off, rec + off, fmt, fmt, W, W, pw, ph, depth, 0)
        d = torch.zeros((nlev * planes, 5), dtype=torch.float64, device="cuda")
        rc = D.lib().odhip_msssim_planes(pairs, nlev * planes, ctypes.c_void_p(d.data_ptr()), None, None)
        assert rc == 0
        torch.cuda.synchronize()
        out.append(d.cpu().numpy().reshape(nlev, planes, 5))
    return out


def _old_takes(D, pipe, info, which):
    """odhip_pipe_metrics_take (which = 1) or take2 (2) of the next step: its number and columns."""
    sse = np.zeros(info.values, np.int64)
    hvs = np.zeros(info.values, np.float64)
    ssim = np.zeros(info.values, np.float64)
    step = ctypes.c_long(-1)
    p = lambda a: a.ctypes.data_as(ctypes.c_void_p)
    if which == 1:
        rc = D.lib().odhip_pipe_metrics_take(pipe._p(), 1, ctypes.byref(step), p(sse), p(hvs))
    else:
        rc = D.lib().odhip_pipe_metrics_take2(pipe._p(), 1, ctypes.byref(step), p(sse), p(hvs), p(ssim))
    assert rc == 1
    return step.value, sse, hvs, ssim


def _run(D, c444, fpr_bits, inter, msssim):
    """Three steps (step, flush, take, sync): the first taken with take3, the others with the two older takes."""
    depth = fpr_bits or 8
    kw = dict(price=True, fpr_bits=fpr_bits, chroma_444=c444)
    kw.update(dict(inter=True) if inter else dict(chroma_cfl=True))
    pipe = D.Pipe(D.QuantTables.load(), F, PW, PH, **kw)
    try:
        pipe.set_metrics(ssim=True, msssim=msssim)
        info = pipe.metrics_layout()
        assert info.flags == (15 if msssim else 7)
        out = []
        for k in range(3):
            pipe.set_pictures(*_pictures(PW, PH, c444, depth, 3, k))
            if inter:
                pipe.set_reference_pictures(*_pictures(PW, PH, c444, depth, 9, k))
            pipe.step()
            pipe.flush()
            if k == 0:
                m = pipe.metrics_take(wait=True)
                assert m.step == 0
            else:
                m = _old_takes(D, pipe, info, k)
                assert m[0] == k
            assert pipe.metrics_take(wait=False) is None
            pipe.sync()
            out.append((m, _own_buffers(D, pipe, depth) if msssim and k == 0 else None))
        return out, pipe.metrics_msssim_weights()
    finally:
        pipe.destroy()


@pytest.mark.parametrize("inter", [False, True], ids=["cfl", "inter"])
@pytest.mark.parametrize("fpr_bits", [0, 10], ids=["u8", "fpr10"])
@pytest.mark.parametrize("c444", [False, True], ids=["420", "444"])
def test_take3_equals_msssim_planes_on_the_pipes_buffers(D, c444, fpr_bits, inter):
    on, weights = _run(D, c444, fpr_bits, inter, True)
    off, _ = _run(D, c444, fpr_bits, inter, False)
    m, own = on[0]
    twin = off[0][0]
    assert m.msssim is not None and twin.msssim is None and twin.msssim_weights is None
    cdec = 0 if c444 else 1
    want = [D.msssim_weights(PW, PH), D.msssim_weights((PW + cdec) >> cdec, (PH + cdec) >> cdec)]
    assert weights.tolist() == want and m.msssim_weights.tolist() == want
    for si in (0, 1):
        assert m.msssim[si].shape == own[si].shape == m.sse[si].shape + (5,)
        assert np.array_equal(m.msssim[si].view(np.int64), own[si].view(np.int64)), (si, m.msssim[si], own[si])
        raw = m.msssim_scores(raw=True)[si]
        assert raw.shape == m.sse[si].shape and ((raw > 0) & (raw <= 1)).all() and np.isfinite(m.msssim_scores()[si]).all()
        # the other columns are the twin's
        assert np.array_equal(m.sse[si], twin.sse[si])
        assert np.array_equal(m.hvs[si].view(np.int64), twin.hvs[si].view(np.int64))
        assert np.array_equal(m.ssim[si].view(np.int64), twin.ssim[si].view(np.int64))
    # the older takes on the same pipe: the same columns as the twin's
    for k in (1, 2):
        for a, b in zip(on[k][0][1:], off[k][0][1:]):
            assert np.array_equal(a.view(np.int64), b.view(np.int64))
        assert on[k][0][1].any() and on[k][0][2].any()
    assert on[2][0][3].any() and not on[1][0][3].any()                 # take returns no SSIM column, take2 does


def test_msssim_alone_and_bad_arguments(D):
    pipe = D.Pipe(D.QuantTables.load(), F, PW, PH, chroma_cfl=True, price=True)
    L = D.lib()
    try:
        assert L.odhip_pipe_set_metrics3(pipe._p(), 16, 2) == -10             # unknown flag
        assert L.odhip_pipe_set_metrics3(pipe._p(), 8, 1) == -10              # a ring of one slot
        for flags in (8, 9, 15):
            assert L.odhip_pipe_set_metrics(pipe._p(), flags, 2) == -10       # the older entry points keep their flags
            assert L.odhip_pipe_set_metrics2(pipe._p(), flags, 2) == -10
        assert pipe.metrics_layout().flags == 0
        assert L.odhip_pipe_metrics_msssim_weights(pipe._p(), None) == -10
        pipe.set_metrics(sse=False, psnrhvs=False, msssim=True)
        assert pipe.metrics_layout().flags == D.METRIC_MSSSIM == 8
        pipe.set_pictures(*_pictures(PW, PH, False, 8, 3))
        pipe.step()
        pipe.flush()
        m = pipe.metrics_take()
        pipe.sync()
        own = _own_buffers(D, pipe, 8)
        assert m.ssim is None
        for si in (0, 1):
            assert np.array_equal(m.msssim[si].view(np.int64), own[si].view(np.int64))
            assert not m.sse[si].any() and not m.hvs[si].any()
    finally:
        pipe.destroy()
    # 4:2:0 chroma of 64 x 24 is 32 x 12: below the floor
    small = D.Pipe(D.QuantTables.load(), F, 64, 24, chroma_cfl=True, price=True)
    try:
        small.set_metrics()
        assert L.odhip_pipe_set_metrics3(small._p(), 15, 2) == -10
        assert L.odhip_pipe_set_metrics3(small._p(), 8, 2) == -10
        assert small.metrics_layout().flags == 3                             # as they were
        small.set_pictures(*_pictures(64, 24, False, 8, 3))
        small.step()
        small.flush()
        m = small.metrics_take()
        small.sync()
        assert m.step == 0 and m.sse[0].any() and m.msssim is None
    finally:
        small.destroy()


def _same(a, b):
    for i in (0, 1):
        assert np.array_equal(a.sse[i], b.sse[i])
        assert np.array_equal(a.hvs[i].view(np.int64), b.hvs[i].view(np.int64))
        assert np.array_equal(a.msssim[i].view(np.int64), b.msssim[i].view(np.int64))


@pytest.mark.parametrize("inter", [False, True], ids=["cfl", "inter"])
def test_late_resolves_measure_msssim_again(D, inter):
    """Margins forced wide: bands of every step are re-decided one step late, inside the next step, which runs the
    inverse and the metrics again; what is taken after that step equals the drained twin's."""
    import torch
    qt = D.QuantTables.for_quality(40)
    n = 3
    inputs = [tuple(torch.from_numpy(a).pin_memory() for a in _pictures(PW, PH, False, 8, 21, k)) for k in range(n)]
    refs = _pictures(PW, PH, False, 8, 9)
    kw = dict(inter=True, price=True) if inter else dict(chroma_cfl=True, price=True)
    D.pvq_ref_set_theta_margin(0.25, True)
    D.set_price_tol_scale(1e7)
    try:
        twin = D.Pipe(qt, F, PW, PH, **kw)
        try:
            if inter:
                twin.set_reference_pictures(*refs)
            twin.set_metrics(msssim=True)
            want = []
            for l, c in inputs:
                twin.feed(l, c)
                twin.step()
                twin.flush()
                want.append(twin.metrics_take())
                twin.sync()
        finally:
            twin.destroy()
        pipe = D.Pipe(qt, F, PW, PH, **kw)
        try:
            if inter:
                pipe.set_reference_pictures(*refs)
            pipe.set_metrics(msssim=True)
            got = []
            for k, (l, c) in enumerate(inputs):
                pipe.feed(l, c)
                pipe.step()
                if k >= 1:
                    got.append(pipe.metrics_take())
            pipe.flush()
            got.append(pipe.metrics_take())
            pipe.sync()
            print("theta reruns %d, price reruns %d" % (pipe.theta_reruns(), pipe.price_reruns()))
            assert pipe.theta_reruns() + pipe.price_reruns() > 0          # the late paths really ran
            assert [m.step for m in got] == list(range(n))
            for k in range(n):
                _same(got[k], want[k])
            own = _own_buffers(D, pipe, 8)
            for si in (0, 1):
                assert np.array_equal(got[-1].msssim[si].view(np.int64), own[si].view(np.int64))
        finally:
            pipe.destroy()
    finally:
        D.pvq_ref_set_theta_margin(0, False)
        D.set_price_tol_scale(1.)
