"""SSIM of every pipe step (ODHIP_METRIC_SSIM in odhip_pipe_set_metrics2, odhip_pipe_metrics_take2).

F = 2 pictures of 128x64, 4:2:0 and 4:4:4, 8-bit planes and full-precision references at 10 bits; one keyframe step with
chroma from luma and one inter step:
- every (set, level, plane) value of take2 equals odhip_ssim_planes on the pipe's own ODHIP_PIPE_BUF_PX /
  ODHIP_PIPE_BUF_RECON buffers, bit for bit, and the weights are odhip_ssim_weight of the plane sizes;
- the SSE and HVS columns equal those of a twin pipe with the bit clear, whose layout does not report it;
- the old odhip_pipe_metrics_take still works on the same pipe.
With the theta margin forced (odhip_pipe_set_test_hooks) the step re-measured inside the next step equals a drained
twin's."""
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
    """odhip_ssim_planes over the pipe's padded source planes and reconstruction levels: (luma [5][F], chroma
    [nlev][2F]) sums."""
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
        d = torch.zeros(nlev * planes, dtype=torch.float64, device="cuda")
        rc = D.lib().odhip_ssim_planes(pairs, nlev * planes, ctypes.c_double(1.0), ctypes.c_void_p(d.data_ptr()), None,
                                       None)
        assert rc == 0
        torch.cuda.synchronize()
        out.append(d.cpu().numpy().reshape(nlev, planes))
    return out


def _run(D, c444, fpr_bits, inter, ssim):
    """Two steps (step, flush, take, sync); returns [(metrics, own-buffer sums)] and the second step's old-style take."""
    depth = fpr_bits or 8
    kw = dict(price=True, fpr_bits=fpr_bits, chroma_444=c444)
    kw.update(dict(inter=True) if inter else dict(chroma_cfl=True))
    pipe = D.Pipe(D.QuantTables.load(), F, PW, PH, **kw)
    try:
        pipe.set_metrics(ssim=ssim)
        info = pipe.metrics_layout()
        assert info.flags == (7 if ssim else 3)
        out = []
        for k in range(2):
            pipe.set_pictures(*_pictures(PW, PH, c444, depth, 3, k))
            if inter:
                pipe.set_reference_pictures(*_pictures(PW, PH, c444, depth, 9, k))
            pipe.step()
            pipe.flush()
            if k == 0:
                m = pipe.metrics_take(wait=True)
                old = None
            else:
                # the entry point from before the third column: same step, same first two columns
                sse = np.zeros(info.values, np.int64)
                hvs = np.zeros(info.values, np.float64)
                step = ctypes.c_long(-1)
                rc = D.lib().odhip_pipe_metrics_take(pipe._p(), 1, ctypes.byref(step),
                                                     sse.ctypes.data_as(ctypes.c_void_p),
                                                     hvs.ctypes.data_as(ctypes.c_void_p))
                assert rc == 1 and step.value == 1
                m, old = None, (sse, hvs)
            assert pipe.metrics_take(wait=False) is None
            pipe.sync()
            out.append((m, _own_buffers(D, pipe, depth) if ssim else None))
        weights = pipe.metrics_ssim_weights()
        return out, old, weights
    finally:
        pipe.destroy()


@pytest.mark.parametrize("inter", [False, True], ids=["cfl", "inter"])
@pytest.mark.parametrize("fpr_bits", [0, 10], ids=["u8", "fpr10"])
@pytest.mark.parametrize("c444", [False, True], ids=["420", "444"])
def test_take2_equals_ssim_planes_on_the_pipes_buffers(D, c444, fpr_bits, inter):
    on, old_on, weights = _run(D, c444, fpr_bits, inter, True)
    off, old_off, _ = _run(D, c444, fpr_bits, inter, False)
    m, own = on[0]
    assert m.step == 0 and m.ssim is not None and off[0][0].ssim is None
    cdec = 0 if c444 else 1
    assert weights == (D.ssim_weight(PW, PH), D.ssim_weight((PW + cdec) >> cdec, (PH + cdec) >> cdec))
    assert m.ssim_weights == weights
    for si in (0, 1):
        assert m.ssim[si].shape == own[si].shape == m.sse[si].shape
        assert np.array_equal(m.ssim[si].view(np.int64), own[si].view(np.int64)), (si, m.ssim[si], own[si])
        raw = m.ssim_scores(raw=True)[si]
        assert ((raw > 0) & (raw <= 1)).all() and np.isfinite(m.ssim_scores()[si]).all()
        # the first two columns are the twin's
        assert np.array_equal(m.sse[si], off[0][0].sse[si])
        assert np.array_equal(m.hvs[si].view(np.int64), off[0][0].hvs[si].view(np.int64))
    assert np.array_equal(old_on[0], old_off[0])
    assert np.array_equal(old_on[1].view(np.int64), old_off[1].view(np.int64))
    assert old_on[0].any() and old_on[1].any()


def test_ssim_alone_and_bad_arguments(D):
    pipe = D.Pipe(D.QuantTables.load(), F, PW, PH, chroma_cfl=True, price=True)
    L = D.lib()
    try:
        assert L.odhip_pipe_set_metrics2(pipe._p(), 8, 2) == -10              # unknown flag
        assert L.odhip_pipe_set_metrics2(pipe._p(), 4, 1) == -10              # a ring of one slot
        assert L.odhip_pipe_set_metrics(pipe._p(), 4, 2) == -10               # the old entry point keeps its two flags
        assert L.odhip_pipe_set_metrics(pipe._p(), 7, 2) == -10
        assert pipe.metrics_layout().flags == 0
        assert L.odhip_pipe_metrics_ssim_weights(pipe._p(), None) == -10
        pipe.set_metrics(sse=False, psnrhvs=False, ssim=True)
        assert pipe.metrics_layout().flags == D.METRIC_SSIM
        pipe.set_pictures(*_pictures(PW, PH, False, 8, 3))
        pipe.step()
        pipe.flush()
        m = pipe.metrics_take()
        pipe.sync()
        own = _own_buffers(D, pipe, 8)
        for si in (0, 1):
            assert np.array_equal(m.ssim[si].view(np.int64), own[si].view(np.int64))
            assert not m.sse[si].any() and not m.hvs[si].any()
    finally:
        pipe.destroy()


def _same(a, b):
    for i in (0, 1):
        assert np.array_equal(a.sse[i], b.sse[i])
        assert np.array_equal(a.hvs[i].view(np.int64), b.hvs[i].view(np.int64))
        assert np.array_equal(a.ssim[i].view(np.int64), b.ssim[i].view(np.int64))


@pytest.mark.parametrize("inter", [False, True], ids=["cfl", "inter"])
def test_late_resolves_measure_ssim_again(D, inter):
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
            twin.set_metrics(ssim=True)
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
            pipe.set_metrics(ssim=True)
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
                assert np.array_equal(got[-1].ssim[si].view(np.int64), own[si].view(np.int64))
        finally:
            pipe.destroy()
    finally:
        D.pvq_ref_set_theta_margin(0, False)
        D.set_price_tol_scale(1.)
