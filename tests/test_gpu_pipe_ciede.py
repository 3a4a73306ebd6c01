"""CIEDE2000 of every pipe step (ODHIP_METRIC_CIEDE in odhip_pipe_set_metrics5, odhip_pipe_metrics_take5).

F = 2 pictures of 64x64 or 96x80, other pictures every step: keyframes with chroma from luma at 4:2:0 and 4:4:4, inter
steps, keyframes with full-precision references at 10 bits, and keyframes without chroma from luma (no late resolve).
The margins are forced wide (odhip_pipe_set_test_hooks), so that bands of every step are re-decided one step late,
inside the next step or the flush, which runs the inverse again:
- ciede[l][f] of a step equals odhip_ciede_pictures over the pipe's own ODHIP_PIPE_BUF_PX and ODHIP_PIPE_BUF_RECON
  buffers - luma level l with chroma level max(l - 1, 0) at 4:2:0, l at 4:4:4 - bit for bit, after the late resolve:
  the value is that of the final reconstruction;
- three fed steps, each measured inside the next step or the flush, equal three steps drained one at a time (step,
  flush, take, sync), bit for bit: the luma chain of step i + 1 does not overwrite what step i's measurement reads;
- the other columns of take5 equal take4's of an identical pipe without the bit, and so do the reconstructions;
- odhip_pipe_metrics_ciede_values is 5F and odhip_pipe_metrics_layout reports the same values with and without the bit.
CIEDE2000 alone (flags = 32); odhip_pipe_set_metrics .. set_metrics4 refuse the bit and leave the metrics as they were;
with the bit clear take5 leaves its ciede array untouched."""
import ctypes
import math
import os
import sys

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))

pytestmark = pytest.mark.gpu

F = 2
EINVAL = -10


@pytest.fixture(scope="module")
def D():
    import daala_amd
    daala_amd.init(0)
    return daala_amd


def _pictures(pw, ph, c444, depth, seed, k=0):
    import _export_check as X
    luma, chroma = X.stack([X.pictures(("natural", "checker")[(i + k) % 2], 10 * k + i, seed, pw, ph, c444)
                            for i in range(F)])
    if depth > 8:
        rng = np.random.RandomState(seed + k)
        up = lambda a: ((a.astype(np.int32) << (depth - 8))
                        + rng.randint(0, 1 << (depth - 8), size=a.shape)).astype(np.int16)
        return up(luma), up(chroma)
    return luma, chroma


def _own_buffers(D, pipe, depth):
    """odhip_ciede_pictures over the pipe's padded source planes and reconstruction levels, paired here as the header
    says: SUM dE00 [5][F]."""
    import torch
    from daala_amd.api import _CiedePair
    fpr = pipe.fpr_bits != 0
    fmt = D.SAMPLE_I16_12 if fpr else D.SAMPLE_U8
    size = 2 if fpr else 1
    cdec = 0 if pipe.chroma_444 else 1
    W, H = pipe.W, pipe.H
    CW, CH = W >> cdec, H >> cdec
    ypx, _ = pipe.buffer(D.BUF_PX, 0, 0, -1)
    cpx, _ = pipe.buffer(D.BUF_PX, 1, 0, -1)
    pairs = (_CiedePair * (5 * F))()
    for l in range(5):
        cl = (max(l - 1, 0) if cdec else l)
        assert cl < pipe.chroma_levels
        yrec, _ = pipe.buffer(D.BUF_RECON, 0, l, -1)
        crec, _ = pipe.buffer(D.BUF_RECON, 1, cl, -1)
        for f in range(F):
            q = pairs[l * F + f]
            q.src[0], q.rec[0] = ypx + f * W * H * size, yrec + f * W * H * size
            for k in (0, 1):
                q.src[1 + k] = cpx + (k * F + f) * CW * CH * size
                q.rec[1 + k] = crec + (k * F + f) * CW * CH * size
            q.src_fmt = q.rec_fmt = fmt
            q.src_stride = q.rec_stride = W
            q.src_cstride = q.rec_cstride = CW
            q.w, q.h, q.depth, q.cdec = pipe.pic_w, pipe.pic_h, depth, cdec
    d = torch.zeros(5 * F, dtype=torch.float64, device="cuda")
    assert D.lib().odhip_ciede_pictures(pairs, 5 * F, ctypes.c_void_p(d.data_ptr()), None) == 0
    torch.cuda.synchronize()
    return d.cpu().numpy().reshape(5, F)


MODES = {
    "420_cfl": dict(size=(64, 64), kw=dict(chroma_cfl=True, price=True)),
    "444_cfl": dict(size=(96, 80), kw=dict(chroma_cfl=True, price=True, chroma_444=True)),
    "inter": dict(size=(96, 80), kw=dict(inter=True, price=True)),
    "fpr10": dict(size=(64, 64), kw=dict(chroma_cfl=True, price=True, fpr_bits=10)),
    "no_cfl": dict(size=(64, 64), kw=dict(chroma_cfl=False, price=True)),
}
NSTEPS = 3


def _make(D, spec, ciede):
    pw, ph = spec["size"]
    kw = spec["kw"]
    depth = kw.get("fpr_bits", 0) or 8
    pipe = D.Pipe(D.QuantTables.for_quality(40), F, pw, ph, **kw)
    if kw.get("inter"):
        pipe.set_reference_pictures(*_pictures(pw, ph, False, depth, 9))
    pipe.set_metrics(ssim=True, msssim=True, fastssim=True, ciede=ciede)
    return pipe


def _inputs(spec):
    import torch
    pw, ph = spec["size"]
    kw = spec["kw"]
    depth = kw.get("fpr_bits", 0) or 8
    return [tuple(torch.from_numpy(a).pin_memory() for a in _pictures(pw, ph, kw.get("chroma_444", False), depth, 21, k))
            for k in range(NSTEPS)]


def _fed(D, pipe, inputs):
    """The steps in flight, each taken once the next step (or the flush) has completed it."""
    got = []
    for k, (l, c) in enumerate(inputs):
        pipe.feed(l, c)
        pipe.step()
        if k >= 1:
            got.append(pipe.metrics_take())
    pipe.flush()
    got.append(pipe.metrics_take())
    pipe.sync()
    assert [m.step for m in got] == list(range(len(inputs)))
    return got


def _recon(D, pipe):
    return [pipe.read(D.BUF_RECON, si, bs).copy() for si in (0, 1) for bs in range(5 if si == 0 else pipe.chroma_levels)]


@pytest.mark.parametrize("mode", sorted(MODES))
def test_take5_equals_ciede_pictures_fed_and_drained(D, mode):
    spec = MODES[mode]
    depth = spec["kw"].get("fpr_bits", 0) or 8
    inputs = _inputs(spec)
    D.pvq_ref_set_theta_margin(0.25, True)
    D.set_price_tol_scale(1e7)
    try:
        # drained: every step measured inside its own flush, then compared with the pipe's own buffers
        twin = _make(D, spec, True)
        try:
            info = twin.metrics_layout()
            assert info.flags == 63 and twin.metrics_ciede_values() == 5 * F
            assert info.values == 5 * F + twin.chroma_levels * 2 * F
            want = []
            for k, (l, c) in enumerate(inputs):
                twin.feed(l, c)
                twin.step()
                twin.flush()
                m = twin.metrics_take()
                twin.sync()
                assert m.step == k and m.ciede.shape == (5, F)
                own = _own_buffers(D, twin, depth)
                assert np.array_equal(m.ciede.view(np.int64), own.view(np.int64)), (k, m.ciede, own)
                assert (m.ciede > 0).all() and np.isfinite(m.ciede_scores()).all()
                want.append(m)
            # other pictures every step, other reconstructions every level
            assert len({v for m in want for v in m.ciede.ravel()}) > NSTEPS * F
        finally:
            twin.destroy()
        pipe = _make(D, spec, True)
        try:
            got = _fed(D, pipe, inputs)
            reruns = pipe.theta_reruns() + pipe.price_reruns()
            own = _own_buffers(D, pipe, depth)
            recon = _recon(D, pipe)
        finally:
            pipe.destroy()
        plain = _make(D, spec, False)
        try:
            assert plain.metrics_layout().flags == 31 and plain.metrics_layout().values == info.values
            rest = _fed(D, plain, inputs)
            precon = _recon(D, plain)
        finally:
            plain.destroy()
    finally:
        D.pvq_ref_set_theta_margin(0, False)
        D.set_price_tol_scale(1.)
    print("%s: late reruns %d" % (mode, reruns))
    if mode != "no_cfl":
        assert reruns > 0                                              # the late paths really ran
    # the last step in flight, measured behind its late resolve: the pipe's own buffers
    assert np.array_equal(got[-1].ciede.view(np.int64), own.view(np.int64)), (got[-1].ciede, own)
    for k in range(NSTEPS):
        assert np.array_equal(got[k].ciede.view(np.int64), want[k].ciede.view(np.int64)), (k, got[k].ciede, want[k].ciede)
        a, b = got[k], rest[k]
        assert b.ciede is None
        for si in (0, 1):
            assert np.array_equal(a.sse[si], b.sse[si])
            for x, y in ((a.hvs, b.hvs), (a.ssim, b.ssim), (a.msssim, b.msssim), (a.fastssim, b.fastssim)):
                assert x[si].any() and np.array_equal(x[si].view(np.int64), y[si].view(np.int64))
    assert len(recon) == len(precon) and all(np.array_equal(x, y) for x, y in zip(recon, precon))


def test_ciede_alone_and_bad_arguments(D):
    pw, ph = 64, 64
    pipe = D.Pipe(D.QuantTables.load(), F, pw, ph, chroma_cfl=True, price=True)
    L = D.lib()
    try:
        assert L.odhip_pipe_set_metrics5(pipe._p(), 64, 2) == EINVAL            # unknown flag
        assert L.odhip_pipe_set_metrics5(pipe._p(), 32, 1) == EINVAL            # a ring of one slot
        assert L.odhip_pipe_set_metrics5(None, 32, 2) == EINVAL
        pipe.set_metrics()
        assert pipe.metrics_layout().flags == 3
        for flags in (32, 35, 63):
            for name in ("odhip_pipe_set_metrics", "odhip_pipe_set_metrics2", "odhip_pipe_set_metrics3",
                         "odhip_pipe_set_metrics4"):
                assert getattr(L, name)(pipe._p(), flags, 2) == EINVAL, (name, flags)
            assert pipe.metrics_layout().flags == 3                            # as they were
        # with the bit clear take5 leaves the array alone
        pipe.set_pictures(*_pictures(pw, ph, False, 8, 3))
        pipe.step()
        pipe.flush()
        info = pipe.metrics_layout()
        sse = np.zeros(info.values, np.int64)
        hvs = np.zeros(info.values, np.float64)
        ciede = np.full(5 * F, -7.0)
        step = ctypes.c_long(-1)
        p = lambda a: a.ctypes.data_as(ctypes.c_void_p)
        assert L.odhip_pipe_metrics_take5(pipe._p(), 1, ctypes.byref(step), p(sse), p(hvs), None, None, None, p(ciede)) == 1
        assert step.value == 0 and sse.any() and (ciede == -7.0).all()
        pipe.sync()
        # the column alone, and the older takes on a pipe that has it
        pipe.set_metrics(sse=False, psnrhvs=False, ciede=True)
        assert pipe.metrics_layout().flags == D.METRIC_CIEDE == 32
        assert L.odhip_pipe_metrics_ciede_values(pipe._p()) == 5 * F
        for k in range(2):
            pipe.set_pictures(*_pictures(pw, ph, False, 8, 3, k))
            pipe.step()
            pipe.flush()
            if k == 0:
                m = pipe.metrics_take()
                assert m.ssim is None and m.fastssim is None and not m.sse[0].any() and not m.hvs[1].any()
            else:
                step = ctypes.c_long(-1)
                assert L.odhip_pipe_metrics_take4(pipe._p(), 1, ctypes.byref(step), p(sse), p(hvs), None, None, None) == 1
                assert step.value == 1 and not sse.any()
            pipe.sync()
            if k == 0:
                own = _own_buffers(D, pipe, 8)
                assert np.array_equal(m.ciede.view(np.int64), own.view(np.int64)), (m.ciede, own)
                want = np.array([[45 - 20 * math.log10(v / (pw * ph)) for v in row] for row in own])
                assert np.array_equal(m.ciede_scores(), want)
    finally:
        pipe.destroy()
