"""FastSSIM of every pipe step (ODHIP_METRIC_FASTSSIM in odhip_pipe_set_metrics4, odhip_pipe_metrics_take4).

F = 2 pictures of 64x64, keyframes with chroma from luma, 4:2:0 and 4:4:4 at 8 bits and 4:2:0 with full-precision
references at 10 bits.  The margins are forced wide (odhip_pipe_set_test_hooks), so that bands of every step are
re-decided one step late, inside the next step or the flush, which runs the inverse and the metrics again:
- the four sums of every (set, level, plane) of the last step equal odhip_fastssim_planes on the pipe's own
  ODHIP_PIPE_BUF_PX / ODHIP_PIPE_BUF_RECON buffers, bit for bit;
- the SSE, HVS, SSIM and MS-SSIM columns of every step equal those of a twin pipe configured through
  odhip_pipe_set_metrics3, whose layout does not report the new bit;
- odhip_pipe_metrics_take3 on the pipe with the flag set still works and returns the twin's columns;
- the scores of PipeMetrics.fastssim_scores are the restatement's product of those sums at the plane sizes, 32x32 for
  4:2:0 chroma;
- the reconstructions and the exported decisions equal the twin's: the bit changes nothing but the column.
FastSSIM alone (flags = 16); odhip_pipe_set_metrics .. set_metrics3 refuse the bit, a ring of one slot and a 64x24
4:2:0 pipe (chroma 32x12) are refused by set_metrics4 and leave the metrics as they were."""
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
    """odhip_fastssim_planes over the pipe's padded source planes and reconstruction levels: (luma [5][F][4], chroma
    [nlev][2F][4]) sums."""
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
        d = torch.zeros((nlev * planes, 4), dtype=torch.float64, device="cuda")
        rc = D.lib().odhip_fastssim_planes(pairs, nlev * planes, ctypes.c_void_p(d.data_ptr()), None)
        assert rc == 0
        torch.cuda.synchronize()
        out.append(d.cpu().numpy().reshape(nlev, planes, 4))
    return out


def _take3(D, pipe, info):
    """odhip_pipe_metrics_take3 of the next step: its number and the four older columns."""
    sse = np.zeros(info.values, np.int64)
    hvs = np.zeros(info.values, np.float64)
    ssim = np.zeros(info.values, np.float64)
    ms = np.zeros((info.values, 5), np.float64)
    step = ctypes.c_long(-1)
    p = lambda a: a.ctypes.data_as(ctypes.c_void_p)
    rc = D.lib().odhip_pipe_metrics_take3(pipe._p(), 1, ctypes.byref(step), p(sse), p(hvs), p(ssim), p(ms))
    assert rc == 1
    return step.value, sse, hvs, ssim, ms


def _run(D, c444, fpr_bits, fast):
    """Three steps in flight (each resolved late, inside the next step or the flush), then a fourth taken with take3."""
    import torch
    depth = fpr_bits or 8
    qt = D.QuantTables.for_quality(40)
    inputs = [tuple(torch.from_numpy(a).pin_memory() for a in _pictures(PW, PH, c444, depth, 21, k)) for k in range(4)]
    pipe = D.Pipe(qt, F, PW, PH, chroma_cfl=True, price=True, chroma_444=c444, fpr_bits=fpr_bits)
    try:
        if fast:
            pipe.set_metrics(ssim=True, msssim=True, fastssim=True)
        else:
            assert D.lib().odhip_pipe_set_metrics3(pipe._p(), 15, 2) == 0
        info = pipe.metrics_layout()
        assert info.flags == (31 if fast else 15)
        got = []
        for k in range(3):
            pipe.feed(*inputs[k])
            pipe.step()
            if k >= 1:
                got.append(pipe.metrics_take())
        pipe.flush()
        got.append(pipe.metrics_take())
        pipe.sync()
        assert [m.step for m in got] == [0, 1, 2]
        reruns = pipe.theta_reruns() + pipe.price_reruns()
        own = _own_buffers(D, pipe, depth) if fast else None
        host = torch.zeros(pipe.export_bytes(), dtype=torch.uint8).pin_memory()
        pipe.set_export(host)
        pipe.feed(*inputs[3])
        pipe.step()
        pipe.flush()
        last = _take3(D, pipe, info)
        assert last[0] == 3 and pipe.metrics_take(wait=False) is None
        pipe.sync()
        recon = [pipe.read(D.BUF_RECON, si, bs) for si in (0, 1) for bs in range(5 if si == 0 else pipe.chroma_levels)]
        export = pipe.decode_export(host.numpy())
        pipe.set_export(None)
        return got, own, last, recon, export, reruns
    finally:
        pipe.destroy()


@pytest.mark.parametrize("c444,fpr_bits", [(False, 0), (True, 0), (False, 10)], ids=["420", "444", "420-fpr10"])
def test_take4_equals_fastssim_planes_and_leaves_the_rest_alone(D, c444, fpr_bits):
    D.pvq_ref_set_theta_margin(0.25, True)
    D.set_price_tol_scale(1e7)
    try:
        got, own, last, recon, export, reruns = _run(D, c444, fpr_bits, True)
        twin, _, tlast, trecon, texport, _ = _run(D, c444, fpr_bits, False)
    finally:
        D.pvq_ref_set_theta_margin(0, False)
        D.set_price_tol_scale(1.)
    print("late reruns %d" % reruns)
    assert reruns > 0                                                  # the late paths really ran
    cdec = 0 if c444 else 1
    for m, t in zip(got, twin):
        assert m.fastssim is not None and t.fastssim is None
        assert m.fastssim_sizes == ((PW, PH), ((PW + cdec) >> cdec, (PH + cdec) >> cdec))
        for si in (0, 1):
            # the older columns are the twin's
            assert np.array_equal(m.sse[si], t.sse[si])
            assert np.array_equal(m.hvs[si].view(np.int64), t.hvs[si].view(np.int64))
            assert np.array_equal(m.ssim[si].view(np.int64), t.ssim[si].view(np.int64))
            assert np.array_equal(m.msssim[si].view(np.int64), t.msssim[si].view(np.int64))
            assert m.fastssim[si].shape == m.sse[si].shape + (4,)
            raw = m.fastssim_scores(raw=True)[si]
            assert raw.shape == m.sse[si].shape and ((raw > 0) & (raw <= 1)).all()
            assert not np.isnan(m.fastssim_scores()[si]).any()           # dB; inf where a plane came back exactly
    # the last step in flight, measured again by its late resolve: the pipe's own buffers
    for si in (0, 1):
        assert np.array_equal(got[-1].fastssim[si].view(np.int64), own[si].view(np.int64)), (si, got[-1].fastssim[si], own[si])
    # its scores are the restatement's product of the own-buffer sums at the plane sizes written out here, not taken
    # from the pipe: 64 x 64 luma, 32 x 32 chroma at 4:2:0 (the level sizes differ, so a wrong size gives other scores)
    import _fastssim_ref as S
    sizes = ((64, 64), (64, 64) if c444 else (32, 32))
    raw = got[-1].fastssim_scores(raw=True)
    for si in (0, 1):
        want = np.array([[S.score(own[si][bs, pl], *sizes[si]) for pl in range(own[si].shape[1])]
                         for bs in range(own[si].shape[0])])
        assert np.array_equal(raw[si].view(np.int64), want.view(np.int64)), (si, raw[si], want)
    if not c444:
        other = S.score(own[1][0, 0], 64, 64)
        assert other != raw[1][0, 0]                                   # the check above can tell the sizes apart
    # take3 on the pipe with the flag set: the twin's columns
    for a, b in zip(last[1:], tlast[1:]):
        assert a.any() and np.array_equal(a.view(np.int64), b.view(np.int64))
    # nothing but the column differs
    assert len(recon) == len(trecon) and all(np.array_equal(a, b) for a, b in zip(recon, trecon))
    assert set(export) == set(texport) and len(export) > 0
    for key in export:
        for a, b in zip(export[key], texport[key]):
            assert np.array_equal(a, b), key


def test_fastssim_alone_and_bad_arguments(D):
    pipe = D.Pipe(D.QuantTables.load(), F, PW, PH, chroma_cfl=True, price=True)
    L = D.lib()
    try:
        assert L.odhip_pipe_set_metrics4(pipe._p(), 32, 2) == -10             # unknown flag
        assert L.odhip_pipe_set_metrics4(pipe._p(), 16, 1) == -10             # a ring of one slot
        for flags in (16, 17, 31):
            assert L.odhip_pipe_set_metrics(pipe._p(), flags, 2) == -10       # the older entry points keep their flags
            assert L.odhip_pipe_set_metrics2(pipe._p(), flags, 2) == -10
            assert L.odhip_pipe_set_metrics3(pipe._p(), flags, 2) == -10
        assert pipe.metrics_layout().flags == 0
        pipe.set_metrics(sse=False, psnrhvs=False, fastssim=True)
        assert pipe.metrics_layout().flags == D.METRIC_FASTSSIM == 16
        pipe.set_pictures(*_pictures(PW, PH, False, 8, 3))
        pipe.step()
        pipe.flush()
        m = pipe.metrics_take()
        pipe.sync()
        own = _own_buffers(D, pipe, 8)
        assert m.ssim is None and m.msssim is None
        for si in (0, 1):
            assert np.array_equal(m.fastssim[si].view(np.int64), own[si].view(np.int64))
            assert not m.sse[si].any() and not m.hvs[si].any()
    finally:
        pipe.destroy()
    # 4:2:0 chroma of 64 x 24 is 32 x 12: below the floor
    small = D.Pipe(D.QuantTables.load(), F, 64, 24, chroma_cfl=True, price=True)
    try:
        small.set_metrics()
        assert L.odhip_pipe_set_metrics4(small._p(), 19, 2) == -10
        assert L.odhip_pipe_set_metrics4(small._p(), 16, 2) == -10
        assert small.metrics_layout().flags == 3                             # as they were
        small.set_pictures(*_pictures(64, 24, False, 8, 3))
        small.step()
        small.flush()
        m = small.metrics_take()
        small.sync()
        assert m.step == 0 and m.sse[0].any() and m.fastssim is None
    finally:
        small.destroy()
