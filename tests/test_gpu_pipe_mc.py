"""GPU: inter steps of the frame-batch pipe that build their own prediction from reference frames and motion-vector
grids (odhip_pipe_set_reference_frames / _set_mvs / _feed_reference_frames / _feed_mvs), against the same pipe given
the recorded od_state_mc_predict output through odhip_pipe_set_reference_pictures.  All comparisons are exact.

Picture sizes that are multiples of 64 are the fixtures' CODED sizes (their planes are coded-size planes, so a pipe
of that picture size predicts exactly the recorded frame).  Full precision: the prediction holds 12-bit samples,
which odhip_pipe_set_reference_pictures can hand over unchanged only from 12-bit pictures (fpr_bits 12: 10-bit
pictures are shifted up by 2 and cannot carry a 12-bit prediction).  So the twin comparison runs at fpr_bits 0 and
12; at fpr_bits 10 the pipe's prediction planes are compared with the recorded prediction, and its pyramid,
reconstructions and decisions with a second pipe whose prediction planes were WRITTEN with the recorded samples."""
import os

import numpy as np
import pytest

import _export_check as X
import _mc_ref as R
from _libs import GOLDEN

pytestmark = pytest.mark.gpu

CASES = R.load_cases(os.path.join(GOLDEN, "mc.npz"))


@pytest.fixture(scope="module")
def D():
    import torch
    import daala_amd
    assert torch.cuda.is_available()
    daala_amd.init(0)
    return daala_amd


def group(prefix):
    """The fixture cases of one recorded frame: same reference frames, one grid and prediction each."""
    g = [c for c in CASES if c["name"].startswith(prefix)]
    assert g
    return g


def frames_of(cases):
    """(luma[slot] [F][H][W], chroma[slot] [2F][h][w]): the frame's two reference slots, once per picture."""
    F = len(cases)
    luma = [np.stack([c["refs"][s][0] for c in cases]) for s in range(2)]
    chroma = [np.stack([c["refs"][s][1] for c in cases] + [c["refs"][s][2] for c in cases]) for s in range(2)]
    assert luma[0].shape[0] == F
    return luma, chroma


def preds_of(cases):
    return (np.stack([c["pred"][0] for c in cases]),
            np.stack([c["pred"][1] for c in cases] + [c["pred"][2] for c in cases]))


def sources(pred_l, pred_c, pw, ph, cdec, fpr_bits, seed):
    """Pictures near the prediction (prediction + noise, at the picture depth), cropped to the picture size."""
    rng = np.random.RandomState(seed)
    out = []
    for pred, (w, h) in ((pred_l, (pw, ph)), (pred_c, ((pw + cdec) >> cdec, (ph + cdec) >> cdec))):
        p = pred[:, :h, :w].astype(np.int64)
        if pred.dtype == np.int16:
            p = p >> (12 - fpr_bits)
        top = (1 << (fpr_bits or 8)) - 1
        p = np.clip(p + rng.randint(-12, 13, size=p.shape)*(top + 1 >> 8), 0, top)
        out.append(p.astype(np.int16 if fpr_bits > 8 else np.uint8))
    return out


def snapshot(D, pipe):
    """Every level's reconstruction, choice records and pulses, and the prediction pyramid, as bytes."""
    pipe.sync()
    out = {}
    for s in (0, 1):
        for bs in range(5 if s == 0 else pipe.chroma_levels):
            for what in (D.BUF_RECON, D.BUF_CHOICE, D.BUF_Y, D.BUF_REF):
                out[(s, bs, what)] = pipe.read(what, s, bs).tobytes()
    return out


def run_steps(D, pipe, torch, nsteps=1):
    """nsteps steps with the export ring and the metrics on; returns [(decoded export, sse, hvs)] per step."""
    slots = [torch.zeros(pipe.export_bytes(), dtype=torch.uint8).pin_memory() for _ in range(nsteps + 1)]
    pipe.set_export_ring(slots)
    pipe.set_metrics(sse=True, psnrhvs=True, depth=nsteps + 1)
    return slots


def drain(pipe, n):
    out = []
    for _ in range(n):
        s, buf, ovf = pipe.export_take(wait=True)
        assert ovf == 0
        dec = pipe.decode_export(buf)
        pipe.export_release(s)
        m = pipe.metrics_take(wait=True)
        out.append((dec, [a.copy() for a in m.sse], [a.copy() for a in m.hvs]))
    return out


def same_outputs(a, b):
    assert len(a) == len(b)
    for (da, sa, ha), (db, sb, hb) in zip(a, b):
        assert X.export_diff(da, db) == []
        for i in (0, 1):
            assert np.array_equal(sa[i], sb[i])
            assert np.array_equal(ha[i], hb[i])


TWINS = [("420_8bit_176x120_f2", 0, False), ("444_8bit_128x128_f3", 0, True),
         ("420_fpr_128x128_f3", 12, False), ("444_fpr_72x56_f2", 12, True)]


@pytest.mark.parametrize("prefix,fpr_bits,c444", TWINS, ids=[t[0] + "_fpr%d" % t[1] for t in TWINS])
def test_frames_and_grids_equal_the_recorded_prediction_pictures(D, prefix, fpr_bits, c444):
    import torch
    cases = group(prefix)
    F = len(cases)
    W, H = cases[0]["w"], cases[0]["h"]                 # the coded size as the picture size: a multiple of 64
    cdec = 0 if c444 else 1
    luma, chroma = frames_of(cases)
    pred_l, pred_c = preds_of(cases)
    src_l, src_c = sources(pred_l, pred_c, W, H, cdec, fpr_bits, 5)
    qt = D.QuantTables.load()
    kw = dict(chroma_cfl=True, price=True, inter=True, chroma_444=c444, fpr_bits=fpr_bits)
    a = D.Pipe(qt, F, W, H, **kw)
    b = D.Pipe(qt, F, W, H, **kw)
    try:
        for p in (a, b):
            p.set_pictures(src_l, src_c)
        a.set_reference_frames(luma, chroma)
        a.set_mvs(np.stack([c["grid"] for c in cases]))
        with pytest.raises(D.DaalaHipError):
            a.set_reference_pictures(pred_l, pred_c)   # a step takes its prediction one way
        b.set_reference_pictures(pred_l, pred_c)
        outs = []
        for p in (a, b):
            run_steps(D, p, torch)
            p.step()
            p.flush()
            outs.append(drain(p, 1))
        same_outputs(outs[0], outs[1])
        sa, sb = snapshot(D, a), snapshot(D, b)
        assert sorted(sa) == sorted(sb)
        for key in sa:
            assert sa[key] == sb[key], key
        dt = np.int16 if fpr_bits else np.uint8
        assert np.array_equal(a.read(D.BUF_PRED, 0, dtype=dt).reshape(pred_l.shape), pred_l)
        assert np.array_equal(a.read(D.BUF_PRED, 1, dtype=dt).reshape(pred_c.shape), pred_c)
    finally:
        a.destroy()
        b.destroy()


@pytest.mark.parametrize("prefix,c444", [("420_fpr_128x128_f3", False), ("444_fpr_72x56_f2", True)])
def test_ten_bit_pictures_against_written_prediction_planes(D, prefix, c444):
    cases = group(prefix)
    F = len(cases)
    W, H = cases[0]["w"], cases[0]["h"]
    luma, chroma = frames_of(cases)
    pred_l, pred_c = preds_of(cases)
    src_l, src_c = sources(pred_l, pred_c, W, H, 0 if c444 else 1, 10, 6)
    qt = D.QuantTables.load()
    kw = dict(chroma_cfl=True, price=True, inter=True, chroma_444=c444, fpr_bits=10)
    a = D.Pipe(qt, F, W, H, **kw)
    b = D.Pipe(qt, F, W, H, **kw)
    try:
        a.set_pictures(src_l, src_c)
        a.set_reference_frames(luma, chroma)
        a.set_mvs(np.stack([c["grid"] for c in cases]))
        a.step()
        a.flush()
        assert np.array_equal(a.read(D.BUF_PRED, 0, dtype=np.int16).reshape(pred_l.shape), pred_l)
        assert np.array_equal(a.read(D.BUF_PRED, 1, dtype=np.int16).reshape(pred_c.shape), pred_c)
        # the twin predicts from frames that ARE the recorded prediction, with all-zero vectors: a plain copy
        zero = np.zeros((F,) + cases[0]["grid"].shape, D.MV_POINT)
        zero["valid"][:, ::8, ::8] = 1
        b.set_pictures(src_l, src_c)
        b.set_reference_frames([pred_l], [pred_c])
        b.set_mvs(zero)
        b.step()
        b.flush()
        sa, sb = snapshot(D, a), snapshot(D, b)
        for key in sa:
            assert sa[key] == sb[key], key
    finally:
        a.destroy()
        b.destroy()


def test_size_that_is_no_multiple_of_64_predicts_the_coded_frame(D):
    cases = group("420_8bit_176x120_f4")
    F = len(cases)
    luma, chroma = frames_of(cases)
    pred_l, pred_c = preds_of(cases)
    src_l, src_c = sources(pred_l, pred_c, 176, 120, 1, 0, 7)
    pipe = D.Pipe(D.QuantTables.load(), F, 176, 120, chroma_cfl=True, price=True, inter=True)
    try:
        assert (pipe.W, pipe.H) == (192, 128)
        pipe.set_pictures(src_l, src_c)
        pipe.set_reference_frames(luma, chroma)
        pipe.set_mvs(np.stack([c["grid"] for c in cases]))
        pipe.step()
        pipe.flush()
        assert np.array_equal(pipe.read(D.BUF_PRED, 0).reshape(pred_l.shape), pred_l)
        assert np.array_equal(pipe.read(D.BUF_PRED, 1).reshape(pred_c.shape), pred_c)
        bad = cases[0]["grid"].copy()
        bad["mvx"][0, 0] = -66*8
        with pytest.raises(D.MotionRangeError):
            pipe.feed_mvs(np.stack([bad]*F))
        with pytest.raises(D.MotionRangeError):
            pipe.set_mvs(np.stack([bad]*F))
    finally:
        pipe.destroy()


def test_three_fed_steps_equal_three_drained_single_steps(D):
    import torch
    # per step: another recorded frame's reference frames and another grid
    plan = [group("420_8bit_176x120_f2")[0], group("420_8bit_176x120_f4")[1], group("420_8bit_176x120_f2")[1]]
    qt = D.QuantTables.load()
    kw = dict(chroma_cfl=True, price=True, inter=True)
    pred_l, pred_c = preds_of([plan[0]])
    src_l, src_c = sources(pred_l, pred_c, 176, 120, 1, 0, 8)
    fed = D.Pipe(qt, 1, 176, 120, **kw)
    one = D.Pipe(qt, 1, 176, 120, **kw)
    try:
        # the fed pipe: three steps back to back, frames and grids of step k + 1 fed from pinned memory behind step k
        fed.set_pictures(src_l, src_c)
        run_steps(D, fed, torch, 3)
        pinned = []
        for k, c in enumerate(plan):
            luma, chroma = frames_of([c])
            if k == 0:
                fed.set_reference_frames(luma, chroma)
                fed.set_mvs(c["grid"][None])
            else:
                hl = [torch.from_numpy(x).pin_memory() for x in luma]
                hc = [torch.from_numpy(x).pin_memory() for x in chroma]
                hg = torch.from_numpy(np.frombuffer(c["grid"].tobytes(), np.uint8).copy()).pin_memory()
                pinned.append((hl, hc, hg))
                fed.feed_reference_frames(hl, hc)
                fed.feed_mvs(hg.numpy().view(D.MV_POINT).reshape((1,) + c["grid"].shape))
            fed.step()
        fed.flush()
        got = drain(fed, 3)
        last = snapshot(D, fed)
        # the single steps: set, step, flush, drain - one at a time
        run_steps(D, one, torch, 3)
        one.set_pictures(src_l, src_c)
        want = []
        for c in plan:
            luma, chroma = frames_of([c])
            one.set_reference_frames(luma, chroma)
            one.set_mvs(c["grid"][None])
            one.step()
            one.flush()
            want += drain(one, 1)
            pl, pc = preds_of([c])
            assert np.array_equal(one.read(D.BUF_PRED, 0).reshape(pl.shape), pl)
        same_outputs(got, want)
        ref = snapshot(D, one)
        for key in ref:
            assert last[key] == ref[key], key
    finally:
        fed.destroy()
        one.destroy()


def test_without_a_grid_nothing_is_allocated(D):
    import torch
    cases = group("444_8bit_128x128_f3")[:1]
    pred_l, pred_c = preds_of(cases)
    src_l, src_c = sources(pred_l, pred_c, 128, 128, 0, 0, 9)
    pipe = D.Pipe(D.QuantTables.load(), 1, 128, 128, chroma_cfl=True, price=True, inter=True, chroma_444=True)
    try:
        pipe.set_pictures(src_l, src_c)
        pipe.set_reference_pictures(pred_l, pred_c)
        pipe.step()
        pipe.flush()
        pipe.sync()
        free0 = torch.cuda.mem_get_info()[0]
        for _ in range(3):
            pipe.step()
        pipe.flush()
        pipe.sync()
        assert torch.cuda.mem_get_info()[0] == free0
        before = snapshot(D, pipe)
        # frames alone (no grid) still change nothing about how a step gets its prediction
        luma, chroma = frames_of(cases)
        pipe.set_reference_frames(luma, chroma)
        pipe.step()
        pipe.flush()
        after = snapshot(D, pipe)
        for key in before:
            assert before[key] == after[key], key
    finally:
        pipe.destroy()
