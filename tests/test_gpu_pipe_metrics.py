"""The metrics of every pipe step (odhip_pipe_set_metrics / Pipe.set_metrics, metrics_take).

- Parity: for each mode the taken values equal the CPU restatement (tests/_metrics_ref.py) of the reconstruction
  levels read back with odhip_pipe_read against the source pictures - every level and plane, SSE exact, the
  PSNR-HVS-M sum within 1e-9 relative.
- Ladder: one natural picture at rising quantisers (set_quants) loses PSNR at every step up.
- Streaming: fed steps with the export ring, taken while later steps run, equal a drained (step, flush, sync) twin;
  a full metrics ring refuses the step (ODHIP_EBUSY); forced late resolves measure again, also without pricing, where
  they re-run the choice kernel.
- Off by default: reconstructions, exports and stage counts are those of a pipe that never called set_metrics.
- Bad arguments are refused and leave the pipe usable."""
import ctypes
import os
import sys

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def D():
    import daala_amd
    daala_amd.init(0)
    return daala_amd


def _pictures(F, pw, ph, c444, depth, seed, k=0):
    import _export_check as X
    luma, chroma = X.stack([X.pictures(("natural", "checker")[(i + k) % 2], 10 * k + i, seed, pw, ph, c444)
                            for i in range(F)])
    if depth > 8:
        rng = np.random.RandomState(seed + k)
        up = lambda a: ((a.astype(np.int32) << (depth - 8))
                        + rng.randint(0, 1 << (depth - 8), size=a.shape)).astype(np.int16)
        return up(luma), up(chroma)
    return luma, chroma


def _check(D, pipe, m, luma, chroma, depth):
    """The taken metrics m == the restatement over the recon levels the pipe holds now."""
    import _metrics_ref as M
    fpr = pipe.fpr_bits != 0
    for si, pics in ((0, luma), (1, chroma)):
        dec = 1 if si and not pipe.chroma_444 else 0
        W, H = pipe.W >> dec, pipe.H >> dec
        nlev = 5 if si == 0 else pipe.chroma_levels
        for bs in range(nlev):
            rec = pipe.read(D.BUF_RECON, si, bs, dtype=np.int16 if fpr else np.uint8).reshape(len(pics), H, W)
            for pl in range(len(pics)):
                src = pics[pl].astype(np.int32)
                r = rec[pl, :src.shape[0], :src.shape[1]]
                r = M.to_depth(r, depth) if fpr else r.astype(np.int32)
                csf = 0 if si == 0 else (1 if pl < pipe.frames else 2)
                assert m.sse[si][bs, pl] == M.sse(src, r), (si, bs, pl)
                want = M.hvs_sum(src, r, csf)
                assert abs(m.hvs[si][bs, pl] - want) <= 1e-9 * want, (si, bs, pl, m.hvs[si][bs, pl], want)


MODES = {
    "420_cfl_priced": dict(size=(256, 144), kw=dict(chroma_cfl=True, price=True)),
    "444_odd": dict(size=(177, 121), kw=dict(chroma_cfl=True, price=True, chroma_444=True)),
    "no_cfl": dict(size=(192, 128), kw=dict(chroma_cfl=False, price=True)),
    "inter": dict(size=(192, 128), kw=dict(inter=True, price=True)),
    "fpr10": dict(size=(192, 128), kw=dict(chroma_cfl=True, price=True, fpr_bits=10)),
    "fpr12": dict(size=(192, 128), kw=dict(chroma_cfl=True, price=True, fpr_bits=12)),
}


@pytest.mark.parametrize("mode", sorted(MODES))
def test_parity(D, mode):
    spec = MODES[mode]
    pw, ph = spec["size"]
    kw = spec["kw"]
    F = 2
    depth = kw.get("fpr_bits", 0) or 8
    c444 = kw.get("chroma_444", False)
    qt = D.QuantTables.load()
    pipe = D.Pipe(qt, F, pw, ph, **kw)
    try:
        pipe.set_metrics(depth=2)
        info = pipe.metrics_layout()
        assert (info.luma_planes, info.chroma_planes, info.depth) == (F, 2 * F, depth)
        assert info.values == 5 * F + pipe.chroma_levels * 2 * F
        for k in range(2):
            luma, chroma = _pictures(F, pw, ph, c444, depth, 3, k)
            pipe.set_pictures(luma, chroma)
            if kw.get("inter"):
                pl, pc = _pictures(F, pw, ph, c444, depth, 9, k)
                pipe.set_reference_pictures(pl, pc)
            pipe.step()
            pipe.flush()
            m = pipe.metrics_take(wait=True)
            assert m is not None and m.step == k
            assert pipe.metrics_take(wait=False) is None
            pipe.sync()
            _check(D, pipe, m, luma, chroma, depth)
            psnr, hvs = m.psnr(), m.psnrhvs()
            assert np.isfinite(psnr[0]).all() and (psnr[0] > 20).all() and np.isfinite(hvs[1]).all()
    finally:
        pipe.destroy()


def test_quality_ladder(D):
    qs = [5, 10, 20, 40, 100]
    F, pw, ph = len(qs), 320, 192
    import _export_check as X
    pic = X.pictures("natural", 0, 4, pw, ph)
    luma, chroma = X.stack([pic] * F)
    pipe = D.Pipe(D.QuantTables.load(), F, pw, ph, chroma_cfl=True, price=True)
    try:
        pipe.set_quants([D.QuantTables.for_quality(q) for q in qs])
        pipe.set_metrics()
        pipe.set_pictures(luma, chroma)
        pipe.step()
        pipe.flush()
        m = pipe.metrics_take()
        pipe.sync()
        for si in (0, 1):
            psnr = m.psnr()[si]                                  # [levels][planes]
            planes = psnr.reshape(psnr.shape[0], -1, F) if si else psnr[:, None, :]
            assert (np.diff(planes, axis=2) < 0).all(), (si, planes)
        assert (np.diff(m.psnrhvs()[0], axis=1) < 0).all()
    finally:
        pipe.destroy()


def _drained(D, pipe, inputs, tables=None):
    out = []
    for k, (l, c) in enumerate(inputs):
        if tables is not None:
            pipe.set_quants(tables[k])
        pipe.feed(l, c)
        pipe.step()
        pipe.flush()
        m = pipe.metrics_take()
        pipe.sync()
        assert m.step == k
        out.append(m)
    return out


def _same(a, b):
    for i in (0, 1):
        assert np.array_equal(a.sse[i], b.sse[i])
        assert np.array_equal(a.hvs[i].view(np.int64), b.hvs[i].view(np.int64))


def _pinned(F, pw, ph, n, c444=False):
    import torch
    return [tuple(torch.from_numpy(a).pin_memory() for a in _pictures(F, pw, ph, c444, 8, 21, k)) for k in range(n)]


@pytest.mark.parametrize("c444", [False, True], ids=["420", "444"])
def test_streamed_steps_equal_drained_steps(D, c444):
    import torch
    F, n = 2, 5
    pw, ph = (177, 121) if c444 else (256, 144)
    qt = D.QuantTables.load()
    q = {v: D.QuantTables.for_quality(v) for v in (5, 20, 40)}
    tables = [[q[5], q[40]], [q[20], q[5]], [q[40], q[20]], [q[5], q[5]], [q[20], q[40]]]
    inputs = _pinned(F, pw, ph, n, c444)
    kw = dict(chroma_cfl=True, price=True, chroma_444=c444)
    twin = D.Pipe(qt, F, pw, ph, **kw)
    try:
        twin.set_metrics()
        want = _drained(D, twin, inputs, tables)
    finally:
        twin.destroy()
    pipe = D.Pipe(qt, F, pw, ph, **kw)
    try:
        pipe.set_export_ring([torch.zeros(pipe.export_bytes(), dtype=torch.uint8).pin_memory() for _ in range(3)])
        pipe.set_metrics(depth=3)
        got = {}
        for k, (l, c) in enumerate(inputs):
            pipe.set_quants(tables[k])
            pipe.feed(l, c)
            pipe.step()
            if k >= 1:
                e = pipe.export_take()
                assert e is not None and e[0] == k - 1
                pipe.export_release(e[0])
                m = pipe.metrics_take()
                assert m is not None and m.step == k - 1
                got[m.step] = m
        assert pipe.metrics_take(wait=True) is None          # the last step is completed by the flush
        pipe.flush()
        m = pipe.metrics_take()
        got[m.step] = m
        pipe.sync()
        assert sorted(got) == list(range(n))
        for k in range(n):
            _same(got[k], want[k])
    finally:
        pipe.destroy()


def test_full_ring_refuses_the_step(D):
    F, pw, ph = 1, 192, 128
    inputs = _pinned(F, pw, ph, 4)
    qt = D.QuantTables.load()
    twin = D.Pipe(qt, F, pw, ph, chroma_cfl=True, price=True)
    try:
        twin.set_metrics()
        want = _drained(D, twin, inputs)
    finally:
        twin.destroy()
    pipe = D.Pipe(qt, F, pw, ph, chroma_cfl=True, price=True)
    try:
        pipe.set_metrics(depth=2)
        for k in range(2):
            pipe.feed(*inputs[k])
            pipe.step()
        pipe.feed(*inputs[2])
        with pytest.raises(D.ExportRingBusyError):
            pipe.step()                                        # both slots hold untaken steps: nothing enqueued
        got = [pipe.metrics_take()]
        pipe.step()                                            # the pictures fed before the refusal
        got.append(pipe.metrics_take())
        pipe.feed(*inputs[3])
        pipe.step()
        pipe.flush()
        while True:
            m = pipe.metrics_take()
            if m is None:
                break
            got.append(m)
        pipe.sync()
        assert [m.step for m in got] == [0, 1, 2, 3]
        for k in range(4):
            _same(got[k], want[k])
    finally:
        pipe.destroy()


@pytest.mark.parametrize("inter", [False, True], ids=["cfl", "inter"])
def test_late_resolves_measure_again(D, inter):
    """Margins forced wide: many bands of every step are re-decided one step late, inside the next step; the values
    taken after that step equal the drained twin's, and the last step's equal the restatement of its final recon."""
    qt = D.QuantTables.for_quality(40)
    F, pw, ph, n = 1, 256, 144, 4
    inputs = _pinned(F, pw, ph, n)
    refs = _pictures(F, pw, ph, False, 8, 9)
    kw = dict(inter=True, price=True) if inter else dict(chroma_cfl=True, price=True)
    D.pvq_ref_set_theta_margin(0.25, True)
    D.set_price_tol_scale(1e7)
    try:
        twin = D.Pipe(qt, F, pw, ph, **kw)
        try:
            if inter:
                twin.set_reference_pictures(*refs)
            twin.set_metrics()
            want = _drained(D, twin, inputs)
        finally:
            twin.destroy()
        pipe = D.Pipe(qt, F, pw, ph, **kw)
        try:
            if inter:
                pipe.set_reference_pictures(*refs)
            pipe.set_metrics(depth=2)
            got = []
            for k, (l, c) in enumerate(inputs):
                pipe.feed(l, c)
                pipe.step()
                if k >= 1:
                    got.append(pipe.metrics_take())
            pipe.flush()
            got.append(pipe.metrics_take())
            pipe.sync()
            assert pipe.theta_reruns() + pipe.price_reruns() > 0      # the late paths really ran
            assert [m.step for m in got] == list(range(n))
            for k in range(n):
                _same(got[k], want[k])
            l, c = (t.numpy() for t in inputs[-1])
            _check(D, pipe, got[-1], l, c, 8)
        finally:
            pipe.destroy()
    finally:
        D.pvq_ref_set_theta_margin(0, False)
        D.set_price_tol_scale(1.)


def _decisions_and_recon(D, pipe):
    return {(what, si, bs): pipe.read(what, si, bs).copy()
            for what in (D.BUF_RECON, D.BUF_CHOICE, D.BUF_Y)
            for si in (0, 1) for bs in range(5 if si == 0 else pipe.chroma_levels)}


@pytest.mark.parametrize("inter", [False, True], ids=["cfl", "inter"])
def test_unpriced_late_resolves_rerun_the_choice(D, inter):
    """price=False: the late resolve of a with-reference chain re-runs the choice KERNEL (a priced step has none)
    before the inverse.  Margin forced wide, device theta of listed bands off by one; three fed steps and a flush
    against a twin driven step, flush, sync, byte for byte over every BUF_RECON, BUF_CHOICE and BUF_Y of both plane sets.
    What a pipe holds right after step k is final only where no resolve is pending (keyframe luma); a plane set whose
    resolve is pending holds the provisional decisions, which the next step overwrites behind the resolve.  So after
    each step the buffers are compared with the twin's read at the same moment (between its step and its flush; for
    final sets that is the twin's final state), after the flush with the twin's final state, and the re-decided steps
    in between are pinned through their metrics: the tail re-run inside the NEXT step measures the twin's values."""
    qt = D.QuantTables.for_quality(40)
    F, pw, ph, n = 1, 256, 144, 3
    inputs = _pinned(F, pw, ph, n)
    refs = _pictures(F, pw, ph, False, 8, 9)
    kw = dict(inter=True, price=False) if inter else dict(chroma_cfl=True, price=False)
    final_sets = () if inter else (0,)
    D.pvq_ref_set_theta_margin(0.25, True)
    try:
        twin = D.Pipe(qt, F, pw, ph, **kw)
        try:
            if inter:
                twin.set_reference_pictures(*refs)
            twin.set_metrics()
            before, after, want = [], [], []
            for k, (l, c) in enumerate(inputs):
                twin.feed(l, c)
                twin.step()
                before.append(_decisions_and_recon(D, twin))
                twin.flush()
                want.append(twin.metrics_take())
                twin.sync()
                after.append(_decisions_and_recon(D, twin))
                for key in before[k]:
                    if key[1] in final_sets:
                        assert np.array_equal(before[k][key], after[k][key]), (k, key)
        finally:
            twin.destroy()
        pipe = D.Pipe(qt, F, pw, ph, **kw)
        try:
            if inter:
                pipe.set_reference_pictures(*refs)
            pipe.set_metrics(depth=2)
            got = []
            for k, (l, c) in enumerate(inputs):
                pipe.feed(l, c)
                pipe.step()
                if k >= 1:
                    got.append(pipe.metrics_take())
                now = _decisions_and_recon(D, pipe)
                for key in now:
                    assert np.array_equal(now[key], before[k][key]), (k, key)
            pipe.flush()
            got.append(pipe.metrics_take())
            pipe.sync()
            print("theta reruns %d, listed %d" % (pipe.theta_reruns(), pipe.theta_listed()))
            assert pipe.theta_reruns() > 0                            # the late path really ran
            now = _decisions_and_recon(D, pipe)
            for key in now:
                assert np.array_equal(now[key], after[-1][key]), ("flushed", key)
            assert [m.step for m in got] == list(range(n))
            for k in range(n):
                _same(got[k], want[k])
        finally:
            pipe.destroy()
    finally:
        D.pvq_ref_set_theta_margin(0, False)


def test_off_by_default(D):
    import torch
    import _export_check as X
    F, pw, ph = 2, 256, 144
    inputs = _pinned(F, pw, ph, 3)
    qt = D.QuantTables.load()
    runs = []
    for how in ("never", "off", "on"):
        pipe = D.Pipe(qt, F, pw, ph, chroma_cfl=True, price=True)
        try:
            if how == "off":
                pipe.set_metrics()
                pipe.set_metrics(sse=False, psnrhvs=False)
            elif how == "on":
                pipe.set_metrics(depth=4)
            slot = torch.zeros(pipe.export_bytes(), dtype=torch.uint8).pin_memory()
            pipe.set_export(slot)
            pipe.record(True)
            digests = []
            for l, c in inputs:
                pipe.feed(l, c)
                pipe.step()
                pipe.flush()
                pipe.sync()
                digests.append([pipe.read(D.BUF_RECON, s, b).tobytes() for s in (0, 1) for b in range(5 - s)])
                digests.append(X.export_diff(pipe.decode_export(slot.numpy()), X.decisions(D, pipe)))
            counts = {k: v[1] for k, v in pipe.timings().items()}
            if how != "on":
                with pytest.raises(D.DaalaHipError):
                    pipe.metrics_take()
            runs.append((digests, counts))
        finally:
            pipe.destroy()
    assert runs[0][0] == runs[1][0] == runs[2][0]
    assert runs[0][1] == runs[1][1] == runs[2][1]


def test_bad_arguments_leave_the_pipe_usable(D):
    F, pw, ph = 1, 128, 64
    qt = D.QuantTables.load()
    pipe = D.Pipe(qt, F, pw, ph, chroma_cfl=True, price=True)
    L = D.lib()
    h = ctypes.c_void_p(pipe.h)
    try:
        assert L.odhip_pipe_set_metrics(h, 4, 2) == -10                  # unknown flag
        assert L.odhip_pipe_set_metrics(h, 3, 1) == -10                  # a ring of one slot
        assert L.odhip_pipe_set_metrics(h, -1, 2) == -10
        step = ctypes.c_long()
        assert L.odhip_pipe_metrics_take(h, 1, ctypes.byref(step), None, None) == -10     # metrics off
        assert L.odhip_pipe_metrics_layout(h, None) == -10
        assert L.odhip_pipe_metrics_counts(h, None, None) == -10
        luma, chroma = _pictures(F, pw, ph, False, 8, 2)
        pipe.set_pictures(luma, chroma)
        pipe.step()
        pipe.set_metrics(sse=True, psnrhvs=False)
        assert L.odhip_pipe_metrics_take(h, 1, None, None, None) == -10                  # no step pointer
        pipe.step()
        pipe.flush()
        m = pipe.metrics_take()
        pipe.sync()
        assert m.step == 0 and (m.sse[0] > 0).all() and not m.hvs[0].any()
        _check_sse_only(D, pipe, m, luma, chroma)
    finally:
        pipe.destroy()


def _check_sse_only(D, pipe, m, luma, chroma):
    import _metrics_ref as M
    for si, pics in ((0, luma), (1, chroma)):
        dec = 0 if si == 0 else 1
        W, H = pipe.W >> dec, pipe.H >> dec
        for bs in range(5 if si == 0 else pipe.chroma_levels):
            rec = pipe.read(D.BUF_RECON, si, bs).reshape(len(pics), H, W)
            for pl in range(len(pics)):
                p = pics[pl]
                assert m.sse[si][bs, pl] == M.sse(p, rec[pl, :p.shape[0], :p.shape[1]])
