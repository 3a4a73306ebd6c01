"""The decision export as a stream (odhip_pipe_set_export_ring / Pipe.set_export_ring): step s of a pipe lands in ring
slot s % n, the host takes it while later steps run and gives the slot back.

A step taken right after the next one is enqueued, with no sync in between, decodes to exactly the decisions of a
twin pipe drained after every step (step, flush, sync), 4:2:0 and 4:4:4, with the pictures and the quantisers
changing from step to step; bands that the late host-libm resolve re-decides are packed again before their step is
complete (never stale); a full ring refuses the next step without enqueuing anything; bad arguments are refused."""
import ctypes
import os
import sys

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def D():
    import daala_amd
    daala_amd.init(0)
    return daala_amd


def _inputs(F, pw, ph, nsteps, c444, seed=7):
    import torch
    import _export_check as X
    sets = [X.stack([X.pictures(("checker", "natural")[(k + i) % 2], 10 * k + i, seed, pw, ph, c444)
                     for i in range(F)]) for k in range(nsteps)]
    return [tuple(torch.from_numpy(a).pin_memory() for a in s) for s in sets]


def _slots(pipe, n):
    import torch
    return [torch.zeros(pipe.export_bytes(), dtype=torch.uint8).pin_memory() for _ in range(n)]


def _recon(D, pipe):
    return [pipe.read(D.BUF_RECON, s, bs) for s in (0, 1) for bs in range(5 if s == 0 else pipe.chroma_levels)]


def _drained(D, pipe, pinned, tables=None):
    """The twin: step, flush, sync after every step; the dense decisions of each step and the last recon."""
    import _export_check as X
    out = []
    for k, (l, c) in enumerate(pinned):
        if tables is not None:
            pipe.set_quants(tables[k])
        pipe.feed(l, c)
        pipe.step()
        pipe.flush()
        pipe.sync()
        out.append(X.decisions(D, pipe))
    return out, _recon(D, pipe)


def _take(D, pipe, got, wait, expect=None):
    t = pipe.export_take(wait=wait)
    if t is None:
        return False
    step, buf, overflow = t
    assert overflow == 0, (step, overflow)
    if expect is not None:
        assert step == expect, (step, expect)
    assert step not in got
    got[step] = pipe.decode_export(buf)
    pipe.export_release(step)
    return True


@pytest.mark.parametrize("c444", [False, True], ids=["420", "444"])
def test_ring_equals_drained_steps(D, c444):
    import _export_check as X
    F, nsteps = 2, 6
    pw, ph = (177, 121) if c444 else (640, 360)
    qt = D.QuantTables.load()
    q = {v: D.QuantTables.for_quality(v) for v in (5, 10, 20, 40)}
    tables = [[q[5], q[40]], [q[20], q[10]], [q[40], q[5]], [q[10], q[20]], [q[20], q[40]], [q[5], q[10]]]
    pinned = _inputs(F, pw, ph, nsteps, c444)
    kw = dict(chroma_cfl=True, price=True, chroma_444=c444)
    twin = D.Pipe(qt, F, pw, ph, **kw)
    try:
        want, want_recon = _drained(D, twin, pinned, tables)
    finally:
        twin.destroy()
    pipe = D.Pipe(qt, F, pw, ph, **kw)
    try:
        slots = _slots(pipe, 3)
        pipe.set_export_ring(slots)
        got = {}
        for k, (l, c) in enumerate(pinned):
            pipe.set_quants(tables[k])
            pipe.feed(l, c)
            pipe.step()
            if k >= 1:
                # step k - 1 while step k runs: its copies were enqueued by this step
                assert _take(D, pipe, got, True, expect=k - 1)
        assert pipe.export_take(wait=True) is None          # the last step is completed by the flush
        pipe.flush()
        assert _take(D, pipe, got, True, expect=nsteps - 1)
        assert pipe.export_take(wait=False) is None
        pipe.sync()
        assert sorted(got) == list(range(nsteps))
        for k in range(nsteps):
            assert X.export_diff(got[k], want[k]) == [], k
        for a, b in zip(_recon(D, pipe), want_recon):
            assert np.array_equal(a, b)
        assert pipe.export_stale() == 0
        pipe.set_export_ring(None)
    finally:
        pipe.destroy()


def test_late_resolves_are_repacked_without_a_flush(D):
    """Margins forced wide (as tests/test_gpu_pipeline.py::test_export_follows_a_late_resolve does): hundreds of bands
    per step are re-decided one step late, inside the NEXT step.  Steps back to back, each taken once the next one is
    enqueued: every taken step is that step's final decisions (the twin drained under the same hooks)."""
    import _export_check as X
    qt = D.QuantTables.for_quality(40)
    pw, ph, F, nsteps = 312, 180, 1, 5
    pinned = _inputs(F, pw, ph, nsteps, False, seed=5)
    D.pvq_ref_set_theta_margin(0.25, True)
    D.set_price_tol_scale(1e7)
    try:
        twin = D.Pipe(qt, F, pw, ph, chroma_cfl=True, price=True)
        try:
            want, want_recon = _drained(D, twin, pinned)
        finally:
            twin.destroy()
        pipe = D.Pipe(qt, F, pw, ph, chroma_cfl=True, price=True)
        try:
            pipe.set_export_ring(_slots(pipe, 2))
            got = {}
            for k, (l, c) in enumerate(pinned):
                pipe.feed(l, c)
                pipe.step()
                if k >= 1:
                    assert _take(D, pipe, got, True, expect=k - 1)
            pipe.flush()
            assert _take(D, pipe, got, True, expect=nsteps - 1)
            pipe.sync()
            assert pipe.theta_reruns() + pipe.price_reruns() > 50 * nsteps     # the late paths really ran
            for k in range(nsteps):
                assert X.export_diff(got[k], want[k]) == [], k
            for a, b in zip(_recon(D, pipe), want_recon):
                assert np.array_equal(a, b)
            assert pipe.export_stale() == 0
            pipe.set_export_ring(None)
        finally:
            pipe.destroy()
    finally:
        D.pvq_ref_set_theta_margin(0, False)
        D.set_price_tol_scale(1.)


def test_full_ring_refuses_the_step_and_arguments_are_checked(D):
    import torch
    import _export_check as X
    qt = D.QuantTables.load()
    pw, ph, F = 256, 144, 1
    pinned = _inputs(F, pw, ph, 4, False, seed=3)
    twin = D.Pipe(qt, F, pw, ph, chroma_cfl=True, price=True)
    try:
        want, _ = _drained(D, twin, pinned)
    finally:
        twin.destroy()
    L = D.lib()
    pipe = D.Pipe(qt, F, pw, ph, chroma_cfl=True, price=True)
    try:
        slots = _slots(pipe, 2)
        with pytest.raises(D.DaalaHipError):
            pipe.set_export_ring(slots[:1])                         # n < 2
        arr = (ctypes.c_void_p * 2)(slots[0].data_ptr(), None)
        assert L.odhip_pipe_set_export_ring(ctypes.c_void_p(pipe.h), arr, 2) == -10      # a NULL slot
        pipe.set_export_ring(slots)
        assert pipe.export_take(wait=True) is None                 # nothing stepped yet
        with pytest.raises(D.DaalaHipError):
            pipe.set_export(torch.zeros(pipe.export_bytes(), dtype=torch.uint8).pin_memory())
        with pytest.raises(D.DaalaHipError):
            pipe.export_release(0)                                  # not taken
        got = {}
        for k in range(2):
            pipe.feed(*pinned[k])
            pipe.step()
        # both slots hold steps nobody released: the third step is refused and enqueues nothing
        pipe.feed(*pinned[2])
        with pytest.raises(D.ExportRingBusyError):
            pipe.step()
        s0 = pipe.export_take(wait=True)
        assert s0 is not None and s0[0] == 0 and s0[2] == 0
        got[0] = pipe.decode_export(s0[1])
        pipe.flush()
        s1 = pipe.export_take(wait=True)
        assert s1 is not None and s1[0] == 1
        got[1] = pipe.decode_export(s1[1])
        with pytest.raises(D.DaalaHipError):
            pipe.export_release(1)                                  # out of order
        with pytest.raises(D.ExportRingBusyError):
            pipe.step()                                             # still full: step 0 is taken, not released
        pipe.export_release(0)
        pipe.step()                                                 # codes the pictures fed before the refusals
        pipe.export_release(1)
        pipe.feed(*pinned[3])
        pipe.step()
        pipe.flush()
        while _take(D, pipe, got, True):
            pass
        assert sorted(got) == [0, 1, 2, 3]
        for k in range(4):
            assert X.export_diff(got[k], want[k]) == [], k
        assert pipe.export_stale() == 0
        pipe.set_export_ring([])
        with pytest.raises(D.DaalaHipError):
            pipe.export_take()                                      # no ring any more
    finally:
        pipe.destroy()
    noref = D.Pipe(qt, F, pw, ph, chroma_cfl=False, price=True)
    try:
        assert noref.export_bytes() == 0
        arr = (ctypes.c_void_p * 2)(slots[0].data_ptr(), slots[1].data_ptr())
        assert L.odhip_pipe_set_export_ring(ctypes.c_void_p(noref.h), arr, 2) == -23      # does not export
    finally:
        noref.destroy()
