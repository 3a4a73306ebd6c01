"""Inter steps export their decisions (odhip_pipe_config.inter with price = 1): every plane of an inter step is coded
against its prediction, so the export holds 9 (4:2:0) or 10 (4:4:4) sections of 8-byte records, luma 64x64 included.

Through the single buffer and through the ring the decoded export is the dense inter buffers - gain index, theta, its
range, the skip and no-reference flags, K of the coded bands and every pulse - and the compiled reference's
decisions; with the late resolves forced, every taken step is that step's final decisions."""
import os
import sys

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from _libs import ref  # noqa: E402

pytestmark = pytest.mark.gpu
needs_ref = pytest.mark.skipif(ref() is None, reason="oracle/_ref (the compiled reference) not present")


@pytest.fixture(scope="module")
def D():
    import daala_amd
    daala_amd.init(0)
    return daala_amd


def _frame(pw, ph, c444, index, seed=3, noise=6):
    """[Y, Cb, Cr] of one picture and its prediction - the scene of the previous index shifted by one sample with a
    little noise (tests/test_gpu_pipeline.py::test_inter_frame_step_equals_compiled_reference)."""
    import _export_check as X
    rng = np.random.RandomState(4 + index)
    cur = X.pictures("natural", 8 + index, seed, pw, ph, c444)
    prev = X.pictures("natural", 7 + index, seed, pw, ph, c444)
    pred = [np.clip(np.roll(p.astype(np.int32), 1, axis=1) + rng.randint(-noise, noise + 1, size=p.shape), 0, 255)
            .astype(np.uint8) for p in prev]
    return cur, pred


def _check_layout(pipe, c444):
    lay = pipe.export_layout()
    n = 10 if c444 else 9
    assert lay["nsections"] == n and pipe.export_bytes() == lay["total_bytes"]
    assert [s["record_bytes"] for s in lay["sections"]] == [8] * n
    assert [s["bs"] for s in lay["sections"]] == list(range(5)) + list(range(n - 5))
    return lay


def _check_flags(D, pipe, host, lay):
    import _export_check as X
    got = X.export_flags(host, lay)
    want = X.dense_flags(D, pipe)
    assert sorted(got) == sorted(want) == list(range(lay["nsections"]))
    for si in want:
        assert np.array_equal(got[si][0], want[si][0]), (si, "noref")
        assert np.array_equal(got[si][1], want[si][1]), (si, "skip")


@pytest.mark.parametrize("size", [(312, 180, False), (1920, 1080, False), (177, 121, True)],
                         ids=["420-312x180", "420-1080p", "444-177x121"])
def test_inter_export_is_the_device_buffers(D, size):
    import torch
    import _export_check as X
    pw, ph, c444 = size
    F, nsteps = 1, 3
    qt = D.QuantTables.for_quality(20)
    frames = [_frame(pw, ph, c444, k) for k in range(nsteps)]
    pinned = [tuple(torch.from_numpy(a).pin_memory() for a in X.stack([f[0]])) for f in frames]
    kw = dict(chroma_cfl=True, price=True, inter=True, chroma_444=c444)
    legacy = D.Pipe(qt, F, pw, ph, **kw)
    ring = D.Pipe(qt, F, pw, ph, **kw)
    try:
        lay = _check_layout(legacy, c444)
        assert ring.export_layout() == lay
        # one prediction for every step, the current pictures fed step by step
        for p in (legacy, ring):
            p.set_pictures(*X.stack([frames[0][0]]))
            p.set_reference_pictures(*X.stack([frames[0][1]]))
        host = torch.zeros(legacy.export_bytes(), dtype=torch.uint8).pin_memory()
        legacy.set_export(host)
        want = []
        for k in range(nsteps):
            legacy.feed(*pinned[k])
            legacy.step()
            legacy.flush()
            legacy.sync()
            dense = X.decisions(D, legacy)
            got = legacy.decode_export(host.numpy())
            assert X.export_diff(got, dense) == [], ("single buffer", k)
            _check_flags(D, legacy, host.numpy(), lay)
            shipped = legacy.export_shipped_bytes(host.numpy())
            assert shipped < sum(y.size * 2 for y, _, _ in dense.values()) / 2
            want.append(dense)
        assert legacy.export_stale() == 0
        legacy.set_export(None)
        slots = [torch.zeros(ring.export_bytes(), dtype=torch.uint8).pin_memory() for _ in range(2)]
        ring.set_export_ring(slots)
        got = {}
        for k in range(nsteps):
            ring.feed(*pinned[k])
            ring.step()
            if k >= 1:
                s, buf, ovf = ring.export_take(wait=True)
                assert (s, ovf) == (k - 1, 0)
                got[s] = ring.decode_export(buf)
                ring.export_release(s)
        ring.flush()
        s, buf, ovf = ring.export_take(wait=True)
        assert (s, ovf) == (nsteps - 1, 0)
        got[s] = ring.decode_export(buf)
        # the last slot is still the device's last step: the flags too
        ring.sync()
        _check_flags(D, ring, buf, lay)
        ring.export_release(s)
        for k in range(nsteps):
            assert X.export_diff(got[k], want[k]) == [], ("ring", k)
        assert ring.export_stale() == 0
        ring.set_export_ring(None)
    finally:
        legacy.destroy()
        ring.destroy()
    # keyframes without chroma from luma and unpriced pipes still do not export
    for kw in (dict(chroma_cfl=False, price=True), dict(inter=True, price=False)):
        p = D.Pipe(qt, 1, 64, 64, **kw)
        try:
            assert p.export_bytes() == 0
        finally:
            p.destroy()


def _ref_diff(got, want, c444, frame=0, frames=1):
    """The decoded export of picture `frame` against the reference's decisions (cpu_frame / cpu_frame444): gain index,
    theta and its range of every band, K and the pulses of the coded ones."""
    bad = []
    import daala_amd as D
    for pli in range(3):
        s = 1 if pli else 0
        plane = frame if pli == 0 else (pli - 1) * frames + frame
        assert len(want[pli]) == (5 if pli == 0 or c444 else 4)
        for bs, (yc, bc) in enumerate(want[pli]):
            yg, bg, coded = got[(s, bs)]
            per = yc.shape[0]
            sl = slice(plane * per, (plane + 1) * per)
            yg, bg, coded = yg[sl], bg[sl], coded[sl]
            if not np.array_equal(bg[..., :3], bc[..., :3]):
                bad.append((pli, bs, "gain index / theta / max_theta"))
            if not np.array_equal(bg[..., 3][coded], bc[..., 3][coded]):
                bad.append((pli, bs, "K"))
            nb, offs, _ = D.pvq_band_layout(bs)
            for i in range(nb):
                on = coded[:, i]
                if not np.array_equal(yg[on, offs[i]:offs[i + 1]], yc[on, offs[i]:offs[i + 1]]):
                    bad.append((pli, bs, "y[band %d]" % i))
    return bad


@needs_ref
@pytest.mark.parametrize("size", [(312, 180, False), (177, 121, True)], ids=["420", "444"])
def test_inter_export_equals_compiled_reference(D, size):
    import torch
    import _export_check as X
    pw, ph, c444 = size
    qt = D.QuantTables.for_quality(40)
    cur, pred = _frame(pw, ph, c444, 0)
    want = []
    if c444:
        import _pipe444_check as C4
        C4.cpu_frame444(qt, cur, pw, ph, inter_pred=pred, decisions=want)
    else:
        import _pipeline_check as C
        C.cpu_frame(qt, cur, pw, ph, inter_pred=pred, decisions=want)
    pipe = D.Pipe(qt, 1, pw, ph, chroma_cfl=True, price=True, inter=True, chroma_444=c444)
    try:
        pipe.set_pictures(*X.stack([cur]))
        pipe.set_reference_pictures(*X.stack([pred]))
        pipe.set_export_ring([torch.zeros(pipe.export_bytes(), dtype=torch.uint8).pin_memory() for _ in range(2)])
        for k in range(3):
            pipe.step()
            if k >= 1:
                s, buf, _ = pipe.export_take(wait=True)
                assert _ref_diff(pipe.decode_export(buf), want, c444) == [], s
                pipe.export_release(s)
        pipe.flush()
        s, buf, _ = pipe.export_take(wait=True)
        assert _ref_diff(pipe.decode_export(buf), want, c444) == [], s
        pipe.export_release(s)
        pipe.set_export_ring(None)
    finally:
        pipe.destroy()


def test_inter_late_resolves_through_the_ring(D):
    import torch
    import _export_check as X
    pw, ph, nsteps = 312, 180, 4
    qt = D.QuantTables.for_quality(40)
    frames = [_frame(pw, ph, False, k) for k in range(nsteps)]
    pinned = [tuple(torch.from_numpy(a).pin_memory() for a in X.stack([f[0]])) for f in frames]
    D.pvq_ref_set_theta_margin(0.25, True)
    D.set_price_tol_scale(1e7)
    pipes = []
    try:
        twin = D.Pipe(qt, 1, pw, ph, price=True, inter=True)
        ring = D.Pipe(qt, 1, pw, ph, price=True, inter=True)
        pipes += [twin, ring]
        for p in pipes:
            p.set_pictures(*X.stack([frames[0][0]]))
            p.set_reference_pictures(*X.stack([frames[0][1]]))
        want = []
        for k in range(nsteps):
            twin.feed(*pinned[k])
            twin.step()
            twin.flush()
            twin.sync()
            want.append(X.decisions(D, twin))
        ring.set_export_ring([torch.zeros(ring.export_bytes(), dtype=torch.uint8).pin_memory() for _ in range(3)])
        got = {}
        for k in range(nsteps):
            ring.feed(*pinned[k])
            ring.step()
            if k >= 1:
                s, buf, _ = ring.export_take(wait=True)
                got[s] = ring.decode_export(buf)
                ring.export_release(s)
        ring.flush()
        s, buf, _ = ring.export_take(wait=True)
        got[s] = ring.decode_export(buf)
        ring.export_release(s)
        ring.sync()
        assert ring.theta_reruns() + ring.price_reruns() > 10 * nsteps, (ring.theta_reruns(), ring.price_reruns())
        assert sorted(got) == list(range(nsteps))
        for k in range(nsteps):
            assert X.export_diff(got[k], want[k]) == [], k
        assert ring.export_stale() == 0
        ring.set_export_ring(None)
    finally:
        for p in pipes:
            p.destroy()
        D.pvq_ref_set_theta_margin(0, False)
        D.set_price_tol_scale(1.)
