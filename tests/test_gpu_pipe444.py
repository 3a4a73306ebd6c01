"""The frame-batch step (odhip_pipe) on 4:4:4 pictures (odhip_pipe_config.chroma_444 = 1): chroma planes
of the picture size, coded at all five levels (4x4 .. 64x64), keyframe chroma predicted from the luma
block of the same level (od_resample_luma_coeffs' copy branch, src/intra.c:95-108).

Every pixel of every level of Y, Cb and Cr, and the gain index / theta / K / pulses of every band, against
the compiled reference run at dec 0 (tests/_pipe444_check.py); with chroma from luma, without it, at 10
bits and as an inter frame; pipelined equals serial, fed equals resident; the export holds ten sections
that decode to the device buffers and the reference's decisions; the 4:2:0 default is untouched."""
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


def _frames(content, F, pw, ph, seed=4321):
    import _pipe444_check as C
    return [C.pictures444(content, 3 + i, seed, pw, ph) for i in range(F)]


def _run(D, pipe, steps):
    for _ in range(steps):
        pipe.step()
    pipe.flush()
    pipe.sync()


def test_default_pipe_is_420_and_444_config_is_validated(D):
    qt = D.QuantTables.load()
    pipe = D.Pipe(qt, 1, 64, 64)
    try:
        assert pipe.chroma_levels == 4 and not pipe.chroma_444
        assert pipe.nblocks(1, 0) == 2 * 8 * 8
    finally:
        pipe.destroy()
    pipe = D.Pipe(qt, 1, 65, 63, chroma_444=True)       # odd sizes: 4:4:4 only
    try:
        assert pipe.chroma_levels == 5
        assert pipe.nblocks(1, 4) == 2 * 2 and pipe.nblocks(1, 0) == 2 * 32 * 16
        # the chroma pictures are [2F][pic_h][pic_w]
        _, nbytes = pipe.buffer(D.BUF_PIC, 1)
        assert nbytes == 2 * 65 * 63
        # and every chroma level exists, 64x64 included
        _, nbytes = pipe.buffer(D.BUF_CHOICE, 1, 4)
        assert nbytes == 4 * 4 * 9 * 16
    finally:
        pipe.destroy()
    with pytest.raises(Exception):
        D.Pipe(qt, 1, 65, 64)                            # odd 4:2:0 stays refused
    import ctypes
    L = D.lib()
    assert L.odhip_pipe_chroma_levels(ctypes.c_void_p(0)) < 0


@needs_ref
@pytest.mark.parametrize("size", [(1920, 1080), (177, 121)])
@pytest.mark.parametrize("content", ["checker", "natural"])
def test_keyframe_cfl_device_priced_equals_reference(D, size, content):
    import _pipe444_check as C
    pw, ph = size
    qt = D.QuantTables.load()
    fr = _frames(content, 1, pw, ph)
    pipe = C.gpu_pipe444(D, qt, fr, pw, ph, chroma_cfl=True, price=True)
    try:
        _run(D, pipe, 2)
        gpu = C.recon444(D, pipe)
        dec = C.decisions444(D, pipe)
    finally:
        pipe.destroy()
    want = []
    cpu, blocks = C.cpu_frame444(qt, fr[0], pw, ph, chroma_cfl=True, decisions=want)
    W, H = (pw + 63) & ~63, (ph + 63) & ~63
    assert blocks == 3 * sum((W >> (2 + bs)) * (H >> (2 + bs)) for bs in range(5))
    assert C.compare_frame444(gpu, cpu) == [], (size, content)
    assert C.compare_decisions444(dec, want) == [], (size, content)
    # the chroma from luma reference is really in use: chroma coded without it differs
    alone, _ = C.cpu_frame444(qt, fr[0], pw, ph, chroma_cfl=False)
    assert any(not np.array_equal(alone[1][bs], cpu[1][bs]) for bs in range(5))


@needs_ref
@pytest.mark.parametrize("mode", ["noref", "fpr10"])
@pytest.mark.parametrize("size", [(640, 360), (177, 121)])
def test_noref_chroma_and_10_bit_equal_reference(D, mode, size):
    import _pipe444_check as C
    pw, ph = size
    qt = D.QuantTables.for_quality(40) if mode == "fpr10" else D.QuantTables.load()
    F = 2
    fr = _frames("natural", F, pw, ph, seed=99)
    kw = dict(chroma_cfl=mode != "noref", price=True)
    if mode == "fpr10":
        rng = np.random.RandomState(10)
        fr = [[((p.astype(np.int32) << 2) + rng.randint(0, 4, size=p.shape)).astype(np.int16) for p in f]
              for f in fr]
        kw["fpr_bits"] = 10
    pipe = C.gpu_pipe444(D, qt, fr, pw, ph, **kw)
    try:
        _run(D, pipe, 2)
        gpu = C.recon444(D, pipe)
        dec = C.decisions444(D, pipe)
    finally:
        pipe.destroy()
    for i in range(F):
        want = []
        cpu, _ = C.cpu_frame444(qt, fr[i], pw, ph, chroma_cfl=kw["chroma_cfl"], fpr_bits=kw.get("fpr_bits", 0),
                                decisions=want)
        assert C.compare_frame444(gpu, cpu, frame=i, frames=F) == [], (mode, size, i)
        assert C.compare_decisions444(dec, want, frame=i, frames=F) == [], (mode, size, i)
        if mode == "fpr10":
            assert int(cpu[1][0].max()) > 255


@needs_ref
@pytest.mark.parametrize("size", [(312, 180), (177, 121)])
def test_inter_step_equals_reference(D, size):
    import _pipe444_check as C
    pw, ph = size
    qt = D.QuantTables.for_quality(40)
    cur = C.pictures444("natural", 8, 3, pw, ph)
    prev = C.pictures444("natural", 8, 5, pw, ph)
    rng = np.random.RandomState(4)
    pred = [np.clip(np.roll(p.astype(np.int32), 1, axis=1) + rng.randint(-6, 7, size=p.shape), 0, 255)
            .astype(np.uint8) for p in prev]
    pipe = C.gpu_pipe444(D, qt, [cur], pw, ph, inter_pred=[pred], price=True)
    try:
        _run(D, pipe, 3)
        gpu = C.recon444(D, pipe)
    finally:
        pipe.destroy()
    cpu, _ = C.cpu_frame444(qt, cur, pw, ph, inter_pred=pred)
    assert C.compare_frame444(gpu, cpu) == [], size
    key, _ = C.cpu_frame444(qt, cur, pw, ph)
    assert not np.array_equal(key[1][2], cpu[1][2])


def _dump(D, pipe):
    out = {}
    for s in (0, 1):
        for bs in range(5):
            for name, what in (("recon", D.BUF_RECON), ("choice", D.BUF_CHOICE), ("band", D.BUF_BAND),
                               ("y", D.BUF_Y)):
                out[(name, s, bs)] = pipe.read(what, s, bs)
    return out


@pytest.mark.parametrize("cfl,price", [(True, True), (True, False), (False, True)])
def test_pipelined_equals_serial(D, cfl, price):
    import _pipe444_check as C
    pw, ph, F = 640, 360, 2
    qt = D.QuantTables.load()
    fr = _frames("checker", F, pw, ph, seed=77)
    pipes = [C.gpu_pipe444(D, qt, fr, pw, ph, chroma_cfl=cfl, price=price, serial=s) for s in (False, True)]
    try:
        dumps = []
        for pipe in pipes:
            _run(D, pipe, 4)
            dumps.append(_dump(D, pipe))
        for key in dumps[0]:
            assert np.array_equal(dumps[0][key], dumps[1][key]), key
        rec = dumps[0][("recon", 1, 0)].reshape(2 * F, pipes[0].H, pipes[0].W)[:, :ph, :pw]
        assert np.abs(rec.astype(np.int32) - np.stack([f[1] for f in fr] + [f[2] for f in fr])).mean() < 12
    finally:
        for pipe in pipes:
            pipe.destroy()


def test_fed_pictures_equal_resident_pictures(D):
    import torch
    import _pipe444_check as C
    pw, ph, F = 320, 184, 2
    qt = D.QuantTables.load()
    sets = [C.stack444(_frames(("checker", "natural")[k % 2], F, pw, ph, seed=7 + k)) for k in range(4)]
    pinned = [(torch.from_numpy(l).pin_memory(), torch.from_numpy(c).pin_memory()) for l, c in sets]
    fed = D.Pipe(qt, F, pw, ph, chroma_cfl=True, price=True, chroma_444=True)
    resident = D.Pipe(qt, F, pw, ph, chroma_cfl=True, price=True, chroma_444=True, serial=True)
    try:
        for l, c in pinned:
            fed.feed(l, c)
            fed.step()
        fed.flush()
        fed.sync()
        resident.set_pictures(*sets[3])
        _run(D, resident, 1)
        want, got = _dump(D, resident), _dump(D, fed)
        for key in want:
            if key[0] in ("recon", "choice"):
                assert np.array_equal(got[key], want[key]), key
        assert np.array_equal(fed.read(D.BUF_PIC, 1), sets[3][1].ravel())
    finally:
        fed.destroy()
        resident.destroy()


@needs_ref
def test_export_has_ten_sections_equal_to_device_and_reference(D):
    import torch
    import _pipe444_check as C
    pw, ph, F = 177, 121, 2
    qt = D.QuantTables.load()
    sets = [_frames("natural", F, pw, ph, seed=s) for s in (5, 6)]
    pipe = D.Pipe(qt, F, pw, ph, chroma_cfl=True, price=True, chroma_444=True)
    try:
        lay = pipe.export_layout()
        assert lay["nsections"] == 10
        assert [s["bs"] for s in lay["sections"]] == [0, 1, 2, 3, 4] * 2
        assert [s["record_bytes"] for s in lay["sections"]] == [4] * 5 + [8] * 5
        host = torch.zeros(pipe.export_bytes(), dtype=torch.uint8).pin_memory()
        pinned = [tuple(torch.from_numpy(a).pin_memory() for a in C.stack444(s)) for s in sets]
        pipe.set_export(host)
        for step in range(4):
            pipe.feed(*pinned[step & 1])
            pipe.step()
            if step < 2:
                continue
            pipe.flush()
            pipe.sync()
            got = pipe.decode_export(host.numpy())
            dev = C.decisions444(D, pipe)
            assert set(got) == set(dev) and len(got) == 10
            for key in sorted(dev):
                yw, bw, cw = dev[key]
                yg, bg, cg = got[key]
                assert np.array_equal(cg, cw), (step, key)
                assert np.array_equal(bg[..., :3], bw[..., :3]), (step, key)
                assert np.array_equal(bg[..., 3][cw], bw[..., 3][cw]), (step, key)
                assert np.array_equal(yg, yw), (step, key)
            assert pipe.export_stale() == 0
            for i in range(F):
                want = []
                C.cpu_frame444(qt, sets[step & 1][i], pw, ph, decisions=want)
                # ... and those are the reference's
                assert C.compare_decisions444(dev, want, frame=i, frames=F) == [], (step, i)
        pipe.set_export(None)
    finally:
        pipe.destroy()


def test_pulse_range_is_reported_on_the_444_chroma_set(D):
    """odhip_pipe_k_range / ODHIP_ERANGE behave as in 4:2:0: a quantiser fine enough for a band to need more
    pulses than int16 holds is reported at the sync, not silently coded otherwise."""
    import _pipe444_check as C
    qt = D.QuantTables.for_quality(1)
    pw, ph = 128, 64
    rng = np.random.RandomState(1)
    fr = [[rng.randint(0, 256, size=(ph, pw)).astype(np.uint8) for _ in range(3)]]
    pipe = C.gpu_pipe444(D, qt, fr, pw, ph, chroma_cfl=True, price=True)
    try:
        pipe.step()
        pipe.flush()
        try:
            pipe.sync()
            in_range = True
        except D.PulseRangeError:
            in_range = False
        assert in_range == (pipe.k_range() == 0)
    finally:
        pipe.destroy()
