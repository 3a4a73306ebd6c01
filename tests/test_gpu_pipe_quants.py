"""Per-picture quantisers in the frame-batch step (odhip_pipe_set_quants / Pipe.set_quants): picture f of a
step coded at quants[f] - luma plane f with pvq_qm_q4[0], Cb plane f with [1], Cr plane F + f with [2].

A quality ladder (one picture replicated at -v 1 .. 100 in one step) against the compiled reference, 4:2:0 and
4:4:4, with and without chroma from luma, at 10 bits and as an inter step; a mixed batch equal byte for byte
to one F = 1 pipe per picture (no reference needed); the uniform table equal to the config's quant; tables
changed between steps without a sync leave every enqueued step as it was (resident, fed, exported); bad
arguments are refused and leave the pipe usable."""
import ctypes
import hashlib
import os
import sys

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from _libs import ref  # noqa: E402

pytestmark = pytest.mark.gpu
needs_ref = pytest.mark.skipif(ref() is None, reason="oracle/_ref (the compiled reference) not present")

LADDER = (1, 5, 10, 20, 40, 100)
EINVAL = -10


@pytest.fixture(scope="module")
def D():
    import daala_amd
    daala_amd.init(0)
    return daala_amd


def _pics420(content, index, seed, pw, ph):
    """[Y, Cb, Cr] uint8 pictures of pw x ph (4:2:0) cut from the bench generators."""
    import bench
    fr = bench.CONTENT[content](index, seed)
    return [np.ascontiguousarray(fr[0][:ph, :pw])] + [np.ascontiguousarray(p[:ph // 2, :pw // 2]) for p in fr[1:]]


def _stack(frames):
    luma = np.stack([f[0] for f in frames])
    chroma = np.concatenate([np.stack([f[1] for f in frames]), np.stack([f[2] for f in frames])])
    return np.ascontiguousarray(luma), np.ascontiguousarray(chroma)


def _fpr10(frames, seed=10):
    rng = np.random.RandomState(seed)
    return [[((p.astype(np.int32) << 2) + rng.randint(0, 4, size=p.shape)).astype(np.int16) for p in f]
            for f in frames]


def _recon(D, pipe):
    """recon[set][bs]: [nplanes][H >> dec][W >> dec] of the last step."""
    rdt = np.uint16 if pipe.fpr_bits else np.uint8
    F, W, H = pipe.frames, pipe.W, pipe.H
    d = 0 if pipe.chroma_444 else 1
    return [[pipe.read(D.BUF_RECON, 0, bs, dtype=rdt).reshape(F, H, W) for bs in range(5)],
            [pipe.read(D.BUF_RECON, 1, bs, dtype=rdt).reshape(2 * F, H >> d, W >> d)
             for bs in range(pipe.chroma_levels)]]


def _decisions(D, pipe):
    import _pipe444_check as C
    import _pipeline_check as P
    return C.decisions444(D, pipe) if pipe.chroma_444 else P.gpu_decisions(D, pipe)


def _run(pipe, steps):
    for _ in range(steps):
        pipe.step()
    pipe.flush()
    pipe.sync()


def _pipe(D, qt, frames, pw, ph, pred=None, **kw):
    pipe = D.Pipe(qt, len(frames), pw, ph, inter=pred is not None, **kw)
    try:
        pipe.set_pictures(*_stack(frames))
        if pred is not None:
            pipe.set_reference_pictures(*_stack(pred))
    except BaseException:
        pipe.destroy()
        raise
    return pipe


def _ladder_against_reference(D, frames, quants, pw, ph, pred=None, **kw):
    import _pipe444_check as C
    import _pipeline_check as P
    F = len(frames)
    pipe = _pipe(D, D.QuantTables.load(), frames, pw, ph, pred=pred, price=True, **kw)
    try:
        pipe.set_quants(quants)
        _run(pipe, 2)
        gpu = _recon(D, pipe)
        dec = _decisions(D, pipe)
    finally:
        pipe.destroy()
    cfl, fpr = kw.get("chroma_cfl", True), kw.get("fpr_bits", 0)
    for f in range(F):
        want = []
        if kw.get("chroma_444"):
            cpu, _ = C.cpu_frame444(quants[f], frames[f], pw, ph, chroma_cfl=cfl, fpr_bits=fpr,
                                    inter_pred=None if pred is None else pred[f], decisions=want)
            assert C.compare_frame444(gpu, cpu, frame=f, frames=F) == [], f
            assert C.compare_decisions444(dec, want, frame=f, frames=F) == [], f
        else:
            cpu = P.cpu_frame(quants[f], frames[f], pw, ph, chroma_cfl=cfl, fpr_bits=fpr, decisions=want)[0]
            assert P.compare_frame(gpu, cpu, frame=f, frames=F) == [], f
            assert P.compare_decisions(dec, want, frame=f, frames=F) == [], f
    # the ladder is a ladder: every rung codes the same picture differently
    for f in range(1, F):
        assert not np.array_equal(gpu[0][0][f], gpu[0][0][0]), f


@needs_ref
@pytest.mark.parametrize("mode", ["cfl", "nocfl", "fpr10"])
def test_ladder_420_equals_reference(D, mode):
    pw, ph = 640, 360
    frames = [_pics420("natural", 2, 11, pw, ph)] * len(LADDER)
    kw = dict(chroma_cfl=mode != "nocfl")
    if mode == "fpr10":
        frames = _fpr10(frames[:1]) * len(LADDER)
        kw["fpr_bits"] = 10
    quants = [D.QuantTables.for_quality(v) for v in LADDER]
    _ladder_against_reference(D, frames, quants, pw, ph, **kw)


@needs_ref
@pytest.mark.parametrize("size", [(320, 180), (177, 121)])
def test_ladder_444_equals_reference(D, size):
    import _pipe444_check as C
    pw, ph = size
    frames = [C.pictures444("natural", 3, 21, pw, ph)] * len(LADDER)
    quants = [D.QuantTables.for_quality(v) for v in LADDER]
    _ladder_against_reference(D, frames, quants, pw, ph, chroma_cfl=True, chroma_444=True)


@needs_ref
def test_ladder_inter_step_equals_reference(D):
    import _pipe444_check as C
    pw, ph = 177, 121
    cur = C.pictures444("natural", 8, 3, pw, ph)
    prev = C.pictures444("natural", 8, 5, pw, ph)
    rng = np.random.RandomState(4)
    pred = [np.clip(np.roll(p.astype(np.int32), 1, axis=1) + rng.randint(-6, 7, size=p.shape), 0, 255)
            .astype(np.uint8) for p in prev]
    quants = [D.QuantTables.for_quality(v) for v in (10, 40, 100)]
    _ladder_against_reference(D, [cur] * 3, quants, pw, ph, pred=[pred] * 3, chroma_444=True)


def _dump(D, pipe, what=("recon", "choice")):
    """{(name, set, level): bytes per plane} of the last step: recon, and the choice records."""
    bufs = {"recon": D.BUF_RECON, "choice": D.BUF_CHOICE, "band": D.BUF_BAND, "y": D.BUF_Y}
    out = {}
    n = (pipe.frames, 2 * pipe.frames)
    for s in (0, 1):
        for bs in range(5 if s == 0 else pipe.chroma_levels):
            for name in what:
                a = pipe.read(bufs[name], s, bs)
                out[(name, s, bs)] = a.reshape(n[s], -1)
    return out


def _single_pipes(D, frames, quants, pw, ph, **kw):
    """What F = 1 pipes, each created with its picture's quantiser, compute: per picture (dump, decisions)."""
    out = []
    for fr, qt in zip(frames, quants):
        pipe = _pipe(D, qt, [fr], pw, ph, **kw)
        try:
            _run(pipe, 2)
            out.append((_dump(D, pipe), _decisions(D, pipe)))
        finally:
            pipe.destroy()
    return out


def _assert_equals_singles(D, pipe, singles):
    F = pipe.frames
    got = _dump(D, pipe)
    dec = _decisions(D, pipe)
    for f, (want, wdec) in enumerate(singles):
        for (name, s, bs), a in want.items():
            planes = [f] if s == 0 else [f, F + f]
            assert np.array_equal(got[(name, s, bs)][planes], a), (f, name, s, bs)
        for key, (yw, bw, cw) in wdec.items():
            s = key[0]
            per = yw.shape[0] // (1 + s)
            rows = np.concatenate([np.arange(p * per, (p + 1) * per) for p in ([f] if s == 0 else [f, F + f])])
            yg, bg, cg = (x[rows] for x in dec[key])
            assert np.array_equal(cg, cw) and np.array_equal(bg, bw), (f, key)
            assert np.array_equal(yg, yw), (f, key)


@pytest.mark.parametrize("mode", ["cfl", "nocfl", "444"])
def test_mixed_batch_equals_single_picture_pipes(D, mode):
    """No reference needed: F = 4 different pictures at four quantisers, byte for byte what four F = 1 pipes
    created with those quantisers compute."""
    import _pipe444_check as C
    pw, ph = (256, 144) if mode != "444" else (177, 121)
    kw = dict(price=True, chroma_cfl=mode != "nocfl", chroma_444=mode == "444")
    if mode == "444":
        frames = [C.pictures444(("checker", "natural")[i % 2], 4 + i, 5, pw, ph) for i in range(4)]
    else:
        frames = [_pics420(("checker", "natural")[i % 2], 4 + i, 5, pw, ph) for i in range(4)]
    quants = [D.QuantTables.for_quality(v) for v in (5, 40, 10, 100)]
    singles = _single_pipes(D, frames, quants, pw, ph, **kw)
    pipe = _pipe(D, D.QuantTables.load(), frames, pw, ph, **kw)
    try:
        _run(pipe, 1)
        uniform = _dump(D, pipe)
        pipe.set_quants(quants)
        _run(pipe, 1)
        _assert_equals_singles(D, pipe, singles)
        # ... and they are not what the config's quant codes
        assert not np.array_equal(_dump(D, pipe)[("recon", 0, 0)], uniform[("recon", 0, 0)])
    finally:
        pipe.destroy()


def _sha(D, pipe):
    return {k: hashlib.sha256(v.tobytes()).hexdigest() for k, v in _dump(D, pipe, ("recon", "choice", "band", "y")).items()}


@pytest.mark.parametrize("cfl,price", [(True, True), (True, False), (False, True)])
def test_uniform_table_equals_config_quant(D, cfl, price):
    pw, ph, F = 320, 184, 2
    qt = D.QuantTables.for_quality(20)
    frames = [_pics420("natural", 7 + i, 3, pw, ph) for i in range(F)]
    hashes, decided = [], []
    for variant in ("never", "same", "reset"):
        pipe = _pipe(D, qt, frames, pw, ph, chroma_cfl=cfl, price=price)
        try:
            if variant == "same":
                pipe.set_quants([D.QuantTables.for_quality(20) for _ in range(F)])
            if variant == "reset":
                pipe.set_quants([D.QuantTables.for_quality(100)] * F)
                _run(pipe, 1)
                pipe.set_quants(None)
            _run(pipe, 3)
            hashes.append(_sha(D, pipe))
            decided.append(_decisions(D, pipe))
        finally:
            pipe.destroy()
    assert hashes[1] == hashes[0]
    # after a step at another quantiser, the pulse slots no choice names still hold that step's candidates (as
    # after any earlier step): everything the step decided is the config quant's
    assert {k: v for k, v in hashes[2].items() if k[0] != "y"} == {k: v for k, v in hashes[0].items() if k[0] != "y"}
    for key, want in decided[0].items():
        assert all(np.array_equal(a, b) for a, b in zip(decided[2][key], want)), key


@pytest.mark.parametrize("mode", ["resident", "feed", "export"])
def test_quants_changed_between_steps_keep_each_step(D, mode):
    """A different table before every step and once more behind the last one, without a sync: the last step
    equals the same steps run serially with a sync after each, and the F = 1 pipes of its pictures."""
    import torch
    pw, ph, F = 256, 144, 2
    qt = D.QuantTables.load()
    q = {v: D.QuantTables.for_quality(v) for v in (1, 5, 10, 40, 100)}
    tables = [[q[5], q[40]], [q[100], q[10]], [q[40], q[1]]]
    junk = [q[1], q[100]]
    if mode == "resident":
        sets = [[_pics420("natural", 20 + i, 8, pw, ph) for i in range(F)]] * 3
    else:
        sets = [[_pics420(("checker", "natural")[(k + i) % 2], 20 + 3 * k + i, 8, pw, ph) for i in range(F)]
                for k in range(3)]
    kw = dict(chroma_cfl=True, price=True)
    for nsteps in ((2, 3) if mode == "resident" else (3,)):
        last = nsteps - 1
        singles = _single_pipes(D, sets[last], tables[last], pw, ph, **kw)
        runs = []
        for serial in (False, True):
            pipe = _pipe(D, qt, sets[0], pw, ph, serial=serial, **kw)
            host = None
            try:
                pinned = [tuple(torch.from_numpy(a).pin_memory() for a in _stack(s)) for s in sets]
                if mode == "export":
                    host = torch.zeros(pipe.export_bytes(), dtype=torch.uint8).pin_memory()
                    pipe.set_export(host)
                for k in range(nsteps):
                    pipe.set_quants(tables[k])
                    if mode != "resident":
                        pipe.feed(*pinned[k])
                    pipe.step()
                    if serial:
                        pipe.sync()
                pipe.set_quants(junk)            # the steps already enqueued keep theirs
                pipe.flush()
                pipe.sync()
                _assert_equals_singles(D, pipe, singles)
                runs.append(_sha(D, pipe))
                if host is not None:
                    got = pipe.decode_export(host.numpy())
                    dev = _decisions(D, pipe)
                    assert set(got) == set(dev)
                    for key in sorted(dev):
                        yw, bw, cw = dev[key]
                        yg, bg, cg = got[key]
                        assert np.array_equal(cg, cw), key
                        assert np.array_equal(bg[..., :3], bw[..., :3]), key
                        assert np.array_equal(bg[..., 3][cw], bw[..., 3][cw]), key
                        assert np.array_equal(yg, yw), key
                    assert pipe.export_stale() == 0
                    pipe.set_export(None)
            finally:
                pipe.destroy()
        assert runs[0] == runs[1], nsteps


def test_bad_tables_are_refused_and_the_pipe_still_codes(D):
    pw, ph, F = 128, 64, 2
    qt = D.QuantTables.load()
    frames = [_pics420("natural", 30 + i, 2, pw, ph) for i in range(F)]
    ref_pipe = _pipe(D, qt, frames, pw, ph, price=True)
    pipe = _pipe(D, qt, frames, pw, ph, price=True)
    from daala_amd.quant import QUALITY_QUANTIZERS
    L = D.lib()
    try:
        _run(ref_pipe, 2)
        want = _sha(D, ref_pipe)

        def call(tables, n=None):
            ptrs = (ctypes.c_void_p * max(1, len(tables)))(
                *[None if t is None else ctypes.cast(ctypes.byref(t.c), ctypes.c_void_p) for t in tables])
            return L.odhip_pipe_set_quants(pipe._p(), ptrs, len(tables) if n is None else n)

        good = D.QuantTables.for_quality(40)
        assert call([good] * (F + 1)) == EINVAL
        assert call([good]) == EINVAL
        assert call([good, None]) == EINVAL
        assert call([good, D.QuantTables(*QUALITY_QUANTIZERS[40], use_masking=0)]) == EINVAL
        assert call([D.QuantTables(*QUALITY_QUANTIZERS[40], hvs_qm=0), good]) == EINVAL
        assert L.odhip_pipe_set_quants(ctypes.c_void_p(0), None, 0) == EINVAL
        with pytest.raises(D.DaalaHipError):
            pipe.set_quants([good])
        # nothing was taken: the pipe codes with its own quant
        _run(pipe, 2)
        assert _sha(D, pipe) == want
        assert call([good, good]) == 0
        _run(pipe, 1)
        assert _sha(D, pipe) != want
    finally:
        pipe.destroy()
        ref_pipe.destroy()
