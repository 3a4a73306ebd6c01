"""GPU: the part of the with-reference stage that follows a band's decision (refb_finish of
daala_amd/csrc/pvq_refbands.hip: skip rules, choice record, gain expansion, synthesis scale, Householder
constants) with the Householder pivot m at EVERY position of the short bands and at every lane joint of the
long ones.  Where a band is spread over a group of lanes the finish moves one pulse from the neighbouring lane
at the pivot and sums over the group; the directed inputs of the other modules put m at 0, 1, mid - 1, mid,
last - 1 and last of a 128-coefficient band only.  Here block b of 96 holds, in every band, a reference with a
UNIQUE maximum of |r16| at a chosen position (the pivot is the first maximum, src/pvq.c:od_compute_householder):

  band 0 (15 coefficients)       b mod 15
  bands 1, 2 (8)                 b mod 8, (b + 4) mod 8
  bands 3 - 5 (32)               (b + 11 j) mod 32, j = 0, 1, 2: the joint of a lane pair is 15 / 16
  band 6 (128)                   the b-th, cyclically, of PIVOTS128: the joints of a quad (31 / 32, 63 / 64,
                                 95 / 96) and of a DPP row of 16 lanes with 8 positions each (7 / 8, 15 / 16)

and x is the reference plus Laplacian noise of about a tenth of the peak, so that theta candidates with pulses
win (only a theta winner has Householder constants).  The bands are built through _pvq_corpus.lift: the
maximum is unique after the quantisation matrix too.  Amplitudes rotate with the block, quantiser steps with
the band (AMPS, QS).  The 96 blocks of 16x16 lie in four rows of 24 (64 x 384): the pulse-fed inverse takes
whole superblocks only.

What the traces of the oracle hold of this is asserted first (test_inputs_hold_every_pivot).  Then the same
planes go through all five callers of the finish:
  (a) odhip_pvq_ref_bands_decided_multi of the default build - k_refb_lean_lane<15 / 8>, k_refb_lean_pair<16, 2>
      and <32, 4> - against the oracle: choice words and pulses, and the pulse-fed inverse (the only reader of
      record words 8 - 15) against the oracle's inverse;
  (b) the row forms k_refb_lean_row<8, 4 / 16> (experiments build, ODHIP_REFB_ROW32=1) against (a), byte for byte;
  (c) the priced stage (k_refb_search_regs<15 / 8, true> decide inside the search, k_refb_choose<32 / 128, 1>
      from the candidate records) against (a)."""
import json
import os
import subprocess
import sys

import numpy as np
import pytest

import _pvq_corpus as C
from _refbands import Mismatch, oracle_traces
from test_gpu_plane_layouts import _oracle_inverse, _pic
from test_gpu_pvq_bands import hip  # noqa: F401
from test_gpu_pvq_corpus import _tables, _to_raster
from test_gpu_pvq_corpus_decided import _compare_decided, _cuda, _oracle_planes
from test_gpu_pvq_refbands import _assert_same_decisions

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
BS = 2                            # 16x16 blocks: bands of 15, 8, 8, 32, 32, 32 and 128 coefficients
NBLOCKS = 96
ROWS, COLS = 4, 24
MODES = [(1, 1), (0, 0)]
PIVOTS128 = (0, 1, 7, 8, 9, 15, 16, 17, 31, 32, 33, 63, 64, 65, 95, 96, 97, 126, 127)
BIG = 40                          # the peak of a reference shape; everything else is at most SMALL
SMALL = 12
AMPS = (20, 400, 8000)            # by block (blk // len(PIVOTS128): every pivot of every size at several)
QS = (37, 243, 1264)              # by band

_cache = {}


def pivot(blk, band):
    if band == 0:
        return blk % 15
    if band in (1, 2):
        return (blk + 4 * (band - 1)) % 8
    if band in (3, 4, 5):
        return (blk + 11 * (band - 3)) % 32
    return PIVOTS128[blk % len(PIVOTS128)]


def _inputs(hip, mode):
    """(x, r, qm, qmi, q_band, beta_band, traces) of a mode, the oracle's traces once per session."""
    if mode in _cache:
        return _cache[mode]
    is_keyframe, pli = mode
    dec = 1 if pli else 0
    qt = _tables(hip, "default")
    qm, qmi = qt.qm_slices(dec, BS)
    n = 4 << BS
    nb = C.NBANDS[BS]
    assert nb == 7 and C.BAND_OFFSETS[nb] == n * n
    rng = np.random.RandomState(4100 + 10 * is_keyframe + pli)
    x = np.zeros((1, n * ROWS, n * COLS), np.int32)
    r = np.zeros((1, n * ROWS, n * COLS), np.int32)
    for blk in range(NBLOCKS):
        vx = np.zeros(n * n, np.int32)
        vr = np.zeros(n * n, np.int32)
        amp = AMPS[(blk // len(PIVOTS128)) % len(AMPS)]
        for b in range(nb):
            a, e = C.BAND_OFFSETS[b], C.BAND_OFFSETS[b + 1]
            sign = rng.choice([-1, 1], size=e - a)
            sr = rng.randint(1, SMALL + 1, size=e - a) * sign
            sr[pivot(blk, b)] = BIG * sign[pivot(blk, b)]
            sx = sr + np.round(rng.laplace(size=e - a) * (BIG / 10.)).astype(np.int64)
            zero = np.zeros(e - a, np.int64)
            vx[a:e] = C.lift(sx, zero, qm[a:e], amp, 15)[0]
            vr[a:e] = C.lift(sr, zero, qm[a:e], amp, 14)[0]
        by, bx = divmod(blk, COLS)
        x[0, by * n:(by + 1) * n, bx * n:(bx + 1) * n] = _to_raster(vx, n)
        r[0, by * n:(by + 1) * n, bx * n:(bx + 1) * n] = _to_raster(vr, n)
    for a in (x, r):
        a.setflags(write=False)
    qb = [QS[b % len(QS)] for b in range(nb)]
    bb = qt.beta_band(pli, BS)
    traces, _ = oracle_traces(x, r, BS, qm, qmi, qb, bb, is_keyframe, pli, hip.OD_PVQ_LAMBDA)
    assert len(traces) == NBLOCKS * nb and all(t["tr"].ncands < 24 for t in traces.values())
    _cache[mode] = (x, r, qm, qmi, qb, bb, traces)
    return _cache[mode]


def conditions(traces):
    """From the oracle's traces: the pivot of every band is the chosen position; per (band size, position) the
    number of bands a theta candidate with pulses won."""
    won = {}
    for (blk, b), t in traces.items():
        p = pivot(blk, b)
        assert t["tr"].m == p, (blk, b, t["tr"].m, p)
        key = (t["n"], p)
        won[key] = won.get(key, 0) + int(t["itheta"] != -1 and t["vk"] > 0)
    return won


def _job(hip, mode):
    x, r, qm, qmi, qb, bb, _ = _inputs(hip, mode)
    return hip.PvqRefJob(_cuda(x), _cuda(r), BS, _cuda(qm), _cuda(qmi), qb, bb, mode[0], mode[1])


def _decided(hip, mode):
    import torch
    hip.pvq_k_range_take()
    job = _job(hip, mode)
    listed = hip.pvq_ref_bands_decided_multi([job], hip.OD_PVQ_LAMBDA)
    torch.cuda.synchronize()
    return job, listed, hip.pvq_k_range_take()


@pytest.mark.parametrize("is_keyframe,pli", MODES)
def test_inputs_hold_every_pivot(hip, is_keyframe, pli):
    won = conditions(_inputs(hip, (is_keyframe, pli))[6])
    print(sorted(won.items()))
    want = ([(15, p) for p in range(15)] + [(8, p) for p in range(8)] + [(32, p) for p in range(32)]
            + [(128, p) for p in PIVOTS128])
    assert sorted(won) == sorted(want)
    assert all(won[k] > 0 for k in want), sorted(k for k in want if not won[k])


@pytest.mark.parametrize("is_keyframe,pli", MODES)
def test_decided_stage_matches_the_oracle_at_every_pivot(hip, is_keyframe, pli):
    """(a): records and pulses of the default build's decided stage, and the pulse-fed inverse."""
    mode = (is_keyframe, pli)
    x, r, _, _, _, _, traces = _inputs(hip, mode)
    conditions(traces)
    job, listed, k_range = _decided(hip, mode)
    mm = Mismatch()
    _compare_decided(job, traces, mm)
    assert mm.total() == 0, mm.summary()
    assert mm.checked["y"] == NBLOCKS * job.nb and k_range == (0, 0)
    # the resolves re-run what they list through other kernels: they must stay the exception here
    assert sum(listed) <= 0.05 * NBLOCKS * job.nb, listed
    dec = 1 if pli else 0
    _, h, w = x.shape
    pw, ph = _pic(dec, w, h)
    got = hip.inverse_levels_pvq_ref([job], dec, pw, ph)[0].cpu().numpy()
    want = _oracle_inverse(_oracle_planes(x, r, BS, traces, is_keyframe), dec, BS, False)
    assert np.array_equal(got, want), mode


@pytest.mark.parametrize("is_keyframe,pli", MODES)
def test_priced_stage_decides_as_the_decided_stage_at_every_pivot(hip, is_keyframe, pli):
    """(c): the per-lane searches that decide inside the priced band stage and the choice kernels behind it."""
    import torch
    mode = (is_keyframe, pli)
    ja, _, _ = _decided(hip, mode)
    jc = _job(hip, mode)
    hip.pvq_ref_choose_priced_multi([jc], hip.OD_PVQ_LAMBDA, fused_bands=True)
    torch.cuda.synchronize()
    _assert_same_decisions([jc], [ja], (is_keyframe, pli, "priced"))


def _outputs(hip):
    out = {}
    for mode in MODES:
        job, listed, k_range = _decided(hip, mode)
        out["choice_%d%d" % mode] = job.choice.cpu().numpy()
        out["y_%d%d" % mode] = job.y.cpu().numpy()
        out["counts_%d%d" % mode] = np.array(list(listed) + list(k_range))
    return out


def _child():
    """In a process that loaded the experiments build with ODHIP_REFB_ROW32=1: both modes' outputs into the .npz
    named on the command line."""
    import daala_amd
    daala_amd.init(0)
    assert hasattr(daala_amd.lib(), "odhip_exp_row_replay_stats"), "the experiments build is expected here"
    out = _outputs(daala_amd)
    np.savez(sys.argv[1], **out)
    print(json.dumps(dict(arrays=len(out))))


def test_row_forms_agree_with_the_default_build_at_every_pivot_experiments_build(hip, tmp_path):
    """(b): k_refb_lean_row<8, 4> for the 32-coefficient bands and <8, 16> for the 128-coefficient ones, byte
    for byte against the default build's lane pairs and quads."""
    import daala_amd
    want = _outputs(hip)
    env = dict(os.environ)
    env.update(ODHIP_LIB=daala_amd.EXPERIMENTS_LIB, ODHIP_REFB_ROW32="1")
    env.pop("ODHIP_REFB_GROUP128", None)
    path = str(tmp_path / "row.npz")
    r = subprocess.run([sys.executable, os.path.abspath(__file__), path], env=env, capture_output=True, text=True,
                       timeout=600, cwd=ROOT)
    assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-2000:]
    got = np.load(path)
    assert sorted(got.files) == sorted(want)
    for name in want:
        a, b = want[name], got[name]
        assert a.dtype == b.dtype and a.shape == b.shape and a.tobytes() == b.tobytes(), name
    assert all(want["y_%d%d" % m].any() for m in MODES)


if __name__ == "__main__":
    sys.path.insert(0, ROOT)
    _child()
