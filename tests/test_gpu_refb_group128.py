"""GPU: the with-reference 128-coefficient bands of the decided stage, searched a lane GROUP per band
(k_refb_lean_pair<32, 4>, a quad per band and 16 bands per wavefront - the default build's form - and
<64, 2>, a pair per band and 32 bands per wavefront: od_lane_search of daala_amd/csrc/pvq_lane.cuh with a
PAD, GroupVector), every decision against the CPU oracle's pvq_theta at speed 1 - gain index, theta,
max_theta, K, the winner's pulses, the choice record (test_gpu_pvq_corpus_decided._compare_decided) - and, in
child processes on the experiments build, byte for byte among k_refb_lean_row<8, 16> (that build's default
for these bands), the quad (ODHIP_REFB_GROUP128=4) and the pair (=2), and against the default build.

The planes are small and directed at what a group can get wrong.  A band's reference is a spike at its
first coefficient wherever a tie is wanted: the Householder reflection is then across that axis, and the
vector a theta candidate searches is the band without its first coefficient - positions 1..127 become the
127 dimensions 0..126 in front of the PAD, with their magnitudes (and ties) as they are; the no-reference
candidates of the same band search all 128.  So both vector lengths occur in such a band, and a tie placed
at band positions p and p + 1 sits on a lane joint for one of them (32 positions per lane of a quad, 64 per
lane of a pair).  _stats counts, from the oracle's traces alone, what the inputs were built to hold; those
counts are conditions on the inputs, asserted before anything is compared.

  level 2 (16x16 blocks) holds one 128-coefficient band per block (band 6), level 3 (32x32) three (6-8).
  Block counts of the level-2 jobs: 1, C - 1, C, C + 1 and 2C + 1 for C = 16 (the quad) and C = 32 (the
  pair) - groups beyond an item's end replay its last band and store nothing -; the level-3 jobs hold 11 and
  2 blocks, so one call mixes two block sizes and hands out more work units (14 and 9 at C = 16) than the
  four wavefronts of a workgroup: wavefronts of a workgroup leave at different times.  A call takes at most
  eight jobs, hence two calls ("a" and "b").

  Quantisers and amplitudes give bands whose every searched candidate has K = 0, the smallest K there is, tens
  of pulses, hundreds, and - the second level-3 job, test_gpu_pvq_corpus_decided._ladder_band: consecutive
  magnitudes below ~1090 at step 124 - K near 2.8 n (luma; 5.5 n and more with the chroma matrix), where the
  projection leaves two pulses and more on most positions.  About the smallest K: od_pvq_compute_k gives no K of
  1, 2 or 3 for 128 coefficients - with a reference K is 0, 6, 15, 23, .. (one step of theta is worth about
  eight pulses whatever the gain), without one it is at least 4 at beta = 1.5 (the luma tables) and 6 at
  beta = 1 - so the searches of K = 4 and 6 stand for "two or three pulses"; unlike K <= 2 they start from
  the projection, which places none of so few."""
import json
import os
import subprocess
import sys

import numpy as np
import pytest

import _pvq_corpus as C
from _libs import P, oracle
from _refbands import Mismatch, oracle_traces
from test_gpu_pvq_bands import hip  # noqa: F401
from test_gpu_pvq_corpus import Q_COARSE, _tables, _to_raster
from test_gpu_pvq_corpus_decided import SCREEN_Q, _compare_decided, _cuda, _ladder_band
from test_gpu_pvq_refbands import MODES

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
N = 128
BIG = 40                          # the tied magnitude of a shape; everything else is at most SMALL
SMALL = 12
AMPS = (3, 20, 400, 8000)
QS = (37, 243, 1264)
# call -> (level, blocks, kind); kind "shapes": SHAPES at rotating amplitudes and steps, "ladder": _ladder_band
CALLS = dict(a=((2, 1, "shapes"), (2, 15, "shapes"), (2, 16, "shapes"), (2, 17, "shapes"), (2, 33, "shapes"),
                (3, 11, "shapes"), (3, 2, "ladder")),
             b=((2, 31, "shapes"), (2, 32, "shapes"), (2, 65, "shapes")))
NBANDS128 = dict(a=1 + 15 + 16 + 17 + 33 + 3 * 11 + 3 * 2, b=31 + 32 + 65)
# band positions of the tied maxima.  With the spike reference the searched vector drops position 0: band
# position p is dimension p - 1 there and dimension p in the no-reference search.
TIED = dict(lane0=(4, 12, 28), lane3=(100, 110, 120), quads=(10, 40, 70, 100), halves=(30, 95),
            joints=(32, 33, 64, 65, 96, 97), last=(126, 127), last_big=(127,))
SHAPES = tuple(TIED) + ("single", "single_last", "zero", "flat", "pairs", "laplace", "noref", "zero_noref")

_cache = {}


def _shape(name, rng):
    """(vx, vr): integer shapes of a band and its reference; x16 = vx*mult, r16 = vr*mult'."""
    sign = rng.choice([-1, 1], size=N)
    v = rng.randint(1, SMALL + 1, size=N) * sign
    if name in TIED:
        v[list(TIED[name])] = BIG * sign[list(TIED[name])]
    elif name in ("single", "single_last"):
        v[:] = 0
        v[127 if name == "single_last" else 9] = BIG     # (single_last with the spike: the PAD's neighbour, 126)
    elif name in ("zero", "zero_noref"):
        v[:] = 0
    elif name == "flat":
        v = 5 * sign
    elif name == "pairs":
        v = (1 + rng.permutation(N) // 2) * sign
    elif name in ("laplace", "noref"):
        v = np.round(rng.laplace(size=N) * 9).astype(np.int64)
    vr = np.zeros(N, np.int64)
    if name == "laplace":
        vr = v + np.round(rng.laplace(size=N) * 6).astype(np.int64)
    elif name not in ("noref", "zero_noref"):
        # the spike; the band's own first coefficient puts theta between 20 and 70 degrees
        rest = float(np.sqrt((v[1:] ** 2).sum()))
        v[0] = int(round(rest * rng.choice([0.4, 1.0, 2.5]))) if name != "zero" else 0
        vr[0] = 50 * rng.choice([-1, 1])
    return v, vr


def _bands128(bs):
    return [b for b in range(C.NBANDS[bs]) if C.BAND_OFFSETS[b + 1] - C.BAND_OFFSETS[b] == N]


def _planes(hip, call, idx, dec):
    """One plane, a row of blocks, of job idx of a call: (x, r, names, qm, qmi, q of the 128-coefficient
    bands); the other bands hold small Laplacian filler."""
    key = ("planes", call, idx, dec)
    if key in _cache:
        return _cache[key]
    bs, nblk, kind = CALLS[call][idx]
    qt = _tables(hip, "default")
    qm, qmi = qt.qm_slices(dec, bs)
    n = 4 << bs
    rng = np.random.RandomState(128000 + 100 * idx + 10 * dec + ord(call))
    x = np.zeros((1, n, n * nblk), np.int32)
    r = np.zeros((1, n, n * nblk), np.int32)
    names = {}
    bands = _bands128(bs)
    q128 = [SCREEN_Q] * len(bands) if kind == "ladder" else [QS[(idx + i) % len(QS)] for i in range(len(bands))]
    end = C.BAND_OFFSETS[C.NBANDS[bs]]
    for blk in range(nblk):
        vx = np.zeros(n * n, np.int32)
        vr = np.zeros(n * n, np.int32)
        vx[:end] = np.round(rng.laplace(size=end) * 30)
        vr[:end] = vx[:end] + np.round(rng.laplace(size=end) * 20)
        for i, b in enumerate(bands):
            a = C.BAND_OFFSETS[b]
            if kind == "ladder":
                order = rng.permutation(N)
                sign = rng.choice([-1, 1], size=N)
                vx[a:a + N] = _ladder_band(1020 + (3 * blk + i) % 78, order, sign, qm[a:a + N])
                vr[a:a + N] = rng.randint(-30, 31, size=N)
                names[(blk, b)] = "ladder@%d" % blk
                continue
            name = SHAPES[(blk + 5 * i + 3 * idx) % len(SHAPES)]
            amp = AMPS[(blk // len(SHAPES) + i + idx) % len(AMPS)]
            sx, sr = _shape(name, rng)
            vx[a:a + N] = C.lift(sx, np.zeros(N, np.int64), qm[a:a + N], amp, 15)[0]
            vr[a:a + N] = C.lift(sr, np.zeros(N, np.int64), qm[a:a + N], amp, 14)[0]
            names[(blk, b)] = "%s@%d" % (name, amp)
        x[0, :, blk * n:(blk + 1) * n] = _to_raster(vx, n)
        r[0, :, blk * n:(blk + 1) * n] = _to_raster(vr, n)
    for a in (x, r):
        a.setflags(write=False)
    _cache[key] = (x, r, names, qm, qmi, q128)
    return _cache[key]


def _per_band(base, bs, v128):
    out = list(base)
    for b, v in zip(_bands128(bs), v128):
        out[b] = v
    return out


def _inputs(hip, call, mode):
    """Per job of a call: (bs, x, r, names, qm, qmi, q_band, beta_band, traces), the oracle's traces once per
    session."""
    key = ("inputs", call, mode)
    if key not in _cache:
        is_keyframe, pli = mode
        dec = 1 if pli else 0
        qt = _tables(hip, "default")
        out = []
        for idx, (bs, _, _) in enumerate(CALLS[call]):
            x, r, names, qm, qmi, q128 = _planes(hip, call, idx, dec)
            qb = _per_band(qt.q_band(pli, bs), bs, q128)
            bb = qt.beta_band(pli, bs)
            traces, _ = oracle_traces(x, r, bs, qm, qmi, qb, bb, is_keyframe, pli, hip.OD_PVQ_LAMBDA)
            assert all(t["tr"].ncands < 24 for t in traces.values())
            out.append((bs, x, r, names, qm, qmi, qb, bb, traces))
        _cache[key] = out
    return _cache[key]


def _searched(t, with_ref):
    """|v| of the vector a candidate of the band searches: the QM-scaled band, or its reflection without the
    Householder pivot (n - 1 dimensions)."""
    tr = t["tr"]
    x16 = np.array(tr.x16[:N], np.int16)
    if not with_ref:
        return np.abs(x16.astype(np.int64))
    out = np.zeros(N, np.int16)
    oracle().odo_apply_householder(P(out), P(x16), P(np.array(tr.r16[:N], np.int16)), N)
    return np.abs(np.delete(out, tr.m).astype(np.int64))


def _stats(inputs):
    """What the traces of the 128-coefficient bands hold of the cases this file is about."""
    st = dict(bands=0, all_k0=0, k123=0, k_least=0, tens=0, hundreds=0, k_ladder=0, fresh=0, chained=0, both_lengths=0,
              beyond_table=0, theta_won=0, noref_won=0)
    ties = {}
    for _, _, _, names, _, _, _, _, traces in inputs:
        for (blk, b), t in traces.items():
            if t["n"] != N:
                continue
            st["bands"] += 1
            st["theta_won" if t["itheta"] != -1 else "noref_won"] += t["vk"] > 0
            tr = t["tr"]
            name = names[(blk, b)].split("@")[0]
            st["all_k0"] += not any(tr.cands[i].k for i in range(tr.ncands) if tr.cands[i].searched)
            lengths = 0
            for with_ref in (1, 0):
                cands = [tr.cands[i] for i in range(tr.ncands) if tr.cands[i].with_ref == with_ref]
                if not any(c.searched and c.k for c in cands):
                    continue
                lengths += 1
                v = _searched(t, with_ref)
                nn = N - with_ref
                # (without the reference the band's own first coefficient, which sets theta, is part of the
                # vector and larger than the tied ones: the ties are those of the second largest magnitude)
                first = 0 if with_ref or name not in TIED else 1
                top = v[first:].max()
                at = set(first + np.flatnonzero(v[first:] == top)) if top > 0 else set()
                if name in TIED and at == {p - with_ref for p in TIED[name]}:
                    what = "%s.%s" % (name, "theta" if with_ref else "noref")
                    ties[what] = ties.get(what, 0) + 1
                if name in ("single", "single_last") and np.count_nonzero(v) == 1:
                    # single_last behind the spike: the only non-zero dimension is the PAD's neighbour
                    what = name + (".theta" if with_ref else ".noref")
                    if name == "single" or at == {127 - with_ref}:
                        ties[what] = ties.get(what, 0) + 1
                if name == "flat" and len(at) >= nn - 1:
                    ties["flat"] = ties.get("flat", 0) + 1
                if name == "pairs" and len(set(v.tolist())) <= N // 2 + 2:
                    ties["pairs"] = ties.get("pairs", 0) + 1
                prev_k = 0
                for c in cands:
                    if c.k == 0:
                        prev_k = 0
                    if not c.searched or c.k == 0:
                        continue
                    y = np.abs(np.array(c.y[:nn], np.int64))
                    assert int(y.sum()) == c.k
                    if c.k != prev_k:
                        st["k123"] += 1 <= c.k <= 3
                        st["k_least"] += c.k in (4, 6)
                        st["tens"] += 10 <= c.k < 100
                        st["hundreds"] += 100 <= c.k
                        st["k_ladder"] += name == "ladder" and 2.5 * N <= c.k
                        st["chained" if 0 < prev_k <= c.k else "fresh"] += 1
                        # the last pulse looks up 1/sqrt(yy + 2*y_j + 1) with yy of the pulses before it
                        st["beyond_table"] += int((y * y).sum()) - 2 * int(y.max()) + 1 + 2 > 512
                    prev_k = c.k
            st["both_lengths"] += lengths == 2
    return st, ties


def _jobs(hip, inputs, mode):
    is_keyframe, pli = mode
    return [hip.PvqRefJob(_cuda(x), _cuda(r), bs, _cuda(qm), _cuda(qmi), qb, bb, is_keyframe, pli)
            for bs, x, r, _, qm, qmi, qb, bb, _ in inputs]


def _run(hip, call, mode, inputs=None):
    import torch
    inputs = inputs or _inputs(hip, call, mode)
    hip.pvq_k_range_take()
    jobs = _jobs(hip, inputs, mode)
    listed = hip.pvq_ref_bands_decided_multi(jobs, hip.OD_PVQ_LAMBDA)
    torch.cuda.synchronize()
    return inputs, jobs, listed, hip.pvq_k_range_take()


def _assert_oracle(inputs, jobs, tag):
    mm = Mismatch()
    for job, inp in zip(jobs, inputs):
        names, traces = inp[3], inp[8]
        assert len(traces) == job.nblocks * job.nb
        _compare_decided(job, traces, mm)
        bad = {k: names.get(w[1:], "(filler)") for k, w in mm.first.items()}
        assert mm.total() == 0, (tag, job.bs, job.nblocks, mm.summary(), bad)
    assert mm.checked["y"] == sum(j.nblocks * j.nb for j in jobs)


@pytest.mark.parametrize("is_keyframe,pli", MODES)
def test_inputs_hold_the_cases(hip, is_keyframe, pli):
    """Conditions on the inputs, from the oracle's traces: every case the group search can get wrong is there,
    on the vector that is really searched."""
    mode = (is_keyframe, pli)
    st, ties = _stats(_inputs(hip, "a", mode) + _inputs(hip, "b", mode))
    print(st, ties)
    assert st["bands"] == NBANDS128["a"] + NBANDS128["b"]
    for what in ("all_k0", "k_least", "tens", "hundreds", "fresh", "chained", "noref_won", "theta_won", "beyond_table"):
        assert st[what] > 0, (what, st)
    assert st["k123"] == 0, st
    assert st["k_ladder"] >= 6 and st["both_lengths"] > 20 and st["chained"] > 50, st
    for what in ("lane0", "lane3", "quads", "halves", "joints", "last", "last_big"):
        assert ties.get(what + ".theta", 0) > 0 and ties.get(what + ".noref", 0) > 0, (what, ties)
    for what in ("single.theta", "single_last.theta", "flat", "pairs"):
        assert ties.get(what, 0) > 0, (what, ties)


@pytest.mark.parametrize("is_keyframe,pli", MODES)
@pytest.mark.parametrize("force_seq", [False, True], ids=["tournament", "force_seq"])
def test_group_search_decides_as_the_oracle(hip, is_keyframe, pli, force_seq, monkeypatch):
    """odhip_pvq_ref_bands_decided_multi on the jobs of each call, every test hook off; and with
    ODHIP_PVQ_FORCE_SEQ=1, the parts of every group combined by the sequential rescan."""
    if force_seq:
        monkeypatch.setenv("ODHIP_PVQ_FORCE_SEQ", "1")
    for call in sorted(CALLS):
        inputs, jobs, listed, k_range = _run(hip, call, (is_keyframe, pli))
        _assert_oracle(inputs, jobs, (call, "force_seq" if force_seq else "plain"))
        assert k_range == (0, 0)
        nbands = sum(j.nblocks * j.nb for j in jobs)
        # the resolves re-run what they list through other kernels: they must stay the exception here
        assert sum(listed) <= 0.1 * nbands, (listed, nbands)


# ---- the tie / degenerate corpus, its 128-coefficient classes ---------------------------------------------
def _corpus_inputs(hip, mode):
    """The "ties" and "spikes" cases of tests/_pvq_corpus.py for n = 128 (all |x| equal, two levels, shuffled
    pairs of equal values, equal maxima 1 .. 64 positions apart, single coefficients - spikes/last_const puts the
    only one next to the PAD), one case per 16x16 block, in two jobs: at the tables' own step the cases that
    keep K inside ODHIP_PVQ_MAX_K there, at the corpus's coarsest step the others."""
    key = ("corpus", mode)
    if key not in _cache:
        is_keyframe, pli = mode
        dec = 1 if pli else 0
        bs, band, n = 2, 6, 16
        qt = _tables(hip, "default")
        qm, qmi = qt.qm_slices(dec, bs)
        a = C.BAND_OFFSETS[band]
        cases = [c for c in C.cases(N, qm[a:a + N]) if c[0].split("/")[0] in ("ties", "spikes")]
        assert any("flat_pos" in c[0] for c in cases) and any("pairs_shuffled" in c[0] for c in cases)
        assert any("spikes/last_const" in c[0] for c in cases)
        fine = qt.q_band(pli, bs)
        out = []
        rng = np.random.RandomState(7)
        for q, group in ((fine[band], [c for c in cases if C._inside(c, fine[band])]),
                         (Q_COARSE, [c for c in cases if not C._inside(c, fine[band])])):
            assert group and all(C._inside(c, q) for c in group)
            x = np.zeros((1, n, n * len(group)), np.int32)
            r = np.zeros((1, n, n * len(group)), np.int32)
            names = {}
            for blk, (name, _, x0, r0) in enumerate(group):
                vx = rng.randint(-30, 31, size=n * n).astype(np.int32)
                vr = rng.randint(-30, 31, size=n * n).astype(np.int32)
                vx[a:a + N], vr[a:a + N] = x0, r0
                names[(blk, band)] = name
                x[0, :, blk * n:(blk + 1) * n] = _to_raster(vx, n)
                r[0, :, blk * n:(blk + 1) * n] = _to_raster(vr, n)
            qb = _per_band(fine, bs, [q])
            bb = qt.beta_band(pli, bs)
            traces, _ = oracle_traces(x, r, bs, qm, qmi, qb, bb, is_keyframe, pli, hip.OD_PVQ_LAMBDA)
            out.append((bs, x, r, names, qm, qmi, qb, bb, traces))
        _cache[key] = out
    return _cache[key]


@pytest.mark.parametrize("is_keyframe,pli", [(1, 1), (0, 0)])
@pytest.mark.parametrize("force_seq", [False, True], ids=["tournament", "force_seq"])
def test_group_search_decides_the_tie_corpus_as_the_oracle(hip, is_keyframe, pli, force_seq, monkeypatch):
    if force_seq:
        monkeypatch.setenv("ODHIP_PVQ_FORCE_SEQ", "1")
    inputs = _corpus_inputs(hip, (is_keyframe, pli))
    assert sum(len(i[3]) for i in inputs) > 60
    _, jobs, _, k_range = _run(hip, None, (is_keyframe, pli), inputs)
    _assert_oracle(inputs, jobs, "tie corpus")
    assert k_range == (0, 0)


# ---- the three forms of the experiments build, and the default build ---------------------------------------
CHILD_MODES = [(1, 1), (0, 0)]


def _outputs(hip):
    out = {}
    for mode in CHILD_MODES:
        for call in sorted(CALLS):
            _, jobs, listed, k_range = _run(hip, call, mode)
            for i, job in enumerate(jobs):
                out["choice_%d%d_%s%d" % (mode + (call, i))] = job.choice.cpu().numpy()
                out["y_%d%d_%s%d" % (mode + (call, i))] = job.y.cpu().numpy()
            out["counts_%d%d_%s" % (mode + (call,))] = np.array(list(listed) + list(k_range))
    return out


def _child():
    """In a process that loaded the experiments build: both modes, with whatever switches the parent set; the
    outputs of every job into the .npz named on the command line."""
    import daala_amd
    daala_amd.init(0)
    assert hasattr(daala_amd.lib(), "odhip_exp_row_replay_stats"), "the experiments build is expected here"
    out = _outputs(daala_amd)
    np.savez(sys.argv[1], **out)
    print(json.dumps(dict(arrays=len(out))))


def test_row_quad_and_pair_searches_agree_experiments_build_and_default_build(hip, tmp_path):
    """The experiments build keeps k_refb_lean_row<8, 16> for these bands unless ODHIP_REFB_GROUP128 is 4 (the
    quad) or 2 (the pair): choice records, pulse buffers, listed-band counts and K-range counts of both modes,
    byte for byte, from one child process per form, and the same from the default build in this process."""
    import daala_amd
    got = dict(default=_outputs(hip))
    for form, value in (("row", None), ("quad", "4"), ("pair", "2")):
        env = dict(os.environ)
        env.update(ODHIP_LIB=daala_amd.EXPERIMENTS_LIB)
        env.pop("ODHIP_REFB_GROUP128", None)
        if value:
            env["ODHIP_REFB_GROUP128"] = value
        path = str(tmp_path / (form + ".npz"))
        r = subprocess.run([sys.executable, os.path.abspath(__file__), path], env=env, capture_output=True,
                           text=True, timeout=600, cwd=ROOT)
        assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-2000:]
        got[form] = np.load(path)
    want = got["default"]
    njobs = sum(len(v) for v in CALLS.values())
    assert len(want) == len(CHILD_MODES) * (2 * njobs + len(CALLS))
    for form in ("row", "quad", "pair"):
        assert sorted(got[form].files) == sorted(want), form
        for name in want:
            a, b = want[name], got[form][name]
            assert a.dtype == b.dtype and a.shape == b.shape and a.tobytes() == b.tobytes(), (form, name)
    assert any(want[n].any() for n in want if n.startswith("y_"))


if __name__ == "__main__":
    sys.path.insert(0, ROOT)
    _child()
