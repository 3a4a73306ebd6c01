"""GPU: the with-reference 32-coefficient bands of the decided stage, searched a lane PAIR per band
(k_refb_lean_pair<16>: od_lane_search of daala_amd/csrc/pvq_lane.cuh with a PAD, PairVector), every
decision against the CPU oracle's pvq_theta at speed 1 - gain index, theta, K, the winner's pulses, the
choice record (test_gpu_pvq_corpus_decided._compare_decided) - and, in a child process on the experiments
build, byte for byte against k_refb_lean_row<8, 4>, the quad form these bands left (ODHIP_REFB_ROW32).

The planes are small and directed at what a pair can get wrong.  A band's reference is a spike at its
first coefficient wherever a tie is wanted: the Householder reflection is then across that axis, and the
vector a theta candidate searches is the band without its first coefficient - positions 1..31 become the
31 dimensions 0..30 in front of the PAD, with their magnitudes (and ties) as they are.  _stats counts,
from the oracle's traces alone, what the inputs were built to hold (K = 0, 2, small K, chains, pulse
counts beyond the 1/sqrt table, products beyond 2^52, the ties where the halves of a pair meet); those
counts are conditions on the inputs, asserted before anything is compared.

Two things about K.  od_pvq_compute_k never gives K = 1 for 32 coefficients (with a reference K is 0, 3, 7,
12, ..; without one it is at least 2, and 2 only at beta = 1.5: one job sets that beta for its band), so
the searches that start from zero are those of K = 2.  And a greedy pulse beyond the 2^52 bound - the
pair's sequential rescan outside ODHIP_PVQ_FORCE_SEQ - needs K near 100 (more pulses, and the last 1 + K/4
of them leave no greedy one behind the projection) on a band that keeps both xy and yy large and still
leaves ~30 pulses to place: one coefficient of 16000 (the flat matrix reaches that inside the pipeline's
peak amplitude) among 30 equal small ones, each just under one projected pulse - the "spiky" job.

  level 0 is 4x4 (no 32-coefficient band); level 1 (8x8) holds band 3, level 2 (16x16) bands 3-5, level 3
  (32x32) bands 3-5 beside its 128-coefficient bands.  Block counts per job: 70 and 42 (no multiple of
  the 32 bands of a wavefront), 21, 9, 7 and 3 (a partial wavefront, idle pairs)."""
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
from test_gpu_pvq_corpus import _tables, _to_raster
from test_gpu_pvq_corpus_decided import _compare_decided, _cuda

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
MODES = [(1, 1), (0, 0)]          # keyframe chroma from luma; an inter job
N = 32
BIG = 40                          # the tied magnitude of a shape; everything else is at most SMALL
SMALL = 12
AMPS = (3, 20, 400, 8000, 270000)
# (table set, level, quantisers of the 32-coefficient bands - per mode where a dict -, their beta where not the
# tables', plane height, plane width)
JOBS = (("default", 1, (37,), None, 16, 280), ("default", 1, (243,), None, 16, 168),
        ("default", 1, (1264,), 6144, 8, 168), ("default", 2, (37, 243, 1264), None, 16, 112),
        ("default", 3, (37, 243, 37), None, 32, 96), ("flat", 1, {(1, 1): (775,), (0, 0): (340,)}, None, 8, 72))
NBANDS32 = 70 + 42 + 21 + 3 * 7 + 3 * 3 + 9
SHAPES = ("lower", "upper", "cross", "mid", "last", "last_big", "single", "single_last", "zero", "flat",
          "laplace", "noref", "zero_noref")

_cache = {}


def _shape(name, rng):
    """(vx, vr): integer shapes of a band and its reference; x16 = vx*mult, r16 = vr*mult'."""
    sign = rng.choice([-1, 1], size=N)
    v = rng.randint(1, SMALL + 1, size=N) * sign
    tied = dict(lower=(4, 8, 12), upper=(20, 24, 28), cross=(6, 22), mid=(15, 16, 17), last=(30, 31),
                last_big=(31,)).get(name)
    if tied:
        v[list(tied)] = BIG * sign[list(tied)]
    elif name in ("single", "single_last"):
        v[:] = 0
        v[31 if name == "single_last" else 9] = BIG
    elif name in ("zero", "zero_noref"):
        v[:] = 0
    elif name == "flat":
        v = 5 * sign
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


def _from_targets(t, qm, headroom):
    """The int32 band whose QM-scaled int16 image is t at the shift pvq_theta derives from the band itself."""
    for shift in range(12):
        x0 = C._preimage(t, qm, shift)
        if C.band_shift(x0, headroom) == shift:
            return x0
    raise AssertionError("no self-consistent shift")


def _spiky(blk, qm):
    """x16 = 16000 at position 1 among 30 coefficients of 205 + 6*blk (just under one projected pulse each at
    K = 90 .. 115), a third of it at the pivot; r16 a spike."""
    t = np.full(N, 205 + 6 * blk, np.int64)
    t[2::2] *= -1
    t[0], t[1] = 16000 // 3, 16000
    tr = np.zeros(N, np.int64)
    tr[0] = 3000
    return _from_targets(t, qm, 15), _from_targets(tr, qm, 14)


def _planes(which, bs, h, w, dec, hip):
    """One plane of h x w at level bs: the 32-coefficient bands of block b hold shape b % len(SHAPES) at
    amplitude (b // len(SHAPES) + band) % len(AMPS) - with the flat matrix: _spiky -, the other bands
    small Laplacian filler."""
    key = ("planes", which, bs, h, w, dec)
    if key in _cache:
        return _cache[key]
    qt = _tables(hip, which)
    qm, qmi = qt.qm_slices(dec, bs)
    n = 4 << bs
    rng = np.random.RandomState(1000 * bs + w + dec)
    x = np.zeros((1, h, w), np.int32)
    r = np.zeros((1, h, w), np.int32)
    names = {}
    nb = C.NBANDS[bs]
    for blk in range((h // n) * (w // n)):
        vx = np.zeros(n * n, np.int32)
        vr = np.zeros(n * n, np.int32)
        end = C.BAND_OFFSETS[nb]
        vx[:end] = np.round(rng.laplace(size=end) * 30)
        vr[:end] = vx[:end] + np.round(rng.laplace(size=end) * 20)
        for b in range(nb):
            a = C.BAND_OFFSETS[b]
            if C.BAND_OFFSETS[b + 1] - a != N:
                continue
            if which == "flat":
                vx[a:a + N], vr[a:a + N] = _spiky(blk, qm[a:a + N])
                names[(blk, b)] = "spiky@%d" % blk
                continue
            name = SHAPES[(blk + 5 * b) % len(SHAPES)]
            amp = AMPS[(blk // len(SHAPES) + b) % len(AMPS)]
            sx, sr = _shape(name, rng)
            vx[a:a + N] = C.lift(sx, np.zeros(N, np.int64), qm[a:a + N], amp, 15)[0]
            vr[a:a + N] = C.lift(sr, np.zeros(N, np.int64), qm[a:a + N], amp, 14)[0]
            names[(blk, b)] = "%s@%d" % (name, amp)
        by, bx = divmod(blk, w // n)
        x[0, by * n:(by + 1) * n, bx * n:(bx + 1) * n] = _to_raster(vx, n)
        r[0, by * n:(by + 1) * n, bx * n:(bx + 1) * n] = _to_raster(vr, n)
    for a in (x, r):
        a.setflags(write=False)
    _cache[key] = (x, r, names, qm, qmi)
    return _cache[key]


def _per_band(base, bs, v32):
    """The per-band list `base` with the entries of the 32-coefficient bands replaced by those of v32."""
    out = list(base)
    it = iter(v32)
    for b in range(C.NBANDS[bs]):
        if C.BAND_OFFSETS[b + 1] - C.BAND_OFFSETS[b] == N:
            out[b] = next(it)
    return out


def _inputs(hip, mode):
    """Per job of JOBS: (bs, x, r, names, qm, qmi, q_band, beta_band, traces), the oracle's traces once
    per session."""
    key = ("inputs", mode)
    if key not in _cache:
        is_keyframe, pli = mode
        dec = 1 if pli else 0
        out = []
        for which, bs, q32, beta, h, w in JOBS:
            qt = _tables(hip, which)
            x, r, names, qm, qmi = _planes(which, bs, h, w, dec, hip)
            qb = _per_band(qt.q_band(pli, bs), bs, q32[mode] if isinstance(q32, dict) else q32)
            bb = qt.beta_band(pli, bs)
            if beta:
                bb = _per_band(bb, bs, [beta] * 3)
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
    """What the traces of the 32-coefficient bands hold of the cases this file is about."""
    st = dict(bands=0, k0=0, k1=0, k2=0, ksmall=0, fresh=0, chained=0, beyond_table=0, rescan_pulses=0,
              theta_won=0, noref_won=0)
    ties = {}
    for bs, _, _, names, _, _, _, _, traces in inputs:
        for (blk, b), t in traces.items():
            if t["n"] != N:
                continue
            st["bands"] += 1
            st["theta_won" if t["itheta"] != -1 else "noref_won"] += t["vk"] > 0
            tr = t["tr"]
            for with_ref in (1, 0):
                cands = [tr.cands[i] for i in range(tr.ncands) if tr.cands[i].with_ref == with_ref]
                if not any(c.searched for c in cands):
                    continue
                v = _searched(t, with_ref)
                nn = N - with_ref
                name = names[(blk, b)].split("@")[0]
                top = v.max()
                at = set(np.flatnonzero(v == top)) if top > 0 else set()
                # positions of the searched vector: the pair's halves are 0..15 and 16..31
                for what, want in (("lower", {3, 7, 11}), ("upper", {19, 23, 27}), ("cross", {5, 21}),
                                   ("mid", {14, 15, 16}), ("last", {29, 30}), ("last_big", {30})):
                    if with_ref and name == what and at == want:
                        ties[what + ".theta"] = ties.get(what + ".theta", 0) + 1
                for what, want in (("lower", {4, 8, 12}), ("cross", {6, 22}), ("mid", {15, 16, 17}),
                                   ("last", {30, 31})):
                    if not with_ref and name == what and at == want:
                        ties[what + ".noref"] = ties.get(what + ".noref", 0) + 1
                if name in ("single", "single_last") and np.count_nonzero(v) == 1:
                    ties[name] = ties.get(name, 0) + 1
                if name == "flat" and len(at) >= nn - 1:
                    ties["flat"] = ties.get("flat", 0) + 1
                prev_k, prev_y = 0, None
                for c in cands:
                    if c.k == 0:
                        st["k0"] += 1
                        prev_k = 0
                    if not c.searched or c.k == 0:
                        continue
                    st["k1"] += c.k == 1
                    st["k2"] += c.k == 2
                    st["ksmall"] += 2 < c.k <= 8
                    y = np.abs(np.array(c.y[:nn], np.int64))
                    assert int(y.sum()) == c.k
                    if c.k != prev_k:
                        chained = 0 < prev_k <= c.k
                        st["chained" if chained else "fresh"] += 1
                        # the last pulse looks up 1/sqrt(yy + 2*y_j + 1) with yy of the pulses before it
                        st["beyond_table"] += int((y * y).sum()) - 2 * int(y.max()) + 1 + 2 > 512
                        # where the search starts: the chain's pulses, or the projection (K > 2)
                        y0 = prev_y if chained else np.floor(c.k * v.astype(np.float64)
                                                             * (1.0 / max(float(v.sum()), 1e-100))).astype(np.int64)
                        if not chained and c.k <= 2:
                            y0 = np.zeros_like(v)
                        greedy = (c.k - 1 - c.k // 4) - int(y0.sum())
                        if greedy > 0:
                            # od_lane_search's bound at the first greedy pulse, in its arithmetic
                            tmax = float(int((v * y0).sum()) + int(top))
                            if not (tmax * tmax) * float(int((y0 * y0).sum()) + 2 * c.k + 1) < 4503599627370496.:
                                st["rescan_pulses"] += greedy
                    prev_k, prev_y = c.k, y
    zero = sum(1 for _, _, _, names, *_ in inputs for nm in names.values() if nm.startswith("zero"))
    return st, ties, zero


def _jobs(hip, inputs, mode):
    is_keyframe, pli = mode
    return [hip.PvqRefJob(_cuda(x), _cuda(r), bs, _cuda(qm), _cuda(qmi), qb, bb, is_keyframe, pli)
            for bs, x, r, _, qm, qmi, qb, bb, _ in inputs]


def _run(hip, mode):
    import torch
    inputs = _inputs(hip, mode)
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
        assert mm.total() == 0, (tag, job.bs, mm.summary(), bad)
    assert mm.checked["y"] == sum(j.nblocks * j.nb for j in jobs)


@pytest.mark.parametrize("is_keyframe,pli", MODES)
def test_inputs_hold_the_cases(hip, is_keyframe, pli):
    """Conditions on the inputs, from the oracle's traces: every case the pair search can get wrong is
    there, on the vector that is really searched."""
    st, ties, zero = _stats(_inputs(hip, (is_keyframe, pli)))
    print(st, ties, zero)
    assert st["bands"] == NBANDS32 and st["k1"] == 0
    for what in ("k0", "k2", "ksmall", "fresh", "chained", "noref_won"):
        assert st[what] > 0, (what, st)
    assert st["theta_won"] > 10 and st["chained"] > 50, st
    assert st["beyond_table"] > 0 and st["rescan_pulses"] > 0, st
    for what in ("lower.theta", "upper.theta", "cross.theta", "mid.theta", "last.theta", "last_big.theta",
                 "cross.noref", "mid.noref", "last.noref", "single", "single_last", "flat"):
        assert ties.get(what, 0) > 0, (what, ties)
    assert zero > 10


@pytest.mark.parametrize("is_keyframe,pli", MODES)
@pytest.mark.parametrize("force_seq", [False, True], ids=["tournament", "force_seq"])
def test_pair_search_decides_as_the_oracle(hip, is_keyframe, pli, force_seq, monkeypatch):
    """odhip_pvq_ref_bands_decided_multi on the five jobs in one call, every test hook off; and with
    ODHIP_PVQ_FORCE_SEQ=1, the halves of every pair combined by the sequential rescan."""
    if force_seq:
        monkeypatch.setenv("ODHIP_PVQ_FORCE_SEQ", "1")
    inputs, jobs, listed, k_range = _run(hip, (is_keyframe, pli))
    _assert_oracle(inputs, jobs, "force_seq" if force_seq else "plain")
    assert k_range == (0, 0)
    nbands = sum(j.nblocks * j.nb for j in jobs)
    # the resolves re-run what they list through other kernels: they must stay the exception here
    assert sum(listed) <= 0.1 * nbands, (listed, nbands)


@pytest.mark.parametrize("is_keyframe,pli", MODES)
@pytest.mark.parametrize("forced", ["theta", "price"])
def test_forced_resolves_list_and_redecide_the_bands(hip, forced, is_keyframe, pli):
    """The theta margin at 0.25 with the perturbation (tests/test_gpu_pvq_refbands.py), and the price margin
    scaled by 1e12: the bands are listed by the stage and re-decided by the resolves, as the oracle decides."""
    try:
        if forced == "theta":
            hip.pvq_ref_set_theta_margin(0.25, True)
        else:
            hip.set_price_tol_scale(1e12)
        inputs, jobs, (nt, npz), k_range = _run(hip, (is_keyframe, pli))
    finally:
        hip.pvq_ref_set_theta_margin(0, False)
        hip.set_price_tol_scale(1.)
    _assert_oracle(inputs, jobs, "forced " + forced)
    assert k_range == (0, 0)
    assert (nt if forced == "theta" else npz) > 20


def _child():
    """In a process that loaded the experiments build: both modes, with whatever switches the parent set;
    the outputs of every job into the .npz named on the command line."""
    import daala_amd
    daala_amd.init(0)
    assert hasattr(daala_amd.lib(), "odhip_exp_row_replay_stats"), "the experiments build is expected here"
    out = {}
    for mode in MODES:
        _, jobs, listed, k_range = _run(daala_amd, mode)
        for i, job in enumerate(jobs):
            out["choice_%d%d_%d" % (mode + (i,))] = job.choice.cpu().numpy()
            out["y_%d%d_%d" % (mode + (i,))] = job.y.cpu().numpy()
        out["counts_%d%d" % mode] = np.array(list(listed) + list(k_range))
    np.savez(sys.argv[1], **out)
    print(json.dumps(dict(arrays=len(out))))


def test_pair_search_equals_the_quad_search_experiments_build(tmp_path):
    """The experiments build keeps k_refb_lean_row<8, 4> for these bands behind ODHIP_REFB_ROW32: choice
    records, pulse buffers, listed-band counts and K-range counts of both modes, byte for byte, from one
    child process per form."""
    import daala_amd
    got = {}
    for form in ("pair", "row"):
        env = dict(os.environ)
        env.update(ODHIP_LIB=daala_amd.EXPERIMENTS_LIB)
        env.pop("ODHIP_REFB_ROW32", None)
        if form == "row":
            env["ODHIP_REFB_ROW32"] = "1"
        path = str(tmp_path / (form + ".npz"))
        r = subprocess.run([sys.executable, os.path.abspath(__file__), path], env=env, capture_output=True,
                           text=True, timeout=600, cwd=ROOT)
        assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-2000:]
        got[form] = np.load(path)
    assert sorted(got["pair"].files) == sorted(got["row"].files) and len(got["pair"].files) == 2 * (2 * len(JOBS) + 1)
    for name in got["pair"].files:
        a, b = got["pair"][name], got["row"][name]
        assert a.dtype == b.dtype and a.shape == b.shape and a.tobytes() == b.tobytes(), name
    assert any(got["pair"][n].any() for n in got["pair"].files if n.startswith("y_"))


if __name__ == "__main__":
    sys.path.insert(0, ROOT)
    _child()
