"""CPU only: the directed corpus of the PVQ band stages (tests/_pvq_corpus.py) is what it says it
is, stays inside what the library's layouts hold, and the oracle's pvq_theta equals the
reference's on every run of it - live against the compiled reference (oracle/_ref) where built,
always against tests/golden/pvq_corpus.npz (tools/make_golden_pvq_corpus.py: the reference's
recorded results)."""
import ctypes
import math
import os

import numpy as np
import pytest

import _pvq_corpus as C
import _pvq_corpus_oracle as R
from _libs import GOLDEN, P, oracle, ref

ODHIP_PVQ_MAX_K = 32767
TRACE_SLOTS = 24


RATE_TOL_REL = RATE_TOL_ABS = 1e-10      # odq_rate_tol (daala_amd/csrc/od_pvq_math.cuh): 1e-10*(|a| + |b|) + 1e-10
THETA_SCALE = 32768 * 2. / math.pi       # OD_THETA_SCALE
THETA_NEAR = 1e-8                        # ten times the device margin of the theta argument


def _costs(o, tr, n, kf, pli):
    """The costs pvq_theta compares in one run, from its trace: the null (or skip) candidate at dist0 - it
    places no pulse and has gain 0, so od_pvq_rate gives it 0 - and every searched candidate at
    dist + lambda*od_pvq_rate (speed 1)."""
    costs = [tr.dist0]
    for i in range(tr.ncands):
        c = tr.cands[i]
        if not c.searched:
            continue
        y = np.array(c.y[:n], np.int32)
        if c.with_ref:
            rate = o.odo_pvq_rate_speed1(c.gain, tr.icgr, c.theta, c.ts, P(y), c.k, n, kf, pli)
        else:
            rate = o.odo_pvq_rate_speed1(c.gain, 0, -1, 0, P(y), c.k, n, kf, pli)
        costs.append(c.dist + R.LAMBDA * rate)
    return costs


def _close_call(costs):
    """Any two costs within twice odq_rate_tol of each other: every pair, a superset of the comparisons
    pvq_theta makes (each candidate against the best so far)."""
    c = np.array(costs, np.float64)
    a = np.abs(c)
    i, j = np.triu_indices(len(c), 1)
    return bool((np.abs(c[i] - c[j]) <= 2 * (RATE_TOL_REL * (a[i] + a[j]) + RATE_TOL_ABS)).any())


def _near_theta(tr, r0):
    """The run searches with a reference and its theta argument lies within THETA_NEAR of an integer."""
    if not r0.any() or not tr.corr > 0:
        return False
    t = .5 + THETA_SCALE * math.acos(tr.corr)
    return abs(t - round(t)) <= THETA_NEAR


@pytest.fixture(scope="module")
def oracle_runs():
    """Every run through the oracle, once: per run the result record, the largest candidate K, ncands,
    whether any two candidate costs are a close call and whether theta sits on a rounding boundary."""
    o = oracle()
    o.odo_pvq_rate_speed1.restype = ctypes.c_double
    tr = R.new_trace()
    out = dict(rows=[], kmax=[], ncands=[], meta=[], close=[], near=[])
    for (matrix, kf, pli, n, name, x0, r0, q0, beta, qm, qmi) in R.runs():
        res = R.theta(o.odo_pvq_theta, x0, r0, n, q0, beta, kf, pli, qm, qmi, trace=tr)
        out["rows"].append(R.record(res))
        out["kmax"].append(max([tr.cands[i].k for i in range(tr.ncands)] + [0]))
        out["ncands"].append(tr.ncands)
        out["meta"].append((matrix, kf, pli, n, name, q0))
        out["close"].append(_close_call(_costs(o, tr, n, kf, pli)))
        out["near"].append(_near_theta(tr, r0))
    return out


@pytest.fixture(scope="module")
def oracle_rows(oracle_runs):
    return oracle_runs["rows"], oracle_runs["kmax"], oracle_runs["ncands"], oracle_runs["meta"]


def _trace(kf, pli, n, matrix="hvs"):
    """Per case of the band (name, x16, r16 as pvq_theta scales them, trace) at the coarsest quantiser
    (what the classes are named for - the scaled vectors, corr, the axis - does not depend on it)."""
    o = oracle()
    qm, qmi, beta, cs = R.band_setup(matrix, pli, n)
    out = []
    for name, _, x0, r0 in cs:
        q0 = C.QUANTIZERS[-1]
        if name.startswith("ladder/"):
            q0 = int(name.split("/")[1].split("_")[0][1:])
        tr = R.new_trace()
        R.theta(o.odo_pvq_theta, x0, r0, n, q0, beta, kf, pli, qm, qmi, trace=tr)
        x16 = np.array(tr.x16[:n], np.int64)
        # the trace's r16 is taken after od_compute_householder moved r16[m]: scale it here
        r16 = C.scale16(r0, qm, tr.rshift).astype(np.int64)
        assert np.array_equal(x16, C.scale16(x0, qm, tr.xshift)), name
        assert tr.xshift == C.band_shift(x0, 15) and tr.rshift == C.band_shift(r0, 14), name
        out.append((name, x0, r0, x16, r16, tr))
    return out


def _collinear(a, b):
    return np.array_equal(np.outer(a, b), np.outer(b, a))


@pytest.mark.parametrize("n", C.SIZES)
@pytest.mark.parametrize("is_keyframe,pli,matrix", [m + ("hvs",) for m in R.MODES] + [(0, 0, "flat")])
def test_every_class_shows_the_property_it_is_named_for(is_keyframe, pli, matrix, n):
    seen = {}
    shifts = set()
    ladders = {}
    for name, x0, r0, x16, r16, tr in _trace(is_keyframe, pli, n, matrix):
        cls, variant = name.split("/")[:2]
        seen.setdefault(cls, set())
        ax, ar = np.abs(x16), np.abs(r16)
        r_null = not r0.any()
        ran = (not r_null) and tr.corr > 0
        shifts.add((tr.xshift, tr.rshift))
        assert not np.isnan(tr.corr), name
        if cls == "nulls":
            if variant.startswith("x0_"):
                assert not x16.any(), name
            if variant.endswith("_r0"):
                assert r_null and not r16.any(), name
            seen[cls].add(variant)
        elif cls in ("collinear", "anti"):
            sign = 1 if cls == "collinear" else -1
            assert _collinear(x16, r16) and sign * int((x16 * r16).sum()) > 0, name
            assert sign * tr.corr > 0.5, (name, tr.corr)       # g, gr are rounded integer square roots
            if tr.corr == sign * 1.0:
                seen[cls].add("corr == +-1")
            if cls == "collinear" and np.array_equal(x16, r16):
                seen[cls].add("x16 == r16")
        elif cls == "gate":
            assert int((x16 * r16).sum()) != 0 or tr.corr == 0.0, name
            if variant.endswith("_plus"):
                assert tr.corr > 0 and ran, (name, tr.corr)
                seen[cls].add("corr > 0")
            elif variant.endswith("_minus"):
                assert tr.corr < 0, (name, tr.corr)
                seen[cls].add("corr < 0")
            else:
                assert tr.corr == 0.0 and not r_null, (name, tr.corr)
                seen[cls].add("corr == 0")
        elif cls == "near1":
            assert tr.corr > 0.5 and not _collinear(x16, r16), (name, tr.corr)
            if int(np.abs(x16 - r16).sum()) == 1:
                seen[cls].add("one LSB")
                if tr.corr == 1.0:
                    seen[cls].add("one LSB, corr clamps to 1")
                else:
                    seen[cls].add("one LSB, corr < 1")
        elif cls == "axis":
            assert ran, (name, tr.corr)
            first = int(np.argmax(ar))
            assert tr.m == first and tr.s == (1 if r16[first] > 0 else -1), (name, tr.m, tr.s)
            nmax = int((ar == ar.max()).sum())
            if variant in ("max_at_0", "max_at_last", "unique_on_spike"):
                assert nmax == 1, name
                assert first == {"max_at_0": 0, "max_at_last": n - 1, "unique_on_spike": n // 2}[variant]
                if variant == "unique_on_spike":
                    assert np.flatnonzero(x16).tolist() == [first], name
                seen[cls].add("unique")
            else:
                assert nmax == (n if variant.startswith("all_equal") else max(2, nmax)), (name, nmax)
                assert nmax >= 2, name
                seen[cls].add("equal maxima")
                if tr.s < 0:
                    seen[cls].add("equal maxima, s = -1")
        elif cls == "ties":
            if variant.startswith("flat_"):
                assert ax.min() == ax.max() > 0, name
                seen[cls].add("flat")
            elif variant.startswith("two_level"):
                assert len(set(ax.tolist())) == 2 and ax.min() > 0, name
                seen[cls].add("two levels")
            elif variant.startswith("pairs_shuffled"):
                counts = np.unique(ax, return_counts=True)[1]
                assert (counts >= 2).sum() >= n // 2, name
                seen[cls].add("pairs")
            else:
                j = int(variant[len("apart"):].split("_")[0])
                top = np.flatnonzero(ax == ax.max())
                assert len(top) == 2 and top[1] - top[0] == j, (name, top)
                seen[cls].add("apart")
            if variant.endswith("_r0"):
                assert r_null, name
            else:
                assert ran and int((ar == ar.max()).sum()) == 1, (name, tr.corr)
                seen[cls].add("ties beside the axis")
        elif cls == "spikes":
            if variant.startswith("floor"):
                vals, counts = np.unique(ax, return_counts=True)
                assert len(vals) == 2 and counts[1] == 1 and vals[0] > 0, name
                seen[cls].add("floor")
            else:
                assert np.count_nonzero(x16) == 1, name
                seen[cls].add("spike")
        elif cls == "ladder":
            q0 = int(variant.split("_")[0][1:])
            ladders.setdefault(q0, []).append(tr.cg >> 8)
            seen[cls].add(q0)
        else:
            raise AssertionError("unknown class " + cls)
    assert set(seen) == set(C.CLASSES)
    assert seen["nulls"] >= {"x0_r0", "x0_rramp", "xramp_r0"}
    assert seen["collinear"] >= {"corr == +-1", "x16 == r16"} and "corr == +-1" in seen["anti"]
    assert seen["gate"] == {"corr > 0", "corr < 0", "corr == 0"}
    assert seen["near1"] >= {"one LSB", "one LSB, corr < 1"}
    assert seen["axis"] == {"unique", "equal maxima", "equal maxima, s = -1"}
    assert seen["ties"] == {"flat", "two levels", "pairs", "apart", "ties beside the axis"}
    assert seen["spikes"] == {"floor", "spike"}
    # the ladders climb from gain index 0 (skip against gain 1) over at least two more boundaries;
    # at the finest quantiser under beta = 1.5 the companded gain of the smallest band the shape has
    # (|x16| = (2, 1, 0, 0)) is already above 1, and the ladder starts there
    assert set(ladders) == set(C.QUANTIZERS)
    beta = R.band_setup(matrix, pli, n)[2]
    for q0, gains in ladders.items():
        assert len(gains) == 16 and gains == sorted(gains), (q0, gains)
        assert len(set(gains)) >= 3, (q0, gains)
        assert gains[0] == 0 or (q0 == min(C.QUANTIZERS) and beta != 4096), (q0, gains)
    # the magnitudes drive both shifts from 0 to their largest values at the pipeline's peak
    assert (0, 0) in shifts and max(s[0] for s in shifts) >= 3 and max(s[1] for s in shifts) >= 4
    amps = {int(c[0].split("/")[2][1:]) for c in R.band_setup(matrix, pli, n)[3] if not c[0].startswith("ladder/")}
    assert amps == set(C.AMPLITUDES)


def test_conditions_on_the_inputs(oracle_rows):
    """No case is dropped from any comparison, no candidate K exceeds ODHIP_PVQ_MAX_K, no trace is
    full: bounds on the inputs (the oracle alone decides them), not on any code under test."""
    rows, kmax, ncands, meta = oracle_rows
    for matrix in ("hvs", "flat"):
        for pli in (0, 1):
            for n in C.SIZES:
                for name, _, x0, r0 in R.band_setup(matrix, pli, n)[3]:
                    assert C.quantizers_for(n, x0), name
                    assert np.abs(x0).max(initial=0) <= 1.05 * C.AMPLITUDES[-1], name
    compared = {(m[0], m[1], m[2], m[3], m[4]) for m in meta}
    want = sum(len(R.band_setup(matrix, pli, n)[3]) for matrix in ("hvs", "flat")
               for _, pli in R.MATRIX_MODES[matrix] for n in C.SIZES)
    assert len(compared) == want
    worst = int(np.argmax(kmax))
    assert kmax[worst] <= ODHIP_PVQ_MAX_K, (meta[worst], kmax[worst])
    assert max(ncands) < TRACE_SLOTS, meta[int(np.argmax(ncands))]
    assert kmax[worst] > 10000            # and the corpus does reach large K
    assert {m[5] for m in meta} == set(C.QUANTIZERS)


def test_close_calls_and_boundary_thetas_are_rare(oracle_runs):
    """What the GPU tests of the priced stages (tests/test_gpu_pvq_corpus_decided.py) rest their cap on the
    resolved bands on: per band size, and per (matrix, mode) within it, at most 2 % of the corpus runs hold
    two candidate costs within twice odq_rate_tol of each other (such a band is handed to the host libm),
    and at most 2 % a theta argument .5 + OD_THETA_SCALE*acos(corr) within 1e-8 of an integer (such a band
    is re-run with the host's theta).  From the oracle's traces and its od_pvq_rate alone."""
    groups = {}
    for m, close, near in zip(oracle_runs["meta"], oracle_runs["close"], oracle_runs["near"]):
        matrix, kf, pli, n, name, _ = m
        for key in ((n,), (n, matrix, kf, pli)):
            g = groups.setdefault(key, dict(runs=0, close=[], near=[]))
            g["runs"] += 1
            if close:
                g["close"].append(m)
            if near:
                g["near"].append(m)
    assert {k[0] for k in groups} == set(C.SIZES)
    for n in C.SIZES:
        g = groups[(n,)]
        print("band size %3d: %5d runs, close calls %d (%.3f %%), near-boundary thetas %d (%.3f %%)%s"
              % (n, g["runs"], len(g["close"]), 100. * len(g["close"]) / g["runs"], len(g["near"]),
                 100. * len(g["near"]) / g["runs"],
                 "".join("\n    close: %s %s q%d" % (m[0], m[4], m[5]) for m in g["close"][:4])))
    for key, g in sorted(groups.items()):
        assert g["runs"] > 500, key
        assert len(g["close"]) <= 0.02 * g["runs"], (key, len(g["close"]), g["runs"], g["close"][:3])
        assert len(g["near"]) <= 0.02 * g["runs"], (key, len(g["near"]), g["runs"], g["near"][:3])


def test_oracle_equals_the_recorded_reference(oracle_rows):
    rows, _, _, meta = oracle_rows
    g = np.load(os.path.join(GOLDEN, "pvq_corpus.npz"))
    assert os.path.getsize(os.path.join(GOLDEN, "pvq_corpus.npz")) < 300 * 1024
    assert int(g["inputs_digest"]) == R.inputs_digest(), "the corpus generator drifted: regenerate the fixture"
    assert int(g["count"]) == len(rows)
    got = np.array(rows, np.int64)
    for i, f in enumerate(R.FIELDS):
        bad = np.flatnonzero(got[:, i] != g[f].astype(np.int64))
        assert len(bad) == 0, (f, len(bad), meta[int(bad[0])])


@pytest.mark.skipif(ref() is None, reason="oracle/_ref (the compiled reference) not present")
def test_oracle_equals_the_compiled_reference(oracle_rows):
    rows, _, _, meta = oracle_rows
    r = ref()
    o = oracle()
    for i, (matrix, kf, pli, n, name, x0, r0, q0, beta, qm, qmi) in enumerate(R.runs()):
        want = R.theta(r.ref_pvq_theta, x0, r0, n, q0, beta, kf, pli, qm, qmi, trace=False)
        assert R.record(want) == rows[i], meta[i]
        if i % 7 == 0:      # out, y and skip_diff themselves (the records hold their CRCs)
            got = R.theta(o.odo_pvq_theta, x0, r0, n, q0, beta, kf, pli, qm, qmi)
            assert np.array_equal(got["out"], want["out"]) and np.array_equal(got["y"], want["y"]), meta[i]
            assert got["skip_diff"] == want["skip_diff"], meta[i]
