"""GPU: the PVQ band stages on the directed corpus (tests/_pvq_corpus.py) - tied, degenerate and
extreme bands that random Laplacian data almost never holds.  Every check is exact equality with
the CPU oracle (itself pinned to the reference on this corpus by tests/test_pvq_corpus_host.py):
the with-reference building blocks band by band, the with-reference and the no-reference band
stage on planes that hold the corpus, the stand-alone search on the tie and spike vectors, and the
band decoder fed with the oracle's own decisions."""
import ctypes

import numpy as np
import pytest

import _pvq_corpus as C
import _pvq_corpus_oracle as R
from _libs import P, oracle
from _refbands import Mismatch, compare_bands, compare_choice, host_rates, oracle_traces
from test_gpu_pvq_bands import _check_level_against_oracle, _cuda, hip  # noqa: F401
from test_gpu_pvq_refbands import MODES

pytestmark = pytest.mark.gpu
Q_COARSE = max(C.QUANTIZERS)
THETA_SCALE = 32768 * 2. / np.pi


def _to_raster(vec, n):
    out = np.zeros((n, n), np.int32)
    oracle().odo_coding_order_to_raster(P(out), n, P(np.ascontiguousarray(vec, np.int32)), n)
    return out


def _tables(hip, which):
    """default: the table set of the other band-stage tests; finer: the next finer quantiser of
    QUALITY_QUANTIZERS; flat: the default quantiser with the flat matrix."""
    if which == "default":
        return hip.QuantTables.load()
    if which == "finer":
        return hip.QuantTables.for_quality(10)
    return hip.QuantTables.for_quality(20, hvs_qm=0)


def _named(names, mm):
    """The mismatch summary with the corpus case of every first offender."""
    lines = [mm.summary()]
    for what, where in sorted(mm.first.items()):
        bs, blk, b = where[:3]
        lines.append("%s: %s" % (what, names.get(bs, {}).get((blk, b), "(filler band)")))
    return "\n".join(lines)


# ---- with-reference building blocks ------------------------------------------------------------
@pytest.mark.parametrize("n", C.SIZES)
@pytest.mark.parametrize("cfl,beta", [(0, 4096), (1, 4096), (0, 6144)])
def test_ref_prepare_and_candidates_match_oracle_on_the_corpus(hip, n, cfl, beta):
    """odhip_pvq_ref_prepare and odhip_pvq_ref_candidates on every corpus band of n coefficients, at
    every quantiser of the corpus that keeps the band's K inside the layout: every record field, x16,
    r16, the reflected vector and the candidate list (the checks of
    test_ref_prepare_and_candidates_match_oracle, here on the directed bands)."""
    import torch
    o = oracle()
    qm, qmi, _, cs = R.band_setup("hvs", cfl, n)
    compared = set()
    ran = checked = 0
    for q0 in C.QUANTIZERS:
        sel = [c for c in cs if q0 in C.quantizers_for(n, c[2])]
        compared |= {c[0] for c in sel}
        x0 = np.stack([c[2] for c in sel])
        r0 = np.stack([c[3] for c in sel])
        x16, r16, xr, prep = hip.pvq_ref_prepare(_cuda(x0), _cuda(r0), _cuda(qm), q0, beta, cfl)
        torch.cuda.synchronize()
        rec = prep.cpu().numpy().view(hip.REFPREP_RECORD)[:, 0]
        x16, r16, xr = x16.cpu().numpy(), r16.cpu().numpy(), xr.cpu().numpy()
        traces = []
        for b, (name, _, xb, rb) in enumerate(sel):
            tr = R.new_trace()
            R.theta(o.odo_pvq_theta, xb, rb, n, q0, beta, cfl, cfl, qm, qmi, trace=tr)
            traces.append(tr)
            w = (name, q0)
            for f in ("xshift", "rshift", "g", "gr", "cg", "cgr", "icgr", "gain_offset", "m", "s"):
                assert rec[f][b] == getattr(tr, f), w + (f,)
            assert rec["corr"][b] == tr.corr, w
            assert rec["r_null"][b] == int(not rb.any()), w
            assert np.array_equal(x16[b], np.array(tr.x16[:n], np.int16)), w
            assert np.array_equal(r16[b], np.array(tr.r16[:n], np.int16)), w
            if not rec["r_null"][b] and tr.corr > 0:
                ran += 1
                want = np.zeros(n, np.int16)
                o.odo_apply_householder(P(want), P(np.array(tr.x16[:n], np.int16)),
                                        P(np.array(tr.r16[:n], np.int16)), n)
                assert np.array_equal(xr[b], np.delete(want, tr.m)), w
        theta = np.floor(.5 + THETA_SCALE * np.arccos(rec["corr"])).astype(np.int32)
        items, nitems = hip.pvq_ref_candidates(prep, _cuda(theta), n, beta)
        torch.cuda.synchronize()
        items = items.cpu().numpy().view(hip.REFCAND_RECORD)[..., 0]
        nitems = nitems.cpu().numpy()
        for b, (name, _, _, _) in enumerate(sel):
            tr = traces[b]
            assert tr.ncands < 24, name
            want = [tr.cands[i] for i in range(tr.ncands) if tr.cands[i].with_ref]
            assert nitems[b] == len(want), (name, q0)
            for i, c in enumerate(want):
                for f in ("gain", "theta", "ts", "k", "qcg", "qtheta"):
                    assert items[f][b, i] == getattr(c, f), (name, q0, i, f)
                checked += 1
    assert compared == {c[0] for c in cs}                    # no case dropped
    assert ran > len(cs) // 3 and checked > len(cs)


# ---- band stages on planes that hold the corpus --------------------------------------------------
def _level_planes(qt, pli, bs, unit=None):
    """unit: the width rounded up to a multiple of it (whole superblocks, for a caller that also runs
    an inverse on the planes); the blocks beyond the corpus hold filler bands."""
    dec = 1 if pli else 0
    qm, qmi = qt.qm_slices(dec, bs)
    qb = qt.q_band(pli, bs)
    # the 64x64 level is as wide as the 32x32 one (it holds a part of the 128-coefficient cases again,
    # from another start)
    w = C.plane_width(3, qt.qm_slices(dec, 3)[0], q_band=qt.q_band(pli, 3)) if bs == 4 else None
    if unit:
        w = -(-(w or C.plane_width(bs, qm, q_band=qb)) // unit) * unit
    x, r, names = C.corpus_planes(bs, qm, _to_raster, w=w, q_band=qb, q_coarse=Q_COARSE, rotate=97 if bs == 4 else 0)
    return x, r, names, qm, qmi, qb


def _plane_traces(x, r, bs, qm, qmi, q_bands, bb, is_keyframe, pli, lam):
    """oracle_traces plane by plane (each plane at its own per-band steps), keyed as one job."""
    per = (x.shape[1] // (4 << bs)) * (x.shape[2] // (4 << bs))
    out = {}
    for p, qb in enumerate(q_bands):
        tr, _ = oracle_traces(x[p:p + 1], r[p:p + 1], bs, qm, qmi, qb, bb, is_keyframe, pli, lam)
        for (blk, b), t in tr.items():
            out[(blk + p * per, b)] = t
    return out


@pytest.mark.parametrize("which", ["default", "finer", "flat"])
@pytest.mark.parametrize("is_keyframe,pli", MODES)
def test_ref_band_stage_matches_oracle_on_the_corpus(hip, is_keyframe, pli, which):
    """odhip_pvq_ref_bands_multi (resolve on) and odhip_pvq_ref_select_synth_multi on planes that hold
    the corpus, at every level: the first plane of a job at the table set's steps with the cases
    those keep inside ODHIP_PVQ_MAX_K, the second at the corpus's coarsest quantiser with the others.
    The host resolve may fire (bands near corr = 1 sit inside the device-acos margin); nothing may be
    reported as out of the pulse range."""
    import torch
    lam = hip.OD_PVQ_LAMBDA
    qt = _tables(hip, which)
    top = 3 if pli else 4
    hip.pvq_k_range_take()
    jobs, meta, names = [], [], {}
    for bs in range(top + 1):
        x, r, nm, qm, qmi, qb = _level_planes(qt, pli, bs)
        bb = qt.beta_band(pli, bs)
        coarse = [Q_COARSE] * len(qb)
        jobs.append(hip.PvqRefJob(_cuda(x), _cuda(r), bs, _cuda(qm), _cuda(qmi), qb, bb, is_keyframe, pli,
                                  q_band2=coarse, plane_split=1))
        meta.append((x, r, qm, qmi, (qb, coarse), bb))
        names[bs] = nm
    # every case of every band size sits in some band of some level
    for n, home in ((15, 0), (8, 1), (32, 2), (128, 3)):
        a = C.BAND_OFFSETS[[b for b in range(C.NBANDS[home]) if C.BAND_OFFSETS[b + 1] - C.BAND_OFFSETS[b] == n][0]]
        want = {c[0] for c in C.cases(n, meta[home][2][a:a + n])}
        assert want <= set(names[home].values()), (n, sorted(want - set(names[home].values()))[:5])
    hip.pvq_ref_bands_multi(jobs, lam)
    torch.cuda.synchronize()
    mm = Mismatch()
    all_traces = []
    for job, (x, r, qm, qmi, qbs, bb) in zip(jobs, meta):
        traces = _plane_traces(x, r, job.bs, qm, qmi, qbs, bb, is_keyframe, pli, lam)
        assert all(t["tr"].ncands < 24 for t in traces.values())
        all_traces.append(traces)
        compare_bands(hip, job, traces, mm)
    assert mm.total() == 0, _named(names, mm)
    assert mm.checked.get("item.y", 0) > 1000
    for job, traces in zip(jobs, all_traces):
        job.rate = _cuda(host_rates(job, traces, is_keyframe, pli))
    hip.pvq_ref_select_synth_multi(jobs, lam)
    torch.cuda.synchronize()
    for job, traces in zip(jobs, all_traces):
        compare_choice(job, traces, mm)
    assert mm.total() == 0, _named(names, mm)
    assert mm.checked["dq"] > 1000
    assert hip.pvq_k_range_take() == (0, 0)


@pytest.mark.parametrize("pli", [0, 1])
def test_noref_band_stage_matches_oracle_on_the_corpus(hip, pli):
    """The coefficient planes of the corpus through the no-reference band stage, choice and synthesis
    at every level (the checks of test_band_stage_matches_oracle): the first plane at the table set's
    steps, the second at the corpus's coarsest quantiser."""
    import torch
    qt = hip.QuantTables.load()
    hip.pvq_k_range_take()
    for bs in range(5 - pli):
        x, _, names, _, _, qb = _level_planes(qt, pli, bs)
        assert names
        _check_level_against_oracle(hip, x[0], bs, pli)
        _check_level_against_oracle(hip, x[1], bs, pli, q_band=[Q_COARSE] * len(qb))
    torch.cuda.synchronize()
    assert hip.pvq_k_range_take() == (0, 0)


# ---- the search alone -----------------------------------------------------------------------------
def _oracle_search(x, k, g2, lam, prev_k=None, y0=None):
    nb, n = x.shape
    y = np.zeros((nb, n), np.int32) if y0 is None else y0.copy()
    cos = np.zeros(nb, np.float64)
    oracle().odo_pvq_search_batch(P(x), n, P(k), P(y), P(g2), ctypes.c_double(lam),
                                  None if prev_k is None else P(prev_k), P(cos), ctypes.c_long(nb))
    return y, cos


@pytest.mark.parametrize("n", [7, 8, 14, 15, 16, 31, 32, 127, 128])
def test_pvq_search_matches_oracle_on_ties_and_spikes(hip, n):
    """odhip_pvq_search_batch on the tie and spike vectors, every K of {1, 2, 3, n - 1, n, n + 1, 2n,
    300} on every vector, from scratch and continued from the previous K's pulses (prev_k): pulses
    and the cosine's bits."""
    vecs = C.search_vectors(n)
    ks = sorted({1, 2, 3, n - 1, n, n + 1, 2 * n, 300})
    x = np.repeat(np.stack([v for _, v in vecs]), len(ks), axis=0)
    k = np.tile(np.array(ks, np.int32), len(vecs))
    g2 = np.tile(np.array([1.0, 0.01, 37.5, 1e4, 1.0], np.float64), len(x) // 5 + 1)[:len(x)].copy()
    label = [(name, kk) for name, _ in vecs for kk in ks]
    yo, co = _oracle_search(x, k, g2, 0.147)
    yg, cg = hip.pvq_search_batch(_cuda(x), _cuda(k), _cuda(g2), 0.147)
    yg, cg = yg.cpu().numpy(), cg.cpu().numpy()
    bad = np.flatnonzero((yg != yo).any(axis=1) | (cg.view(np.int64) != co.view(np.int64)))
    assert len(bad) == 0, (len(bad), label[int(bad[0])])
    # continued: from the pulses of K to those of the next K of the list (and a few pulses more)
    k2 = np.tile(np.array(ks[1:] + [ks[-1] + 5], np.int32), len(vecs))
    yo2, co2 = _oracle_search(x, k2, g2, 0.147, prev_k=k, y0=yo)
    yg2, cg2 = hip.pvq_search_batch(_cuda(x), _cuda(k2), _cuda(g2), 0.147, prev_k=_cuda(k), y=_cuda(yo))
    yg2, cg2 = yg2.cpu().numpy(), cg2.cpu().numpy()
    bad = np.flatnonzero((yg2 != yo2).any(axis=1) | (cg2.view(np.int64) != co2.view(np.int64)))
    assert len(bad) == 0, (len(bad), label[int(bad[0])], "continued")
    assert len(vecs) > 40 and np.abs(yo).sum(axis=1).tolist() == k.tolist()


# ---- closed loop through the decoder ---------------------------------------------------------------
@pytest.mark.parametrize("is_keyframe,pli", MODES)
def test_decoder_returns_what_pvq_theta_synthesised_on_the_corpus(hip, is_keyframe, pli):
    """odhip_pvq_decode_bands fed the oracle's final decision for every corpus band (gain code, itheta,
    noref, y): the oracle decoder's output, which is the `out` pvq_theta synthesised."""
    o = oracle()
    nbands = 0
    skips = set()
    for n in C.SIZES:
        qm, qmi, beta, cs = R.band_setup("hvs", pli, n)
        compared = set()
        for q0 in C.QUANTIZERS:
            sel = [c for c in cs if q0 in C.quantizers_for(n, c[2])]
            compared |= {c[0] for c in sel}
            refv = np.stack([c[3] for c in sel])
            y = np.zeros((len(sel), n), np.int32)
            sym = np.zeros((len(sel), 4), np.int32)
            want = np.zeros((len(sel), n), np.int32)
            info = np.zeros((len(sel), 2), np.int32)
            for i, (name, _, x0, r0) in enumerate(sel):
                res = R.theta(o.odo_pvq_theta, x0, r0, n, q0, beta, is_keyframe, pli, qm, qmi)
                noref = 1 if res["itheta"] == -1 else 0
                y[i] = res["y"]
                sym[i] = (res["ret"], res["itheta"], noref, 0)
                kk = ctypes.c_int(-1)
                info[i, 1] = o.odo_pvq_decode_band(P(want[i]), P(np.ascontiguousarray(r0)), P(y[i]), n, q0, beta,
                                                   res["ret"], res["itheta"], noref, is_keyframe, pli, P(qm), P(qmi),
                                                   ctypes.byref(kk))
                info[i, 0] = kk.value
                assert np.array_equal(want[i], res["out"]) and kk.value == res["k"], (name, q0)
            out, ginfo = hip.pvq_decode_bands(_cuda(refv), _cuda(y), _cuda(sym), _cuda(qm), _cuda(qmi), q0, beta,
                                              is_keyframe, pli)
            bad = np.flatnonzero((out.cpu().numpy() != want).any(axis=1) | (ginfo.cpu().numpy() != info).any(axis=1))
            assert len(bad) == 0, (len(bad), sel[int(bad[0])][0], q0)
            nbands += len(sel)
            skips |= set(info[:, 1].tolist())
        assert compared == {c[0] for c in cs}
    assert nbands > 2000 and 0 in skips and 1 in skips
