"""GPU: the PRICED PVQ band stages - the kernels a pricing pipe runs - on the directed corpus
(tests/_pvq_corpus.py), every decision against the CPU oracle's pvq_theta at speed 1, never against
another GPU form:

  odhip_pvq_ref_bands_decided_multi   k_refb_lean_lane<8 / 15>, k_refb_lean_row<8, 4 / 16> behind
                                      k_refb_prep_corner / k_refb_prep_row, items ordered heavy first
  odhip_pvq_noref_bands_priced_multi  k_decide_corner<0 / 1>, k_decide_lane32, k_decide_pair128
                                      (k_decide_quad128 in the experiments build)
  odhip_pvq_choose_priced_multi       k_choose<1>
  the two resolves                    k_refb_cands_list, k_refb_search_list, k_refb_choose_list,
                                      k_choose_list: with every hook off (a condition: at most 5 % of
                                      the bands may take them) and forced by the test hooks

tests/test_gpu_pvq_corpus.py runs the same planes through the kernels that export every candidate.
What the corpus holds that random Laplacian planes do not: equal maxima of |r16|, equal |x16| at
every lane distance, collinear and anti-collinear references, bands one LSB off a gate, gain ladders,
max |x0| = 270000.  tests/test_pvq_corpus_host.py shows that close calls and boundary thetas stay far
below the 5 % cap on this corpus.

The planes are those of tests/test_gpu_pvq_corpus.py (64 rows, the first plane of a job at the table
set's steps, the second at the corpus's coarsest quantiser) with the width rounded up to whole
superblocks, so that the pulse-fed inverses run on them too.  The oracle is what takes the time: every
trace set is computed once per session (_traces).

One thing the corpus cannot show is the MARGIN of the row searches' single-precision screen: with the
margin at zero every corpus decision stays right.  Section 3 shows it on bands of consecutive magnitudes
(not a corpus class), by the replay counters the experiments build keeps for k_refb_lean_row."""
import os
import subprocess
import sys

import numpy as np
import pytest

import _pvq_corpus as C
from _libs import P, oracle
from _refbands import Mismatch, _coding
from test_gpu_plane_layouts import _oracle_inverse, _pic
from test_gpu_pvq_bands import hip  # noqa: F401
from test_gpu_pvq_corpus import Q_COARSE, _level_planes, _named, _plane_traces, _tables
from test_gpu_pvq_refbands import MODES

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
RESOLVED_CAP = 0.05      # of the bands of a call; see tests/test_pvq_corpus_host.py for what entitles to it

_cache = {}


def _cuda(a):
    import torch
    return torch.from_numpy(np.array(a, order="C")).cuda()      # (a copy: the shared planes are read-only)


def _planes(hip, which, pli, bs):
    """(x, r, names, qm, qmi, q_band, beta_band) of one level, once per session."""
    key = ("planes", which, pli, bs)
    if key not in _cache:
        qt = _cache.setdefault(("tables", which), _tables(hip, which))
        x, r, names, qm, qmi, qb = _level_planes(qt, pli, bs, unit=32 if pli else 64)
        for a in (x, r):
            a.setflags(write=False)
        _cache[key] = (x, r, names, qm, qmi, qb, qt.beta_band(pli, bs))
    return _cache[key]


def _traces(hip, which, mode, bs):
    """The oracle's pvq_theta (speed 1) on every band of both planes of one level, once per session.
    mode: (is_keyframe, pli) with the corpus's references, or ("noref", pli): an all-zero reference on a
    keyframe, the case in which pvq_theta runs exactly the no-reference candidates."""
    key = ("traces", which, mode, bs)
    if key not in _cache:
        pli = mode[1]
        x, r, _, qm, qmi, qb, bb = _planes(hip, which, pli, bs)
        is_keyframe = 1 if mode[0] == "noref" else mode[0]
        if mode[0] == "noref":
            r = np.zeros_like(x)
        tr = _plane_traces(x, r, bs, qm, qmi, (qb, [Q_COARSE] * len(qb)), bb, is_keyframe, pli, hip.OD_PVQ_LAMBDA)
        assert all(t["tr"].ncands < 24 for t in tr.values())
        _cache[key] = tr
    return _cache[key]


def _levels(pli):
    return range(4 if pli else 5)


def _assert_no_case_dropped(hip, which, pli):
    """Every case of every band size sits in some band of its home level."""
    for n, home in ((15, 0), (8, 1), (32, 2), (128, 3)):
        _, _, names, qm = _planes(hip, which, pli, home)[:4]
        a = C.BAND_OFFSETS[[b for b in range(C.NBANDS[home]) if C.BAND_OFFSETS[b + 1] - C.BAND_OFFSETS[b] == n][0]]
        want = {c[0] for c in C.cases(n, qm[a:a + n])}
        assert want <= set(names.values()), (n, sorted(want - set(names.values()))[:5])


def _oracle_planes(x, r, bs, traces, is_keyframe):
    """The planes the oracle's `out` vectors make: DC kept, the positions PVQ never codes (64x64 blocks
    beyond coefficient 512) zero on a keyframe and the reference's own on an inter frame - the rule of
    _refbands.compare_choice's dq.tail."""
    o = oracle()
    nplanes, h, w = x.shape
    n = 4 << bs
    d = np.zeros_like(x) if is_keyframe or r is None else np.array(r)
    blk = 0
    for p in range(nplanes):
        for by in range(h // n):
            for bx in range(w // n):
                vec = _coding(o, x[p], by, bx, n)
                b = 0
                while (blk, b) in traces:
                    t = traces[(blk, b)]
                    vec[t["off"]:t["off"] + t["n"]] = t["out"]
                    b += 1
                assert b == C.NBANDS[bs]
                tile = np.ascontiguousarray(d[p, by * n:(by + 1) * n, bx * n:(bx + 1) * n])
                o.odo_coding_order_to_raster(P(tile), n, P(vec), n)
                d[p, by * n:(by + 1) * n, bx * n:(bx + 1) * n] = tile
                blk += 1
    return d


def _want_pixels(hip, which, mode, bs):
    """The oracle's inverse of the oracle's planes, once per session."""
    key = ("pixels", which, mode, bs)
    if key not in _cache:
        pli = mode[1]
        x, r = _planes(hip, which, pli, bs)[:2]
        noref = mode[0] == "noref"
        d = _oracle_planes(x, None if noref else r, bs, _traces(hip, which, mode, bs), noref or mode[0])
        _cache[key] = _oracle_inverse(d, 1 if pli else 0, bs, False)
    return _cache[key]


def _neg_deinterleave(x, ref):
    """src/pvq_decoder.c:53-59."""
    if x < 2 * ref - 1:
        return ref - 1 - (x >> 1) if x & 1 else ref + (x >> 1)
    return x + 1


def _implied_skip(t, is_keyframe, pli):
    """The skip code the decoder derives from what pvq_theta returned (src/pvq_decoder.c:190-241, the
    encoder's :611-622): 0, 1 = OD_PVQ_SKIP_ZERO, 2 = OD_PVQ_SKIP_COPY."""
    icgr = t["tr"].icgr
    if t["itheta"] == -1:
        return int(t["ret"] + (0 if is_keyframe else 1) == 0)
    skip = 0
    if is_keyframe:
        qg = _neg_deinterleave(t["ret"], icgr)
    else:
        qg = _neg_deinterleave(t["ret"], icgr + 1) - 1
        if qg == 0:
            skip = 1 if icgr else 2
    if qg == icgr and t["itheta"] == 0 and not (is_keyframe and pli != 0):
        skip = 2
    return skip


# ---- 1. the with-reference decided stage -----------------------------------------------------------
def _ref_jobs(hip, which, is_keyframe, pli):
    jobs, names = [], {}
    for bs in _levels(pli):
        x, r, nm, qm, qmi, qb, bb = _planes(hip, which, pli, bs)
        jobs.append(hip.PvqRefJob(_cuda(x), _cuda(r), bs, _cuda(qm), _cuda(qmi), qb, bb, is_keyframe, pli,
                                  q_band2=[Q_COARSE] * len(qb), plane_split=1))
        names[bs] = nm
    return jobs, names


def _compare_decided(job, traces, mm):
    """The choice record and the winner's pulses of every band the oracle traced."""
    ch = job.choice.cpu().numpy()
    y = job.y.cpu().numpy()
    for (blk, b), t in traces.items():
        w = (job.bs, blk, b)
        c = ch[blk, b]
        noref = int(t["itheta"] == -1)
        mm.check("choice.noref", int(c[2]) == noref, w)
        mm.check("choice.itheta", int(c[3]) == t["itheta"], w)
        mm.check("choice.maxth", int(c[4]) == t["max_theta"], w)
        mm.check("choice.k", int(c[5]) == t["vk"], w)
        mm.check("choice.skip", int(c[6]) == _implied_skip(t, job.is_keyframe, job.pli), w)
        mm.check("choice.ret", int(c[7]) == t["ret"], w)
        # a theta winner holds n - 1 pulses
        nn = t["n"] - (0 if noref else 1)
        want = t["y"][:nn]
        slot = int(c[9])
        mm.check("choice.yslot", (slot < 0) == (t["vk"] == 0) and slot < y.shape[0], w)
        if 0 <= slot < y.shape[0]:
            mm.check("y", np.array_equal(y[slot, blk, t["off"]:t["off"] + nn].astype(np.int32), want), w)
        else:
            mm.check("y", not want.any(), w)


def _check_ref_decided(hip, which, is_keyframe, pli, tag):
    """The decided stage on every level of the mode in one call, under whatever hooks the caller set:
    records, pulses, K range and reconstruction against the oracle.  Returns the two resolve counts and
    the number of bands."""
    import torch
    lam = hip.OD_PVQ_LAMBDA
    mode = (is_keyframe, pli)
    hip.pvq_k_range_take()
    jobs, names = _ref_jobs(hip, which, is_keyframe, pli)
    _assert_no_case_dropped(hip, which, pli)
    nt, npz = hip.pvq_ref_bands_decided_multi(jobs, lam)
    torch.cuda.synchronize()
    nbands = sum(j.nblocks * j.nb for j in jobs)
    print("%s %s kf=%d pli=%d: %d bands re-run with the host's theta, %d re-decided with the host libm, of %d"
          % (tag, which, is_keyframe, pli, nt, npz, nbands))
    mm = Mismatch()
    for job in jobs:
        traces = _traces(hip, which, mode, job.bs)
        assert len(traces) == job.nblocks * job.nb
        _compare_decided(job, traces, mm)
    assert mm.total() == 0, _named(names, mm)
    assert mm.checked["y"] > 1000 and mm.checked["y"] == nbands
    assert hip.pvq_k_range_take() == (0, 0)
    dec = 1 if pli else 0
    for job in jobs:
        _, h, w = job.coef.shape
        pw, ph = _pic(dec, w, h)
        got = hip.inverse_levels_pvq_ref([job], dec, pw, ph)[0].cpu().numpy()
        assert np.array_equal(got, _want_pixels(hip, which, mode, job.bs)), (tag, which, mode, job.bs)
    return nt, npz, nbands


@pytest.mark.parametrize("which,is_keyframe,pli", [("default",) + m for m in MODES]
                         + [(w,) + m for w in ("flat", "finer") for m in ((1, 1), (0, 0))])
def test_ref_decided_stage_matches_oracle_on_the_corpus(hip, which, is_keyframe, pli):
    """odhip_pvq_ref_bands_decided_multi with every test hook off, every level of the mode in one call (the
    K = 1 and the K in the thousands bands of all levels mixed by the heavy-first order): choice words 2-7,
    the winner's pulses through word 9, no band out of the pulse range, and the pulse-fed inverse equal to
    the oracle's inverse of the oracle's planes.  The resolves may fire (bands near corr = 1, exact cost
    ties between identical candidates), but on at most 5 % of the bands: beyond that this would no longer
    test the lean kernels."""
    nt, npz, nbands = _check_ref_decided(hip, which, is_keyframe, pli, "plain")
    assert nt + npz <= RESOLVED_CAP * nbands, (nt, npz, nbands)


@pytest.mark.parametrize("is_keyframe,pli", [(1, 1), (0, 0)])
@pytest.mark.parametrize("forced", ["theta", "price", "both"])
def test_ref_decided_stage_under_forced_margins_matches_oracle_on_the_corpus(hip, forced, is_keyframe, pli):
    """The same comparison with the resolves forced: theta margin 0.25 with the perturbation (the device
    theta of every listed band deliberately wrong: k_refb_cands_list, k_refb_search_list re-run it with the
    host's), the price margin scaled by 1e12 (every decision a close call: re-run by the exporting kernels,
    decided by k_refb_choose_list from host rates), and both at once."""
    try:
        if forced in ("theta", "both"):
            hip.pvq_ref_set_theta_margin(0.25, True)
        if forced in ("price", "both"):
            hip.set_price_tol_scale(1e12)
        nt, npz, _ = _check_ref_decided(hip, "default", is_keyframe, pli, "forced " + forced)
    finally:
        hip.pvq_ref_set_theta_margin(0, False)
        hip.set_price_tol_scale(1.)
    if forced in ("theta", "both"):
        assert nt > 20
    if forced in ("price", "both"):
        assert npz > 50


# ---- 2. the no-reference priced stage, fused and unfused -------------------------------------------
FORMS = ("choice_kernel", "decided", "resolved")


def _check_noref_priced(hip, pli, form):
    import torch
    lam = hip.OD_PVQ_LAMBDA
    mode = ("noref", pli)
    hip.pvq_k_range_take()
    jobs, names = [], {}
    for bs in _levels(pli):
        x, _, nm, qm, qmi, qb, bb = _planes(hip, "default", pli, bs)
        jobs.append(hip.PvqJob(_cuda(x), bs, _cuda(qm), _cuda(qmi), qb, bb, q_band2=[Q_COARSE] * len(qb),
                               plane_split=1))
        names[bs] = nm
    _assert_no_case_dropped(hip, "default", pli)
    if form == "choice_kernel":
        hip.pvq_noref_bands_multi(jobs, lam)
        redone = hip.pvq_choose_priced_multi(jobs, lam)
    elif form == "decided":
        redone = hip.pvq_choose_priced_multi(jobs, lam, fused_bands=True)
    else:
        hip.set_price_tol_scale(1e12)
        try:
            redone = hip.pvq_choose_priced_multi(jobs, lam, fused_bands=True)
        finally:
            hip.set_price_tol_scale(1.)
    torch.cuda.synchronize()
    nbands = sum(j.nblocks * hip.pvq_band_layout(j.bs)[0] for j in jobs)
    print("%s pli=%d: %d bands re-decided with the host libm, of %d" % (form, pli, redone, nbands))
    mm = Mismatch()
    for job in jobs:
        traces = _traces(hip, "default", mode, job.bs)
        ch = job.cands["choice"].cpu().numpy()
        y = job.cands["y"].cpu().numpy()
        assert len(traces) == ch.shape[0] * ch.shape[1]
        for (blk, b), t in traces.items():
            w = (job.bs, blk, b)
            qg = int(ch[blk, b, 1])
            mm.check("choice.qg", qg == t["ret"], w)
            # only the chosen slot: the fused stage does not write losers
            got = np.zeros(t["n"], np.int32)
            if qg:
                slot = int(ch[blk, b, 0])
                mm.check("choice.slot", slot in (0, 1), w)
                if slot in (0, 1):
                    got = y[slot, blk, t["off"]:t["off"] + t["n"]].astype(np.int32)
            mm.check("y", np.array_equal(got, t["y"]), w)
            mm.check("k", int(np.abs(got).sum()) == t["vk"], w)
    assert mm.total() == 0, _named(names, mm)
    assert mm.checked["y"] > 1000 and mm.checked["y"] == nbands
    assert hip.pvq_k_range_take() == (0, 0)
    dec = 1 if pli else 0
    for job in jobs:
        _, h, w = job.coef.shape
        pw, ph = _pic(dec, w, h)
        got = hip.inverse_levels_pvq([job], dec, pw, ph)[0].cpu().numpy()
        assert np.array_equal(got, _want_pixels(hip, "default", mode, job.bs)), (form, pli, job.bs)
    if form == "resolved":
        assert redone > 100
    else:
        assert redone <= RESOLVED_CAP * nbands, (redone, nbands)


@pytest.mark.parametrize("pli,form", [(p, f) for p in (0, 1) for f in FORMS],
                         ids=["%s-%s" % ("chroma" if p else "luma", f) for p in (0, 1) for f in FORMS])
def test_noref_priced_stage_matches_oracle_on_the_corpus(hip, pli, form):
    """Both planes of every level through the device-priced no-reference choice - choice_kernel:
    odhip_pvq_noref_bands_multi + odhip_pvq_choose_priced_multi (k_choose<1>); decided:
    odhip_pvq_noref_bands_priced_multi (the k_decide_* kernels); resolved: the latter with the price margin
    scaled by 1e12 (k_choose_list after the host-libm resolve) - against pvq_theta with an all-zero reference
    on a keyframe: the gain index, the chosen slot's pulses, their magnitudes' sum, no band out of the pulse
    range, and odhip_inverse_levels_pvq against the oracle's inverse of the oracle's planes.  With the hook
    off at most 5 % of the bands may be re-decided by the host."""
    _check_noref_priced(hip, pli, form)


def test_noref_decided_stage_quad_per_band_experiments_build():
    """ODHIP_PVQ_QUAD128=1 - the 128-coefficient bands decided by a lane QUAD per band, k_decide_quad128,
    which only the EXPERIMENTS build of the library holds and calls bit-identical - : the luma case of the
    decided form above in a child process that loads that build with the switch set."""
    import daala_amd
    env = dict(os.environ)
    env.update(ODHIP_LIB=daala_amd.EXPERIMENTS_LIB, ODHIP_PVQ_QUAD128="1")
    r = subprocess.run([sys.executable, "-m", "pytest", os.path.abspath(__file__), "-q", "-x", "-m", "gpu", "-k",
                        "test_noref_priced_stage_matches_oracle_on_the_corpus and luma-decided"], env=env,
                       capture_output=True, text=True, timeout=900, cwd=ROOT)
    assert r.returncode == 0 and "1 passed" in r.stdout, r.stdout[-2000:] + r.stderr[-1000:]


# ---- 3. the row searches' single-precision screen inside the decided stage ---------------------------
SCREEN_BS = 3            # 32x32 blocks: bands 6, 7, 8 hold 128 coefficients (k_refb_lean_row<8, 16>)
SCREEN_Q = 124


def _ladder_band(top, order, sign, qm):
    """The int32 band whose QM-scaled int16 image is sign*(X - order) for the X nearest below `top` at which
    pvq_theta's own shift of the band reproduces that image (a band on a shift boundary has none)."""
    for x_top in range(top, top - 40, -1):
        t = sign * (x_top - order)
        for shift in range(12):
            x0 = C._preimage(t, qm, shift)
            if C.band_shift(x0, 15) == shift:
                return x0
    raise AssertionError("no self-consistent shift near %d" % top)


def _screen_planes(hip, q):
    """One keyframe-luma plane of 32x32 blocks whose three 128-coefficient bands are x16 = the integers X,
    X - 1, .., X - 127 in shuffled positions with random signs (tests/test_gpu_row_screen.py's ladders, here
    through the whole stage), X between 1020 and 1097 - about the largest a band of 128 keeps inside 16 bits
    with pvq_theta's headroom - coded at step q.  That puts K near 2.8 n: the projection leaves two pulses on
    most positions, xy + |x| starts beyond 2^18, and the few greedy pulses that remain (none would from
    K = 4 n on) choose between neighbours of the ladder - closer than the screen's margin, no duplicates: such
    a pulse must be replayed.  Not a corpus class: nothing here is tied or degenerate."""
    from test_gpu_pvq_corpus import _to_raster
    qt = _tables(hip, "default")
    bs = SCREEN_BS
    n = 4 << bs
    qm, qmi = qt.qm_slices(0, bs)
    qb = list(qt.q_band(0, bs))
    bb = qt.beta_band(0, bs)
    rng = np.random.RandomState(128)
    h, w = 64, 1280
    x = np.zeros((1, h, w), np.int32)
    r = np.zeros((1, h, w), np.int32)
    nblocks = (h // n) * (w // n)
    for blk in range(nblocks):
        vx = rng.randint(-30, 31, size=n * n).astype(np.int32)
        vr = rng.randint(-30, 31, size=n * n).astype(np.int32)
        vx[512:] = 0
        vr[512:] = 0
        for b in (6, 7, 8):
            a = C.BAND_OFFSETS[b]
            qb[b] = q
            order = rng.permutation(128)
            sign = rng.choice([-1, 1], size=128)
            vx[a:a + 128] = _ladder_band(1020 + (3 * blk + b - 6) % 78, order, sign, qm[a:a + 128])
        by, bx = divmod(blk, w // n)
        x[0, by * n:(by + 1) * n, bx * n:(bx + 1) * n] = _to_raster(vx, n)
        r[0, by * n:(by + 1) * n, bx * n:(bx + 1) * n] = _to_raster(vr, n)
    return x, r, qm, qmi, qb, bb


def _near_tie_pulses(traces):
    """From the oracle's traces alone: the greedy pulses of the 128-coefficient bands' no-reference searches
    that start from scratch (src/pvq_encoder.c:121-146: the projection places floor(K|x_j|/L1) pulses, the
    last 1 + K/4 are placed with the rate term, what is left is greedy) with xy + max|x| already beyond 2^18
    after the projection - xy only grows, so every one of them is a near tie of two neighbours of the ladder."""
    total = 0
    for t in traces.values():
        if t["n"] != 128:
            continue
        tr = t["tr"]
        ax = np.abs(np.array(tr.x16[:128], np.int64))
        prev_k = 0
        for i in range(tr.ncands):
            c = tr.cands[i]
            if c.with_ref or not c.searched:
                continue
            fresh = not (0 < prev_k <= c.k)
            prev_k = c.k
            if not fresh or c.k <= 2:
                continue
            y = np.floor(c.k * ax.astype(np.float64) * (1.0 / max(float(ax.sum()), 1e-100))).astype(np.int64)
            greedy = c.k - (1 + c.k // 4) - int(y.sum())
            if greedy > 0 and int((ax * y).sum()) + int(ax.max()) > 1 << 18:
                total += greedy
    return total


def _screen_child():
    """In a process that loaded the experiments build: the decided stage on _screen_planes against the oracle,
    and the replay counters k_refb_lean_row keeps there.  Prints one line of JSON."""
    import ctypes
    import json
    import torch
    import daala_amd
    daala_amd.init(0)
    L = daala_amd.lib()
    assert hasattr(L, "odhip_exp_row_replay_stats"), "the experiments build is expected here"
    x, r, qm, qmi, qb, bb = _screen_planes(daala_amd, SCREEN_Q)
    job = daala_amd.PvqRefJob(_cuda(x), _cuda(r), SCREEN_BS, _cuda(qm), _cuda(qmi), qb, bb, 1, 0)
    stats = (ctypes.c_ulonglong * 4)()
    assert L.odhip_exp_row_replay_stats(stats, 1) == 0
    daala_amd.pvq_k_range_take()
    nt, npz = daala_amd.pvq_ref_bands_decided_multi([job], daala_amd.OD_PVQ_LAMBDA)
    torch.cuda.synchronize()
    assert L.odhip_exp_row_replay_stats(stats, 1) == 0
    traces = _plane_traces(x, r, SCREEN_BS, qm, qmi, (qb,), bb, 1, 0, daala_amd.OD_PVQ_LAMBDA)
    mm = Mismatch()
    _compare_decided(job, traces, mm)
    print(json.dumps(dict(bad=mm.total(), summary=mm.summary() if mm.total() else "", checked=mm.checked["y"],
                          near=_near_tie_pulses(traces), listed=[nt, npz], k_range=list(daala_amd.pvq_k_range_take()),
                          pulses=int(stats[0]), replays=int(stats[1]), bands=int(stats[3]))))


def test_row_screen_replays_near_ties_inside_the_decided_stage_experiments_build():
    """The single-precision screen of the row searches (daala_amd/csrc/pvq_row.cuh) inside k_refb_lean_row:
    128-coefficient bands of consecutive magnitudes (_screen_planes) are decided as the oracle decides them,
    and the screen hands their near ties to the literal scan - the experiments build counts the replayed
    pulses of k_refb_lean_row (odhip_exp_row_replay_stats), so a child process loads that build.  With the
    margin at zero the decisions on these bands stay right (single precision still orders magnitudes one
    apart) but nothing is replayed: the count is what shows that the margin is there.  At least a quarter of
    the pulses _near_tie_pulses counts must be replayed (at such a pulse the best candidate's neighbour on
    the ladder, one below it in magnitude, is in its class unless it already took a pulse)."""
    import json
    import daala_amd
    env = dict(os.environ)
    env.update(ODHIP_LIB=daala_amd.EXPERIMENTS_LIB)
    r = subprocess.run([sys.executable, os.path.abspath(__file__)], env=env, capture_output=True, text=True,
                       timeout=600, cwd=ROOT)
    assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-2000:]
    out = json.loads(r.stdout.strip().splitlines()[-1])
    print(out)
    assert out["bad"] == 0, out["summary"]
    assert out["checked"] == 80 * 9 and out["k_range"] == [0, 0]
    assert out["near"] > 300                    # a condition on the inputs
    assert out["bands"] >= 240 and out["pulses"] >= out["near"]
    assert out["replays"] >= out["near"] // 4, out


if __name__ == "__main__":
    sys.path.insert(0, ROOT)
    _screen_child()
