"""GPU parity of the PVQ band stage (pvq_theta's no-reference path, candidates,
choice and dequantisation) against the CPU oracle, band by band."""
import ctypes

import numpy as np
import pytest

from _band_oracle import MAXN, Cand, Trace, band_trace, block_vector  # noqa: F401 (Trace: __graft_entry__.smoke)
from _libs import P, oracle, synth_frame

pytestmark = pytest.mark.gpu
cd = ctypes.c_double


@pytest.fixture(scope="module")
def hip():
    import torch
    import daala_amd
    assert torch.cuda.is_available()
    daala_amd.init(0)
    return daala_amd


def _cuda(a):
    import torch
    return torch.from_numpy(np.ascontiguousarray(a)).cuda()


def _oracle_pyramid(px, dec, pic):
    h, w = px.shape
    lv = [np.zeros((h, w), np.int32) for _ in range(5 - dec)]
    arr = (ctypes.c_void_p * 5)(*[l.ctypes.data for l in lv])
    c = np.zeros((h, w), np.int32)
    oracle().odo_forward_pyramid_plane(arr, P(c), P(px), w, w, h, dec, pic[0], pic[1])
    return lv


def _check_level_against_oracle(hip, coef, bs, pli, q_band=None):
    """The band stage, choice and synthesis of one plane at level bs against the oracle's pvq_theta, band
    by band (q_band: other per-band steps than the table set's)."""
    import torch
    qt = hip.QuantTables.load()
    o = oracle()
    lam = hip.OD_PVQ_LAMBDA
    h, w = coef.shape
    n = 4 << bs
    qm, qmi = qt.qm_slices(pli, bs)
    qb = list(q_band) if q_band is not None else qt.q_band(pli, bs)
    bb = qt.beta_band(pli, bs)
    nb, offs, ln = hip.pvq_band_layout(bs)
    tc = _cuda(coef[None])
    cands = hip.pvq_noref_bands(tc, bs, _cuda(qm), qb, bb, lam, cos_dist=True)
    torch.cuda.synchronize()
    dq, qg = hip.pvq_select_synth_noref(tc, bs, _cuda(qmi), qb, bb, lam, cands)
    c = hip.unpack_cands(cands)
    dq = dq.cpu().numpy()[0]
    qg = qg.cpu().numpy()
    want_dq = np.zeros_like(coef)
    nsearched = 0
    for by in range(h // n):
        for bx in range(w // n):
            blk = by * (w // n) + bx
            vec = block_vector(coef, n, bx, by)
            outvec = np.zeros(n * n, np.int32)
            outvec[0] = vec[0]
            for band in range(nb):
                a, b = offs[band], offs[band + 1]
                m = b - a
                qi = np.ascontiguousarray(qmi[a:b])
                tr, nr = band_trace(vec[a:b], qb[band], bb[band], qm[a:b], qi, lam)
                assert c["cg"][blk, band] == tr.cg
                assert c["dist0"][blk, band] == tr.dist0
                best_cost, best_qg, best_y = tr.dist0, 0, None
                for slot in range(2):
                    if slot >= len(nr):
                        assert c["gain"][blk, band, slot] == 0 and c["flags"][blk, band, slot] == 0
                        continue
                    cnd = nr[slot]
                    assert c["gain"][blk, band, slot] == cnd.gain
                    assert c["k"][blk, band, slot] == cnd.k
                    assert c["flags"][blk, band, slot] == cnd.searched
                    if cnd.searched:
                        nsearched += 1
                        assert c["cos_dist"][blk, band, slot] == cnd.cos_dist
                        assert c["dist"][blk, band, slot] == cnd.dist
                        yy = np.array(cnd.y[:m], np.int32)
                        assert np.array_equal(c["y"][slot, blk, a:b], yy)
                        assert c["moment"][blk, band, slot] == int((np.arange(m) * np.abs(yy)).sum())
                        if cnd.dist <= best_cost:
                            best_cost, best_qg, best_y = cnd.dist, cnd.gain, yy
                assert qg[blk, band] == best_qg
                if best_qg:
                    gexp = o.odo_gain_expand(best_qg << 8, qb[band], bb[band])
                    syn = np.zeros(m, np.int32)
                    o.odo_pvq_synthesis_partial(P(syn), P(best_y), None, m, 1, gexp, 0, 0, 1,
                                                P(qi))
                    outvec[a:b] = syn
            blkout = np.zeros((n, n), np.int32)
            o.odo_coding_order_to_raster(P(blkout), n, P(outvec), n)
            want_dq[by * n:(by + 1) * n, bx * n:(bx + 1) * n] = blkout
    assert nsearched > 0
    assert np.array_equal(dq, want_dq), bs


@pytest.mark.parametrize("pli,dec", [(0, 0), (1, 1)])
def test_band_stage_matches_oracle(hip, pli, dec):
    W, H = 128, 128
    planes = synth_frame(W, H, seed=5)
    rng = np.random.RandomState(17)
    # stronger texture so that gains > 1 and multi-pulse searches occur
    planes[0] = np.clip(planes[0].astype(int) + rng.randint(-60, 61, size=(H, W)), 0, 255).astype(np.uint8)
    px = planes[0] if dec == 0 else planes[1]
    levels = _oracle_pyramid(px, dec, (W, H))
    for bs in range(5 - dec):
        _check_level_against_oracle(hip, levels[bs], bs, pli)


# (192, 128): an odd number of superblocks per row (3x2 of luma, 3x2 tiles of 32 of 4:2:0 chroma) - one
# workgroup per superblock instead of walkers and superblock pairs - with interior edges both ways;
# (64, 64): a single luma superblock, a 32x32 chroma plane without any edge strip
INVERSE_SIZES = [(256, 192), (192, 128), (64, 64)]


@pytest.mark.parametrize("size", INVERSE_SIZES, ids=lambda s: "%dx%d" % s)
@pytest.mark.parametrize("dec", [0, 1])
def test_inverse_from_pvq_equals_synth_then_inverse(hip, dec, size):
    """odhip_inverse_level_pvq (dequantise on load, no dq plane) must give the
    same pixels as select_synth + inverse_level, at every level, with and
    without a host rate table."""
    import torch
    W, H = size
    planes = synth_frame(W, H, seed=21)
    rng = np.random.RandomState(4)
    src = planes[0] if dec == 0 else planes[1]
    src = np.clip(src.astype(int) + rng.randint(-70, 71, size=src.shape), 0, 255).astype(np.uint8)
    px = _cuda(np.stack([src, src[::-1].copy()]))
    pli = 0 if dec == 0 else 1
    levels = hip.forward_pyramid(px, dec, W, H)
    qt = hip.QuantTables.load()
    for bs in range(5 - dec):
        qm, qmi = qt.qm_slices(pli, bs)
        for use_rate in (False, True):
            job = hip.PvqJob(levels[bs], bs, _cuda(qm), _cuda(qmi), qt.q_band(pli, bs),
                             qt.beta_band(pli, bs), dq=torch.empty_like(levels[bs]))
            if use_rate:
                job.rate = torch.from_numpy(rng.uniform(0, 60, size=tuple(job.cands["band"].shape[:2]) + (2,))).cuda()
            hip.pvq_noref_bands_multi([job], hip.OD_PVQ_LAMBDA)
            hip.pvq_select_synth_noref_multi([job], hip.OD_PVQ_LAMBDA)
            want = hip.inverse_level(job.dq, dec, bs, W, H)
            qg_a = job.cands["choice"][..., 1].clone()
            hip.pvq_choose_multi([job], hip.OD_PVQ_LAMBDA)
            assert torch.equal(job.cands["choice"][..., 1], qg_a)
            got = hip.inverse_level_pvq(job, dec, W, H)
            assert torch.equal(got, want), (dec, bs, use_rate)
            if use_rate:
                # the rate table must be able to change choices (cost = dist + lambda*rate)
                job.rate = None
                hip.pvq_choose_multi([job], hip.OD_PVQ_LAMBDA)
                assert not torch.equal(job.cands["choice"][..., 1], qg_a) or bs == 4


@pytest.mark.parametrize("size", INVERSE_SIZES, ids=lambda s: "%dx%d" % s)
@pytest.mark.parametrize("dec", [0, 1])
def test_inverse_levels_in_one_launch_equal_level_by_level(hip, dec, size):
    import torch
    W, H = size
    planes = synth_frame(W, H, seed=27)
    rng = np.random.RandomState(5)
    src = planes[0] if dec == 0 else planes[1]
    src = np.clip(src.astype(int) + rng.randint(-70, 71, size=src.shape), 0, 255).astype(np.uint8)
    px = _cuda(np.stack([src, src[::-1].copy(), src[:, ::-1].copy()]))
    pli = 0 if dec == 0 else 1
    levels = hip.forward_pyramid(px, dec, W, H)
    qt = hip.QuantTables.load()
    jobs = []
    for bs in range(5 - dec):
        qm, qmi = qt.qm_slices(pli, bs)
        jobs.append(hip.PvqJob(levels[bs], bs, _cuda(qm), _cuda(qmi), qt.q_band(pli, bs),
                               qt.beta_band(pli, bs)))
    hip.pvq_noref_bands_multi(jobs, hip.OD_PVQ_LAMBDA)
    hip.pvq_choose_multi(jobs, hip.OD_PVQ_LAMBDA)
    want = [hip.inverse_level_pvq(j, dec, W, H) for j in jobs]
    got = hip.inverse_levels_pvq(jobs, dec, W, H)
    for bs, (g, w_) in enumerate(zip(got, want)):
        assert torch.equal(g, w_), (dec, bs)
    # a subset of levels, in a different order
    got2 = hip.inverse_levels_pvq([jobs[2], jobs[0]], dec, W, H)
    assert torch.equal(got2[0], want[2]) and torch.equal(got2[1], want[0])


@pytest.mark.parametrize("dec,size", [(0, (256, 192)), (1, (256, 192)), (0, (64, 128)), (1, (128, 64))])
def test_priced_choice_inside_the_search_equals_the_choice_kernel(hip, dec, size):
    """odhip_pvq_noref_bands_priced_multi (the search kernels decide from their registers) and
    odhip_pvq_noref_bands_multi + odhip_pvq_choose_priced_multi (a choice kernel reads the
    records) leave identical choice records and identical pulses of every chosen candidate (the
    fused stage does not write a losing second candidate or the second half of a record unless
    the decision was a close call); and with the decision margin forced wide - every band a
    close call - the host-libm resolve re-decides bands to the same result, byte for byte."""
    import torch
    W, H = size              # the small ones: fewer blocks than a wavefront has lanes at the upper levels
    big = W*H > 20000
    planes = synth_frame(W, H, seed=29)
    rng = np.random.RandomState(6)
    src = planes[0] if dec == 0 else planes[1]
    src = np.clip(src.astype(int) + rng.randint(-70, 71, size=src.shape), 0, 255).astype(np.uint8)
    px = _cuda(np.stack([src, src[::-1].copy()]))
    pli = 0 if dec == 0 else 1
    levels = hip.forward_pyramid(px, dec, W, H)
    qt = hip.QuantTables.load()
    lam = hip.OD_PVQ_LAMBDA

    def jobs():
        out = []
        for bs in range(5 - dec):
            qm, qmi = qt.qm_slices(pli, bs)
            out.append(hip.PvqJob(levels[bs], bs, _cuda(qm), _cuda(qmi), qt.q_band(pli, bs),
                                  qt.beta_band(pli, bs)))
        return out

    a, b, c = jobs(), jobs(), jobs()
    hip.pvq_noref_bands_multi(a, lam)
    assert hip.pvq_choose_priced_multi(a, lam) == 0
    assert hip.pvq_choose_priced_multi(b, lam, fused_bands=True) == 0
    hip.set_price_tol_scale(1e12)
    try:
        redone = hip.pvq_choose_priced_multi(c, lam, fused_bands=True)
    finally:
        hip.set_price_tol_scale(1.)
    assert redone > (100 if big else 10)
    torch.cuda.synchronize()
    nonzero = 0
    second = 0
    for ja, jb, jc in zip(a, b, c):
        # every decision listed as a close call (c): everything is written, as by the unfused stage
        for key in ("choice", "band", "y"):
            assert torch.equal(ja.cands[key], jc.cands[key]), (ja.bs, key, "resolved")
        # decided in the search (b): the choice and the chosen candidate's pulses; what nobody
        # reads (a losing candidate, the band records: every band is decided by the lanes that
        # prepared it) is not written
        assert torch.equal(ja.cands["choice"], jb.cands["choice"]), (ja.bs, "choice")
        nb, offs, ln = hip.pvq_band_layout(ja.bs)
        band_of = torch.zeros(ln, dtype=torch.long, device="cuda")
        for bnd in range(nb):
            band_of[offs[bnd]:offs[bnd + 1]] = bnd
        ch = ja.cands["choice"]
        for slot in (0, 1):
            picked = (ch[:, :, 0] == slot) & (ch[:, :, 1] != 0)     # [B][nb]
            per_coef = picked[:, band_of]                             # [B][len]
            per_coef[:, 0] = False                                    # the DC slot belongs to no band
            assert torch.equal(ja.cands["y"][slot][per_coef], jb.cands["y"][slot][per_coef]), (ja.bs, slot)
            if slot:
                second += int(picked.sum())

        nonzero += int((ch.view(-1, 4)[:, 1] != 0).sum())
    assert nonzero > (1000 if big else 100) and second > (100 if big else 0)
    # pricing really changes decisions: the distortion-only choice differs somewhere
    d = jobs()
    hip.pvq_noref_bands_multi(d, lam)
    hip.pvq_choose_multi(d, lam)
    assert any(not torch.equal(ja.cands["choice"], jd.cands["choice"]) for ja, jd in zip(a, d))


def test_decided_kernels_leave_the_oracles_candidates_and_cosine_distances(hip):
    """odhip_pvq_noref_bands_priced_multi on a 64x128 luma plane and its 32x64 chroma pair, nine jobs in
    one set of launches: two 64x64 blocks, so the last wavefront of every kernel, lane pair and quad is
    partly dead.  With the decision margin forced wide every band with a searched candidate is a close
    call, so the kernels that decide in place write everything they hold: both candidates of every band -
    the padded 15-coefficient one included - their record and their cosine distances are the oracle's."""
    import torch
    W, H = 64, 128
    planes = synth_frame(W, H, seed=41)
    rng = np.random.RandomState(3)
    noisy = [np.clip(p.astype(int) + rng.randint(-70, 71, size=p.shape), 0, 255).astype(np.uint8) for p in planes]
    qt = hip.QuantTables.load()
    lam = hip.OD_PVQ_LAMBDA
    jobs = []
    for dec, pli, px in ((0, 0, noisy[0][None]), (1, 1, np.stack([noisy[1], noisy[2]]))):
        levels = hip.forward_pyramid(_cuda(px), dec, W, H)
        for bs in range(5 - dec):
            qm, qmi = qt.qm_slices(pli, bs)
            job = hip.PvqJob(levels[bs], bs, _cuda(qm), _cuda(qmi), qt.q_band(pli, bs), qt.beta_band(pli, bs))
            job.cands = hip.alloc_pvq_cands(job.nblocks, bs, "cuda", cos_dist=True)
            jobs.append((pli, job))
    hip.set_price_tol_scale(1e12)
    try:
        hip.pvq_choose_priced_multi([j for _, j in jobs], lam, fused_bands=True)
    finally:
        hip.set_price_tol_scale(1.)
    torch.cuda.synchronize()
    nsearched = 0
    for pli, job in jobs:
        bs = job.bs
        n = 4 << bs
        qm, qmi = qt.qm_slices(pli, bs)
        qb, bb = qt.q_band(pli, bs), qt.beta_band(pli, bs)
        nb, offs, _ = hip.pvq_band_layout(bs)
        c = hip.unpack_cands(job.cands)
        coef = job.coef.cpu().numpy()
        nplanes, h, w = coef.shape
        for p in range(nplanes):
            for by in range(h // n):
                for bx in range(w // n):
                    blk = (p*(h // n) + by)*(w // n) + bx
                    vec = block_vector(coef[p], n, bx, by)
                    for band in range(nb):
                        a, b = offs[band], offs[band + 1]
                        _, nr = band_trace(vec[a:b], qb[band], bb[band], qm[a:b], np.ascontiguousarray(qmi[a:b]), lam)
                        for slot in range(2):
                            at = (bs, blk, band, slot)
                            if slot >= len(nr) or not nr[slot].searched:
                                assert c["cos_dist"][blk, band, slot] == 0, at
                                continue
                            cnd = nr[slot]
                            nsearched += 1
                            yy = np.array(cnd.y[:b - a], np.int32)
                            assert c["cos_dist"][blk, band, slot] == cnd.cos_dist, at
                            assert c["gain"][blk, band, slot] == cnd.gain and c["k"][blk, band, slot] == cnd.k, at
                            assert c["flags"][blk, band, slot] == 1 and c["dist"][blk, band, slot] == cnd.dist, at
                            assert np.array_equal(c["y"][slot, blk, a:b], yy), at
                            assert c["yy"][blk, band, slot] == int((yy*yy).sum()), at
                            assert c["moment"][blk, band, slot] == int((np.arange(b - a)*np.abs(yy)).sum()), at
    assert nsearched > 1000


def test_pair_search_sequential_combine_equals_exact_combine(hip, monkeypatch):
    """The 128-coefficient band is searched by two lanes per band; the halves of
    the greedy argmax are combined by an exact-arithmetic argument, with a
    literal sequential rescan when its bound does not hold.
    ODHIP_PVQ_FORCE_SEQ=1 forces the rescan: both must give the same records
    and pulses (the default path is checked against the oracle above)."""
    import torch
    W, H = 256, 192
    planes = synth_frame(W, H, seed=33)
    rng = np.random.RandomState(9)
    src = np.clip(planes[0].astype(int) + rng.randint(-90, 91, size=planes[0].shape), 0, 255)
    px = _cuda(src.astype(np.uint8)[None])
    levels = hip.forward_pyramid(px, 0, W, H)
    qt = hip.QuantTables.load()
    for bs in (2, 3, 4):
        qm, _ = qt.qm_slices(0, bs)
        outs = []
        for force in ("0", "1"):
            monkeypatch.setenv("ODHIP_PVQ_FORCE_SEQ", force)
            job = hip.PvqJob(levels[bs], bs, _cuda(qm), None, qt.q_band(0, bs), qt.beta_band(0, bs))
            hip.pvq_noref_bands_multi([job], hip.OD_PVQ_LAMBDA)
            torch.cuda.synchronize()
            outs.append((job.cands["band"].clone(), job.cands["y"].clone()))
        assert torch.equal(outs[0][0], outs[1][0]), bs
        assert torch.equal(outs[0][1], outs[1][1]), bs
        k = hip.unpack_cands({"band": outs[0][0], "y": outs[0][1], "choice": outs[0][1]})["k"]
        assert k.max() > 8   # multi-pulse searches did run


def test_pulse_count_above_layout_limit_is_reported_not_searched(hip):
    """A band whose K exceeds ODHIP_PVQ_MAX_K (32767; only reachable with absurd
    quantisers) must come back as flags == 2 with k saturated, must not be
    searched (no hang: K pulses x n candidates would run for minutes) and must
    never be chosen."""
    import torch
    rng = np.random.RandomState(3)
    coef = (rng.randint(-(1 << 19), 1 << 19, size=(1, 64, 64))).astype(np.int32)
    qt = hip.QuantTables.load()
    qm, qmi = qt.qm_slices(0, 0)
    tc = _cuda(coef)
    job = hip.PvqJob(tc, 0, _cuda(qm), _cuda(qmi), [1], [4096], dq=torch.empty_like(tc))
    hip.pvq_noref_bands_multi([job], hip.OD_PVQ_LAMBDA)
    hip.pvq_choose_multi([job], hip.OD_PVQ_LAMBDA)
    torch.cuda.synchronize()
    c = hip.unpack_cands(job.cands)
    over = c["flags"] == 2
    assert over.any()
    assert (c["k"][over] == 32767).all()
    qg = c["choice"][..., 1]
    for slot in range(2):
        bad = over[..., slot] & (qg == c["gain"][..., slot]) & (qg != 0)
        assert not bad.any()
    assert (c["yy"][over] == 0).all()


def test_jobs_argument_validation(hip):
    """Every bad argument table is ODHIP_EINVAL before anything is launched (the output buffers keep their
    content), and a valid call on the same context afterwards still matches the oracle.  (The twin of
    test_ref_jobs_argument_validation; a luma job of the wrong size is a matter of the with-reference jobs
    only.)"""
    import torch
    from daala_amd.api import _Job
    L = hip.lib()
    lam = cd(hip.OD_PVQ_LAMBDA)
    EINVAL = -10
    bs, pli = 1, 0
    rng = np.random.RandomState(23)
    coef = (rng.laplace(size=(2, 32, 32)) * 200).astype(np.int32)
    qt = hip.QuantTables.load()
    qm, qmi = qt.qm_slices(pli, bs)
    job = hip.PvqJob(_cuda(coef), bs, _cuda(qm), _cuda(qmi), qt.q_band(pli, bs), qt.beta_band(pli, bs))
    for name in ("band", "y", "choice"):
        job.cands[name].view(torch.uint8).fill_(0x5a)
    kept = {name: job.cands[name].clone() for name in ("band", "y", "choice")}
    stages = (L.odhip_pvq_noref_bands_multi, L.odhip_pvq_noref_bands_priced_multi)

    def call(fn, structs, njobs=None):
        arr = (_Job * max(len(structs), 1))(*structs)
        return fn(arr, len(structs) if njobs is None else njobs, lam, None)

    def bad(cands=None, **fields):
        st = job.struct()
        for k, v in (cands or {}).items():
            setattr(st.cands, k, v)
        for k, v in fields.items():
            setattr(st, k, v)
        return [st]

    addr = lambda t, off: ctypes.c_void_p(t.data_ptr() + off)  # noqa: E731
    zero_q = (ctypes.c_int32 * 12)(*list(job.q_band))
    zero_q[1] = 0
    cases = {
        "record pointer off 64": bad(cands={"band": addr(job.cands["band"], 16)}),
        "pulse pointer off 16": bad(cands={"y": addr(job.cands["y"], 2)}),
        "choice pointer off 16": bad(cands={"choice": addr(job.cands["choice"], 4)}),
        "no choice buffer": bad(cands={"choice": None}),
        "q_band entry 0": bad(q_band=ctypes.addressof(zero_q)),
        "q_band2, plane_split 0": bad(q_band2=ctypes.addressof(job.q_band), plane_split=0),
        "q_band2, plane_split nplanes": bad(q_band2=ctypes.addressof(job.q_band), plane_split=2),
        "width off the block size": bad(w=32 - 4),
    }
    for fn in stages + (L.odhip_pvq_choose_priced_multi, L.odhip_pvq_select_synth_noref_multi):
        assert call(fn, [job.struct()], njobs=0) == EINVAL
        assert call(fn, [job.struct()] * 17) == EINVAL          # kMaxJobs is 16
        for what, structs in cases.items():
            assert call(fn, structs) == EINVAL, (fn.__name__, what)
    torch.cuda.synchronize()
    for name, t in kept.items():
        assert torch.equal(job.cands[name], t), name
    _check_level_against_oracle(hip, coef[0], bs, pli)
