"""GPU: the decided with-reference band stage (odhip_pvq_ref_bands_decided_multi) on its own hand-over
format - a 32-byte record per band in a library buffer, x16 stored for the bands with no-reference
candidates and xr for the bands with theta candidates alone - and the list-driven preparation that
rebuilds the job's public records and vectors for the bands a resolve re-runs (k_refb_prep_list).

One call of six jobs, the smallest shapes at which these kernels can go wrong:
  - a 64x128 luma plane through the no-reference stage and its 32x64 Cb / Cr pair against it, chroma
    levels 0..3 (128 / 32 / 8 / 2 blocks per plane: the top level leaves every wavefront partly dead);
  - an inter job of 65 8x8 blocks (one more than a wavefront of blocks) with a reference plane;
  - an inter job of 63 8x8 blocks (one less) with a per-plane quantiser table (d_q_plane).
The oracle (tests/_refbands.py: pvq_theta at speed 1) runs once per session on these jobs.

Which flags can occur.  The searches read xr where ODHIP_REFBAND_THETA is set (the reference is not all
zero and corr > 0) and x16 where ODHIP_REFBAND_NOREF is (keyframe luma, corr < .5 or cg < 2 in Q8).  A band
without THETA has corr <= 0 or corr = 0 (all-zero reference), hence corr < .5, hence NOREF: a band with
NEITHER flag cannot exist, and the test asserts that none does, beside the presence of the other three."""
import os
import subprocess
import sys

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)

from _refbands import Mismatch, compare_bands, make_planes, oracle_traces  # noqa: E402
from test_gpu_pvq_corpus_decided import _compare_decided  # noqa: E402
from test_gpu_refprep_corner import _chroma_like, _cuda, _decisions, _ref_job_class  # noqa: E402

pytestmark = pytest.mark.gpu

LW, LH = 128, 64
POISON = 0x5a


def _luma(hip, rng):
    """The luma plane at levels 1..4 through the no-reference stage, its choice and its synthesis."""
    import torch
    qt = hip.QuantTables.load()
    jobs = {}
    for bs in range(1, 5):
        qm, qmi = qt.qm_slices(0, bs)
        coef = _cuda(make_planes(rng, 1, LH, LW, bs)[0])
        jobs[bs] = hip.PvqJob(coef, bs, _cuda(qm), _cuda(qmi), qt.q_band(0, bs), qt.beta_band(0, bs),
                              dq=torch.zeros_like(coef))
    lst = [jobs[bs] for bs in range(1, 5)]
    hip.pvq_noref_bands_multi(lst, hip.OD_PVQ_LAMBDA)
    hip.pvq_choose_multi(lst, hip.OD_PVQ_LAMBDA)
    hip.pvq_select_synth_noref_multi(lst, hip.OD_PVQ_LAMBDA)
    torch.cuda.synchronize()
    return jobs


def _build(hip):
    """Fresh jobs (their own zeroed output and work buffers) over the same content every time ->
    (jobs, meta, keep); meta[i] = (x, r, qm, qmi, band steps per plane, beta, is_keyframe, pli)."""
    Job = _ref_job_class(hip)
    qt = hip.QuantTables.load()
    rng = np.random.RandomState(4242)
    luma = _luma(hip, rng)
    jobs, meta = [], []
    h, w = LH // 2, LW // 2
    for bs in range(4):
        n = 4 << bs
        dq = luma[bs + 1].dq.cpu().numpy()
        # od_resample_luma_coeffs: the upper-left quarter of the decoded luma block one size up
        r = dq.reshape(1, LH // (2 * n), 2 * n, LW // (2 * n), 2 * n)[:, :, :n, :, :n].reshape(1, h, w)
        r = np.ascontiguousarray(np.concatenate([r, r]))
        x = _chroma_like(rng, r, bs)
        qm, qmi = qt.qm_slices(1, bs)
        q1, q2, bb = qt.q_band(1, bs), qt.q_band(2, bs), qt.beta_band(1, bs)
        decoy = _cuda(rng.randint(-4000, 4000, size=x.shape).astype(np.int32))
        job = Job(_cuda(x), decoy, bs, _cuda(qm), _cuda(qmi), q1, bb, 1, 1, q_band2=q2, plane_split=1)
        job.luma_job = luma[bs + 1]
        jobs.append(job)
        meta.append((x, r, qm, qmi, [q1, q2], bb, 1, 1))
    # 65 and 63 blocks of 8x8 (bands of 15, 8, 8 and 32 coefficients), inter, a reference plane
    for (ph, pw), qplane in (((40, 104), False), ((56, 72), True)):
        qm, qmi = qt.qm_slices(0, 1)
        x, r = make_planes(rng, 1, ph, pw, 1, zero_ref_frac=0.1)
        q1, bb = qt.q_band(0, 1), qt.beta_band(0, 1)
        job = Job(_cuda(x), _cuda(r), 1, _cuda(qm), _cuda(qmi), q1, bb, 0, 0)
        steps = [q1]
        if qplane:
            steps = [[max(1, int(v) * 3 // 2) for v in q1]]
            rows = np.zeros((1, 12), np.int32)
            rows[0, :len(steps[0])] = steps[0]
            job.q_plane = _cuda(rows)
        jobs.append(job)
        meta.append((x, r, qm, qmi, steps, bb, 0, 0))
    assert [j.nblocks for j in jobs] == [256, 64, 16, 4, 65, 63]
    return jobs, meta, luma


def _oracle(hip, jobs, meta):
    """Per job {(blk, band): trace}: one oracle pass per plane, at its own band steps."""
    out = []
    for job, (x, r, qm, qmi, steps, bb, is_keyframe, pli) in zip(jobs, meta):
        per = job.nblocks // x.shape[0]
        traces = {}
        for p in range(x.shape[0]):
            t, _ = oracle_traces(x[p:p + 1], r[p:p + 1], job.bs, qm, qmi, steps[p], bb, is_keyframe, pli,
                                 hip.OD_PVQ_LAMBDA)
            traces.update({(blk + p * per, b): v for (blk, b), v in t.items()})
        assert len(traces) == job.nblocks * job.nb
        out.append(traces)
    return out


def _decided(hip, jobs):
    """The decided stage on `jobs` under whatever hooks are set -> (decisions, the two resolve counts)."""
    import torch
    nt, npz = hip.pvq_ref_bands_decided_multi(jobs, hip.OD_PVQ_LAMBDA)
    torch.cuda.synchronize()
    return _decisions(jobs), nt, npz


def _assert_oracle_decisions(jobs, traces, only=None):
    mm = Mismatch()
    for i, (job, tr) in enumerate(zip(jobs, traces)):
        if only is None or i in only:
            _compare_decided(job, tr, mm)
    assert mm.total() == 0, mm.summary()
    return mm


def _assert_same(a, b, tag):
    for i, ((ca, wa), (cb, wb)) in enumerate(zip(a, b)):
        assert np.array_equal(ca, cb), (tag, i, "choice")
        assert np.array_equal(wa, wb), (tag, i, "pulses")


@pytest.fixture(scope="module")
def hip():
    import torch
    import daala_amd
    assert torch.cuda.is_available()
    daala_amd.init(0)
    return daala_amd


@pytest.fixture(scope="module")
def plain(hip):
    """Hooks off, once: the jobs the decided stage filled, the oracle's traces, the decisions."""
    jobs, meta, keep = _build(hip)
    dec, nt, npz = _decided(hip, jobs)
    return dict(jobs=jobs, meta=meta, keep=keep, traces=_oracle(hip, jobs, meta), dec=dec, nt=nt, npz=npz)


def test_decided_stage_matches_oracle_and_every_flag_kind_occurs(hip, plain):
    import torch
    mm = _assert_oracle_decisions(plain["jobs"], plain["traces"])
    assert mm.checked["y"] == sum(j.nblocks * j.nb for j in plain["jobs"])
    # the flags, from the exporting stage's records of the same jobs (fresh buffers)
    jobs, _, keep = _build(hip)
    assert hip.pvq_ref_bands_multi(jobs, hip.OD_PVQ_LAMBDA) == 0
    torch.cuda.synchronize()
    flags = np.concatenate([j.unpack()["rec"]["flags"].ravel() for j in jobs]).astype(np.int64)
    theta = (flags & hip.REFBAND_THETA) != 0
    noref = (flags & hip.REFBAND_NOREF) != 0
    counts = dict(theta_only=int((theta & ~noref).sum()), noref_only=int((~theta & noref).sum()),
                  both=int((theta & noref).sum()), neither=int((~theta & ~noref).sum()),
                  r_null=int(((flags & hip.REFBAND_R_NULL) != 0).sum()))
    print("bands by flags:", counts)
    assert counts["theta_only"] > 0 and counts["noref_only"] > 0 and counts["both"] > 0, counts
    assert counts["r_null"] > 0, counts
    # (no THETA means corr <= 0, which is below .5: NOREF - see the module's docstring)
    assert counts["neither"] == 0, counts


def test_forced_theta_margin_resolves_through_the_list_preparation(hip, plain):
    jobs, _, keep = _build(hip)
    hip.pvq_ref_set_theta_margin(0.25, True)
    try:
        dec, nt, _ = _decided(hip, jobs)
    finally:
        hip.pvq_ref_set_theta_margin(0, False)
    assert nt > 0
    _assert_same(plain["dec"], dec, "theta margin")


def test_forced_price_margin_resolves_through_the_list_preparation(hip, plain):
    jobs, _, keep = _build(hip)
    hip.set_price_tol_scale(1e12)
    try:
        _, _, npz = _decided(hip, jobs)
    finally:
        hip.set_price_tol_scale(1.)
    assert npz > 0
    _assert_oracle_decisions(jobs, plain["traces"])


def test_decided_stage_reads_no_public_array_and_leaves_the_exporting_stage_alone(hip, plain):
    import torch
    jobs, _, keep = _build(hip)
    for j in jobs:
        j.band.fill_(POISON)
        j.x16.fill_(POISON * 257)
        j.xr.fill_(POISON * 257)
    dec, nt, npz = _decided(hip, jobs)
    assert (nt, npz) == (plain["nt"], plain["npz"])
    _assert_same(plain["dec"], dec, "poisoned public arrays")
    # the exporting stage on the same jobs afterwards: every record, vector, candidate and search
    assert hip.pvq_ref_bands_multi(jobs, hip.OD_PVQ_LAMBDA) == 0
    torch.cuda.synchronize()
    mm = Mismatch()
    for job, tr in zip(jobs, plain["traces"]):
        compare_bands(hip, job, tr, mm)
    assert mm.total() == 0, mm.summary()
    for what in ("rec.corr", "x16", "r16", "xr", "item.y"):
        assert mm.checked.get(what, 0) > 100, (what, mm.summary())
    # ... and the decided stage once more behind it
    dec2, _, _ = _decided(hip, jobs)
    _assert_same(plain["dec"], dec2, "after the exporting stage")


def test_inter_job_and_per_plane_quantiser_job(hip, plain):
    """Jobs 4 and 5 of the call: is_keyframe = 0 with a reference plane, and d_q_plane."""
    jobs = plain["jobs"]
    assert jobs[4].is_keyframe == 0 and jobs[5].q_plane is not None
    mm = _assert_oracle_decisions(jobs, plain["traces"], only=(4, 5))
    assert mm.checked["y"] == (65 + 63) * 4
    # the per-plane steps really differ from the table's: the oracle at the table's steps decides otherwise
    x, r, qm, qmi, _, bb, kf, pli = plain["meta"][5]
    qt = hip.QuantTables.load()
    other, _ = oracle_traces(x, r, 1, qm, qmi, qt.q_band(0, 1), bb, kf, pli, hip.OD_PVQ_LAMBDA)
    assert any(other[k]["ret"] != t["ret"] or not np.array_equal(other[k]["y"], t["y"])
               for k, t in plain["traces"][5].items())


def test_experiments_build_decides_byte_for_byte_the_same(hip, plain, tmp_path):
    import daala_amd
    if not os.path.exists(daala_amd.EXPERIMENTS_LIB):
        pytest.skip("the experiments build is not present")
    path = str(tmp_path / "exp.npz")
    env = dict(os.environ)
    env.update(ODHIP_LIB=daala_amd.EXPERIMENTS_LIB)
    r = subprocess.run([sys.executable, os.path.abspath(__file__), path], env=env, capture_output=True, text=True,
                       timeout=300, cwd=ROOT)
    assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-2000:]
    got = np.load(path)
    assert sorted(got.files) == sorted("%d.%s" % (i, k) for i in range(len(plain["dec"])) for k in ("choice", "pulses"))
    for i, (ch, win) in enumerate(plain["dec"]):
        assert np.array_equal(got["%d.choice" % i], ch), i
        assert np.array_equal(got["%d.pulses" % i], win), i


if __name__ == "__main__":
    # the child of the last test: the plain decisions with whatever library the environment names
    import daala_amd
    daala_amd.init(0)
    assert hasattr(daala_amd.lib(), "odhip_exp_row_replay_stats"), "the experiments build is expected here"
    dump = {}
    for i, (ch, win) in enumerate(_decided(daala_amd, _build(daala_amd)[0])[0]):
        dump["%d.choice" % i] = ch
        dump["%d.pulses" % i] = win
    np.savez(sys.argv[1], **dump)
