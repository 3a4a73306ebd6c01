"""GPU parity of k_refb_prep_corner - the preparation of bands 0-2 of a with-reference block in one
lane - where that kernel can go wrong: a partly filled wavefront, a job without bands 1-2, plane sets
that split (Cb / Cr quantisers, chroma plane p reading luma plane p mod F), every kind of reference
(the luma band stage's choices and pulses at 4:2:0 and 4:4:4, a reference plane) and per-plane
quantiser rows.

Luma planes are 192x64, 4:2:0 chroma planes 96x32: chroma levels 0..3 then have 192 / 48 / 12 / 3
blocks per plane - whole wavefronts at 4x4, partial ones above, and a level-0 job with band 0 only.

Three checks per case:
  - after odhip_pvq_ref_bands_multi every record field, x16, r16, xr, candidate and search equals
    the CPU oracle's (tests/_refbands.py), band by band - the yardstick;
  - with the theta margin forced wide (the contexts' test hook) the decided stage's choices and
    pulses equal the plain run's;
  - the experiments build's split path (two k_refb_prep_lane launches, ODHIP_REFB_PREP_SPLIT) in a
    child process on the same inputs: records, x16, r16, xr, the bands listed under the forced
    margin and the decided choices byte for byte those of the default library.
The work-class keys of the decided stage live in library scratch without an accessor; they decide
which lane takes which band, never a band's result, and are covered through the decisions.

One more case goes through the whole frame-batch step: full-precision references at 10 bits
against the compiled reference (oracle/_ref)."""
import ctypes
import os
import subprocess
import sys

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)

from _refbands import Mismatch, compare_bands, make_planes, oracle_traces  # noqa: E402

pytestmark = pytest.mark.gpu

LW, LH = 192, 64
CASES = ("cfl420-f1", "cfl420-f2", "cfl444-f1", "inter-luma", "inter-chroma", "qplane-f2")
KEPT = ("band", "x16", "r16", "xr")


def _cuda(a):
    import torch
    return torch.from_numpy(np.ascontiguousarray(a)).cuda()


def _ref_job_class(hip):
    class Job(hip.PvqRefJob):
        """PvqRefJob with the two optional inputs the Python class leaves NULL: the luma job a
        keyframe chroma job takes its reference from, and per-plane quantiser rows."""
        luma_job = None
        q_plane = None

        def struct(self):
            st = super().struct()
            if self.luma_job is not None:
                self._luma_struct = self.luma_job.struct()
                st.luma = ctypes.cast(ctypes.pointer(self._luma_struct), ctypes.c_void_p)
            if self.q_plane is not None:
                st.d_q_plane = ctypes.c_void_p(self.q_plane.data_ptr())
            return st
    return Job


def _luma_stage(hip, rng, F, levels):
    """F luma coefficient planes per level through the no-reference band stage, its choice and its
    synthesis: {level: job}; job.dq is what the decoder would see."""
    import torch
    qt = hip.QuantTables.load()
    jobs = {}
    for bs in levels:
        qm, qmi = qt.qm_slices(0, bs)
        coef = _cuda(make_planes(rng, F, LH, LW, bs)[0])
        jobs[bs] = hip.PvqJob(coef, bs, _cuda(qm), _cuda(qmi), qt.q_band(0, bs), qt.beta_band(0, bs),
                              dq=torch.zeros_like(coef))
    lst = [jobs[bs] for bs in levels]
    hip.pvq_noref_bands_multi(lst, hip.OD_PVQ_LAMBDA)
    hip.pvq_choose_multi(lst, hip.OD_PVQ_LAMBDA)
    hip.pvq_select_synth_noref_multi(lst, hip.OD_PVQ_LAMBDA)
    torch.cuda.synchronize()
    return jobs


def _chroma_like(rng, ref, bs):
    """Chroma coefficients that follow their reference with a per-block sign and gain, plus noise."""
    n = 4 << bs
    nplanes, h, w = ref.shape
    noise = make_planes(rng, nplanes, h, w, bs)[0]
    up = lambda a: np.kron(a, np.ones((n, n)))  # noqa: E731
    x = np.zeros_like(ref)
    for p in range(nplanes):
        sign = up(rng.choice([1, 1, -1], size=(h // n, w // n)))
        gain = up(rng.choice([0.3, 0.8, 1.5], size=(h // n, w // n)))
        mix = up(rng.choice([0.05, 0.3, 1.0], size=(h // n, w // n)))
        x[p] = np.clip(sign * gain * ref[p] + mix * noise[p], -(1 << 21), 1 << 21).astype(np.int32)
    return x


def _build(hip, case):
    """-> (jobs, meta, keep): meta[i] = (coef, ref, qm, qmi, per-plane band steps, beta, is_keyframe,
    pli) of job i for the oracle; keep = what the jobs point to."""
    Job = _ref_job_class(hip)
    qt = hip.QuantTables.load()
    rng = np.random.RandomState(1000 + CASES.index(case))
    jobs, meta, keep = [], [], []
    if case.startswith("inter"):
        pli = 1 if case == "inter-chroma" else 0
        nplanes, h, w = (2, LH // 2, LW // 2) if pli else (1, LH, LW)
        for bs in range(5 - pli):
            qm, qmi = qt.qm_slices(pli, bs)
            x, r = make_planes(rng, nplanes, h, w, bs)
            q1, bb = qt.q_band(pli, bs), qt.beta_band(pli, bs)
            q2 = qt.q_band(2, bs) if pli else None
            jobs.append(Job(_cuda(x), _cuda(r), bs, _cuda(qm), _cuda(qmi), q1, bb, 0, pli, q_band2=q2,
                            plane_split=1))
            meta.append((x, r, qm, qmi, [q1, q2] if pli else [q1], bb, 0, pli))
        return jobs, meta, keep
    F = int(case[-1])
    c444 = case.startswith("cfl444")
    dec = 0 if c444 else 1
    luma = _luma_stage(hip, rng, F, range(dec, 5))
    keep.append(luma)
    h, w = LH >> dec, LW >> dec
    for bs in range(5 - dec):
        n = 4 << bs
        dq = luma[bs + dec].dq.cpu().numpy()
        if c444:
            r = dq
        else:
            # od_resample_luma_coeffs: the upper-left quarter of the decoded luma block one size up
            r = dq.reshape(F, LH // (2 * n), 2 * n, LW // (2 * n), 2 * n)[:, :, :n, :, :n].reshape(F, h, w)
        r = np.ascontiguousarray(np.concatenate([r, r]))      # chroma plane p: luma plane p mod F
        x = _chroma_like(rng, r, bs)
        qm, qmi = qt.qm_slices(dec, bs)
        q1, q2, bb = qt.q_band(1, bs), qt.q_band(2, bs), qt.beta_band(1, bs)
        # the plane the kernels must NOT read: the reference comes from the luma job
        decoy = _cuda(rng.randint(-4000, 4000, size=x.shape).astype(np.int32))
        job = Job(_cuda(x), decoy, bs, _cuda(qm), _cuda(qmi), q1, bb, 1, 1, q_band2=q2, plane_split=F)
        job.luma_job = luma[bs + dec]
        steps = [q1] * F + [q2] * F
        if case.startswith("qplane"):
            steps = [[max(1, int(v) * (p + 2) // 2) for v in (q1 if p < F else q2)] for p in range(2 * F)]
            rows = np.zeros((2 * F, 12), np.int32)
            for p, row in enumerate(steps):
                rows[p, :len(row)] = row
            job.q_plane = _cuda(rows)
        jobs.append(job)
        meta.append((x, r, qm, qmi, steps, bb, 1, 1))
    return jobs, meta, keep


def _decisions(jobs):
    """Per job (choice records without word 9 - it names the pulse slot -, the winners' pulses)."""
    out = []
    for j in jobs:
        ch = j.choice.cpu().numpy()
        y = j.y.cpu().numpy()
        win = np.zeros((ch.shape[0], j.len), np.int16)
        for band in range(j.nb):
            lo, hi = j.offsets[band], j.offsets[band + 1]
            slot = ch[:, band, 9]
            idx = np.nonzero(slot >= 0)[0]
            v = y[slot[idx], idx, lo:hi].copy()
            v[ch[idx, band, 2] == 0, -1] = 0      # a theta winner holds n - 1 pulses (the last is a pad)
            win[idx, lo:hi] = v
        out.append((np.delete(ch, 9, axis=2), win))
    return out


def _run(hip, case, with_oracle):
    """Everything one case computes, once: {name: array} for the byte comparison of the two builds,
    the oracle's verdict, and the decided stage plain / under the forced margin."""
    import torch
    lam = hip.OD_PVQ_LAMBDA
    jobs, meta, keep = _build(hip, case)
    out = {}
    assert hip.pvq_ref_bands_multi(jobs, lam) == 0
    torch.cuda.synchronize()
    for i, j in enumerate(jobs):
        for f in KEPT:
            out["%d.%s" % (i, f)] = getattr(j, f).cpu().numpy().copy()
    mm = None
    if with_oracle:
        mm = Mismatch()
        for job, (x, r, qm, qmi, steps, bb, is_keyframe, pli) in zip(jobs, meta):
            per = job.nblocks // x.shape[0]
            traces = {}
            # one oracle pass per plane: its own band steps
            for p in range(x.shape[0]):
                q = steps[p] if len(steps) == x.shape[0] else steps[min(p, len(steps) - 1)]
                t, _ = oracle_traces(x[p:p + 1], r[p:p + 1], job.bs, qm, qmi, q, bb, is_keyframe, pli, lam)
                traces.update({(blk + p * per, b): v for (blk, b), v in t.items()})
            compare_bands(hip, job, traces, mm)
    # the bands listed under a forced theta margin (the record's flag is set where the band is listed)
    hip.pvq_ref_set_theta_margin(0.25, True)
    try:
        hip.pvq_ref_bands_multi(jobs, lam, resolve=False)
        torch.cuda.synchronize()
        for i, j in enumerate(jobs):
            out["%d.listed" % i] = (j.unpack()["rec"]["flags"] & hip.REFBAND_UNCERTAIN) != 0
    finally:
        hip.pvq_ref_set_theta_margin(0, False)
    # the decided stage, plain and under the forced margin
    nt, _ = hip.pvq_ref_bands_decided_multi(jobs, lam)
    torch.cuda.synchronize()
    assert nt == 0
    plain = _decisions(jobs)
    for j in jobs:
        j.choice.zero_()
        j.y.zero_()
    hip.pvq_ref_set_theta_margin(0.25, True)
    try:
        nt, _ = hip.pvq_ref_bands_decided_multi(jobs, lam)
    finally:
        hip.pvq_ref_set_theta_margin(0, False)
    torch.cuda.synchronize()
    forced = _decisions(jobs)
    for i, (ch, win) in enumerate(plain):
        out["%d.choice" % i] = ch
        out["%d.pulses" % i] = win
    return dict(out=out, mm=mm, plain=plain, forced=forced, relisted=nt,
                listed=sum(int(out["%d.listed" % i].sum()) for i in range(len(jobs))))


@pytest.fixture(scope="module")
def hip():
    import torch
    import daala_amd
    assert torch.cuda.is_available()
    daala_amd.init(0)
    return daala_amd


@pytest.fixture(scope="module")
def runs(hip):
    cache = {}

    def get(case):
        if case not in cache:
            cache[case] = _run(hip, case, True)
        return cache[case]
    return get


@pytest.fixture(scope="module")
def split_runs(tmp_path_factory):
    """Every case through the experiments library's split path, in one child process."""
    import daala_amd
    path = str(tmp_path_factory.mktemp("refprep") / "split.npz")
    env = dict(os.environ)
    env.update(ODHIP_LIB=daala_amd.EXPERIMENTS_LIB, ODHIP_REFB_PREP_SPLIT="1")
    r = subprocess.run([sys.executable, os.path.abspath(__file__), path], env=env, capture_output=True, text=True,
                       timeout=600, cwd=ROOT)
    assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-2000:]
    return np.load(path)


@pytest.mark.parametrize("case", CASES)
def test_corner_preparation_matches_oracle(runs, case):
    mm = runs(case)["mm"]
    assert mm.total() == 0, mm.summary()
    for what in ("rec.corr", "x16", "r16", "xr", "flag.flip", "item.y"):
        assert mm.checked.get(what, 0) > 100, (what, mm.summary())


@pytest.mark.parametrize("case", CASES)
def test_decided_stage_under_a_forced_theta_margin_equals_the_plain_one(runs, case):
    r = runs(case)
    assert r["listed"] > 20 and r["relisted"] > 20
    for i, ((ca, wa), (cb, wb)) in enumerate(zip(r["plain"], r["forced"])):
        assert np.array_equal(ca, cb), (case, i, "choice")
        assert np.array_equal(wa, wb), (case, i, "pulses")


@pytest.mark.parametrize("case", CASES)
def test_default_library_equals_the_split_path_of_the_experiments_library(runs, split_runs, case):
    out = runs(case)["out"]
    names = [k for k in split_runs.files if k.startswith(case + "/")]
    assert sorted(names) == sorted(case + "/" + k for k in out)
    for k, v in out.items():
        assert np.array_equal(v, split_runs[case + "/" + k]), (case, k)


def test_full_precision_references_at_10_bits_equal_the_compiled_reference(hip):
    """The frame-batch step at 192x64 with fpr_bits = 10 (keyframe, chroma from luma, every band decided
    inside its search): reconstructed samples and every band's decision against the reference's own C
    functions in full-precision-references mode."""
    from _libs import ref, synth_frame
    if ref() is None:
        pytest.skip("oracle/_ref not present")
    import _pipeline_check as C
    qt = hip.QuantTables.for_quality(40)
    rng = np.random.RandomState(10)
    pics = []
    for pl in synth_frame(LW, LH, seed=5):
        p8 = np.clip(pl.astype(np.int32) + rng.randint(-30, 31, size=pl.shape), 0, 255)
        pics.append(((p8 << 2) + rng.randint(0, 4, size=p8.shape)).astype(np.int16))
    want = []
    cpu, _, _ = C.cpu_frame(qt, pics, LW, LH, fpr_bits=10, decisions=want)
    gpu, _, dec = C.gpu_device_priced(hip, qt, pics, LW, LH, fpr_bits=10, decisions=True)
    assert C.compare_frame(gpu, cpu) == []
    assert C.compare_decisions(dec, want) == []
    assert int(cpu[1][0].max()) > 255


if __name__ == "__main__":
    # the child of split_runs: every case with whatever library and switches the environment names
    import daala_amd
    daala_amd.init(0)
    assert hasattr(daala_amd.lib(), "odhip_exp_row_replay_stats"), "the experiments build is expected here"
    dump = {}
    for c in CASES:
        for k, v in _run(daala_amd, c, False)["out"].items():
            dump[c + "/" + k] = v
    np.savez(sys.argv[1], **dump)
