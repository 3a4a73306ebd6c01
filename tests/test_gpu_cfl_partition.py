"""GPU: chroma-from-luma reference planes at a block-size map (k_cfl_part in daala_amd/csrc/partition_kernels.hip;
include/daala_hip.h "Chroma-from-luma reference planes at a block-size map").  Every comparison is exact.

  device == oracle  odhip_cfl_refs_partition against the planes of tests/_cfl_partition_ref.py (od_resample_luma_coeffs
                    leaf by leaf) and so against the host entry point (tests/test_cfl_partition_host.py): two luma
                    planes with different maps, planes_per_frame 1 and 2, dec 1 and 0, poison laid first, guard bands
  uniform maps      levels 1..4 are the top-left quarters; on dequantised planes they equal odhip_cfl_refs_from_luma of
                    the same uniform jobs, which reads the pulses instead of the plane
  end to end        keyframe_partition_420 at the decided map and at a mixed one: the reference planes against the
                    oracle on the returned luma dq, every chroma leaf's bands and choices against odo_pvq_theta with
                    is_keyframe = 1 (the CfL flip on leaves of a map), the reconstruction against
                    tests/_partition_ref.py::inverse
"""
import numpy as np
import pytest

import _cfl_partition_ref as C
import _partition_ref as R
from _libs import P, oracle
from _refbands import Mismatch, compare_bands, compare_choice, host_rates, oracle_traces
from test_gpu_partition_bands import _np_gather, _np_scatter, _pictures

pytestmark = pytest.mark.gpu

GUARD = 256                     # int32 entries before and after d_ref: the base stays 16-byte aligned
GUARD_VALUE = 0x3c3c3c3c


@pytest.fixture(scope="module")
def hip():
    import torch
    import daala_amd
    assert torch.cuda.is_available()
    daala_amd.init(0)
    return daala_amd


def _cuda(a):
    import torch
    return torch.from_numpy(np.array(a)).cuda()             # a copy: the shared cases are read-only


def _guarded_refs(hip, luma, bmaps, dec, ppf):
    """cfl_refs_partition into the middle of a guarded, poisoned buffer: the planes, after checking the guards."""
    import torch
    nplanes, h, w = luma.shape
    n = nplanes * ppf * (h >> dec) * (w >> dec)
    buf = torch.full((n + 2 * GUARD,), GUARD_VALUE, dtype=torch.int32, device="cuda")
    out = buf[GUARD:GUARD + n].view(nplanes * ppf, h >> dec, w >> dec)
    out.fill_(C.POISON)
    got = hip.cfl_refs_partition(luma, bmaps, dec, planes_per_frame=ppf, out=out)
    assert got is out
    host = buf.cpu().numpy()
    assert (host[:GUARD] == GUARD_VALUE).all() and (host[-GUARD:] == GUARD_VALUE).all()
    return host[GUARD:GUARD + n].reshape(out.shape)


# ---- 1: the device call is the oracle, leaf by leaf -------------------------------------------------

@pytest.mark.parametrize("dec", [1, 0])
@pytest.mark.parametrize("index", range(len(C.CASES)), ids=C.CASE_IDS)
def test_device_planes_equal_the_oracle_and_the_host_call(hip, index, dec):
    luma, bmaps, want = C.case(index)
    tluma, tmaps = _cuda(luma), _cuda(bmaps)
    for ppf in (1, 2):
        got = _guarded_refs(hip, tluma, tmaps, dec, ppf)
        assert not (got == C.POISON).any()                          # every sample is written
        for q in range(2 * ppf):
            assert np.array_equal(got[q], want[dec][q // ppf]), (ppf, q)
    assert np.array_equal(tluma.cpu().numpy(), luma)
    # the host entry point, the kernel's own code on the CPU, gives the same planes
    for f in range(2):
        assert np.array_equal(hip.cfl_refs_partition_host(luma[f], bmaps[f], dec), want[dec][f])
    # one map for every plane
    one = hip.cfl_refs_partition(tluma, tmaps[1], dec, planes_per_frame=1).cpu().numpy()
    assert np.array_equal(one[1], want[dec][1])
    assert np.array_equal(one[0], C.expected(luma[0], bmaps[1], dec))


# ---- 2: uniform maps --------------------------------------------------------------------------------

def _quarters(planes, n):
    """The top-left n/2 x n/2 of every n x n block of [nplanes][h][w], as planes of h/2 x w/2."""
    nplanes, h, w = planes.shape
    return planes.reshape(nplanes, h // n, n, w // n, n)[:, :, :n // 2, :, :n // 2].reshape(nplanes, h // 2, w // 2)


@pytest.mark.parametrize("level", [1, 2, 3, 4])
def test_uniform_maps_are_the_top_left_quarters(hip, level):
    luma, _, _ = C.case(3)                                          # 192 x 128: w/N is no power of two
    bmap = _cuda(R.uniform(level, 3, 2))
    got = hip.cfl_refs_partition(_cuda(luma), bmap, 1, planes_per_frame=2).cpu().numpy()
    want = _quarters(luma, 4 << level)
    for q in range(4):
        assert np.array_equal(got[q], want[q // 2]), q


@pytest.mark.parametrize("level", [1, 2, 3, 4])
def test_uniform_maps_equal_the_pulse_fed_references_of_the_uniform_jobs(hip, level):
    """odhip_cfl_refs_from_luma dequantises the chosen pulses of ONE uniform luma job on the fly; at a uniform map the
    dense job of pvq_partition_noref is that job, and its scattered dq is what odhip_cfl_refs_partition reads."""
    import torch
    W, H = 192, 128
    px = _cuda(_pictures(0, 3, 2, 1, seed=40 + level))
    bmap = _cuda(R.uniform(level, 3, 2))
    qt = hip.QuantTables.load()
    lam = hip.OD_PVQ_LAMBDA
    coef = hip.forward_partition(px, bmap, 0, W, H)
    res = hip.pvq_partition_noref(coef, bmap, 0, qt.size_tables(0, 0), lam)
    assert list(res.jobs) == [level] and torch.equal(res.jobs[level].dq, res.dq)
    got = hip.cfl_refs_partition(res.dq, bmap, 1, planes_per_frame=2)
    pulse = hip.cfl_refs_from_luma([res.jobs[level]], refs=[torch.zeros_like(got)], copies=2)[0]
    dq = res.dq.cpu().numpy()
    assert (dq != 0).sum() > 1000
    if level == 4:
        # a 64x64 block codes 512 of its 32x32 corner's 1024 positions: the pulse-fed form leaves the others zero,
        # the plane-fed form copies them - equal only because the plane holds zeros there
        o = oracle()
        first = np.zeros(64 * 64, np.int32)
        first[:512] = 1
        coded = np.zeros((64, 64), np.int32)
        o.odo_coding_order_to_raster(P(coded), 64, P(first), 64)
        uncoded = coded[:32, :32] == 0
        assert coded[:32, :32].sum() == 512 and uncoded.sum() == 512
        corners = dq.reshape(2, H // 64, 64, W // 64, 64)[:, :, :32, :, :32]
        assert not corners.transpose(0, 1, 3, 2, 4)[..., uncoded].any()
    # copy k of luma plane p: plane k*nplanes + p there, plane p*2 + k here
    want = pulse.view(2, 2, H // 2, W // 2).transpose(0, 1).reshape(4, H // 2, W // 2)
    assert torch.equal(got, want)
    assert np.array_equal(got.cpu().numpy()[::2], _quarters(dq, 4 << level))


# ---- 3: a 4:2:0 keyframe at its map -----------------------------------------------------------------

@pytest.mark.parametrize("which", ["decided", "mixed"])
def test_keyframe_420_at_a_map_matches_the_oracle_leaf_by_leaf(hip, which):
    """Two 128 x 128 frames, one textured and one flat with edges.  Luma: the no-reference stage, distortion-only
    choice.  Cb and Cr: the host prices every searched candidate between the band stage and the choice, as
    tests/test_gpu_partition_bands.py::test_ref_composition_matches_the_oracle_leaf_by_leaf does; the reference is
    gathered from the planes under test, which are themselves compared with the oracle on the returned luma dq."""
    import torch
    W = H = 128
    lam = hip.OD_PVQ_LAMBDA
    qt = hip.QuantTables.load()
    luma_px = _pictures(0, 2, 2, 1, seed=120)
    chroma_px = _pictures(1, 2, 2, 2, seed=120)
    cb_px, cr_px = chroma_px[0::2], chroma_px[1::2]
    if which == "decided":
        tmaps, relisted = hip.bsize_decide(_cuda(luma_px), qt.quantizer)
        maps = tmaps.cpu().numpy()
        assert maps.shape == (2, 16, 16) and all(R.is_quadtree(m) for m in maps)
    else:
        maps = np.stack([C.maps(2)["mixed"]] * 2)
        tmaps = _cuda(maps[0])                                      # one map for every frame
    lv = hip.partition_leaves_host(maps, 2, 64, 64, 1)
    mm = Mismatch()
    all_traces = {}

    def price(pli, jobs):
        if pli == 0:
            return
        torch.cuda.synchronize()
        for s, job in jobs.items():
            x, r = job.coef.cpu().numpy(), job.ref.cpu().numpy()
            qm, qmi = qt.qm_slices(pli, s)
            traces, _ = oracle_traces(x, r, s, qm, qmi, qt.q_band(pli, s), qt.beta_band(pli, s), 1, pli, lam)
            all_traces[pli, s] = traces
            compare_bands(hip, job, traces, mm)
            job.rate = _cuda(host_rates(job, traces, 1, pli))

    pvq, ref, recon = hip.keyframe_partition_420(_cuda(luma_px), _cuda(cb_px), _cuda(cr_px), tmaps, qt, lam, W, H,
                                                 price=price)
    assert mm.total() == 0, mm.summary()
    # the reference planes are the oracle's chroma-from-luma of the luma planes the inverse takes
    luma_dq = pvq[0].dq.cpu().numpy()
    nref = ref.cpu().numpy()
    assert nref.shape == (2, 64, 64) and (luma_dq != 0).sum() > 1000
    for f in range(2):
        assert np.array_equal(nref[f], C.expected(luma_dq[f], maps[f], 1)), f
    assert np.array_equal(recon[0].cpu().numpy()[0], R.inverse(luma_dq[0], maps[0], 0, W, H, False))
    flips = {0: 0, 1: 0}
    for pli, px in ((1, cb_px), (2, cr_px)):
        ncoef = hip.forward_partition(_cuda(px), tmaps, 1, W, H).cpu().numpy()
        res = pvq[pli]
        assert np.array_equal(res.leaves.counts, lv.counts) and sorted(res.jobs) == lv.sizes()
        want = np.zeros_like(ncoef)
        for s, job in res.jobs.items():
            # what the oracle was given: the leaves of the source and of the planes under test
            assert np.array_equal(job.coef.cpu().numpy(), _np_gather(ncoef, lv, s))
            assert np.array_equal(job.ref.cpu().numpy(), _np_gather(nref, lv, s))
            traces = all_traces[pli, s]
            compare_choice(job, traces, mm)
            _np_scatter(want, job.dq.cpu().numpy(), lv, s)
            n = 4 << s
            hd = lv.dense_rows(s)
            nb = sum(1 for key in traces if key[0] == 0)
            for p in range(2):
                for i in range(int(lv.counts[s, p])):               # the leaves, not the dense set's padding
                    blk = (p * (hd // n) + i // (64 // n)) * (64 // n) + i % (64 // n)
                    flips[int(bool(traces[blk, 0]["flip"]))] += nb
        assert mm.total() == 0, mm.summary()
        assert np.array_equal(res.dq.cpu().numpy(), want)
        got_px = recon[pli].cpu().numpy()
        for f in range(2):
            assert np.array_equal(got_px[f], R.inverse(want[f], maps[f], 1, W, H, False)), (pli, f)
    print("chroma leaves %s, bands with / without the CfL flip %d / %d\n%s"
          % (lv.counts.sum(axis=1).tolist(), flips[1], flips[0], mm.summary()))
    assert mm.checked.get("item.y", 0) > 300 and mm.checked["dq"] > 300
    assert flips[1] >= 1 and flips[0] >= 1
