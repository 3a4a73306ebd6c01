"""GPU: the PVQ band stages on the leaves of a block-size map (daala_amd/csrc/partition_kernels.hip; include/daala_hip.h
"the PVQ band stages on the leaves of a block-size map") - leaf lists, gather, scatter and the two compositions
pvq_partition_noref / pvq_partition_ref.  Every comparison is exact.

  lists             k_part_rows / k_part_scan against odhip_partition_leaves_host, itself pinned to the encoder's walk
                    by tests/test_partition_leaves_host.py
  gather, scatter   k_part_copy against a numpy copy by the host lists: zero padding over a poisoned buffer, sizes
                    without a leaf, a single leaf, a plane without a leaf of a size another plane has, 192 samples wide
                    (w/N no power of two)
  compositions      every band of every leaf against odo_pvq_theta on that block's vector (tests/_band_oracle.py,
                    tests/_refbands.py), the scattered planes through inverse_partition against
                    tests/_partition_ref.py::inverse of the oracle's planes
  uniform maps      the composition equals the existing job on the whole plane, byte for byte
"""
import functools

import numpy as np
import pytest

import _partition_ref as R
from _band_oracle import band_trace, block_vector
from _libs import P, oracle, synth_frame
from _refbands import Mismatch, compare_bands, compare_choice, host_rates, oracle_traces

pytestmark = pytest.mark.gpu

NB = 5
POISON = 0x5a5a5a5a
# (name, dec, nsbx, planes per frame): luma 128x128 and 192x128, 4:2:0 chroma 64x64 with Cb and Cr of a frame adjacent
SHAPES = [("y128", 0, 2, 1), ("c64", 1, 2, 2), ("y192", 0, 3, 1)]
SHAPE_IDS = [s[0] for s in SHAPES]


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


# ---- CPU side: maps, host lists, numpy copies ------------------------------------------------------

@functools.lru_cache(maxsize=None)
def _maps(nsbx):
    """Frame maps of nsbx x 2 superblocks: all five sizes mixed, the deep corners, 4x4 against 64x64, one whole
    64x64 superblock among 32x32 ones (a single leaf of its size), all 64x64 / all 4x4 (a plane without a leaf of a
    size the other frame has)."""
    rng = np.random.RandomState(11 + nsbx)
    for _ in range(200):
        mixed = R.random_map(rng, nsbx, 2, 0.6)
        if R.leaf_sizes(mixed) == [0, 1, 2, 3, 4]:
            break
    assert R.leaf_sizes(mixed) == [0, 1, 2, 3, 4]
    single = R.uniform(3, nsbx, 2)
    single[8:16, 0:8] = 4
    lone = R.uniform(4, nsbx, 2)
    lone[0:8, 8:16] = R.deep_corner(2)
    maps = {"mixed": mixed, "corners": R.corners(nsbx, 2), "extremes": R.extremes(nsbx, 2), "single": single,
            "lone": lone, "all64": R.uniform(4, nsbx, 2), "all4": R.uniform(0, nsbx, 2)}
    for m in maps.values():
        assert R.is_quadtree(m)
        m.setflags(write=False)
    return maps


def _size(dec, nsbx):
    return 128 >> dec, (64 * nsbx) >> dec


def _host_leaves(hip, names, dec, nsbx, ppf):
    h, w = _size(dec, nsbx)
    maps = np.stack([_maps(nsbx)[n] for n in names])
    return hip.partition_leaves_host(maps, len(names) * ppf, h, w, dec, planes_per_frame=ppf), maps


def _np_gather(planes, lv, s):
    """The dense set of size s of int32 planes [nplanes][h][w] by the host lists lv."""
    nplanes, h, w = planes.shape
    n = 4 << s
    nbx = w // n
    out = np.zeros((nplanes, lv.dense_rows(s), w), np.int32)
    for p in range(nplanes):
        for i, idx in enumerate(lv.list(s)[p, :lv.counts[s, p]]):
            by, bx = divmod(int(idx), nbx)
            r, c = divmod(i, nbx)
            out[p, r * n:(r + 1) * n, c * n:(c + 1) * n] = planes[p, by * n:(by + 1) * n, bx * n:(bx + 1) * n]
    return out


def _np_scatter(dst, dense, lv, s):
    nplanes, h, w = dst.shape
    n = 4 << s
    nbx = w // n
    for p in range(nplanes):
        for i, idx in enumerate(lv.list(s)[p, :lv.counts[s, p]]):
            by, bx = divmod(int(idx), nbx)
            r, c = divmod(i, nbx)
            dst[p, by * n:(by + 1) * n, bx * n:(bx + 1) * n] = dense[p, r * n:(r + 1) * n, c * n:(c + 1) * n]


def _pictures(dec, nsbx, nframes, ppf, seed):
    """uint8 [nframes*ppf][h][w]: even frames noisy texture, odd frames flat areas cut by sharp edges."""
    h, w = _size(dec, nsbx)
    rng = np.random.RandomState(seed)
    out = []
    for f in range(nframes):
        for v in range(ppf):
            if f & 1:
                px = np.full((h, w), 60 + 20 * v, np.int32)
                px[:, w // 2 + 3:] = 200
                px[h // 4:h // 4 + 9, :] = 16
                px[-20:, :20] = 255
            else:
                base = synth_frame(w << dec, h << dec, seed=seed + f)[(1 + v) if dec else 0].astype(np.int32)
                px = base + rng.randint(-60, 61, size=base.shape)
            out.append(np.clip(px, 0, 255).astype(np.uint8))
    return np.stack(out)


# ---- 1: device lists and counts --------------------------------------------------------------------

@pytest.mark.parametrize("shape", SHAPES, ids=SHAPE_IDS)
def test_device_lists_equal_the_host_lists(hip, shape):
    _, dec, nsbx, ppf = shape
    names = list(_maps(nsbx))
    if ppf == 1:
        names = names[:4] if nsbx == 2 else names       # 4 planes of 128x128, 7 of 192x128
    want, maps = _host_leaves(hip, names, dec, nsbx, ppf)
    h, w = _size(dec, nsbx)
    got = hip.partition_leaves(_cuda(maps), len(names) * ppf, h, w, dec, planes_per_frame=ppf)
    assert np.array_equal(got.counts, want.counts)
    assert np.array_equal(got.lists.cpu().numpy().view(np.uint32), want.lists)
    # one map for every plane
    one = hip.partition_leaves(_cuda(maps[0]), 2, h, w, dec)
    assert np.array_equal(one.counts[:, 0], want.counts[:, 0]) and np.array_equal(one.counts[:, 1], want.counts[:, 0])


# ---- 2, 3: gather and scatter ----------------------------------------------------------------------

@pytest.mark.parametrize("names", [("mixed", "lone"), ("all64", "all4"), ("single", "corners", "extremes", "mixed")],
                         ids=lambda n: "+".join(n))
@pytest.mark.parametrize("shape", SHAPES, ids=SHAPE_IDS)
def test_gather_and_scatter_equal_numpy_copies(hip, shape, names):
    import torch
    _, dec, nsbx, ppf = shape
    h, w = _size(dec, nsbx)
    lv, maps = _host_leaves(hip, names, dec, nsbx, ppf)
    nplanes = len(names) * ppf
    dl = hip.partition_leaves(_cuda(maps), nplanes, h, w, dec, planes_per_frame=ppf)
    rng = np.random.RandomState(5)
    src = rng.randint(-(1 << 30), 1 << 30, size=(nplanes, h, w)).astype(np.int32)
    tsrc = _cuda(src)
    back = torch.full((nplanes, h, w), POISON, dtype=torch.int32, device="cuda")
    for s in range(NB - dec):
        hd = lv.dense_rows(s)
        assert dl.dense_rows(s) == hd
        want = _np_gather(src, lv, s)
        out = torch.full((nplanes, hd, w), POISON, dtype=torch.int32, device="cuda")
        got = hip.partition_gather(tsrc, dl, s, out=out)
        assert got is out and np.array_equal(got.cpu().numpy(), want), s      # the zero padding is written
        if hd == 0:
            assert not lv.counts[s].any()
        hip.partition_scatter(back, got, dl, s)
    # the leaves tile the planes: the scatter of every size gives the source back, over the poison
    assert np.array_equal(back.cpu().numpy(), src)
    assert np.array_equal(tsrc.cpu().numpy(), src)
    if names == ("all64", "all4") and dec == 0:
        assert list(lv.counts[4]) == [2 * nsbx, 0] and list(lv.counts[0]) == [0, 32 * 16 * nsbx]
    if names[0] == "single":
        assert lv.counts[4 - dec, 0] == 1 and lv.dense_rows(4 - dec) == 64 >> dec


def test_scatter_writes_the_leaves_only(hip):
    import torch
    lv, maps = _host_leaves(hip, ("mixed",), 0, 2, 1)
    dl = hip.partition_leaves(_cuda(maps), 1, 128, 128, 0)
    rng = np.random.RandomState(6)
    for s in range(NB):
        dense = rng.randint(-1000, 1000, size=(1, lv.dense_rows(s), 128)).astype(np.int32)
        dst = torch.full((1, 128, 128), POISON, dtype=torch.int32, device="cuda")
        hip.partition_scatter(dst, _cuda(dense), dl, s)
        want = np.full((1, 128, 128), POISON, np.int32)
        _np_scatter(want, dense, lv, s)
        assert np.array_equal(dst.cpu().numpy(), want), s


# ---- 4: the no-reference composition ---------------------------------------------------------------

def _check_noref_job(hip, job, dense, counts, qt, pli, lam):
    """Records, pulses, choice and dequantised blocks of one dense job against odo_pvq_theta on every listed leaf;
    returns the oracle's dequantised dense set."""
    o = oracle()
    s = job.bs
    n = 4 << s
    nplanes, hd, w = dense.shape
    qm, qmi = qt.qm_slices(pli, s)
    qb, bb = qt.q_band(pli, s), qt.beta_band(pli, s)
    nb, offs, ln = hip.pvq_band_layout(s)
    c = hip.unpack_cands(job.cands)
    qg = c["choice"][..., 1]
    want = np.zeros_like(dense)
    nsearched = 0
    for p in range(nplanes):
        for i in range(int(counts[p])):
            by, bx = divmod(i, w // n)
            blk = (p * (hd // n) + by) * (w // n) + bx
            vec = block_vector(dense[p], n, bx, by)
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
                        assert c["dist"][blk, band, slot] == cnd.dist
                        yy = np.array(cnd.y[:m], np.int32)
                        assert np.array_equal(c["y"][slot, blk, a:b], yy)
                        if cnd.dist <= best_cost:
                            best_cost, best_qg, best_y = cnd.dist, cnd.gain, yy
                assert qg[blk, band] == best_qg
                if best_qg:
                    gexp = o.odo_gain_expand(best_qg << 8, qb[band], bb[band])
                    syn = np.zeros(m, np.int32)
                    o.odo_pvq_synthesis_partial(P(syn), P(best_y), None, m, 1, gexp, 0, 0, 1, P(qi))
                    outvec[a:b] = syn
            blkout = np.zeros((n, n), np.int32)
            o.odo_coding_order_to_raster(P(blkout), n, P(outvec), n)
            want[p, by * n:(by + 1) * n, bx * n:(bx + 1) * n] = blkout
    assert np.array_equal(job.dq.cpu().numpy(), want), s      # the padding blocks dequantise to zero
    return want, nsearched


@pytest.mark.parametrize("dec,quality", [(0, 10), (0, 40), (1, 20)], ids=["y128-v10", "y128-v40", "c64-v20"])
def test_noref_composition_matches_the_oracle_leaf_by_leaf(hip, dec, quality):
    ppf = 1 + dec
    pli = dec
    h, w = _size(dec, 2)
    W, H = 128, 128
    names = ("mixed", "corners")
    lv, maps = _host_leaves(hip, names, dec, 2, ppf)
    px = _pictures(dec, 2, 2, ppf, seed=70 + dec)
    qt = hip.QuantTables.for_quality(quality)
    lam = hip.OD_PVQ_LAMBDA
    tmaps = _cuda(maps)
    coef = hip.forward_partition(_cuda(px), tmaps, dec, W, H, planes_per_frame=ppf)
    res = hip.pvq_partition_noref(coef, tmaps, dec, qt.size_tables(pli, dec), lam, planes_per_frame=ppf)
    assert np.array_equal(res.leaves.counts, lv.counts) and sorted(res.jobs) == lv.sizes()
    ncoef = coef.cpu().numpy()
    want = np.zeros_like(ncoef)
    nsearched = 0
    for s, job in res.jobs.items():
        dense = _np_gather(ncoef, lv, s)
        assert np.array_equal(job.coef.cpu().numpy(), dense)
        want_dense, k = _check_noref_job(hip, job, dense, lv.counts[s], qt, pli, lam)
        nsearched += k
        _np_scatter(want, want_dense, lv, s)
    print("leaves %s, candidates searched and compared %d" % (lv.counts.sum(axis=1).tolist(), nsearched))
    assert nsearched > 100
    assert np.array_equal(res.dq.cpu().numpy(), want)
    got_px = hip.inverse_partition(res.dq, tmaps, dec, W, H, planes_per_frame=ppf).cpu().numpy()
    for p in range(len(names) * ppf):
        assert np.array_equal(got_px[p], R.inverse(want[p], maps[p // ppf], dec, W, H, False)), p


# ---- 5: the with-reference composition -------------------------------------------------------------

def test_ref_composition_matches_the_oracle_leaf_by_leaf(hip):
    """Inter luma: the reference is the transform, at the same maps, of the picture shifted by (3, 2).  The host prices
    every searched candidate between the band stage and the choice, as in tests/test_gpu_pvq_refbands.py; bands inside
    the device-acos margin are settled by the resolve call of the composition."""
    dec, pli, is_keyframe = 0, 0, 0
    W = H = 128
    names = ("mixed", "corners")
    lv, maps = _host_leaves(hip, names, dec, 2, 1)
    px = _pictures(dec, 2, 2, 1, seed=90)
    shifted = np.roll(px, (2, 3), axis=(1, 2))
    qt = hip.QuantTables.load()
    lam = hip.OD_PVQ_LAMBDA
    tmaps = _cuda(maps)
    coef = hip.forward_partition(_cuda(px), tmaps, dec, W, H)
    ref = hip.forward_partition(_cuda(shifted), tmaps, dec, W, H)
    ncoef, nref = coef.cpu().numpy(), ref.cpu().numpy()
    mm = Mismatch()
    all_traces = {}

    def price(jobs):
        import torch
        torch.cuda.synchronize()
        for s, job in jobs.items():
            x, r = _np_gather(ncoef, lv, s), _np_gather(nref, lv, s)
            assert np.array_equal(job.coef.cpu().numpy(), x) and np.array_equal(job.ref.cpu().numpy(), r)
            qm, qmi = qt.qm_slices(pli, s)
            traces, _ = oracle_traces(x, r, s, qm, qmi, qt.q_band(pli, s), qt.beta_band(pli, s), is_keyframe, pli, lam)
            all_traces[s] = traces
            compare_bands(hip, job, traces, mm)
            job.rate = _cuda(host_rates(job, traces, is_keyframe, pli))

    res = hip.pvq_partition_ref(coef, ref, tmaps, dec, qt.size_tables(pli, dec), lam, is_keyframe, pli, price=price)
    assert mm.total() == 0, mm.summary()
    assert mm.checked.get("item.y", 0) > 300 and sorted(res.jobs) == lv.sizes() == [0, 1, 2, 3, 4]
    want = np.zeros_like(ncoef)
    for s, job in res.jobs.items():
        compare_choice(job, all_traces[s], mm)
        _np_scatter(want, job.dq.cpu().numpy(), lv, s)
    print("leaves %s, reruns %d\n%s" % (lv.counts.sum(axis=1).tolist(), res.reruns, mm.summary()))
    assert mm.total() == 0, mm.summary()
    assert mm.checked["dq"] > 300
    assert np.array_equal(res.dq.cpu().numpy(), want)


# ---- 6: a uniform map is the existing job on the whole plane ---------------------------------------

@pytest.mark.parametrize("dec", [0, 1])
def test_uniform_maps_equal_the_uniform_jobs(hip, dec):
    import torch
    ppf = 1 + dec
    pli = dec
    h, w = _size(dec, 2)
    px = _cuda(_pictures(dec, 2, 2, ppf, seed=50 + dec))
    shifted = torch.roll(px, (1, 2), dims=(1, 2))
    qt = hip.QuantTables.load()
    lam = hip.OD_PVQ_LAMBDA
    tables = qt.size_tables(pli, dec)
    split = {}
    if dec:
        # planes keep their identity in the dense sets: the last two of the four take the Cr steps
        tables = [t + (qt.q_band(2, s),) for s, t in enumerate(tables)]
        split = {"plane_split": 2}
        assert any(t[4] != t[2] for t in tables)
    for s in range(NB - dec):
        bmap = _cuda(R.uniform(s + dec, 2, 2))
        coef = hip.forward_partition(px, bmap, dec, 128, 128)
        ref = hip.forward_partition(shifted, bmap, dec, 128, 128)
        qm, qmi, qb, bb = tables[s][:4]
        qb2 = {"q_band2": tables[s][4], **split} if dec else {}
        # no reference
        job = hip.PvqJob(coef, s, qm, qmi, qb, bb, dq=torch.empty_like(coef), **qb2)
        hip.pvq_noref_bands_multi([job], lam)
        hip.pvq_select_synth_noref_multi([job], lam)
        res = hip.pvq_partition_noref(coef, bmap, dec, tables, lam, **split)
        assert list(res.jobs) == [s] and torch.equal(res.jobs[s].coef, coef)
        assert torch.equal(res.dq, job.dq), s
        for key in ("band", "y", "choice"):
            assert torch.equal(res.jobs[s].cands[key], job.cands[key]), (s, key)
        # with a reference
        rjob = hip.PvqRefJob(coef, ref, s, qm, qmi, qb, bb, 0, pli, **qb2)
        hip.pvq_ref_bands_multi([rjob], lam)
        hip.pvq_ref_select_synth_multi([rjob], lam)
        rres = hip.pvq_partition_ref(coef, ref, bmap, dec, tables, lam, 0, pli, **split)
        assert list(rres.jobs) == [s] and torch.equal(rres.jobs[s].ref, ref)
        assert torch.equal(rres.dq, rjob.dq), s
        for key in ("band", "y", "choice"):
            assert torch.equal(getattr(rres.jobs[s], key), getattr(rjob, key)), (s, key)
