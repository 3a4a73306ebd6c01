"""GPU: motion compensation from motion-vector grids (mc_kernels.hip) against the reference's recorded
od_state_mc_predict outputs (tests/golden/mc.npz) and, beyond them, against tests/_mc_ref.py.  All exact."""
import os

import numpy as np
import pytest

import _mc_ref as R
from _libs import GOLDEN

pytestmark = pytest.mark.gpu

CASES = R.load_cases(os.path.join(GOLDEN, "mc.npz"))
IDS = [c["name"] for c in CASES]


@pytest.fixture(scope="module")
def D():
    import torch
    import daala_amd
    assert torch.cuda.is_available()
    daala_amd.init(0)
    return daala_amd


def plane_sets(case):
    """(dec, [slot] -> [nplanes][h][w]) for luma and for chroma (Cb, then Cr) and the recorded predictions."""
    dec = 0 if case["c444"] else 1
    luma = (0, [case["refs"][s][0][None] for s in range(2)], case["pred"][0][None])
    chroma = (dec, [np.stack([case["refs"][s][1], case["refs"][s][2]]) for s in range(2)],
              np.stack([case["pred"][1], case["pred"][2]]))
    return luma, chroma


@pytest.mark.parametrize("case", CASES, ids=IDS)
def test_leaves_equal_the_fixture_walk(D, case):
    got = D.mc_leaves(case["grid"], case["w"], case["h"])[0]
    want = np.array(sorted(R.leaf_desc(*leaf) for leaf in R.leaves(case["grid"]["valid"])), np.uint32)
    assert np.array_equal(got, want)


@pytest.mark.parametrize("case", CASES, ids=IDS)
def test_prediction_equals_the_reference(D, case):
    import torch
    for dec, refs, want in plane_sets(case):
        got = D.mc_predict([torch.from_numpy(r).cuda() for r in refs], case["grid"], dec=dec)
        torch.cuda.synchronize()
        assert np.array_equal(got.cpu().numpy(), want), (case["name"], dec)


def random_planes(rng, n, h, w, fpr):
    # smooth content with hard edges and full-range samples: the clamps of both filter passes are reached
    p = rng.randint(0, 4096 if fpr else 256, size=(n, h, w))
    p[:, ::7, :] = 0
    p[:, :, 5::11] = 4095 if fpr else 255
    return p.astype(np.int16 if fpr else np.uint8)


@pytest.mark.parametrize("fpr", [0, 1])
@pytest.mark.parametrize("dec", [0, 1])
def test_three_pictures_three_slots_random_vectors(D, fpr, dec):
    import torch
    rng = np.random.RandomState(40 + 2*fpr + dec)
    pats = [c["grid"]["valid"] for c in CASES if (c["w"], c["h"]) == (192, 128)][:3]
    assert len(pats) == 3
    grids = np.stack([R.random_grid(v, rng, (dec,), nrefs=3) for v in pats])
    h, w = 128 >> dec, 192 >> dec
    nplanes = 6 if dec else 3              # chroma sets: all Cb planes, then all Cr
    refs = [random_planes(rng, nplanes, h, w, fpr) for _ in range(3)]
    got = D.mc_predict([torch.from_numpy(r).cuda() for r in refs], grids, dec=dec).cpu().numpy()
    for p in range(nplanes):
        want = R.mc_predict_plane([r[p] for r in refs], grids[p % 3], dec, fpr)
        assert np.array_equal(got[p], want), p


def test_device_grid_equals_host_grid(D):
    import torch
    c = CASES[0]
    refs = [torch.from_numpy(c["refs"][s][0][None]).cuda() for s in range(2)]
    dgrid = torch.from_numpy(np.frombuffer(c["grid"].tobytes(), np.uint8).copy()).cuda()
    got = D.mc_predict(refs, dgrid, dec=0).cpu().numpy()
    assert np.array_equal(got[0], c["pred"][0])


def wrapping_launches(valid, dec):
    """{(lanes across a tile, lg)} of the launches of one picture whose work is more than their blocks take in one
    pass, by launch_predict's arithmetic (mc_kernels.hip): at most 4096 blocks in x, each of 256 / tile^2 tiles per
    pass, for count << 2*ltiles tiles of work - k_mc_predict's grid-stride loop then comes round again."""
    nv, nh = valid.shape[0] - 1, valid.shape[1] - 1
    count = [0]*4
    for leaf in R.leaves(valid):
        count[leaf[2]] += 1
    out = set()
    for lg in range(4):
        lb = lg + 3 - dec
        ts = 16 if lb >= 4 else 8 if lb == 3 else 4
        groups = 256//(ts*ts)
        most = nh*nv >> 2*lg
        units = most << 2*(lb - 4) if lb >= 4 else (most + groups - 1)//groups
        nwork = count[lg] << 2*max(lb - 4, 0)
        if min(units, 4096)*groups < nwork:
            out.add((ts, lg))
    return out


def test_1080p(D):
    import torch
    import _mc_patterns as MP
    rng = np.random.RandomState(77)
    nh, nv = 1920 // 8, 1088 // 8
    src = CASES[0]["grid"]["valid"][:-1, :-1]          # 16 x 24 cells: whole 64x64 cells, tiled
    valid = np.zeros((nv + 1, nh + 1), np.uint8)
    valid[:nv, :nh] = np.tile(src, (nv // src.shape[0] + 1, nh // src.shape[1] + 1))[:nv, :nh]
    valid[nv, :], valid[:, nh] = valid[0, :], valid[:, 0]
    # A launch wraps when its leaves cover more than half of the frame (4096 blocks take 16384 8x8 cells of any one
    # size at dec = 0, and more at dec = 1, where nothing wraps at this size), so no one pattern makes two launches
    # wrap.  The tiled pattern is mostly 8x8 leaves: its 8-lane-tile launch wraps.  A second picture has 64x64
    # leaves in its left 17 columns of cells and 32x32 leaves in the rest: a 16-lane-tile launch wraps.  The
    # 4-lane-tile template (dec = 1, 8x8 leaves) takes 16 leaves per block: it would wrap beyond 65536 leaves, twice
    # what this size holds.
    large = MP.build(1920, 1088, lambda lg, x, y: lg == 3 and x >= 17*8, lambda lg, x, y: lg == 3)
    wraps = wrapping_launches(valid, 0) | wrapping_launches(large, 0)
    assert (8, 0) in wrapping_launches(valid, 0) and (16, 3) in wrapping_launches(large, 0), wraps
    assert {ts for ts, _ in wraps} == {8, 16}
    assert not wrapping_launches(valid, 1) and not wrapping_launches(large, 1)
    grids = np.stack([R.random_grid(valid, rng, (0, 1), nrefs=2, reach=40),
                      R.random_grid(large, rng, (0, 1), nrefs=2, reach=40)])
    for dec, fpr in ((0, 0), (1, 1)):
        h, w = 1088 >> dec, 1920 >> dec
        refs = [random_planes(rng, 2, h, w, fpr) for _ in range(2)]
        got = D.mc_predict([torch.from_numpy(r).cuda() for r in refs], grids, dec=dec).cpu().numpy()
        for p in range(2):
            want = R.mc_predict_plane([r[p] for r in refs], grids[p], dec, fpr)
            assert np.array_equal(got[p], want), (dec, fpr, p)


def test_one_context_small_large_small(D):
    """The per-context scratch of the motion compensation (grid copy, leaf buckets, counters) and of SSIM (tile
    partials) in one fresh context: a 64x64 input, a 192x128 input, the 64x64 input again.  The scratch grows for the
    second and is kept for the third: the first and the third results are equal, and all are the references'."""
    import math
    import torch
    import _ssim_ref as S
    from test_gpu_ssim import _dev, _odd, _planes, _planes_call
    rng = np.random.RandomState(91)
    big = next(c for c in CASES if (c["w"], c["h"]) == (192, 128) and not c["fpr"])
    valid = np.zeros((9, 9), np.uint8)                 # one 64x64 cell of a recorded pattern
    valid[:8, :8] = big["grid"]["valid"][:8, :8]
    valid[8, :], valid[:, 8] = valid[0, :], valid[:, 0]
    grid = R.random_grid(valid, rng, (0,), nrefs=2, reach=40)
    refs = [random_planes(rng, 1, 64, 64, 0) for _ in range(2)]
    _, big_refs, big_want = plane_sets(big)[0]
    pairs = []
    for i, (w, h) in enumerate(((64, 64), (192, 128))):
        src, rec, ssrc, srec = _planes(60 + i, w, h, 8, "u8")
        pairs.append(((_dev(ssrc, _odd(w, 1)), _dev(srec, _odd(w, 3)), w, h, 8, D.SAMPLE_U8), S.terms(src, rec, 8)))
    mc, ssim = [], []
    ctx = D.Context(0)
    try:
        with ctx:
            for r, g, (item, _) in ((refs, grid, pairs[0]), (big_refs, big["grid"], pairs[1]), (refs, grid, pairs[0])):
                mc.append(D.mc_predict([torch.from_numpy(p).cuda() for p in r], g, dec=0).cpu().numpy())
                rc, out, _ = _planes_call(D, [item])
                assert rc == 0
                ssim.append(out)
    finally:
        ctx.destroy()
    assert np.array_equal(mc[0][0], R.mc_predict_plane([r[0] for r in refs], grid, 0, 0))
    assert np.array_equal(mc[1], big_want)
    assert np.array_equal(mc[2], mc[0])
    for got, (_, t) in ((ssim[0], pairs[0]), (ssim[1], pairs[1])):
        exact = math.fsum(t.ravel().tolist())
        assert abs(got[0] - exact) <= t.size * 2.0 ** -53 * math.fsum(np.abs(t).ravel().tolist())
    assert ssim[2].view(np.int64)[0] == ssim[0].view(np.int64)[0]


def test_vector_out_of_range_is_refused_and_nothing_written(D):
    import torch
    c = CASES[0]
    g = c["grid"].copy()
    g["mvx"][0, 0] = -66*8
    assert not R.grid_in_range(g, 0)
    refs = [torch.from_numpy(c["refs"][s][0][None]).cuda() for s in range(2)]
    out = torch.full_like(refs[0], 123)
    with pytest.raises(D.MotionRangeError):
        D.mc_predict(refs, g, dec=0, out=out)
    torch.cuda.synchronize()
    assert bool((out == 123).all())
