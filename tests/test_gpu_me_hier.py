"""GPU: the coarse-to-fine motion search (me_kernels.hip: odhip_me_downsample / odhip_me_costs3 / odhip_me_search3,
and the pipe's odhip_pipe_set_motion_search3) against the numpy yardstick tests/_me_hier_ref.py.  Every comparison is
exact integer equality.

Unless said otherwise the shapes are those of test_gpu_me.py: coded 128 x 64, pictures 120 x 56 and 119 x 55, two
pictures, two reference slots, 4:2:0."""
import ctypes

import numpy as np
import pytest

import _mc_ref as R
import _me_cost_ref as C
import _me_hier_ref as HR
import test_gpu_pipe_mc as PM
from test_gpu_me import content, cuda, same_search, check_shape
from test_gpu_me_cost import planes, dev, PICS
from test_gpu_pipe_me_cost import crop, frames, SIZES

pytestmark = pytest.mark.gpu

W, H, F = 128, 64, 2
EINVAL, EIMPL = -10, -23


@pytest.fixture(scope="module")
def D():
    import torch
    import daala_amd
    assert torch.cuda.is_available()
    daala_amd.init(0)
    return daala_amd


# ---- 1. the halving ----
@pytest.mark.parametrize("w,h", [(121, 57), (64, 64)])
def test_downsample_equals_halve(D, w, h):
    import torch
    rng = np.random.RandomState(w)
    p = rng.randint(0, 256, size=(3, h, w)).astype(np.uint8)
    want = np.stack([HR.halve(x) for x in p])
    assert np.array_equal(D.me_downsample(cuda(p)[0]).cpu().numpy(), want)
    # an odd stride, an odd base and a padded plane stride, on both sides
    sw = w + 2 + (w & 1 ^ 1)
    big = torch.full((3, h + 3, sw), 7, dtype=torch.uint8, device="cuda")
    big[:, 1:1 + h, 1:1 + w] = cuda(p)[0]
    src = big[:, 1:1 + h, 1:1 + w]
    oh, ow = want.shape[1:]
    dw = ow + 1 + (ow & 1)
    out = torch.full((3, oh + 2, dw), 0x5a, dtype=torch.uint8, device="cuda")
    dst = out[:, 1:1 + oh, 1:1 + ow]
    assert src.stride(1) % 2 == 1 and dst.stride(1) % 2 == 1 and src.stride(0) > h*src.stride(1)
    rc = D.lib().odhip_me_downsample(ctypes.c_void_p(dst.data_ptr()), dst.stride(1), ctypes.c_int64(dst.stride(0)),
                                     ctypes.c_void_p(src.data_ptr()), src.stride(1), ctypes.c_int64(src.stride(0)),
                                     w, h, 3, None)
    assert rc == 0
    torch.cuda.synchronize()
    got = out.cpu().numpy()
    assert np.array_equal(got[:, 1:1 + oh, 1:1 + ow], want)
    got[:, 1:1 + oh, 1:1 + ow] = 0x5a
    assert np.all(got == 0x5a)             # nothing beside the planes is written


# ---- 2. the levels' costs ----
def level_cands(D, lg, level):
    """Every point of the frame's four edges (the clipped and the empty blocks are among them), then random points;
    vectors that are multiples of the level's step, up to the search's reach of 1223 eighth-pels."""
    rng = np.random.RandomState(50 + lg + 4*level)
    s, step = 1 << lg, 8 << level
    xs, ys = list(range(0, W//8 + 1, s)), list(range(0, H//8 + 1, s))
    pts = [(x, y) for x in xs for y in (ys[0], ys[-1])] + [(x, y) for y in ys for x in (xs[0], xs[-1])]
    pts += [(xs[rng.randint(len(xs))], ys[rng.randint(len(ys))]) for _ in range(32)]
    top = 1223//step
    c = np.zeros(len(pts), D.ME_CAND)
    for i, (vx, vy) in enumerate(pts):
        far = top if i % 3 == 0 else 6
        c[i] = (rng.randint(F), vx, vy, rng.randint(2), step*rng.randint(-far, far + 1), step*rng.randint(-far, far + 1))
    c["mvx"][0], c["mvy"][1] = step*top, -step*top
    return c


@pytest.mark.parametrize("lg", [0, 1, 2, 3])
def test_level_costs_equal_the_yardstick(D, lg):
    levels = min(2, lg + 1)
    pic = lg & 1
    pw, ph = PICS[pic]
    src, _, refs, _ = planes(1, pic)
    d_src, _, d_refs, _ = dev(1, pic)
    spyr = [HR.pyramid(s, 2) for s in src]
    rpyr = [[HR.pyramid(p, 2) for p in r] for r in refs]
    for level in range(levels + 1):
        c = level_cands(D, lg, level)
        want = [C.plane_dist(spyr[k["pic"]][level], pw, ph, rpyr[k["slot"]][k["pic"]][level], int(k["vx"]), int(k["vy"]),
                             lg, int(k["mvx"]), int(k["mvy"]), level, C.SAD_METRIC) for k in c]
        got = D.me_costs3(d_src, d_refs, pw, ph, lg, c, level, levels)
        assert got.dtype == np.uint32 and got.tolist() == want, level
        # the blocks of the right-hand points are empty at the two smallest sizes
        assert (0 in want or lg >= 2) and max(want) > 0
        if level == 0:
            assert np.array_equal(got, D.me_costs(d_src, d_refs, pw, ph, lg, c))
            assert np.array_equal(got, D.me_costs3(d_src, d_refs, pw, ph, lg, c, 0, 0))
        # a candidate that names nothing, or whose vector is no multiple of the level's step, is flagged
        bad = c[:5].copy()
        bad["pic"][0], bad["slot"][1], bad["vx"][2] = F, 2, W//8 + 1
        bad["mvx"][3] += 4 << level
        bad["mvy"][4] -= 1
        assert D.me_costs3(d_src, d_refs, pw, ph, lg, bad, level, levels).tolist() == [0xffffffff]*5


# ---- 3. the search ----
LEVELS = [(lg, lv) for lg in range(4) for lv in range(min(2, lg + 1) + 1)]


@pytest.mark.parametrize("lg,levels", LEVELS)
def test_search_equals_the_yardstick(D, lg, levels):
    # four of the 32 combinations per size and number of levels, every value of every parameter among them, rotated
    # so that the sizes see different ones
    for k in range(4):
        i = (k + lg + levels) & 1
        rng_, refine, res = (0, 3)[i], (1, 2)[k >> 1], (3, 0)[(k ^ k >> 1 ^ lg) & 1]
        flags = (0, D.ME_CHROMA | D.ME_SATD)[(k >> 1 ^ levels) & 1]
        lam, lam2 = ((0, 0), (5, 3))[(i + (k >> 1) + (lg >> 1)) & 1]
        pic = (lg + k) & 1
        pw, ph = PICS[pic]
        src, csrc, refs, crefs = planes(1, pic)
        d_src, d_csrc, d_refs, d_crefs = dev(1, pic)
        got = D.me_search3(d_src, d_refs, pw, ph, lg, rng_, res, lam, lam2, flags, d_csrc, d_crefs, 1, levels, refine)
        want = HR.search(src, csrc, pw, ph, refs, crefs, lg, rng_, res, lam, lam2, flags, 1, levels, refine)
        same_search(got, want, (rng_, refine, res, lam, lam2, flags, pic))
        check_shape(D, got[0], got[1], lg, W, H)
        if not levels:
            two = D.me_search2(d_src, d_refs, pw, ph, lg, rng_, res, lam, lam2, flags, d_csrc, d_crefs, 1)
            assert got[0].tobytes() == two[0].tobytes() and got[1].tobytes() == two[1].tobytes()


@pytest.mark.parametrize("flags", [1, 3], ids=["chroma", "both"])
def test_444_chroma_slides_round_the_centres(D, flags):
    pw, ph = PICS[1]
    src, csrc, refs, crefs = planes(0, 1)
    d_src, d_csrc, d_refs, d_crefs = dev(0, 1)
    got = D.me_search3(d_src, d_refs, pw, ph, 1, 3, 1, 5, 3, flags, d_csrc, d_crefs, 0, 2, 2)
    want = HR.search(src, csrc, pw, ph, refs, crefs, 1, 3, 1, 5, 3, flags, 0, 2, 2)
    same_search(got, want, "444")
    assert np.abs(got[0]["mvx"]).max() > 8*3


def test_the_planted_displacement_is_found(D):
    src, refs, mv, pts = HR.planted()
    got = D.me_search3(cuda(src)[0], cuda(*refs), 250, 180, 2, 20, 3, 3, 3, 0, None, None, 0, 2, 2)
    want = HR.search(src, None, 250, 180, refs, None, 2, 20, 3, 3, 3, 0, 0, 2, 2)
    same_search(got, want, "planted")
    assert len(pts) == 20
    for vx, vy in pts:
        pt = got[0][0, vy, vx]
        assert (int(pt["mvx"]), int(pt["mvy"]), int(pt["ref"])) == (mv[0], mv[1], 1), (vx, vy)
    # ... out of the exhaustive search's reach
    wide = D.me_search(cuda(src)[0], cuda(*refs), 250, 180, 2, 32, 3, 3)
    assert not np.any((wide[0]["mvx"] == mv[0]) & (wide[0]["mvy"] == mv[1]))


@pytest.mark.parametrize("lg", [1, 3])
def test_the_longest_search_stays_legal(D, lg):
    from _me_ref import smooth_noise
    rng = np.random.RandomState(3)
    big = smooth_noise(rng, 128 + 300, 128 + 300)
    src = np.ascontiguousarray(big[150:278, 150:278])[None]
    # the scene moved by more than the frame leaves room for: the best matches lie outside it
    refs = [np.ascontiguousarray(big[150 - 120:278 - 120, 150 + 90:278 + 90])[None],
            np.ascontiguousarray(big[150 + 101:278 + 101, 150 - 131:278 - 131])[None]]
    got = D.me_search3(cuda(src)[0], cuda(*refs), 128, 128, lg, 32, 0, 1, 1, 0, None, None, 0, 2, 2)
    want = HR.search(src, None, 128, 128, refs, None, lg, 32, 0, 1, 1, 0, 0, 2, 2)
    same_search(got, want, "range 32, two levels")
    check_shape(D, got[0], got[1], lg, 128, 128)
    assert max(np.abs(got[0]["mvx"]).max(), np.abs(got[0]["mvy"]).max()) > 8*32
    for dec in (0, 1):
        assert D.mc_check_grid(got[0], 128, 128, dec=dec, nrefs=2) == 0
        assert R.grid_in_range(got[0][0], dec)


def test_flat_content_gives_zero_vectors_in_slot_zero(D):
    pw, ph = PICS[0]
    src = np.full((F, ph, pw), 100, np.uint8)
    refs = [np.full((F, H, W), 90, np.uint8)]*2
    for lg in range(4):
        for levels in range(1, min(2, lg + 1) + 1):
            grid, cost = D.me_search3(cuda(src)[0], cuda(*refs), pw, ph, lg, 7, 0, 0, 0, 0, None, None, 1, levels, 2)
            assert not grid["mvx"].any() and not grid["mvy"].any() and not grid["ref"].any(), (lg, levels)


def test_refused_jobs_launch_nothing(D):
    import torch
    d_src, d_csrc, d_refs, d_crefs = dev(1)
    pw, ph = PICS[0]
    L = D.lib()
    shape = (F, H//8 + 1, W//8 + 1)
    grid = torch.full(shape + (D.MV_POINT.itemsize,), 0xab, dtype=torch.uint8, device="cuda")
    cost = torch.full(shape, 0x5a5a5a5a, dtype=torch.int32, device="cuda")
    cands = torch.zeros(D.ME_CAND.itemsize, dtype=torch.uint8, device="cuda")
    out = torch.full((1,), 0x5a5a5a5a, dtype=torch.int32, device="cuda")
    keep = []

    def job(**kw):
        j, scratch = D.api._me_job3(d_src, d_refs, pw, ph, 1, 3, 0, 5, 3, 3, d_csrc, d_crefs, 1, 2, 2)
        keep.append(scratch)
        j.base.luma.grid, j.base.luma.cost = grid.data_ptr(), cost.data_ptr()
        for k, v in kw.items():
            setattr(j.base.luma if k in ("range", "lambda_", "log_size") else j, k, v)
        return j

    def search(j):
        return L.odhip_me_search3(ctypes.byref(j), None)

    def costs(j, level=1):
        return L.odhip_me_costs3(ctypes.byref(j), ctypes.c_void_p(cands.data_ptr()), ctypes.c_long(1), level,
                                 ctypes.c_void_p(out.data_ptr()), None)

    for kw in (dict(levels=3), dict(levels=-1), dict(levels=2, log_size=0), dict(scratch=None),
               dict(scratch_bytes=job().scratch_bytes - 1)):
        assert search(job(**kw)) == EINVAL, kw
        assert costs(job(**kw)) == EINVAL, kw
    for kw in (dict(refine=0), dict(refine=9), dict(lambda_=(1 << 19) + 1), dict(range=33), dict(range=-1)):
        assert search(job(**kw)) == EINVAL, kw
    j = job()
    j.base.lambda_subpel = (1 << 19) + 1
    assert search(j) == EINVAL and costs(job(), level=3) == EINVAL
    with D.Context(0) as ctx:
        ctx.set_fpr(True)
        assert search(job()) == EIMPL and costs(job()) == EIMPL
    torch.cuda.synchronize()
    assert bool((grid == 0xab).all()) and bool((cost == 0x5a5a5a5a).all()) and int(out[0]) == 0x5a5a5a5a
    # ... and the same job, unchanged, runs
    assert search(job()) == 0 and costs(job()) == 0
    torch.cuda.synchronize()
    assert not bool((grid == 0xab).all()) and int(out[0]) != 0x5a5a5a5a


# ---- 4. in the pipe ----
def alone(D, pics, luma, chroma, cdec, par):
    lg, rng_, res, lam, lam2, flags, levels, refine = par
    pw, ph = SIZES[cdec]
    return D.me_search3(cuda(pics[0])[0], cuda(*luma), pw, ph, lg, rng_, res, lam, lam2, flags, cuda(pics[1])[0],
                        cuda(*chroma), cdec, levels, refine)


def test_pipe_search_equals_the_stand_alone_search_and_a_pipe_given_its_grid(D):
    import torch
    cdec = 1
    PW, PH = SIZES[cdec]
    pics = crop(content()[0], cdec, 7)
    luma, chroma = frames(cdec)
    qt = D.QuantTables.load()
    kw = dict(chroma_cfl=True, price=True, inter=True)
    a = D.Pipe(qt, F, PW, PH, **kw)
    b = D.Pipe(qt, F, PW, PH, **kw)
    par = (1, 3, 0, 5, 3, D.ME_CHROMA | D.ME_SATD, 2, 2)
    try:
        outs = []
        for p in (a, b):
            p.set_pictures(*pics)
            p.set_reference_frames(luma, chroma)
            PM.run_steps(D, p, torch)
        L = D.lib()
        for args in ((1, 3, 0, 5, 3, 3, 3, 2), (0, 3, 0, 5, 3, 3, 2, 2), (1, 3, 0, 5, 3, 3, 1, 0), (1, 3, 0, 5, 3, 3, 1, 9),
                     (1, 3, 0, (1 << 19) + 1, 3, 3, 1, 2), (1, 3, 0, 5, 3, 3, -1, 2)):
            assert L.odhip_pipe_set_motion_search3(a._p(), *args) == EINVAL, args
        a.set_motion_search3(*par)
        a.step()
        a.flush()
        outs.append(PM.drain(a, 1))
        grid, cost = a.read_mvs(want_cost=True)
        same_search((grid, cost), alone(D, pics, luma, chroma, cdec, par), "pipe")
        assert grid["mvx"].any() and grid["ref"].any()
        b.set_mvs(grid)
        b.step()
        b.flush()
        outs.append(PM.drain(b, 1))
        assert np.array_equal(b.read_mvs(), grid)
        PM.same_outputs(outs[0], outs[1])
        sa, sb = PM.snapshot(D, a), PM.snapshot(D, b)
        assert sorted(sa) == sorted(sb)
        for key in sa:
            assert sa[key] == sb[key], key
        for s in (0, 1):
            assert a.read(D.BUF_PRED, s).tobytes() == b.read(D.BUF_PRED, s).tobytes()
        # another size and number of levels on the same pipe: more points, so more scratch
        small = (0, 3, 0, 5, 3, D.ME_CHROMA, 1, 1)
        a.set_motion_search3(1, -1)
        a.set_motion_search3(*small)
        a.step()
        a.flush()
        PM.drain(a, 1)
        same_search(a.read_mvs(want_cost=True), alone(D, pics, luma, chroma, cdec, small), "8 x 8 blocks")
        # without levels it is odhip_pipe_set_motion_search2, whatever refine says
        a.set_motion_search3(1, -1)
        a.set_motion_search3(1, 7, 0, 5, 3, 3, 0, 5)
        a.step()
        a.flush()
        PM.drain(a, 1)
        g3 = a.read_mvs(want_cost=True)
        a.set_motion_search2(1, -1)
        a.set_motion_search2(1, 7, 0, 5, 3, 3)
        a.step()
        a.flush()
        PM.drain(a, 1)
        g2 = a.read_mvs(want_cost=True)
        assert g3[0].tobytes() == g2[0].tobytes() and g3[1].tobytes() == g2[1].tobytes()
        assert not np.array_equal(g2[0], grid)
    finally:
        a.destroy()
        b.destroy()


@pytest.mark.parametrize("c444", [False, True], ids=["420", "444"])
def test_three_fed_steps_equal_three_drained_single_steps(D, c444):
    import torch
    cdec = 0 if c444 else 1
    PW, PH = SIZES[cdec]
    qt = D.QuantTables.load()
    kw = dict(chroma_cfl=True, price=True, inter=True, chroma_444=c444)
    pics, refs = [], []
    for k in range(3):
        src = content(seed=1 + k)[0] if k else content()[0][::-1]
        pics.append(crop(np.ascontiguousarray(src), cdec, 20 + k))
        refs.append(frames(cdec, k))
    fed = D.Pipe(qt, F, PW, PH, **kw)
    one = D.Pipe(qt, F, PW, PH, **kw)
    par = (2, 3, 1, 2, 1, D.ME_CHROMA | D.ME_SATD, 2, 1)
    try:
        for p in (fed, one):
            p.set_reference_frames(*refs[0])
            p.set_motion_search3(*par)
            PM.run_steps(D, p, torch, 3)
        fed.set_pictures(*pics[0])
        pinned = []
        for k in range(3):
            if k:
                pinned.append([torch.from_numpy(x).pin_memory() for x in pics[k]])
                fed.feed(*pinned[-1])
                hl = [torch.from_numpy(np.ascontiguousarray(x)).pin_memory() for x in refs[k][0]]
                hc = [torch.from_numpy(np.ascontiguousarray(x)).pin_memory() for x in refs[k][1]]
                pinned.append((hl, hc))
                fed.feed_reference_frames(hl, hc)
            fed.step()
        fed.flush()
        got = PM.drain(fed, 3)
        last = PM.snapshot(D, fed)
        last_grid = fed.read_mvs(want_cost=True)
        want = []
        for k in range(3):
            one.set_pictures(*pics[k])
            one.set_reference_frames(*refs[k])
            one.step()
            one.flush()
            want += PM.drain(one, 1)
            g = one.read_mvs(want_cost=True)
            same_search(g, alone(D, pics[k], refs[k][0], refs[k][1], cdec, par), k)
        PM.same_outputs(got, want)
        same_search(last_grid, g, "last step")
        ref = PM.snapshot(D, one)
        for key in ref:
            assert last[key] == ref[key], key
    finally:
        fed.destroy()
        one.destroy()
