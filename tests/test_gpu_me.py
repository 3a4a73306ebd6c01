"""GPU: the block-matching motion search (me_kernels.hip: odhip_me_search / _limits / _costs, and the pipe's
odhip_pipe_set_motion_search / odhip_pipe_mvs_read) against the numpy yardstick tests/_me_ref.py and the compiled
reference's recorded costs (tests/golden/me.npz).  Every comparison is exact integer equality.

Unless said otherwise the coded size is 128 x 64, the picture 120 x 56, two pictures, two reference slots: the
smallest frame with more than one 64 x 64 cell, a picture edge inside a block on the right and at the bottom, and
points whose clipped block is empty (vx = 16 at 8 x 8 blocks)."""
import ctypes
import functools

import numpy as np
import pytest

import _mc_ref as R
import _me_ref as M
import test_gpu_pipe_mc as PM
from test_me_ref import load_golden

pytestmark = pytest.mark.gpu

W, H, PW, PH, F = 128, 64, 120, 56, 2
EINVAL, EIMPL = -10, -23


@pytest.fixture(scope="module")
def D():
    import torch
    import daala_amd
    assert torch.cuda.is_available()
    daala_amd.init(0)
    return daala_amd


@functools.lru_cache(maxsize=None)
def content(seed=1, w=W, h=H, pw=PW, ph=PH):
    """(src [2][ph][pw], refs: two slots [2][h][w]).  Picture 0: smoothed noise, the slots are the same scene moved
    by a few pixels plus noise; picture 1: slot 0 displaced by a planted 1/8-pel vector, slot 1 unrelated."""
    rng = np.random.RandomState(seed)
    big = M.smooth_noise(rng, h + 32, w + 32)

    def cut(dx, dy, noise):
        p = big[16 + dy:16 + dy + h, 16 + dx:16 + dx + w].astype(int) + rng.randint(-noise, noise + 1, size=(h, w))
        return np.clip(p, 0, 255).astype(np.uint8)

    src0 = cut(0, 0, 0)[:ph, :pw]
    r0 = [cut(2, -1, 3), M.smooth_noise(rng, h, w)]
    r1 = [cut(-3, 2, 2), M.smooth_noise(rng, h, w)]
    src1 = M.displaced(r0[1], 13, -6)[:ph, :pw]
    src = np.ascontiguousarray(np.stack([src0, src1]))
    return src, [np.stack(r0), np.stack(r1)]


def cuda(*arrays):
    import torch
    return [torch.from_numpy(np.ascontiguousarray(a)).cuda() for a in arrays]


def check_shape(D, grid, cost, lg, w, h):
    """Only leaves of the requested size; the points between the searched ones are all zero."""
    s = 1 << lg
    for leaves in D.mc_leaves(grid, w, h):
        assert len(leaves) == (w >> 3)*(h >> 3) >> 2*lg
        assert np.all((leaves >> 24 & 3) == lg) and np.all(leaves >> 28 == 3)
    mask = np.ones(grid.shape[1:], bool)
    mask[::s, ::s] = False
    assert not grid[:, mask].tobytes().strip(b"\0")
    assert np.all(grid["valid"][:, ::s, ::s] == 1) and np.all(grid["reserved"] == 0)
    if cost is not None:
        assert not cost[:, mask].any()


def same_search(got, want, what):
    for name in ("mvx", "mvy", "valid", "ref"):
        bad = np.argwhere(got[0][name] != want[0][name])
        assert bad.size == 0, (what, name, bad[:5].tolist(), got[0][name][tuple(bad[0])], want[0][name][tuple(bad[0])])
    assert np.array_equal(got[1], want[1]), (what, np.argwhere(got[1] != want[1])[:5].tolist())


# ---- 1. costs ----
def test_costs_equal_the_recorded_reference(D):
    g = load_golden()
    src, plane = cuda(g["src"][None], g["plane"][None])
    cases = np.array(g["cases"])
    want = np.array(g["sad"])
    for lg in range(4):
        pick = cases[:, 2] == lg
        c = np.zeros(int(pick.sum()), D.ME_CAND)
        c["vx"], c["vy"], c["mvx"], c["mvy"] = cases[pick, 0], cases[pick, 1], cases[pick, 3], cases[pick, 4]
        got = D.me_costs(src, [plane], g["pic_w"], g["pic_h"], lg, c)
        assert np.array_equal(got, want[pick]), (lg, got.tolist(), want[pick].tolist())


@pytest.mark.parametrize("lg", [0, 1, 2, 3])
def test_costs_equal_the_yardstick(D, lg):
    src, refs = content()
    rng = np.random.RandomState(10 + lg)
    s = 1 << lg
    xs, ys = list(range(0, W//8 + 1, s)), list(range(0, H//8 + 1, s))
    # every point of the frame's four edges (its corners with them), then every phase pair at random points
    pts = [(x, y) for x in xs for y in (ys[0], ys[-1])] + [(x, y) for y in ys for x in (xs[0], xs[-1])]
    pts += [(xs[rng.randint(len(xs))], ys[rng.randint(len(ys))]) for _ in range(64)]
    c = np.zeros(len(pts), D.ME_CAND)
    n0 = len(pts) - 64
    for i, (vx, vy) in enumerate(pts):
        fx, fy = ((i - n0) % 8, (i - n0)//8) if i >= n0 else (rng.randint(8), rng.randint(8))
        c[i] = (rng.randint(F), vx, vy, rng.randint(2), 8*rng.randint(-33, 33) + fx, 8*rng.randint(-33, 33) + fy)
    if lg == 0:
        assert any(M.clip_of(*M.block_of(vx, vy, lg), PW, PH) is None for vx, vy in pts)
    got = D.me_costs(*cuda(src), cuda(*refs), PW, PH, lg, c)
    want = [M.bma_sad(src[k["pic"]], PW, PH, refs[k["slot"]][k["pic"]], int(k["vx"]), int(k["vy"]), lg, int(k["mvx"]),
                      int(k["mvy"])) for k in c]
    assert got.tolist() == want
    # a candidate that names nothing is flagged, not evaluated
    bad = c[:3].copy()
    bad["pic"][0], bad["slot"][1], bad["vx"][2] = F, 2, W//8 + 1
    assert D.me_costs(*cuda(src), cuda(*refs), PW, PH, lg, bad).tolist() == [0xffffffff]*3


# ---- 2. the full search, 5. its shape ----
@pytest.mark.parametrize("rng_", [0, 3, 7])
@pytest.mark.parametrize("lg", [0, 1, 2, 3])
def test_search_equals_the_yardstick(D, lg, rng_):
    src, refs = content()
    d_src, d_refs = cuda(src)[0], cuda(*refs)
    for res in (3, 0):
        for lam in (0, 5):
            got = D.me_search(d_src, d_refs, PW, PH, lg, rng_, res, lam)
            want = M.search(src, PW, PH, refs, lg, rng_, res, lam)
            same_search(got, want, (res, lam))
            check_shape(D, got[0], got[1], lg, W, H)


def test_odd_strides_and_a_larger_plane_stride_change_nothing(D):
    import torch
    src, refs = content()
    want = D.me_search(cuda(src)[0], cuda(*refs), PW, PH, 1, 3, 0, 5)
    wide = torch.full((F, PH + 3, PW + 7), 77, dtype=torch.uint8, device="cuda")
    wide[:, :PH, :PW] = cuda(src)[0]
    d_refs = []
    for r in refs:
        t = torch.full((F, H + 1, W + 5), 99, dtype=torch.uint8, device="cuda")
        t[:, :H, :W] = cuda(r)[0]
        d_refs.append(t[:, :H, :W])
    view = wide[:, :PH, :PW]
    assert view.stride(1) % 2 == 1 and view.stride(0) > PH*view.stride(1) and d_refs[0].stride(1) % 2 == 1
    got = D.me_search(view, d_refs, PW, PH, 1, 3, 0, 5)
    same_search(got, want, "strides")
    got = D.me_search(view, d_refs, PW, PH, 1, 3, 0, 5, want_cost=False)
    assert got[1] is None and np.array_equal(got[0], want[0])


# ---- 3. legality ----
def test_long_range_search_stays_legal(D):
    rng = np.random.RandomState(3)
    big = M.smooth_noise(rng, 128 + 160, 128 + 160)
    src = np.ascontiguousarray(big[80:208, 80:208])[None]
    # the scene moved by more than the frame leaves room for: the best matches lie outside it
    refs = [np.ascontiguousarray(big[80 - 45:208 - 45, 80 + 50:208 + 50])[None],
            np.ascontiguousarray(big[80 + 58:208 + 58, 80 - 61:208 - 61])[None]]
    got = D.me_search(cuda(src)[0], cuda(*refs), 128, 128, 3, 32, 0, 1)
    want = M.search(src, 128, 128, refs, 3, 32, 0, 1)
    same_search(got, want, "range 32")
    check_shape(D, got[0], got[1], 3, 128, 128)
    assert np.abs(got[0]["mvx"]).max() > 8*16 or np.abs(got[0]["mvy"]).max() > 8*16
    for dec in (0, 1):
        assert D.mc_check_grid(got[0], 128, 128, dec=dec, nrefs=2) == 0
        assert R.grid_in_range(got[0][0], dec)
    for lg in range(4):
        for vy in range(0, 17, 1 << lg):
            for vx in range(0, 17, 1 << lg):
                assert D.me_limits(128, 128, lg, vx, vy) == M.limits(128, 128, lg, vx, vy), (lg, vx, vy)


# ---- 4. ties ----
def test_flat_content_gives_zero_vectors_in_slot_zero(D):
    src = np.full((F, PH, PW), 100, np.uint8)
    refs = [np.full((F, H, W), 90, np.uint8), np.full((F, H, W), 90, np.uint8)]
    for lg in range(4):
        grid, cost = D.me_search(cuda(src)[0], cuda(*refs), PW, PH, lg, 7, 0, 0)
        assert not grid["mvx"].any() and not grid["mvy"].any() and not grid["ref"].any()
        for vy in range(0, H//8 + 1, 1 << lg):
            for vx in range(0, W//8 + 1, 1 << lg):
                c = M.clip_of(*M.block_of(vx, vy, lg), PW, PH)
                area = 0 if c is None else (c[1] - c[0])*(c[3] - c[2])
                assert np.all(cost[:, vy, vx] == 8*10*area), (lg, vx, vy)


def test_identical_slots_give_slot_zero(D):
    src, refs = content()
    for lg, lam in ((0, 0), (2, 5)):
        grid, cost = D.me_search(cuda(src)[0], cuda(refs[0], refs[0], refs[0]), PW, PH, lg, 3, 0, lam)
        assert not grid["ref"].any()
        one = D.me_search(cuda(src)[0], cuda(refs[0]), PW, PH, lg, 3, 0, lam)
        same_search((grid, cost), one, "three equal slots")


# ---- 6. refusals ----
def test_refused_jobs_launch_nothing(D):
    import torch
    src, refs = content()
    d_src, d_refs = cuda(src)[0], cuda(*refs)
    L = D.lib()
    shape = (F, H//8 + 1, W//8 + 1)
    grid = torch.full(shape + (D.MV_POINT.itemsize,), 0xab, dtype=torch.uint8, device="cuda")
    cost = torch.full(shape, 0x5a5a5a5a, dtype=torch.int32, device="cuda")
    cands = torch.zeros(D.ME_CAND.itemsize, dtype=torch.uint8, device="cuda")
    sad = torch.full((1,), 0x5a5a5a5a, dtype=torch.int32, device="cuda")

    def job(**kw):
        j = D.api._me_job(d_src, d_refs, PW, PH, 1, 3, 0, 5)
        j.grid, j.cost = grid.data_ptr(), cost.data_ptr()
        for k, v in kw.items():
            setattr(j, k, v)
        return j

    def search(j):
        return L.odhip_me_search(ctypes.byref(j), None)

    def costs(j, n=1, c=cands, out=sad):
        return L.odhip_me_costs(ctypes.byref(j), ctypes.c_void_p(c.data_ptr() if c is not None else 0), ctypes.c_long(n),
                                ctypes.c_void_p(out.data_ptr() if out is not None else 0), None)

    no_ref1 = (ctypes.c_void_p * 3)(d_refs[0].data_ptr(), None, None)
    bad = [dict(coded_w=120), dict(coded_h=0), dict(coded_w=32768), dict(pic_w=0), dict(pic_w=W + 1), dict(pic_h=H + 1),
           dict(npics=0), dict(nrefs=0), dict(nrefs=4), dict(log_size=-1), dict(log_size=4), dict(src_stride=PW - 1),
           dict(ref_stride=W - 1), dict(src_plane_stride=PW*PH - 1), dict(ref_plane_stride=W*H - 1), dict(src=None),
           dict(ref=no_ref1)]
    for kw in bad:
        assert search(job(**kw)) == EINVAL, kw
        assert costs(job(**kw)) == EINVAL, kw
    for kw in (dict(range=-1), dict(range=33), dict(res=-1), dict(res=4), dict(lambda_=-1), dict(lambda_=(1 << 20) + 1),
               dict(grid=None)):
        assert search(job(**kw)) == EINVAL, kw
    assert L.odhip_me_search(None, None) == EINVAL
    assert costs(job(), c=None) == EINVAL and costs(job(), out=None) == EINVAL and costs(job(), n=-1) == EINVAL
    # 12-bit references
    with D.Context(0) as ctx:
        ctx.set_fpr(True)
        assert search(job()) == EIMPL and costs(job()) == EIMPL
    lim = (ctypes.c_int * 4)()
    for args in ((120, 64, 0, 0, 0), (128, 64, 4, 0, 0), (128, 64, 1, 17, 0), (128, 64, 1, 0, -1), (128, 64, 1, 3, 0)):
        assert L.odhip_me_limits(*args, lim) == EINVAL, args
    assert L.odhip_me_limits(128, 64, 1, 0, 0, None) == EINVAL
    torch.cuda.synchronize()
    assert bool((grid == 0xab).all()) and bool((cost == 0x5a5a5a5a).all()) and int(sad[0]) == 0x5a5a5a5a
    # ... and the same job, unchanged, runs
    assert search(job()) == 0 and costs(job(), n=0) == 0
    torch.cuda.synchronize()
    assert not bool((grid == 0xab).all())


def chroma_of(luma, cdec, seed):
    rng = np.random.RandomState(seed)
    step = 1 << cdec
    cb = 128 + (luma[:, ::step, ::step].astype(int) - 128)//3 + rng.randint(-2, 3, size=luma[:, ::step, ::step].shape)
    cr = 128 - (luma[:, ::step, ::step].astype(int) - 128)//4
    return np.clip(np.concatenate([cb, cr]), 0, 255).astype(np.uint8)


def test_pipe_refusals(D):
    src, refs = content()
    qt = D.QuantTables.load()
    luma, chroma = refs, [chroma_of(r, 1, 5) for r in refs]
    intra = D.Pipe(qt, F, PW, PH, chroma_cfl=True, price=True)
    fpr = D.Pipe(qt, F, PW, PH, chroma_cfl=True, price=True, inter=True, fpr_bits=12)
    pipe = D.Pipe(qt, F, PW, PH, chroma_cfl=True, price=True, inter=True)
    L = D.lib()
    try:
        assert L.odhip_pipe_set_motion_search(intra._p(), 1, 3, 0, 0) == EINVAL
        fpr.set_reference_frames([r.astype(np.int16) << 4 for r in luma], [c.astype(np.int16) << 4 for c in chroma])
        assert L.odhip_pipe_set_motion_search(fpr._p(), 1, 3, 0, 0) == EIMPL
        assert L.odhip_pipe_set_motion_search(pipe._p(), 1, 3, 0, 0) == EINVAL      # no reference frames yet
        pipe.set_motion_search(1, -1)                                               # off while off: fine
        pipe.set_reference_frames(luma, chroma)
        for args in ((-1, 3, 0, 0), (4, 3, 0, 0), (1, 33, 0, 0), (1, 3, -1, 0), (1, 3, 4, 0), (1, 3, 0, -1)):
            assert L.odhip_pipe_set_motion_search(pipe._p(), *args) == EINVAL, args
        zero = np.zeros((F, H//8 + 1, W//8 + 1), D.MV_POINT)
        zero["valid"][:, ::8, ::8] = 1
        pipe.set_mvs(zero)
        assert L.odhip_pipe_set_motion_search(pipe._p(), 1, 3, 0, 0) == EINVAL      # a resident grid: one way
        pipe.set_mvs(None)
        grid = np.zeros_like(zero)
        assert L.odhip_pipe_mvs_read(pipe._p(), grid.ctypes.data_as(ctypes.c_void_p), None) == EINVAL   # no step yet
        pipe.set_motion_search(1, 3, 0, 0)
        for fn in (L.odhip_pipe_set_mvs, L.odhip_pipe_feed_mvs):
            assert fn(pipe._p(), zero.ctypes.data_as(ctypes.c_void_p)) == EINVAL
        with pytest.raises(D.DaalaHipError):
            pipe.set_reference_pictures(src, chroma_of(src, 1, 6))
        pipe.set_motion_search(1, -1)
        pipe.set_mvs(zero)                                                          # off again: grids are accepted
    finally:
        for p in (intra, fpr, pipe):
            p.destroy()


# ---- 7. in the pipe ----
@pytest.mark.parametrize("c444", [False, True], ids=["420", "444"])
def test_pipe_search_equals_the_stand_alone_search_and_a_pipe_given_its_grid(D, c444):
    import torch
    src, refs = content()
    cdec = 0 if c444 else 1
    src_c = chroma_of(src, cdec, 7)
    luma, chroma = refs, [chroma_of(r, cdec, 8 + i) for i, r in enumerate(refs)]
    qt = D.QuantTables.load()
    kw = dict(chroma_cfl=True, price=True, inter=True, chroma_444=c444)
    a = D.Pipe(qt, F, PW, PH, **kw)
    b = D.Pipe(qt, F, PW, PH, **kw)
    par = (1, 7, 0, 5)
    try:
        outs = []
        for p in (a, b):
            p.set_pictures(src, src_c)
            p.set_reference_frames(luma, chroma)
            PM.run_steps(D, p, torch)
        a.set_motion_search(*par)
        a.step()
        a.flush()
        outs.append(PM.drain(a, 1))
        grid, cost = a.read_mvs(want_cost=True)
        alone = D.me_search(cuda(src)[0], cuda(*luma), PW, PH, *par)
        same_search((grid, cost), alone, "pipe")
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
    finally:
        a.destroy()
        b.destroy()


@pytest.mark.parametrize("c444", [False, True], ids=["420", "444"])
def test_three_fed_steps_equal_three_drained_single_steps(D, c444):
    import torch
    cdec = 0 if c444 else 1
    qt = D.QuantTables.load()
    kw = dict(chroma_cfl=True, price=True, inter=True, chroma_444=c444)
    _, refs = content()
    luma, chroma = refs, [chroma_of(r, cdec, 8 + i) for i, r in enumerate(refs)]
    pics = []
    for k in range(3):
        src = content(seed=1 + k)[0] if k else content()[0][::-1]
        pics.append((np.ascontiguousarray(src), chroma_of(src, cdec, 20 + k)))
    fed = D.Pipe(qt, F, PW, PH, **kw)
    one = D.Pipe(qt, F, PW, PH, **kw)
    par = (2, 3, 1, 2)
    try:
        for p in (fed, one):
            p.set_reference_frames(luma, chroma)
            p.set_motion_search(*par)
            PM.run_steps(D, p, torch, 3)
        # three steps back to back, the pictures of step k + 1 fed from pinned memory behind step k
        fed.set_pictures(*pics[0])
        pinned = []
        for k in range(3):
            if k:
                pinned.append([torch.from_numpy(x).pin_memory() for x in pics[k]])
                fed.feed(*pinned[-1])
            fed.step()
        fed.flush()
        got = PM.drain(fed, 3)
        last = PM.snapshot(D, fed)
        last_grid = fed.read_mvs(want_cost=True)
        want = []
        for k in range(3):
            one.set_pictures(*pics[k])
            one.step()
            one.flush()
            want += PM.drain(one, 1)
            g = one.read_mvs(want_cost=True)
            same_search(g, D.me_search(cuda(pics[k][0])[0], cuda(*luma), PW, PH, *par), k)
        PM.same_outputs(got, want)
        same_search(last_grid, g, "last step")
        ref = PM.snapshot(D, one)
        for key in ref:
            assert last[key] == ref[key], key
    finally:
        fed.destroy()
        one.destroy()
