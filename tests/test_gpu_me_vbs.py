"""GPU: the motion search at variable block sizes (me_kernels.hip: odhip_me_search_vbs, and the pipe's
odhip_pipe_set_motion_search_vbs) against the numpy yardstick tests/_me_vbs_ref.py.  Every comparison is exact integer
equality.

Unless said otherwise the shape is the standard small one of _me_vbs_ref.scene: coded 128 x 64, pictures 120 x 56, two
pictures, two reference slots, 4:2:0, range 3, refine 1, one level, 1/8 pel."""
import ctypes

import numpy as np
import pytest

import _mc_ref as R
import _me_vbs_ref as V
import test_gpu_pipe_mc as PM
from test_gpu_me import cuda, same_search
from test_me_vbs_ref import result, PAR, PENALTY, SIZES

pytestmark = pytest.mark.gpu

EINVAL, EIMPL = -10, -23
BOTH = 3                                        # ME_CHROMA | ME_SATD


@pytest.fixture(scope="module")
def D():
    import torch
    import daala_amd
    assert torch.cuda.is_available()
    daala_amd.init(0)
    return daala_amd


def run(D, planes, pw, ph, log_min, log_max, flags=0, penalty=PENALTY, par=PAR):
    src, csrc, refs, crefs = planes
    return D.me_search_vbs(cuda(src)[0], cuda(*refs), pw, ph, log_min, log_max, par["rng"], par["res"], par["lam"],
                           par["lam_subpel"], flags, None if csrc is None else cuda(csrc)[0],
                           None if crefs is None else cuda(*crefs), par["cdec"], par["levels"], par["refine"], penalty,
                           want_cell_dist=True)


def same_result(D, got, want, nrefs, what):
    """grid, cost and cell_dist equal the yardstick's; the library's own check accepts the grid at both decimations and
    its walk finds the yardstick's leaves."""
    same_search(got[:2], (want["grid"], want["cost"]), what)
    assert got[2].dtype == np.uint32 and np.array_equal(got[2], want["cell_dist"]), what
    h, w = want["grid"].shape[1] - 1 << 3, want["grid"].shape[2] - 1 << 3
    for dec in (0, 1):
        assert D.mc_check_grid(got[0], w, h, dec=dec, nrefs=nrefs) == 0, (what, dec)
    for leaves, mine in zip(D.mc_leaves(got[0], w, h), want["leaves"]):
        assert leaves.tolist() == sorted(R.leaf_desc(*l) for l in mine), what
    assert np.all(got[0]["reserved"] == 0)


CASES = [(lo, hi, flags, 2) for lo, hi in SIZES for flags in (0, BOTH)] + [(0, 3, 0, 1), (0, 3, BOTH, 3)]


@pytest.mark.parametrize("log_min,log_max,flags,nslots", CASES)
def test_grid_cost_and_cell_dist_equal_the_yardstick(D, log_min, log_max, flags, nslots):
    got = run(D, V.scene(nslots), V.PW, V.PH, log_min, log_max, flags)
    same_result(D, got, result(log_min, log_max, flags, nslots), nslots, (log_min, log_max, flags, nslots))
    if (log_min, log_max) == (0, 3):
        assert len({int(x) >> 24 & 3 for leaves in D.mc_leaves(got[0], V.W, V.H) for x in leaves}) >= 3


def test_a_picture_that_ends_inside_8x8_cells_from_rows_of_any_alignment(D):
    import torch
    pw, ph = 117, 53
    src, csrc, refs, crefs = V.scene()
    planes = (np.ascontiguousarray(src[:, :ph, :pw]), np.ascontiguousarray(csrc[:, :27, :59]), refs, crefs)
    want = V.search(*planes[:2], pw, ph, refs, crefs, 0, 3, PAR["rng"], PAR["res"], PAR["lam"], PAR["lam_subpel"], BOTH,
                    PAR["cdec"], PAR["levels"], PAR["refine"], PENALTY)
    got = run(D, planes, pw, ph, 0, 3, BOTH)
    same_result(D, got, want, 2, "117 x 53")
    # the last column and row of cells that hold a part of the picture are cut: 5 of 8 columns, 5 of 8 rows
    assert want["cell_dist"][:, :, :, 14].any() and want["cell_dist"][:, :, 6, :].any()
    # the same pictures inside a larger buffer: an odd base, an odd stride, a padded plane stride
    big = torch.full((V.F, ph + 3, pw + 4), 9, dtype=torch.uint8, device="cuda")
    big[:, 1:1 + ph, 2:2 + pw] = cuda(planes[0])[0]
    view = big[:, 1:1 + ph, 2:2 + pw]
    assert view.stride(1) % 2 == 1 and view.data_ptr() % 2 == 1
    again = D.me_search_vbs(view, cuda(*refs), pw, ph, 0, 3, PAR["rng"], PAR["res"], PAR["lam"], PAR["lam_subpel"], BOTH,
                            cuda(planes[1])[0], cuda(*crefs), 1, PAR["levels"], PAR["refine"], PENALTY,
                            want_cell_dist=True)
    for a, b in zip(got, again):
        assert a.tobytes() == b.tobytes()


@pytest.mark.parametrize("pw,ph,n", [(117, 53, 4), (128, 64, 1), (3, 64, 2)])
def test_cell_dist_alone_equals_the_yardstick(D, pw, ph, n):
    import torch
    rng = np.random.RandomState(pw + n)
    src = rng.randint(0, 256, size=(V.F, ph, pw)).astype(np.uint8)
    # predictions at both ends of the sample range against the source, so that a byte beyond the picture would show
    preds = [rng.randint(0, 256, size=(V.F, V.H, V.W)).astype(np.uint8) for _ in range(n)]
    preds[0][:] = 255 - np.pad(src, ((0, 0), (0, V.H - ph), (0, V.W - pw)), mode="edge")
    want = np.stack([V.cell_dist(src, pw, ph, p) for p in preds]).astype(np.uint32)
    refs = cuda(preds[0])
    assert np.array_equal(D.me_cell_dist(cuda(src)[0], refs, pw, ph, cuda(*preds)), want)
    # rows of any alignment: an odd base and an odd stride
    big = torch.zeros((V.F, ph + 2, pw + 2 + (pw & 1 ^ 1)), dtype=torch.uint8, device="cuda")
    big[:, 1:1 + ph, 2:2 + pw] = cuda(src)[0]
    view = big[:, 1:1 + ph, 2:2 + pw]
    assert view.stride(1) % 2 == 1 and view.data_ptr() % 2 == 1
    assert np.array_equal(D.me_cell_dist(view, refs, pw, ph, cuda(*preds)), want)
    # a prediction that is not 8-byte aligned is refused
    job = D.api._me_job(cuda(src)[0], refs, pw, ph, 0, 0, 0, 0)
    ptrs = (ctypes.c_void_p * 1)(refs[0].data_ptr() + 4)
    assert D.lib().odhip_me_cell_dist(ctypes.byref(job), ptrs, 1, ctypes.c_void_p(refs[0].data_ptr()), None) == EINVAL
    assert D.lib().odhip_me_cell_dist(ctypes.byref(job), ptrs, 5, ctypes.c_void_p(refs[0].data_ptr()), None) == EINVAL


@pytest.mark.parametrize("lg", [0, 1, 2, 3])
def test_one_size_is_the_coarse_to_fine_search_byte_for_byte(D, lg):
    src, csrc, refs, crefs = V.scene()
    levels = min(2, lg + 1)
    par = dict(PAR, levels=levels)
    got = run(D, (src, csrc, refs, crefs), V.PW, V.PH, lg, lg, BOTH, par=par)
    want = D.me_search3(cuda(src)[0], cuda(*refs), V.PW, V.PH, lg, PAR["rng"], PAR["res"], PAR["lam"], PAR["lam_subpel"],
                        BOTH, cuda(csrc)[0], cuda(*crefs), 1, levels, PAR["refine"])
    assert got[0].tobytes() == want[0].tobytes() and got[1].tobytes() == want[1].tobytes() and got[2] is None
    assert got[0]["mvx"].any()


def test_split_penalty_extremes(D):
    src, csrc, refs, crefs = V.scene()
    # a picture equal to its reference: every D is 0, and 0 < 0 is false - nothing splits at no penalty
    same = (np.ascontiguousarray(refs[0][:, :V.PH, :V.PW]), None, refs, None)
    grid, cost, dist = run(D, same, V.PW, V.PH, 0, 3, penalty=0)
    assert not dist.any() and not grid["mvx"].any() and not grid["mvy"].any() and not grid["ref"].any()
    for leaves in D.mc_leaves(grid, V.W, V.H):
        assert len(leaves) == 2 and np.all(leaves >> 24 & 3 == 3)
    # the largest penalty splits nothing either, whatever the content
    grid, cost, dist = run(D, (src, csrc, refs, crefs), V.PW, V.PH, 0, 3, penalty=1 << 24)
    assert dist.any()
    for leaves in D.mc_leaves(grid, V.W, V.H):
        assert len(leaves) == 2 and np.all(leaves >> 24 & 3 == 3)
    # the left 64 x 64 cell of picture 0, on the threshold: 8 D_2 + penalty == 8 D_3 keeps it whole, one less splits it
    base = result(0, 3)
    d = base["cell_dist"]
    edge = 8*(int(d[3, 0, :, :8].sum()) - int(d[2, 0, :, :8].sum()))
    assert 0 < edge <= 1 << 24
    for penalty, split in ((edge, 0), (edge - 1, 1)):
        got = run(D, (src, csrc, refs, crefs), V.PW, V.PH, 0, 3, penalty=penalty)
        want = V.search(src, csrc, V.PW, V.PH, refs, crefs, 0, 3, PAR["rng"], PAR["res"], PAR["lam"], PAR["lam_subpel"],
                        0, PAR["cdec"], PAR["levels"], PAR["refine"], penalty, uni=dict(base["uni"]))
        same_result(D, got, want, 2, penalty)
        assert got[0]["valid"][0, 4, 4] == split


def test_a_picture_of_one_cell_in_a_frame_of_64(D):
    src, csrc, refs, crefs = V.scene()
    planes = (np.ascontiguousarray(src[:, :8, :8]), np.ascontiguousarray(csrc[:, :4, :4]),
              [np.ascontiguousarray(r[:, :, :64]) for r in refs], [np.ascontiguousarray(c[:, :, :32]) for c in crefs])
    want = V.search(planes[0], planes[1], 8, 8, planes[2], planes[3], 0, 3, PAR["rng"], PAR["res"], PAR["lam"],
                    PAR["lam_subpel"], BOTH, PAR["cdec"], PAR["levels"], PAR["refine"], 0)
    got = run(D, planes, 8, 8, 0, 3, BOTH, penalty=0)
    same_result(D, got, want, 2, "8 x 8")
    # all cells but one are empty; a cell whose distortions are all 0 is kept, at any size and no penalty
    assert not got[2][:, :, 1:, :].any() and not got[2][:, :, :, 1:].any()
    for g in got[0]:
        assert not g["valid"][2::4, 6].any() and not g["valid"][6, 2::4].any()       # the 32 x 32 cells off the corner
        assert not g["valid"][1::2, 5::2].any() and not g["valid"][5::2, 1::2].any()  # their 16 x 16 cells


def test_the_cells_legality_holds_where_the_uniform_one_would_not(D):
    src, refs = V.border_scene()
    par = dict(rng=32, res=3, lam=0, lam_subpel=0, cdec=1, levels=1, refine=8)
    want = V.search(src, None, V.W, V.H, refs, None, 0, 3, 32, 3, 0, 0, 0, 1, 1, 8, PENALTY)
    got = run(D, (src, None, refs, None), V.W, V.H, 0, 3, par=par)
    same_result(D, got, want, 1, "border")
    # the 8 x 8 search alone takes the vector the mixed grid may not hold
    small = D.me_search3(cuda(src)[0], cuda(*refs), V.W, V.H, 0, 32, 3, 0, 0, 0, None, None, 1, 1, 8)[0]
    assert int(small["mvx"][0, 4, 8]) <= -8*66 and not V.mv_ok_cells(8, int(small["mvx"][0, 4, 8]), 3, V.W >> 3)
    mine = int(got[0]["mvx"][0, 4, 8])
    assert mine != int(small["mvx"][0, 4, 8]) and V.mv_ok_cells(8, mine, 3, V.W >> 3)


def test_refused_jobs_launch_nothing(D):
    import torch
    src, csrc, refs, crefs = V.scene()
    d_src, d_csrc, d_refs, d_crefs = cuda(src)[0], cuda(csrc)[0], cuda(*refs), cuda(*crefs)
    L = D.lib()
    shape = (V.F, V.H//8 + 1, V.W//8 + 1)
    grid = torch.full(shape + (D.MV_POINT.itemsize,), 0xab, dtype=torch.uint8, device="cuda")
    cost = torch.full(shape, 0x5a5a5a5a, dtype=torch.int32, device="cuda")
    dist = torch.full((4, V.F, V.H//8, V.W//8), 0x5a5a5a5a, dtype=torch.int32, device="cuda")
    keep = []

    def job(**kw):
        j, scratch = D.api._me_job4(d_src, d_refs, V.PW, V.PH, 0, 3, 3, 0, 2, 1, BOTH, d_csrc, d_crefs, 1, 1, 1, PENALTY)
        scratch.fill_(0x77)
        keep.append(scratch)
        j.base.base.luma.grid, j.base.base.luma.cost, j.cell_dist = grid.data_ptr(), cost.data_ptr(), dist.data_ptr()
        for k, v in kw.items():
            setattr(j.base.base.luma if k in ("range", "lambda_", "log_size", "res") else j.base if k in (
                "levels", "refine", "scratch", "scratch_bytes") else j, k, v)
        return j

    def search(j):
        return L.odhip_me_search_vbs(ctypes.byref(j), None)

    short = job().base.scratch_bytes - 1
    for kw in (dict(log_min=-1), dict(log_min=4), dict(log_size=4), dict(split_penalty=-1),
               dict(split_penalty=(1 << 24) + 1), dict(scratch=None), dict(scratch_bytes=short), dict(levels=3),
               dict(levels=-1), dict(refine=0), dict(refine=9), dict(range=33), dict(range=-1), dict(res=4),
               dict(lambda_=(1 << 19) + 1)):
        assert search(job(**kw)) == EINVAL, kw
    with D.Context(0) as ctx:
        ctx.set_fpr(True)
        assert search(job()) == EIMPL
    torch.cuda.synchronize()
    assert bool((grid == 0xab).all()) and bool((cost == 0x5a5a5a5a).all()) and bool((dist == 0x5a5a5a5a).all())
    assert all(bool((s == 0x77).all()) for s in keep)
    # ... and the same job, unchanged, runs
    assert search(job()) == 0
    torch.cuda.synchronize()
    assert not bool((grid == 0xab).any(dim=-1).all()) and not bool((dist == 0x5a5a5a5a).any())


# ---- in the pipe ----
VBS = (0, 3, 3, 0, 2, 1, BOTH, 1, 1, PENALTY)   # log_min, log_max, range, res, lambdas, flags, levels, refine, penalty


def alone(D, planes, par=VBS, pw=V.PW, ph=V.PH):
    src, csrc, refs, crefs = planes
    lo, hi, rng_, res, lam, lam2, flags, levels, refine, penalty = par
    return D.me_search_vbs(cuda(src)[0], cuda(*refs), pw, ph, lo, hi, rng_, res, lam, lam2, flags, cuda(csrc)[0],
                           cuda(*crefs), 1, levels, refine, penalty)


def test_pipe_search_equals_the_stand_alone_search_and_a_pipe_given_its_grid(D):
    import torch
    planes = V.scene()
    src, csrc, refs, crefs = planes
    qt = D.QuantTables.load()
    kw = dict(chroma_cfl=True, price=True, inter=True)
    a = D.Pipe(qt, V.F, V.PW, V.PH, **kw)
    b = D.Pipe(qt, V.F, V.PW, V.PH, **kw)
    try:
        outs = []
        for p in (a, b):
            p.set_pictures(src, csrc)
            p.set_reference_frames(refs, crefs)
            PM.run_steps(D, p, torch)
        L = D.lib()
        for args in ((-1, 3, 3, 0, 2, 1, 3, 1, 1, 16), (2, 1, 3, 0, 2, 1, 3, 1, 1, 16), (0, 4, 3, 0, 2, 1, 3, 1, 1, 16),
                     (0, 3, 3, 0, 2, 1, 3, 1, 1, -1), (0, 3, 3, 0, 2, 1, 3, 1, 1, (1 << 24) + 1),
                     (0, 3, 33, 0, 2, 1, 3, 1, 1, 16), (0, 3, 3, 0, 2, 1, 3, 3, 1, 16), (0, 3, 3, 0, 2, 1, 3, 1, 9, 16),
                     (0, 3, 3, 0, (1 << 19) + 1, 1, 3, 1, 1, 16), (0, 3, 3, 0, 2, 1, 4, 1, 1, 16)):
            assert L.odhip_pipe_set_motion_search_vbs(a._p(), *args) == EINVAL, args
        assert L.odhip_pipe_set_motion_search_vbs(None, *VBS) == EINVAL
        a.set_motion_search_vbs(*VBS)
        with pytest.raises(D.DaalaHipError):
            a.set_mvs(np.zeros((V.F, V.H//8 + 1, V.W//8 + 1), D.MV_POINT))     # a step takes its grids one way
        a.step()
        a.flush()
        outs.append(PM.drain(a, 1))
        grid, cost = a.read_mvs(want_cost=True)
        same_search((grid, cost), alone(D, planes), "pipe")
        want = result(0, 3, BOTH)
        same_search((grid, cost), (want["grid"], want["cost"]), "pipe against the yardstick")
        assert len({int(x) >> 24 & 3 for leaves in D.mc_leaves(grid, V.W, V.H) for x in leaves}) >= 3
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
        # other sizes on the same pipe, then one size: the coarse-to-fine search at that size
        a.set_motion_search_vbs(0, 0, -1)
        a.set_motion_search_vbs(1, 2, 3, 0, 2, 1, 0, 2, 1, 0)
        a.step()
        a.flush()
        PM.drain(a, 1)
        same_search(a.read_mvs(want_cost=True), alone(D, planes, (1, 2, 3, 0, 2, 1, 0, 2, 1, 0)), "16 to 32")
        a.set_motion_search_vbs(0, 0, -1)
        a.set_motion_search_vbs(2, 2, 3, 0, 2, 1, BOTH, 2, 1, 5)
        a.step()
        a.flush()
        PM.drain(a, 1)
        g1 = a.read_mvs(want_cost=True)
        a.set_motion_search3(2, -1)
        a.set_motion_search3(2, 3, 0, 2, 1, BOTH, 2, 1)
        a.step()
        a.flush()
        PM.drain(a, 1)
        g3 = a.read_mvs(want_cost=True)
        assert g1[0].tobytes() == g3[0].tobytes() and g1[1].tobytes() == g3[1].tobytes()
    finally:
        a.destroy()
        b.destroy()


def test_the_pipe_setter_refuses_full_precision_references(D):
    qt = D.QuantTables.load()
    p = D.Pipe(qt, 1, 64, 64, chroma_cfl=True, price=True, inter=True, fpr_bits=12)
    try:
        assert D.lib().odhip_pipe_set_motion_search_vbs(p._p(), *VBS) == EIMPL
    finally:
        p.destroy()
    p = D.Pipe(qt, 1, 64, 64, chroma_cfl=True, price=True)
    try:
        assert D.lib().odhip_pipe_set_motion_search_vbs(p._p(), *VBS) == EINVAL      # not an inter pipe
    finally:
        p.destroy()


def test_two_fed_steps_equal_two_drained_single_steps(D):
    import torch
    qt = D.QuantTables.load()
    kw = dict(chroma_cfl=True, price=True, inter=True)
    scenes = [V.scene(), V.scene(seed=5)]
    fed = D.Pipe(qt, V.F, V.PW, V.PH, **kw)
    one = D.Pipe(qt, V.F, V.PW, V.PH, **kw)
    try:
        for p in (fed, one):
            p.set_reference_frames(scenes[0][2], scenes[0][3])
            p.set_motion_search_vbs(*VBS)
            PM.run_steps(D, p, torch, 2)
        fed.set_pictures(scenes[0][0], scenes[0][1])
        pinned = []
        for k in range(2):
            if k:
                pinned.append([torch.from_numpy(x).pin_memory() for x in scenes[k][:2]])
                fed.feed(*pinned[-1])
                hl = [torch.from_numpy(np.ascontiguousarray(x)).pin_memory() for x in scenes[k][2]]
                hc = [torch.from_numpy(np.ascontiguousarray(x)).pin_memory() for x in scenes[k][3]]
                pinned.append((hl, hc))
                fed.feed_reference_frames(hl, hc)
            fed.step()
        fed.flush()
        got = PM.drain(fed, 2)
        last = PM.snapshot(D, fed)
        last_grid = fed.read_mvs(want_cost=True)
        want = []
        for k in range(2):
            one.set_pictures(scenes[k][0], scenes[k][1])
            one.set_reference_frames(scenes[k][2], scenes[k][3])
            one.step()
            one.flush()
            want += PM.drain(one, 1)
            g = one.read_mvs(want_cost=True)
            same_search(g, alone(D, scenes[k]), k)
        PM.same_outputs(got, want)
        same_search(last_grid, g, "last step")
        ref = PM.snapshot(D, one)
        for key in ref:
            assert last[key] == ref[key], key
    finally:
        fed.destroy()
        one.destroy()
