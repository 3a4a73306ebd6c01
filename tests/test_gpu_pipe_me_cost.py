"""GPU: the pipe's motion search with chroma in the cost and SATD as the sub-pel metric
(odhip_pipe_set_motion_search2): its grids equal odhip_me_search2 on the same pictures and frames, a pipe given
those grids codes the same, fed pictures and reference frames change nothing, and without flags it is
odhip_pipe_set_motion_search.  Shapes as in test_gpu_me.py; the pipe codes 4:2:0 pictures of even sizes only, so
4:2:0 runs at 120 x 56 and 4:4:4 at the odd 119 x 55."""
import ctypes

import numpy as np
import pytest

import test_gpu_pipe_mc as PM
from test_gpu_me import content, cuda, same_search, chroma_of

pytestmark = pytest.mark.gpu

W, H, F = 128, 64, 2
SIZES = {1: (120, 56), 0: (119, 55)}      # by cdec
EINVAL = -10


@pytest.fixture(scope="module")
def D():
    import torch
    import daala_amd
    assert torch.cuda.is_available()
    daala_amd.init(0)
    return daala_amd


def crop(src, cdec, seed):
    """(luma [F][ph][pw], chroma [2F][..]) at the chroma format's picture size."""
    pw, ph = SIZES[cdec]
    c = chroma_of(src, cdec, seed)
    return (np.ascontiguousarray(src[:, :ph, :pw]), np.ascontiguousarray(c[:, :ph >> cdec, :pw >> cdec]))


def frames(cdec, k=0):
    _, refs = content(seed=1 + k)
    return refs, [np.roll(chroma_of(r, cdec, 8 + i + 2*k), (i, 1 - i), axis=(1, 2)) for i, r in enumerate(refs)]


def alone(D, pics, luma, chroma, cdec, par):
    lg, rng_, res, lam, lam2, flags = par
    pw, ph = SIZES[cdec]
    return D.me_search2(cuda(pics[0])[0], cuda(*luma), pw, ph, lg, rng_, res, lam, lam2, flags, cuda(pics[1])[0],
                        cuda(*chroma), cdec)


@pytest.mark.parametrize("c444", [False, True], ids=["420", "444"])
def test_pipe_search_equals_the_stand_alone_search_and_a_pipe_given_its_grid(D, c444):
    import torch
    cdec = 0 if c444 else 1
    PW, PH = SIZES[cdec]
    pics = crop(content()[0], cdec, 7)
    luma, chroma = frames(cdec)
    qt = D.QuantTables.load()
    kw = dict(chroma_cfl=True, price=True, inter=True, chroma_444=c444)
    a = D.Pipe(qt, F, PW, PH, **kw)
    b = D.Pipe(qt, F, PW, PH, **kw)
    par = (1, 7, 0, 5, 3, D.ME_CHROMA | D.ME_SATD)
    try:
        outs = []
        for p in (a, b):
            p.set_pictures(*pics)
            p.set_reference_frames(luma, chroma)
            PM.run_steps(D, p, torch)
        L = D.lib()
        for args in ((1, 7, 0, 5, -1, 3), (1, 7, 0, 5, (1 << 20) + 1, 3), (1, 7, 0, 5, 3, 4), (1, 7, 0, 5, 3, -1)):
            assert L.odhip_pipe_set_motion_search2(a._p(), *args) == EINVAL, args
        a.set_motion_search2(*par)
        a.step()
        a.flush()
        outs.append(PM.drain(a, 1))
        grid, cost = a.read_mvs(want_cost=True)
        same_search((grid, cost), alone(D, pics, luma, chroma, cdec, par), "pipe")
        assert grid["mvx"].any() and grid["ref"].any()
        # not the luma search's grids
        plain = D.me_search(cuda(pics[0])[0], cuda(*luma), PW, PH, 1, 7, 0, 5)
        assert not np.array_equal(plain[0], grid)
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
        # without flags and with one lambda it is odhip_pipe_set_motion_search; off and on again works
        a.set_motion_search2(1, -1)
        a.set_motion_search2(1, 7, 0, 5, 5, 0)
        a.step()
        a.flush()
        PM.drain(a, 1)
        g2 = a.read_mvs(want_cost=True)
        a.set_motion_search(1, -1)
        a.set_motion_search(1, 7, 0, 5)
        a.step()
        a.flush()
        PM.drain(a, 1)
        g1 = a.read_mvs(want_cost=True)
        assert g1[0].tobytes() == g2[0].tobytes() and g1[1].tobytes() == g2[1].tobytes()
        same_search(g1, plain, "no flags")
        a.set_motion_search2(*par)
        a.step()
        a.flush()
        PM.drain(a, 1)
        same_search(a.read_mvs(want_cost=True), (grid, cost), "on again")
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
    par = (2, 3, 1, 2, 1, D.ME_CHROMA | D.ME_SATD)
    try:
        for p in (fed, one):
            p.set_reference_frames(*refs[0])
            p.set_motion_search2(*par)
            PM.run_steps(D, p, torch, 3)
        # three steps back to back, the pictures AND the reference frames of step k + 1 fed from pinned memory behind
        # step k: the search of step k reads chroma pictures and chroma frames the feeds must not overwrite early
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
