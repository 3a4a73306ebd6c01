"""GPU: the motion search at variable block sizes (me_kernels.hip: odhip_me_search_vbs with me_vbs.cuh) on frames of
more than one row of 64x64 cells, against the numpy yardstick tests/_me_vbs_ref.py.  Every comparison is exact integer
equality.

tests/test_gpu_me_vbs.py runs coded frames of 128 x 64 and 64 x 64.  Here the frames are 192 x 128 (scene A: three cells
across and two down, 384 8x8 cells and 425 points, so two workgroups per picture in k_me_cell_dist and k_me_vbs_grid, and
a second row of decision words in k_me_vbs_decide) and 64 x 192 (scene B: one cell across, three down): the cell above
and the cell below are real, and a row of decision words is indexed.  Scene A_even is scene A cut to the even picture
size a 4:2:0 pipe takes, for the pipe.  The four border scenes make the legality of the
cells (legal_axis with od_me_mv_ok_cells) bite at either end of either axis.  tests/test_me_vbs_ref.py asserts that the
content gives patterns in which a slip in any of these would show."""
import numpy as np
import pytest

import _me_vbs_ref as V
import test_gpu_pipe_mc as PM
from test_gpu_me import cuda, same_search
from test_gpu_me_vbs import BOTH, alone, run, same_result
from test_me_vbs_ref import PAR, PENALTY, FRAMES, EDGES, BORDER_PAR, frame_scene, frame_result, border_result

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def D():
    import torch
    import daala_amd
    assert torch.cuda.is_available()
    daala_amd.init(0)
    return daala_amd


CASES = [(name,) + case for name in sorted(FRAMES) for case in FRAMES[name][1]]


@pytest.mark.parametrize("name,log_min,log_max,flags,levels,penalty", CASES)
def test_grid_cost_and_cell_dist_equal_the_yardstick(D, name, log_min, log_max, flags, levels, penalty):
    size = FRAMES[name][0]
    got = run(D, frame_scene(name), size["pw"], size["ph"], log_min, log_max, flags, penalty, dict(PAR, levels=levels))
    want = frame_result(name, log_min, log_max, flags, levels, penalty)
    assert got[0].shape == (V.F, size["h"]//8 + 1, size["w"]//8 + 1)
    same_result(D, got, want, 2, (name, log_min, log_max, flags, levels, penalty))
    kinds = {int(x) >> 24 & 3 for leaves in D.mc_leaves(got[0], size["w"], size["h"]) for x in leaves}
    assert len(kinds) >= 2 and kinds <= set(range(log_min, log_max + 1))


@pytest.mark.parametrize("pw,ph", [(185, 117), (192, 128)])
def test_cell_dist_alone_on_more_cells_than_a_workgroup(D, pw, ph):
    w, h = 192, 128
    rng = np.random.RandomState(pw)
    src = rng.randint(0, 256, size=(V.F, ph, pw)).astype(np.uint8)
    # the first prediction is the source inverted, its edge repeated beyond the picture: a cell written from another
    # cell's place, or a byte beyond the picture, would show
    preds = [rng.randint(0, 256, size=(V.F, h, w)).astype(np.uint8) for _ in range(2)]
    preds[0][:] = 255 - np.pad(src, ((0, 0), (0, h - ph), (0, w - pw)), mode="edge")
    want = np.stack([V.cell_dist(src, pw, ph, p) for p in preds]).astype(np.uint32)
    assert want.shape == (2, V.F, 16, 24) and len({int(x) for x in want[0].ravel()}) > 256
    got = D.me_cell_dist(cuda(src)[0], cuda(preds[0]), pw, ph, cuda(*preds))
    assert got.dtype == np.uint32 and np.array_equal(got, want)


@pytest.mark.parametrize("edge", EDGES)
def test_the_cells_legality_holds_at_every_edge(D, edge):
    src, refs = V.border_scene(edge=edge)
    h, w = refs[0].shape[1:]
    rng_, res, lam, lam2, flags, cdec, levels, refine = BORDER_PAR
    par = dict(rng=rng_, res=res, lam=lam, lam_subpel=lam2, cdec=cdec, levels=levels, refine=refine)
    got = run(D, (src, None, refs, None), w, h, 0, 3, flags, PENALTY, par)
    want = border_result(edge)
    same_result(D, got, want, 1, edge)
    name = "mvx" if edge in ("left", "right") else "mvy"
    sign = -1 if edge in ("left", "top") else 1
    sizes = V.point_sizes(want["grid"]["valid"][0])
    uniform = {}

    def alone_at(lg, at):                       # the search at one size alone, under that size's own legality
        if lg not in uniform:
            uniform[lg] = D.me_search3(cuda(src)[0], cuda(*refs), w, h, lg, rng_, res, lam, lam2, flags, None, None, cdec,
                                       levels, refine)[0]
        return int(uniform[lg][name][at])

    # In the middle of the axis, lines 2 and 4: the 8 x 8 search alone takes the vector the mixed grid may not hold.
    # The mixed grid holds a record there at the right and bottom edges, 8 x 8 leaves; at the left and top edges those
    # points are not valid (the leaves round them are larger), and its record on that line is the one at line 0, which
    # it takes from the 32 x 32 search.
    held = 0
    for k in (0, 2, 4):
        at = (0, k, 8) if name == "mvx" else (0, 8, k)
        if k:
            best = alone_at(0, at)
            assert sign*best >= 8*66 and not V.mv_ok_cells(8, best, 3, 16), (k, best)
        if not got[0]["valid"][at]:
            continue
        own = alone_at(sizes[at[2], at[1]], at)
        mine = int(got[0][name][at])
        assert not V.mv_ok_cells(8, own, 3, 16), (k, own)
        assert mine != own and V.mv_ok_cells(8, mine, 3, 16) and mine == (-480 if sign < 0 else 48), (k, mine, own)
        held += 1
    assert held == (1 if sign < 0 else 3)


def test_pipe_search_on_two_rows_of_cells_equals_the_stand_alone_search_and_a_pipe_given_its_grid(D):
    """Scene A in a frame-batch pipe.  A 4:2:0 pipe takes pictures of even sizes only, so the pictures are scene A's
    without their last column and row, 184 x 116 in the same coded 192 x 128."""
    import torch
    size = FRAMES["A_even"][0]
    w, h, pw, ph = size["w"], size["h"], size["pw"], size["ph"]
    planes = frame_scene("A_even")
    want = frame_result("A_even", 0, 3, BOTH, 1, 16)
    for v in want["grid"]["valid"]:             # as in scene A: the second row of cells is worth comparing
        assert v[12, 4::8].any() and not v[12, 4::8].all() and not np.array_equal(v[:9], v[8:])
    src, csrc, refs, crefs = planes
    vbs = (0, 3, 3, 0, 2, 1, BOTH, 1, 1, 16)
    qt = D.QuantTables.load()
    kw = dict(chroma_cfl=True, price=True, inter=True)
    a = D.Pipe(qt, V.F, pw, ph, **kw)
    b = D.Pipe(qt, V.F, pw, ph, **kw)
    try:
        assert (a.W, a.H) == (w, h)
        outs = []
        for p in (a, b):
            p.set_pictures(src, csrc)
            p.set_reference_frames(refs, crefs)
            PM.run_steps(D, p, torch)
        a.set_motion_search_vbs(*vbs)
        a.step()
        a.flush()
        outs.append(PM.drain(a, 1))
        grid, cost = a.read_mvs(want_cost=True)
        same_search((grid, cost), alone(D, planes, vbs, pw, ph), "pipe")
        same_search((grid, cost), (want["grid"], want["cost"]), "pipe against the yardstick")
        assert len({int(x) >> 24 & 3 for leaves in D.mc_leaves(grid, w, h) for x in leaves}) == 4
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
