"""CPU: the coarse-to-fine motion search's yardstick (tests/_me_hier_ref.py) against the functions that are pinned
to the compiled reference (_me_cost_ref.plane_dist, _me_cost_ref.search), a planted displacement beyond the
exhaustive search's reach, and odhip_me_search3 / odhip_me_costs3 / odhip_me_scratch_bytes refusing bad jobs on the
host, before any HIP call (there is no GPU here).  Every comparison is exact integer equality."""
import ctypes
import functools

import numpy as np
import pytest

import _me_cost_ref as C
import _me_hier_ref as HR
import _me_ref as M
from test_gpu_me_cost import planes, PICS
from test_me_cost_host import job2, FAKE, W, H, F

EINVAL = -10


def test_halve_on_a_hand_written_plane():
    p = np.array([[0, 1, 2, 3, 255],
                  [4, 5, 6, 8, 255],
                  [10, 20, 30, 41, 7]], np.uint8)
    # the odd last column and row are replicated: (255 + 255 + 255 + 255 + 2) >> 2, (10 + 20 + 10 + 20 + 2) >> 2 ..
    want = np.array([[(0 + 1 + 4 + 5 + 2) >> 2, (2 + 3 + 6 + 8 + 2) >> 2, 255],
                     [(10 + 20 + 10 + 20 + 2) >> 2, (30 + 41 + 30 + 41 + 2) >> 2, 7]], np.uint8)
    assert want.tolist() == [[3, 5, 255], [15, 36, 7]]
    got = HR.halve(p)
    assert got.dtype == np.uint8 and got.tolist() == want.tolist()
    pyr = HR.pyramid(p, 2)
    assert [a.shape for a in pyr] == [(3, 5), (2, 3), (1, 2)]
    # level 2 rounds twice
    assert pyr[2].tolist() == [[(3 + 5 + 15 + 36 + 2) >> 2, (255 + 255 + 7 + 7 + 2) >> 2]]


@pytest.mark.parametrize("level", [1, 2])
def test_level_sads_equal_plane_dist_at_that_decimation(level):
    src, _, refs, _ = planes(1, 1)
    pw, ph = PICS[1]                       # 119 x 55: the levels' picture sizes round up
    rng = np.random.RandomState(40 + level)
    seen = dict(clipped=0, empty=0, edge=0, whole=0)
    for lg in range(max(level - 1, 0), 4):
        s = 1 << lg
        xs, ys = list(range(0, W//8 + 1, s)), list(range(0, H//8 + 1, s))
        pts = [(xs[0], ys[0]), (xs[-1], ys[-1]), (xs[0], ys[-1]), (xs[-1], ys[0])]
        pts += [(xs[rng.randint(len(xs))], ys[rng.randint(len(ys))]) for _ in range(6)]
        for vx, vy in pts:
            f, slot = rng.randint(F), rng.randint(2)
            sl, rl = HR.pyramid(src[f], level)[level], HR.pyramid(refs[slot][f], level)[level]
            assert sl.shape == (C.plane_sz(ph, level), C.plane_sz(pw, level))
            cx, cy, rad = 2*rng.randint(-9, 10), 2*rng.randint(-9, 10), 2
            got = HR.level_sads(sl, pw, ph, rl, vx, vy, lg, level, cx, cy, rad)
            step = 8 << level
            for dy in range(-rad, rad + 1):
                for dx in range(-rad, rad + 1):
                    want = C.plane_dist(sl, pw, ph, rl, vx, vy, lg, step*(cx + dx), step*(cy + dy), level, C.SAD_METRIC)
                    assert got[dy + rad, dx + rad] == want, (lg, vx, vy, cx, cy, dx, dy)
            c = C.plane_clip(vx, vy, lg, level, pw, ph)
            n = 8 << lg >> level
            seen["empty"] += c is None
            seen["edge"] += vx in (xs[0], xs[-1]) or vy in (ys[0], ys[-1])
            if c is not None:
                whole = (c[1] - c[0], c[3] - c[2]) == (n, n)
                seen["whole"] += whole
                seen["clipped"] += not whole
    assert all(seen.values()), seen


@pytest.mark.parametrize("flags", [0, 1, 2, 3], ids=["none", "chroma", "satd", "both"])
def test_no_levels_is_the_exhaustive_search(flags):
    src, csrc, refs, crefs = planes(1, 0)
    pw, ph = PICS[0]
    want = C.search(src, csrc, pw, ph, refs, crefs, 2, 3, 0, 5, 3, flags, 1)
    got = HR.search(src, csrc, pw, ph, refs, crefs, 2, 3, 0, 5, 3, flags, 1, 0, 2)
    assert got[0].tobytes() == want[0].tobytes() and np.array_equal(got[1], want[1])


@functools.lru_cache(maxsize=None)
def planted_search():
    src, refs, mv, pts = HR.planted()
    return HR.search(src, None, 250, 180, refs, None, 2, 20, 3, 3, 3, 0, 0, 2, 2)


def test_a_planted_displacement_beyond_the_exhaustive_reach_is_found():
    src, refs, mv, pts = HR.planted()
    assert len(pts) == 20
    grid, cost = planted_search()
    for vx, vy in pts:
        pt = grid[0, vy, vx]
        assert (int(pt["mvx"]), int(pt["mvy"]), int(pt["ref"])) == (mv[0], mv[1], 1), (vx, vy, pt)
        assert cost[0, vy, vx] == 3*(abs(mv[0]) + abs(mv[1]))
    # the exhaustive search at its widest never gets there
    wide, _ = M.search(src, 250, 180, refs, 2, 32, 3, 3)
    assert not np.any((wide["mvx"] == mv[0]) & (wide["mvy"] == mv[1]))
    assert np.abs(wide["mvx"]).max() <= 256 and np.abs(wide["mvy"]).max() <= 256


# ---- through the ABI, without a GPU ----
@pytest.fixture(scope="module")
def api():
    from daala_amd import build
    build.build()
    import daala_amd
    return daala_amd


def job3(D, levels=2, refine=2, scratch=FAKE, scratch_bytes=None, **kw):
    L = D.lib()
    j = D.MeJob3(base=job2(D, **kw), levels=levels, refine=refine)
    j.scratch = scratch
    j.scratch_bytes = L.odhip_me_scratch_bytes(ctypes.byref(j)) if scratch_bytes is None else scratch_bytes
    return j


def test_sizeof_and_scratch_bytes(api):
    L = api.lib()
    # (what = 3 stays 0: tests/test_me_cost_host.py pins it)
    assert L.odhip_me_sizeof(4) == ctypes.sizeof(api.MeJob3) == ctypes.sizeof(api.MeJob2) + 24
    assert L.odhip_me_scratch_bytes(ctypes.byref(job3(api, levels=0))) == 0
    assert L.odhip_me_scratch_bytes(None) == 0
    one = L.odhip_me_scratch_bytes(ctypes.byref(job3(api, levels=1)))
    two = L.odhip_me_scratch_bytes(ctypes.byref(job3(api, levels=2)))
    # at least the pyramids' samples: the source picture's and two slots' levels, F pictures each
    lv1 = 60*28 + 2*64*32
    assert one >= F*lv1 and two >= one + F*(30*14 + 2*32*16) and two > one > 0


def test_bad_jobs_are_refused_on_the_host(api):
    L = api.lib()

    def search(j):
        return L.odhip_me_search3(ctypes.byref(j), None)

    def costs(j, n=1, c=FAKE, out=FAKE, level=0):
        return L.odhip_me_costs3(ctypes.byref(j), ctypes.c_void_p(c), ctypes.c_long(n), level, ctypes.c_void_p(out), None)

    need = L.odhip_me_scratch_bytes(ctypes.byref(job3(api)))
    # levels outside 0 .. min(2, log_size + 1), missing or short scratch
    for kw in (dict(levels=-1), dict(levels=3), dict(levels=2, luma_log_size=0), dict(scratch=None),
               dict(scratch_bytes=need - 1), dict(scratch_bytes=0)):
        assert search(job3(api, **kw)) == EINVAL, kw
        assert costs(job3(api, **kw)) == EINVAL, kw
    # refine and the lambda bound, with levels > 0 only
    for kw in (dict(refine=0), dict(refine=9), dict(refine=-1), dict(luma_lambda_=(1 << 19) + 1),
               dict(lambda_subpel=(1 << 19) + 1)):
        assert search(job3(api, **kw)) == EINVAL, kw
        assert search(job3(api, levels=1, **kw)) == EINVAL, kw
    # everything odhip_me_search2 refuses, at every number of levels
    no_cref1 = (ctypes.c_void_p * 3)(FAKE, None, None)
    for levels in (0, 1, 2):
        for kw in (dict(flags=4), dict(cdec=2), dict(lambda_subpel=-1), dict(lambda_subpel=(1 << 20) + 1),
                   dict(csrc=None), dict(cref=no_cref1), dict(csrc_stride=1), dict(luma_coded_w=120),
                   dict(luma_pic_w=W + 1), dict(luma_npics=0), dict(luma_nrefs=4), dict(luma_log_size=4),
                   dict(luma_src_stride=1), dict(luma_ref_plane_stride=W*H - 1), dict(luma_src=None),
                   dict(luma_range=-1), dict(luma_range=33), dict(luma_res=4), dict(luma_lambda_=-1),
                   dict(luma_lambda_=(1 << 20) + 1), dict(luma_grid=None)):
            assert search(job3(api, levels=levels, **kw)) == EINVAL, (levels, kw)
    assert search(job3(api, levels=0, luma_lambda_=(1 << 20) + 1)) == EINVAL
    assert L.odhip_me_search3(None, None) == EINVAL
    assert L.odhip_me_costs3(None, None, ctypes.c_long(0), 0, None, None) == EINVAL
    assert costs(job3(api), c=None) == EINVAL and costs(job3(api), out=None) == EINVAL and costs(job3(api), n=-1) == EINVAL
    assert costs(job3(api), level=3) == EINVAL and costs(job3(api), level=-1) == EINVAL
    assert costs(job3(api, levels=1), level=2) == EINVAL
    # the halving refuses on the host too
    ds = L.odhip_me_downsample
    ds.argtypes = [ctypes.c_void_p, ctypes.c_int, ctypes.c_int64, ctypes.c_void_p, ctypes.c_int, ctypes.c_int64,
                   ctypes.c_int, ctypes.c_int, ctypes.c_int, ctypes.c_void_p]
    for args in ((None, 3, 6, FAKE, 5, 15, 5, 3, 1), (FAKE, 3, 6, None, 5, 15, 5, 3, 1), (FAKE, 2, 6, FAKE, 5, 15, 5, 3, 1),
                 (FAKE, 3, 5, FAKE, 5, 15, 5, 3, 1), (FAKE, 3, 6, FAKE, 4, 15, 5, 3, 1), (FAKE, 3, 6, FAKE, 5, 14, 5, 3, 1),
                 (FAKE, 3, 6, FAKE, 5, 15, 0, 3, 1), (FAKE, 3, 6, FAKE, 5, 15, 5, 0, 1), (FAKE, 3, 6, FAKE, 5, 15, 5, 3, 0)):
        assert ds(*args, None) == EINVAL, args


def test_the_pipe_entry_point_refuses_without_a_pipe(api):
    assert api.lib().odhip_pipe_set_motion_search3(None, 1, 3, 0, 0, 0, 0, 1, 2) == EINVAL
