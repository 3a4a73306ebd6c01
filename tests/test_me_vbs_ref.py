"""CPU: the yardstick of the motion search at variable block sizes (tests/_me_vbs_ref.py) - that its restated uniform
search is _me_hier_ref's, that its legality predicate is the uniform one where the two must agree and bites where they
differ (at all four edges of a frame), that the test content gives decisions worth comparing (on one row of 64x64 cells
and on frames of several), that every grid it makes keeps the grid's rule and the legal range - and the host side of
odhip_me_search_vbs: sizes, scratch and refusals before any HIP call."""
import ctypes
import functools
import hashlib

import numpy as np
import pytest

import _mc_patterns as P
import _mc_ref as R
import _me_ref as M
import _me_hier_ref as HR
import _me_vbs_ref as V

EINVAL = -10
FAKE = 0x10000
# the standard small job: range 3, 1/8 pel, lambdas 2 and 1, one level, refine 1
PAR = dict(rng=3, res=0, lam=2, lam_subpel=1, cdec=1, levels=1, refine=1)
PENALTY = 16
SIZES = [(0, 3), (1, 3), (0, 1), (2, 3)]


@functools.lru_cache(maxsize=None)
def result(log_min, log_max, flags=0, nslots=2):
    src, csrc, refs, crefs = V.scene(nslots)
    return V.search(src, csrc, V.PW, V.PH, refs, crefs, log_min, log_max, PAR["rng"], PAR["res"], PAR["lam"],
                    PAR["lam_subpel"], flags, PAR["cdec"], PAR["levels"], PAR["refine"], PENALTY)


def test_the_restated_search_is_the_uniform_yardstick():
    src, csrc, refs, crefs = V.scene()
    for lg, flags, levels in ((0, 3, 1), (1, 0, 2), (3, 3, 0)):
        want = HR.search(src, csrc, V.PW, V.PH, refs, crefs, lg, 3, 0, 2, 1, flags, 1, levels, 1)
        nf = src.shape[0]
        got = [V.search_picture((src[f], csrc[f], csrc[nf + f]), V.PW, V.PH,
                                [(r[f], c[f], c[nf + f]) for r, c in zip(refs, crefs)], lg, 3, 0, 2, 1, flags, 1, levels,
                                1, lambda v, mv, n: M.mv_ok(v, mv, lg, n)) for f in range(nf)]
        assert np.array_equal(np.stack([g for g, _ in got]), want[0]), lg
        assert np.array_equal(np.stack([c for _, c in got]), want[1]), lg


def test_the_predicate_is_the_uniform_one_at_the_top_size_and_never_wider():
    for n in (8, 16, 24):
        for lg_top in range(4):
            for v in range(n + 1):
                for mv in list(range(-8*140, 8*140, 37)) + [0, -8*62, -8*62 - 1, 8*61, 8*61 + 1]:
                    cells = V.mv_ok_cells(v, mv, lg_top, n)
                    if v % (1 << lg_top) == 0:
                        assert cells == M.mv_ok(v, mv, lg_top, n), (n, lg_top, v, mv)
                    # whatever smaller leaf inside the cells has the point as a corner is allowed what the cell is
                    for lg in range(lg_top + 1):
                        if cells and v % (1 << lg) == 0:
                            assert M.mv_ok(v, mv, lg, n), (n, lg_top, lg, v, mv)
                assert V.mv_ok_cells(v, 0, lg_top, n)


def test_the_content_gives_decisions_worth_comparing():
    o = result(0, 3)
    sizes = {lg for leaves in o["leaves"] for _, _, lg, _, _ in leaves}
    assert len(sizes) >= 3, sizes
    for lg in (1, 2, 3):
        half = 1 << lg >> 1
        unsplit = sum(l[2] == lg for leaves in o["leaves"] for l in leaves)
        split = sum(int(g["valid"][half::1 << lg, half::1 << lg].sum()) for g in o["grid"])
        assert split and unsplit, (lg, split, unsplit)
    # a decision to split that the grid's rule overrules (a corner on an edge shared with an unsplit neighbour) is there
    # too: the pattern is more than the decisions
    blocked = 0
    for f, g in enumerate(o["grid"]):
        d = {lg: o["cell_dist"][lg][f] for lg in range(4)}
        for lg in (1, 2):
            size, half = 1 << lg, 1 << lg >> 1
            for y in range(0, V.H >> 3, size):
                for x in range(0, V.W >> 3, size):
                    px, py = x & ~(2*size - 1), y & ~(2*size - 1)
                    blocked += bool(g["valid"][py + size, px + size] and V.splits(d, 0, 3, PENALTY, lg, x, y)
                                    and not g["valid"][y + half, x + half])
    assert blocked


@pytest.mark.parametrize("log_min,log_max", SIZES)
def test_every_grid_keeps_the_rule_and_the_legal_range(log_min, log_max):
    o = result(log_min, log_max)
    for f, g in enumerate(o["grid"]):
        assert P.rule_violations(g["valid"]) == []
        assert P.unread_points(g["valid"]) == []
        for dec in (0, 1):
            assert V.check_grid(g, dec, 2) and R.grid_in_range(g, dec)
        assert {l[2] for l in o["leaves"][f]} <= set(range(log_min, log_max + 1))
        assert not g[g["valid"] == 0].tobytes().strip(b"\0") and not o["cost"][f][g["valid"] == 0].any()
    assert o["cell_dist"].shape == (log_max - log_min + 1, V.F, V.H >> 3, V.W >> 3)
    # the picture ends with the last but one row and column of 8x8 cells: the last ones are empty
    assert not o["cell_dist"][:, :, -1, :].any() and not o["cell_dist"][:, :, :, -1].any() and o["cell_dist"].any()


def test_one_size_is_the_uniform_search():
    src, csrc, refs, crefs = V.scene()
    for lg in range(4):
        o = result(lg, lg)
        want = HR.search(src, csrc, V.PW, V.PH, refs, crefs, lg, 3, 0, 2, 1, 0, 1, min(1, lg + 1), 1)
        assert np.array_equal(o["grid"], want[0]) and np.array_equal(o["cost"], want[1])


def test_the_closed_form_of_the_pattern_is_build():
    rng = np.random.RandomState(11)
    for w, h, p in ((128, 64, 0.7), (192, 128, 0.8), (64, 64, 1.0), (128, 128, 0.5)):
        for _ in range(6):
            table = {}

            def split(lg, x, y):
                return table.setdefault((lg, x, y), rng.rand() < p)

            for lg in (3, 2, 1):                # (drawn in a fixed order, whoever asks first)
                for y in range(0, h >> 3, 1 << lg):
                    for x in range(0, w >> 3, 1 << lg):
                        split(lg, x, y)
            want = P.build(w, h, lambda lg, x, y: split(lg, x - (1 << lg >> 1), y - (1 << lg >> 1)),
                           lambda lg, x, y: True)
            assert np.array_equal(V.closed_form_valid(split, w, h), want)


def test_legality_bites():
    src, refs = V.border_scene()
    par = (32, 3, 0, 0, 0, 1, 1, 8)             # range 32 at one level, refine 8, full-pel, no lambda
    small = V.uniform(src, None, V.W, V.H, refs, None, 0, 0, *par)[0]
    mixed = V.uniform(src, None, V.W, V.H, refs, None, 0, 3, *par)[0]
    nh = V.W >> 3
    for vy in (2, 4):
        best = int(small["mvx"][0, vy, 8])
        # the 8x8 search's best vector at x = 64: the block whole in the border, legal there, illegal for a 64-wide leaf
        assert best <= -8*66 and M.mv_ok(8, best, 0, nh) and not V.mv_ok_cells(8, best, 3, nh)
        got = int(mixed["mvx"][0, vy, 8])
        assert got != best and V.mv_ok_cells(8, got, 3, nh) and got < 0
        # ... and one point further right the two agree: that point belongs to the second cell alone
        assert small["mvx"][0, vy, 9] == mixed["mvx"][0, vy, 9]
    # the search as a whole stays in range with 64-wide leaves on its points, which the 8x8 search's vectors do not
    wide = small.copy()
    wide["valid"] = 0
    wide["valid"][:, ::8, ::8] = 1
    assert not R.grid_in_range(wide[0], 0)
    wide = mixed.copy()
    wide["valid"] = 0
    wide["valid"][:, ::8, ::8] = 1
    assert R.grid_in_range(wide[0], 0) and R.grid_in_range(wide[0], 1)


# ---- frames of more than one row of 64x64 cells (tests/test_gpu_me_vbs_frames.py runs them on the GPU) ----
# name: the scene's sizes and patches, and the search: log_min, log_max, flags, levels, penalty
PATCHES_A = ((0, 70, 60, 50, 44, 5, -4), (1, 20, 70, 90, 40, -6, 3), (0, 130, 10, 40, 100, 3, 4), (1, 100, 20, 30, 30, 4, 4))
FRAMES = {
    # three cells across and two down: 384 8x8 cells and 425 points, more than a workgroup of either
    "A": (dict(w=192, h=128, pw=185, ph=117, patches=PATCHES_A),
          ((0, 3, 0, 1, PENALTY), (0, 3, 3, 1, PENALTY), (1, 2, 0, 2, 0))),
    # scene A one column and one row shorter, for the pipe: at 4:2:0 it takes pictures of even sizes only
    "A_even": (dict(w=192, h=128, pw=184, ph=116, patches=PATCHES_A), ((0, 3, 3, 1, PENALTY),)),
    # one cell across and three down; at two levels the 8x8 search has one and the larger sizes two
    "B": (dict(w=64, h=192, pw=61, ph=181, patches=((0, 10, 60, 40, 44, 5, -4), (1, 20, 100, 30, 60, -6, 3),
                                                    (0, 30, 140, 20, 30, 3, 4))),
          ((0, 3, 3, 2, PENALTY),)),
}
EDGES = ("left", "right", "top", "bottom")
BORDER_PAR = (32, 3, 0, 0, 0, 1, 1, 8)          # range 32 at one level, refine 8, full-pel, no lambda


@functools.lru_cache(maxsize=None)
def frame_scene(name):
    return V.scene(2, 4, **FRAMES[name][0])


@functools.lru_cache(maxsize=None)
def frame_result(name, log_min, log_max, flags, levels, penalty):
    assert (log_min, log_max, flags, levels, penalty) in FRAMES[name][1]       # the yardstick is slow: these and no more
    size = FRAMES[name][0]
    src, csrc, refs, crefs = frame_scene(name)
    return V.search(src, csrc, size["pw"], size["ph"], refs, crefs, log_min, log_max, PAR["rng"], PAR["res"], PAR["lam"],
                    PAR["lam_subpel"], flags, PAR["cdec"], levels, PAR["refine"], penalty)


@functools.lru_cache(maxsize=None)
def border_uniform(edge, log_max):
    """The 8x8 search of border_scene(edge=edge) under the legality of leaves of 8 << log_max: (G, C)."""
    src, refs = V.border_scene(edge=edge)
    h, w = refs[0].shape[1:]
    return V.uniform(src, None, w, h, refs, None, 0, log_max, *BORDER_PAR)


@functools.lru_cache(maxsize=None)
def border_result(edge):
    src, refs = V.border_scene(edge=edge)
    h, w = refs[0].shape[1:]
    return V.search(src, None, w, h, refs, None, 0, 3, *BORDER_PAR, PENALTY, uni={0: border_uniform(edge, 3)})


def overruled(o, f, w, h, penalty, first_row=0):
    """How many decisions to split of picture f, in rows of 8x8 cells from first_row on, the grid's rule overrules."""
    g = o["grid"][f]
    d = {lg: o["cell_dist"][lg][f] for lg in range(4)}
    n = 0
    for lg in (1, 2):
        size, half = 1 << lg, 1 << lg >> 1
        for y in range(first_row, h >> 3, size):
            for x in range(0, w >> 3, size):
                px, py = x & ~(2*size - 1), y & ~(2*size - 1)
                n += bool(g["valid"][py + size, px + size] and V.splits(d, 0, 3, penalty, lg, x, y)
                          and not g["valid"][y + half, x + half])
    return n


def test_scene_a_gives_rows_of_cells_worth_comparing():
    o = frame_result("A", 0, 3, 0, 1, PENALTY)
    valid = [g["valid"] for g in o["grid"]]
    assert valid[0].shape == (17, 25)
    for f, v in enumerate(valid):
        assert P.rule_violations(v) == [] and P.unread_points(v) == []
        # (a) a split and an unsplit 64x64 cell below the first row of cells
        assert v[12, 4::8].any() and not v[12, 4::8].all(), f
        # (d) the two rows of cells differ, so a row of decision words taken for another shows
        assert not np.array_equal(v[:9], v[8:]), f
        # (e) leaves of all four sizes
        assert {l[2] for l in o["leaves"][f]} == {0, 1, 2, 3}, f
    assert not np.array_equal(valid[0], valid[1])                                  # (d) nor are the pictures alike
    # (b) over both pictures a valid and an invalid midpoint on a horizontal 64x64 edge inside the frame, and on a
    # vertical one
    across = np.concatenate([v[8, 4::8] for v in valid])
    down = np.concatenate([v[4::8, 8:-1:8].ravel() for v in valid])
    assert across.any() and not across.all() and down.any() and not down.all()
    # (c) decisions to split below the first row of cells that the rule overrules (3 and 10 of them)
    assert sum(overruled(o, f, 192, 128, PENALTY, 8) for f in (0, 1)) >= 1
    # as tried: the picture ends inside the last column and row of cells, and these are the patterns
    assert [v[4::8, 4::8].tolist() for v in valid] == [[[1, 1, 1], [0, 1, 1]], [[1, 0, 0], [1, 1, 0]]]
    assert [v[8, 4::8].tolist() for v in valid] == [[0, 1, 1], [1, 0, 0]]
    assert o["cell_dist"][:, :, 14, :].any() and o["cell_dist"][:, :, :, 23].any()
    assert not o["cell_dist"][:, :, 15, :].any()


def test_scene_b_gives_a_column_of_cells_worth_comparing():
    o = frame_result("B", 0, 3, 3, 2, PENALTY)
    valid = [g["valid"] for g in o["grid"]]
    assert valid[0].shape == (25, 9)
    for v in valid:
        assert P.rule_violations(v) == [] and P.unread_points(v) == []
    # (b) a valid and an invalid midpoint on a horizontal 64x64 edge inside the frame
    across = np.concatenate([v[8:-1:8, 4] for v in valid])
    assert across.any() and not across.all()
    # (c) decisions to split below the first row of cells that the rule overrules
    assert sum(overruled(o, f, 64, 192, PENALTY, 8) for f in (0, 1)) >= 1
    # the middle cell splits in both pictures, between two unsplit cells in one and two split ones in the other: on
    # either side it has met a neighbour of either kind
    split = np.array([v[4::8, 4] for v in valid])
    assert split[:, 1].all()
    for side in (0, 2):
        assert split[:, side].any() and not split[:, side].all(), side
    # as tried: picture 0 splits the middle cell only, picture 1 all three down to 8x8
    assert split.tolist() == [[0, 1, 0], [1, 1, 1]]
    assert [sorted({l[2] for l in leaves}) for leaves in o["leaves"]] == [[2, 3], [0, 1, 2]]
    assert across.tolist() == [0, 0, 1, 1]


@pytest.mark.parametrize("edge", EDGES)
def test_legality_bites_at_every_edge(edge):
    """test_legality_bites on the axis across `edge`, at the point in the middle of that axis - a multiple of the top
    size with a cell on both sides - in rows (columns) 2 and 4 of the other axis."""
    src, refs = V.border_scene(edge=edge)
    h, w = refs[0].shape[1:]
    assert (w, h) == ((128, 64) if edge in ("left", "right") else (64, 128)) and src.shape == (1, h, w)
    small = border_uniform(edge, 0)[0]
    mixed = border_uniform(edge, 3)[0]
    name = "mvx" if edge in ("left", "right") else "mvy"
    sign = -1 if edge in ("left", "top") else 1
    n = 16

    def at(g, v, k):                            # the component across the edge at step v of that axis, line k
        return int(g[name][0, k, v] if name == "mvx" else g[name][0, v, k])

    for k in (2, 4):
        best = at(small, 8, k)
        # the 8x8 search's best vector: the block whole in the border, legal there, illegal for a 64-wide leaf
        assert sign*best >= 8*66 and M.mv_ok(8, best, 0, n) and not V.mv_ok_cells(8, best, 3, n)
        got = at(mixed, 8, k)
        assert got != best and V.mv_ok_cells(8, got, 3, n) and sign*got > 0
        assert (best, got) == ((-528, -480) if sign < 0 else (528, 48))
        # ... and one point further from the edge the two agree: that point belongs to the far cell alone
        assert at(small, 8 - sign, k) == at(mixed, 8 - sign, k)
    # the search as a whole stays in range with 64-wide leaves on its points, which the 8x8 search's vectors do not
    wide = small.copy()
    wide["valid"] = 0
    wide["valid"][:, ::8, ::8] = 1
    assert not R.grid_in_range(wide[0], 0)
    wide = mixed.copy()
    wide["valid"] = 0
    wide["valid"][:, ::8, ::8] = 1
    assert R.grid_in_range(wide[0], 0) and R.grid_in_range(wide[0], 1)


def test_the_sized_scenes_are_the_old_ones_by_default():
    def digest(scene):
        h = hashlib.sha1()
        for part in scene:
            for a in (part if isinstance(part, list) else [part]):
                h.update(a.tobytes())
                h.update(str(a.shape).encode())
        return h.hexdigest()

    # recorded before the scenes took sizes
    assert digest(V.scene()) == "f5766018b2a109f3332a446abacb798055124fe1"
    assert digest(V.scene(3)) == "01b880fd35720c3f2f3a9484932b95e53b14cdf0"
    assert digest(V.scene(seed=5)) == "b626de5c3a9bc338b4b4bd2e690d06768851fdad"
    assert digest(V.border_scene()) == "62f598c3971fa7d22264271c256091e94a0726db"
    for a, b in ((V.scene(), V.scene(2, 4, V.PATCHES, V.W, V.H, V.PW, V.PH)),
                 (V.border_scene(), V.border_scene(9, "left", V.W, V.H, V.W, V.H))):
        for x, y in zip(a, b):
            assert np.array_equal(np.stack(x), np.stack(y))
    src, refs = V.border_scene()
    right, top, bottom = (V.border_scene(edge=e) for e in ("right", "top", "bottom"))
    assert np.array_equal(right[1][0], refs[0][:, :, ::-1]) and np.array_equal(right[0], src[:, :, ::-1])
    assert np.array_equal(top[1][0][0], refs[0][0].T) and np.array_equal(top[0][0], src[0].T)
    assert np.array_equal(bottom[1][0][0], right[1][0][0].T) and np.array_equal(bottom[0][0], right[0][0].T)


# ---- the host side of the library ----
@pytest.fixture(scope="module")
def api():
    from daala_amd import build
    build.build()
    import daala_amd
    return daala_amd


def job4(D, log_min=0, log_max=3, penalty=PENALTY, levels=1, **kw):
    refs = (ctypes.c_void_p * 3)(FAKE, FAKE, None)
    luma = D.MeJob(V.W, V.H, V.PW, V.PH, V.F, 2, log_max, 3, 0, 2, V.PW, V.W, V.PW*V.PH, V.W*V.H, FAKE, refs, FAKE, FAKE)
    j3 = D.MeJob3(base=D.MeJob2(luma=luma, lambda_subpel=1), levels=levels, refine=1)
    j = D.MeJob4(base=j3, log_min=log_min, split_penalty=penalty)
    L = D.lib()
    j.base.scratch, j.base.scratch_bytes = FAKE, L.odhip_me_vbs_scratch_bytes(ctypes.byref(j))
    for k, v in kw.items():
        setattr(j.base.base.luma if k in ("range", "lambda_", "grid", "res", "nrefs") else j.base if k in (
            "scratch", "scratch_bytes", "refine") else j, k, v)
    return j


def test_sizes_and_scratch(api):
    L = api.lib()
    assert L.odhip_me_sizeof(5) == ctypes.sizeof(api.MeJob4) == ctypes.sizeof(api.MeJob3) + 16
    assert L.odhip_me_sizeof(3) == 0 and L.odhip_me_sizeof(6) == 0
    points, frame, cells = V.F*(V.H//8 + 1)*(V.W//8 + 1), V.F*V.H*V.W, V.F*(V.H//8)*(V.W//8)
    for log_min, log_max in SIZES:
        n = log_max - log_min + 1
        j = job4(api, log_min, log_max)
        # per size a grid, its costs and a prediction; the d arrays; and room for the search's own scratch
        assert j.base.scratch_bytes >= n*(points*16 + frame) + n*cells*4
    # one size: the uniform search's scratch
    for lg in range(4):
        j = job4(api, lg, lg)
        assert j.base.scratch_bytes == L.odhip_me_scratch_bytes(ctypes.byref(j.base)) > 0
    assert L.odhip_me_vbs_scratch_bytes(None) == 0
    assert L.odhip_me_vbs_scratch_bytes(ctypes.byref(job4(api, log_min=2, log_max=1))) == 0


def test_bad_jobs_are_refused_on_the_host(api):
    L = api.lib()

    def search(j):
        return L.odhip_me_search_vbs(ctypes.byref(j), None)

    assert L.odhip_me_search_vbs(None, None) == EINVAL
    for kw in (dict(log_min=-1), dict(log_min=2, log_max=1), dict(log_max=4), dict(penalty=-1),
               dict(penalty=(1 << 24) + 1), dict(scratch=None), dict(levels=3), dict(levels=-1), dict(range=33),
               dict(range=-1), dict(res=4), dict(lambda_=(1 << 19) + 1), dict(refine=0), dict(refine=9), dict(grid=None),
               dict(nrefs=4), dict(split_penalty=1 << 25)):
        assert search(job4(api, **kw)) == EINVAL, kw
    j = job4(api)
    j.base.scratch_bytes -= 1
    assert search(j) == EINVAL
    j = job4(api)
    j.base.base.lambda_subpel = (1 << 19) + 1
    assert search(j) == EINVAL
    # the levels are the largest size's to refuse: two are too many for 8x8 blocks alone
    assert search(job4(api, 0, 0, levels=2)) == EINVAL
    assert api.lib().odhip_pipe_set_motion_search_vbs(None, 0, 3, 3, 0, 2, 1, 0, 1, 1, PENALTY) == EINVAL
