"""CPU: the yardstick of the motion search at variable block sizes (tests/_me_vbs_ref.py) - that its restated uniform
search is _me_hier_ref's, that its legality predicate is the uniform one where the two must agree and bites where they
differ, that the test content gives decisions worth comparing, that every grid it makes keeps the grid's rule and the
legal range - and the host side of odhip_me_search_vbs: sizes, scratch and refusals before any HIP call."""
import ctypes
import functools

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
    L.odhip_me_vbs_scratch_bytes.restype = ctypes.c_size_t
    j.base.scratch, j.base.scratch_bytes = FAKE, L.odhip_me_vbs_scratch_bytes(ctypes.byref(j))
    for k, v in kw.items():
        setattr(j.base.base.luma if k in ("range", "lambda_", "grid", "res", "nrefs") else j.base if k in (
            "scratch", "scratch_bytes", "refine") else j, k, v)
    return j


def test_sizes_and_scratch(api):
    L = api.lib()
    L.odhip_me_sizeof.restype = ctypes.c_size_t
    L.odhip_me_scratch_bytes.restype = ctypes.c_size_t
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
