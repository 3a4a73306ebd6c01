"""GPU: the motion searches of me_kernels.hip (odhip_me_search / _search2 / _search3 and their test surfaces
odhip_me_costs / _costs2 / _costs3, odhip_me_downsample) at the extremes the other search tests leave out, against the
numpy yardsticks tests/_me_ref.py, _me_cost_ref.py and _me_hier_ref.py.  Every comparison is exact integer equality.

  saturated blocks   0 against 255, flat and as a checkerboard of period 1: the packed 16-bit sums of slide_sad hold
                     exactly 64 quad SADs of such samples, and the Hadamard path sees full-range differences
  slots, pictures    three slots with different content and three pictures, one slot and one picture
  tiny pictures      1 x 1, 9 x 5 and 5 x 9 in a 64 x 64 coded frame: byte paths, empty blocks, levels of 1 to 3 samples
  the largest lambdas  2^20 (odhip_me_search2) and 2^19 (odhip_me_search3) at range 32: the cost stays inside int32

A yardstick result is computed once per set of parameters and shared (functools.lru_cache)."""
import functools

import numpy as np
import pytest

import _me_cost_ref as C
import _me_hier_ref as HR
import _me_ref as M
from test_gpu_me import cuda, same_search, check_shape, chroma_of

pytestmark = pytest.mark.gpu

CHROMA_SATD = C.CHROMA | C.SATD


@pytest.fixture(scope="module")
def D():
    import torch
    import daala_amd
    assert torch.cuda.is_available()
    daala_amd.init(0)
    return daala_amd


# ---- content: name -> (src [F][ph][pw], {cdec: csrc [2F][..]}, refs per slot [F][H][W], {cdec: crefs per slot}) ----
SETS = {}


def planes_of(name):
    if name not in SETS:
        kind, arg = name.split(":")
        SETS[name] = {"flat": saturated, "checker": saturated, "scene": scene, "tiny": tiny}[kind](kind, arg)
    return SETS[name]


def size_of(arg):
    return tuple(int(v) for v in arg.split("x"))


def saturated(kind, arg):
    """One picture of arg = "pw x ph" in a 64 x 64 coded frame, two slots.  flat: the picture 0, the slots 255;
    checker: a 0 / 255 checkerboard of period 1 against its inverse.  Every plane alike."""
    pw, ph = size_of(arg)

    def pair(h, w, hp, wp):
        y, x = np.mgrid[0:h, 0:w]
        board = (((x + y) & 1)*255 if kind == "checker" else np.zeros((h, w))).astype(np.uint8)
        return board[:hp, :wp], 255 - board

    src, ref = pair(64, 64, ph, pw)
    csrc, crefs = {}, {}
    for cdec in (0, 1):
        s, r = pair(64 >> cdec, 64 >> cdec, C.plane_sz(ph, cdec), C.plane_sz(pw, cdec))
        csrc[cdec], crefs[cdec] = np.stack([s, s]), [np.stack([r, r])]*2
    return np.ascontiguousarray(src[None]), csrc, [ref[None], ref[None].copy()], crefs


W2, H2, PW2, PH2 = 128, 64, 119, 55
SHIFTS = ((2, -1), (-3, 2), (1, 3))


def scene(kind, arg):
    """arg = "F x slots" of three pictures and three slots, coded 128 x 64, pictures 119 x 55.  Per picture one scene
    of smoothed noise as test_gpu_me.content builds it; every slot holds a cut of it, each displaced its own way, with
    little noise in the slot of the picture's number (the planted best slot) and more in the others."""
    nf, ns = size_of(arg)
    rng = np.random.RandomState(11)
    src, refs = [], [[] for _ in range(3)]
    for f in range(3):
        big = M.smooth_noise(rng, H2 + 32, W2 + 32)

        def cut(dx, dy, noise):
            p = big[16 + dy:16 + dy + H2, 16 + dx:16 + dx + W2].astype(int) + rng.randint(-noise, noise + 1,
                                                                                          size=(H2, W2))
            return np.clip(p, 0, 255).astype(np.uint8)

        src.append(cut(0, 0, 0)[:PH2, :PW2])
        for s in range(3):
            refs[s].append(cut(SHIFTS[s][0], SHIFTS[s][1], 2 if s == f else 9))
    src = np.ascontiguousarray(np.stack(src)[:nf])
    refs = [np.ascontiguousarray(np.stack(r)[:nf]) for r in refs[:ns]]
    csrc, crefs = {}, {}
    for cdec in (0, 1):
        csrc[cdec] = np.ascontiguousarray(chroma_of(src, cdec, 7))
        crefs[cdec] = [np.roll(chroma_of(r, cdec, 8 + i), (i, 1 - i), axis=(1, 2)) for i, r in enumerate(refs)]
    return src, csrc, refs, crefs


def tiny(kind, arg):
    """Two pictures of arg = "pw x ph" in a 64 x 64 coded frame, two slots, random full-range samples everywhere."""
    pw, ph = size_of(arg)
    rng = np.random.RandomState(100*pw + ph)
    src = rng.randint(0, 256, size=(2, ph, pw)).astype(np.uint8)
    refs = [rng.randint(0, 256, size=(2, 64, 64)).astype(np.uint8) for _ in range(2)]
    csrc, crefs = {}, {}
    for cdec in (0, 1):
        csrc[cdec] = rng.randint(0, 256, size=(4, C.plane_sz(ph, cdec), C.plane_sz(pw, cdec))).astype(np.uint8)
        crefs[cdec] = [rng.randint(0, 256, size=(4, 64 >> cdec, 64 >> cdec)).astype(np.uint8) for _ in range(2)]
    return src, csrc, refs, crefs


def pic_size(name):
    src = planes_of(name)[0]
    return src.shape[2], src.shape[1]


# ---- the yardsticks, once per set of parameters ----
@functools.lru_cache(maxsize=None)
def yard1(name, lg, rng_, res, lam):
    src, _, refs, _ = planes_of(name)
    return M.search(src, *pic_size(name), refs, lg, rng_, res, lam)


@functools.lru_cache(maxsize=None)
def yard2(name, lg, rng_, res, lam, lam2, flags, cdec):
    src, csrc, refs, crefs = planes_of(name)
    return C.search(src, csrc[cdec], *pic_size(name), refs, crefs[cdec], lg, rng_, res, lam, lam2, flags, cdec)


@functools.lru_cache(maxsize=None)
def yard3(name, lg, rng_, res, lam, lam2, flags, cdec, levels, refine):
    src, csrc, refs, crefs = planes_of(name)
    return HR.search(src, csrc[cdec], *pic_size(name), refs, crefs[cdec], lg, rng_, res, lam, lam2, flags, cdec,
                     levels, refine)


def run1(D, name, lg, rng_, res, lam):
    src, _, refs, _ = planes_of(name)
    got = D.me_search(cuda(src)[0], cuda(*refs), *pic_size(name), lg, rng_, res, lam)
    same_search(got, yard1(name, lg, rng_, res, lam), ("search", name, lg, rng_, res, lam))
    return got


def run2(D, name, lg, rng_, res, lam, lam2, flags, cdec):
    src, csrc, refs, crefs = planes_of(name)
    got = D.me_search2(cuda(src)[0], cuda(*refs), *pic_size(name), lg, rng_, res, lam, lam2, flags,
                       cuda(csrc[cdec])[0], cuda(*crefs[cdec]), cdec)
    same_search(got, yard2(name, lg, rng_, res, lam, lam2, flags, cdec),
                ("search2", name, lg, rng_, res, lam, lam2, flags, cdec))
    return got


def run3(D, name, lg, rng_, res, lam, lam2, flags, cdec, levels, refine):
    src, csrc, refs, crefs = planes_of(name)
    got = D.me_search3(cuda(src)[0], cuda(*refs), *pic_size(name), lg, rng_, res, lam, lam2, flags,
                       cuda(csrc[cdec])[0], cuda(*crefs[cdec]), cdec, levels, refine)
    same_search(got, yard3(name, lg, rng_, res, lam, lam2, flags, cdec, levels, refine),
                ("search3", name, lg, rng_, res, lam, lam2, flags, cdec, levels, refine))
    return got


def most_levels(lg):
    return min(2, lg + 1)


# ---- 1. saturated blocks ----
def flat_dist(vx, vy, lg, pw, ph, dec, metric):
    """A plane's distortion where every difference inside the clipped block is +-255 and, under SATD, the block of
    differences is flat or a checkerboard - one Hadamard coefficient holds it all: 16 * 255 at 4 x 4, 64 * 255 per
    8 x 8 tile."""
    c = C.plane_clip(vx, vy, lg, dec, pw, ph)
    if c is None:
        return 0
    w, h = c[1] - c[0], c[3] - c[2]
    if metric == C.SATD_METRIC and w == h == 4:
        return (16*255 + 2) >> 2
    if metric == C.SATD_METRIC and w == h and w in (8, 16, 32, 64):
        return (w//8)**2*((64*255 + 4) >> 3)
    return 255*w*h


def flat_cost(vx, vy, lg, pw, ph, cdec, metric, chroma):
    d = flat_dist(vx, vy, lg, pw, ph, 0, metric)
    if chroma:
        d += 2*(flat_dist(vx, vy, lg, pw, ph, cdec, metric) >> 2)
    return 8*d


SAT_PICS = ("64x64", "61x63")


# res 0: stage 2 costs the winner again, under SATD where flagged - the Hadamard path at full-range differences; res 3:
# the cost is stage 1's own, the sums of slide_sad - only blocks of 32 and 64 samples hold more than 64 quad SADs a lane
SAT_RUNS = [(lg, 0) for lg in range(4)] + [(2, 3), (3, 3)]


@pytest.mark.parametrize("which", ["plain", "420", "444", "hier"])
@pytest.mark.parametrize("lg,res", SAT_RUNS)
@pytest.mark.parametrize("pic", SAT_PICS)
@pytest.mark.parametrize("kind", ["flat", "checker"])
def test_saturated_searches_equal_the_yardstick(D, kind, pic, lg, res, which):
    """Range 32: a lane's packed sums run to the flush, whole groups of four columns (64 x 64) and a partial byte mask
    beside them (61 x 63).  plain: odhip_me_search; 420 / 444: odhip_me_search2 with chroma and SATD; hier:
    odhip_me_search3 at the most levels the size allows and refine 8, without flags on the whole picture and with both
    at 4:2:0 on the cut one.  Flat content ties everywhere: the zero vector in slot 0 at the closed-form cost."""
    name = kind + ":" + pic
    pw, ph = pic_size(name)
    lam, lam2 = ((0, 0), (5, 3))[SAT_PICS.index(pic)]
    flags, cdec = {"plain": (0, 0), "420": (CHROMA_SATD, 1), "444": (CHROMA_SATD, 0),
                   "hier": ((0, 0), (CHROMA_SATD, 1))[SAT_PICS.index(pic)]}[which]
    if which == "plain":
        grid, cost = run1(D, name, lg, 32, res, lam)
    elif which == "hier":
        grid, cost = run3(D, name, lg, 32, res, lam, lam2, flags, cdec, most_levels(lg), 8)
    else:
        grid, cost = run2(D, name, lg, 32, res, lam, lam2, flags, cdec)
    check_shape(D, grid, cost, lg, 64, 64)
    if kind == "flat":
        metric = C.SATD_METRIC if flags & C.SATD and res < 3 else C.SAD_METRIC
        assert not grid["mvx"].any() and not grid["mvy"].any() and not grid["ref"].any()
        for vy in range(0, 9, 1 << lg):
            for vx in range(0, 9, 1 << lg):
                assert cost[0, vy, vx] == flat_cost(vx, vy, lg, pw, ph, cdec, metric, bool(flags & C.CHROMA)), (vx, vy)
    else:
        assert grid["mvx"].any() or grid["mvy"].any()     # an odd offset matches the inverse board exactly


def sat_cands(D, lg, step, seed):
    """The zero vector at every point of the size's lattice, in both slots in turn; then all 64 pairs of eighth-pel
    phases (of multiples of `step` eighth-pels where step > 1) at points taken in turn, full-pel parts up to +-33."""
    rng = np.random.RandomState(seed)
    pts = [(vx, vy) for vy in range(0, 9, 1 << lg) for vx in range(0, 9, 1 << lg)]
    c = np.zeros(len(pts) + 64, D.ME_CAND)
    for i, (vx, vy) in enumerate(pts):
        c[i] = (0, vx, vy, i & 1, 0, 0)
    for i in range(64):
        vx, vy = pts[(5*i) % len(pts)]
        fx, fy = (i % 8, i//8) if step == 1 else (0, 0)
        c[len(pts) + i] = (0, vx, vy, i & 1, step*(8*rng.randint(-33, 34) + fx), step*(8*rng.randint(-33, 34) + fy))
    return c, len(pts)


@pytest.mark.parametrize("lg", [0, 1, 2, 3])
@pytest.mark.parametrize("pic", SAT_PICS)
@pytest.mark.parametrize("kind", ["flat", "checker"])
def test_saturated_costs_equal_the_yardstick(D, kind, pic, lg):
    name = kind + ":" + pic
    pw, ph = pic_size(name)
    src, csrc, refs, crefs = planes_of(name)
    d_src, d_refs = cuda(src)[0], cuda(*refs)
    c, npts = sat_cands(D, lg, 1, 70 + lg)
    args = [(int(k["vx"]), int(k["vy"]), lg, int(k["mvx"]), int(k["mvy"])) for k in c]
    # odhip_me_costs
    want = [M.bma_sad(src[0], pw, ph, refs[k["slot"]][0], *a) for k, a in zip(c, args)]
    assert D.me_costs(d_src, d_refs, pw, ph, lg, c).tolist() == want
    assert want[:npts] == [flat_dist(a[0], a[1], lg, pw, ph, 0, C.SAD_METRIC) for a in args[:npts]]
    # odhip_me_costs2, both metrics, both chroma formats
    for cdec in (1, 0):
        d_csrc, d_crefs = cuda(csrc[cdec])[0], cuda(*crefs[cdec])
        for metric in (C.SAD_METRIC, C.SATD_METRIC):
            want = [list(C.cand_dist((src[0], csrc[cdec][0], csrc[cdec][1]), pw, ph,
                                     (refs[k["slot"]][0], crefs[cdec][k["slot"]][0], crefs[cdec][k["slot"]][1]), *a,
                                     cdec, metric)) for k, a in zip(c, args)]
            got = D.me_costs2(d_src, d_refs, pw, ph, lg, c, metric, D.ME_CHROMA, d_csrc, d_crefs, cdec)
            assert got.tolist() == want, (cdec, metric)
            for a, w in zip(args[:npts], want):
                assert w == [flat_dist(a[0], a[1], lg, pw, ph, d, metric) for d in (0, cdec, cdec)], (a, cdec, metric)
    # odhip_me_costs3, every level
    levels = most_levels(lg)
    spyr = HR.pyramid(src[0], levels)
    rpyr = [HR.pyramid(r[0], levels) for r in refs]
    for level in range(levels + 1):
        c, npts = sat_cands(D, lg, 8 << level, 80 + lg + 4*level)
        want = [C.plane_dist(spyr[level], pw, ph, rpyr[k["slot"]][level], int(k["vx"]), int(k["vy"]), lg,
                             int(k["mvx"]), int(k["mvy"]), level, C.SAD_METRIC) for k in c]
        assert D.me_costs3(d_src, d_refs, pw, ph, lg, c, level, levels).tolist() == want, level
        if kind == "flat" or level == 0:
            assert want[:npts] == [flat_dist(int(k["vx"]), int(k["vy"]), lg, pw, ph, level, C.SAD_METRIC)
                                   for k in c[:npts]], level
        elif pic == "64x64":
            assert not any(want[:npts])        # the halved checkerboard and its inverse are both 128 everywhere


# ---- 2. three distinct slots, one slot, three pictures, one picture ----
# the calls of the issue on a scene: (which search, lg, flags, cdec, res)
SCENE_RUNS = [("search", 1, 0, 0, 0), ("search2", 2, CHROMA_SATD, 1, 0), ("search2", 0, CHROMA_SATD, 0, 0)]
SCENE_RUNS += [("search3", lg, flags, 1, res) for lg in (1, 3) for flags in (0, CHROMA_SATD) for res in (0, 3)]
SCENE_IDS = ["%s-lg%d-flags%d-%s-res%d" % (r[0], r[1], r[2], ("444", "420")[r[3]], r[4]) for r in SCENE_RUNS]


def scene_run(D, name, which, lg, flags, cdec, res):
    if which == "search":
        return run1(D, name, lg, 3, res, 5)
    if which == "search2":
        return run2(D, name, lg, 3, res, 5, 3, flags, cdec)
    return run3(D, name, lg, 3, res, 5, 3, flags, cdec, 2, 2)


@pytest.mark.parametrize("which,lg,flags,cdec,res", SCENE_RUNS, ids=SCENE_IDS)
def test_three_distinct_slots_and_three_pictures(D, which, lg, flags, cdec, res):
    grid, cost = scene_run(D, "scene:3x3", which, lg, flags, cdec, res)
    assert grid.shape[0] == 3
    check_shape(D, grid, cost, lg, W2, H2)
    slots = grid["ref"][:, ::1 << lg, ::1 << lg]
    won = [int((slots == s).sum()) for s in range(3)]
    print("points won per slot:", won)
    assert all(won), won


@pytest.mark.parametrize("which,lg,flags,cdec,res", SCENE_RUNS, ids=SCENE_IDS)
def test_one_slot_and_one_picture(D, which, lg, flags, cdec, res):
    grid, cost = scene_run(D, "scene:1x1", which, lg, flags, cdec, res)
    assert grid.shape[0] == 1 and not grid["ref"].any()
    check_shape(D, grid, cost, lg, W2, H2)


def test_one_slot_of_the_scene_is_the_scene_with_one_slot(D):
    """Picture 0 and slot 0 are the same planes in both sets: their costs against slot 0 are the same numbers."""
    one, three = planes_of("scene:1x1"), planes_of("scene:3x3")
    assert np.array_equal(one[0][0], three[0][0]) and np.array_equal(one[2][0][0], three[2][0][0])
    assert len(three[2]) == 3 and len(one[2]) == 1
    assert not np.array_equal(three[2][0], three[2][1]) and not np.array_equal(three[2][1], three[2][2])


# ---- 3. tiny pictures ----
@pytest.mark.parametrize("w,h", [(1, 1), (2, 1), (7, 3), (9, 5)])
def test_downsample_of_tiny_planes(D, w, h):
    rng = np.random.RandomState(10*w + h)
    p = rng.randint(0, 256, size=(3, h, w)).astype(np.uint8)
    want = np.stack([HR.halve(x) for x in p])
    assert want.shape[1:] == ((h + 1) >> 1, (w + 1) >> 1)
    assert np.array_equal(D.me_downsample(cuda(p)[0]).cpu().numpy(), want)


@pytest.mark.parametrize("pic", ["1x1", "9x5", "5x9"])
def test_tiny_pictures(D, pic):
    name = "tiny:" + pic
    pw, ph = pic_size(name)
    for lg in (0, 1):
        # most blocks are empty at level 0, and every block of some points is empty at every level
        empty = [C.plane_clip(vx, vy, lg, j, pw, ph) is None for j in range(most_levels(lg) + 1)
                 for vy in range(0, 9, 1 << lg) for vx in range(0, 9, 1 << lg)]
        npts = len(empty)//(most_levels(lg) + 1)
        assert sum(empty[:npts]) > npts//2
        assert any(all(empty[p::npts]) for p in range(npts))
        for flags in (0, CHROMA_SATD):
            for levels in range(1, most_levels(lg) + 1):
                grid, cost = run3(D, name, lg, 3, 0, 5, 3, flags, 1, levels, 2)
                check_shape(D, grid, cost, lg, 64, 64)
            grid, cost = run2(D, name, lg, 7, 0, 5, 3, flags, 1)
            check_shape(D, grid, cost, lg, 64, 64)
            # a point whose block is empty in every plane costs nothing and keeps the zero vector in slot 0
            for vy in range(0, 9, 1 << lg):
                for vx in range(0, 9, 1 << lg):
                    if C.plane_clip(vx, vy, lg, 0, pw, ph) is None and C.plane_clip(vx, vy, lg, 1, pw, ph) is None:
                        pt = grid[:, vy, vx]
                        assert not cost[:, vy, vx].any() and not (pt["mvx"].any() or pt["mvy"].any() or pt["ref"].any())
    run1(D, name, 3, 7, 0, 5)


# ---- 4. the largest lambdas ----
def worst_cost(lg, lam, mv_max):
    """8 (D_Y + 2 (D_C >> 2)) + lambda (|mvx| + |mvy|) at its largest: saturated planes, both components mv_max."""
    blk = 8 << lg
    return 8*(255*blk*blk + 2*(255*blk*blk >> 2)) + lam*2*mv_max


@pytest.mark.parametrize("name,lg", [("flat:61x63", 3), ("checker:61x63", 2), ("scene:1x3", 2)])
def test_the_largest_lambdas(D, name, lg):
    lam2, lam3 = 1 << 20, 1 << 19
    assert worst_cost(3, lam2, 8*32 + 7) < 1 << 31 and worst_cost(3, lam3, 1223) < 1 << 31
    w, h = planes_of(name)[2][0].shape[2], planes_of(name)[2][0].shape[1]
    for flags in (0, CHROMA_SATD):
        grid, cost = run2(D, name, lg, 32, 0, lam2, lam2, flags, 1)
        check_shape(D, grid, cost, lg, w, h)
        assert int(yard2(name, lg, 32, 0, lam2, lam2, flags, 1)[1].max()) < 1 << 31
        grid, cost = run3(D, name, lg, 32, 0, lam3, lam3, flags, 1, 2, 8)
        check_shape(D, grid, cost, lg, w, h)
        assert int(yard3(name, lg, 32, 0, lam3, lam3, flags, 1, 2, 8)[1].max()) < 1 << 31
