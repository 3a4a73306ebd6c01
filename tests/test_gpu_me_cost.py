"""GPU: the motion search with chroma planes in the cost and SATD as the sub-pel metric (me_kernels.hip:
odhip_me_search2 / odhip_me_costs2) against the numpy yardstick tests/_me_cost_ref.py and the compiled reference's
recorded per-plane distortions (tests/golden/me_cost.npz).  Every comparison is exact integer equality.

The shapes are those of test_gpu_me.py: coded 128 x 64, two pictures, two reference slots, the pictures 120 x 56 and
119 x 55 (the odd size makes the 4:2:0 chroma picture size round up), 4:2:0 and 4:4:4."""
import ctypes
import functools

import numpy as np
import pytest

import _me_cost_ref as C
import _me_ref as M
import _mc_ref as R
from test_gpu_me import content, cuda, same_search, check_shape, chroma_of
from test_me_cost_ref import load_golden

pytestmark = pytest.mark.gpu

W, H, F = 128, 64, 2
PICS = ((120, 56), (119, 55))
EINVAL, EIMPL = -10, -23


@pytest.fixture(scope="module")
def D():
    import torch
    import daala_amd
    assert torch.cuda.is_available()
    daala_amd.init(0)
    return daala_amd


@functools.lru_cache(maxsize=None)
def planes(cdec, pic=0):
    """(src [2][ph][pw], csrc [4][..], refs: two slots [2][H][W], crefs: two slots [4][H >> cdec][W >> cdec])."""
    pw, ph = PICS[pic]
    src, refs = content()
    src = np.ascontiguousarray(src[:, :ph, :pw])
    full = chroma_of(content()[0], cdec, 7)
    csrc = np.ascontiguousarray(full[:, :C.plane_sz(ph, cdec), :C.plane_sz(pw, cdec)])
    # chroma frames that follow their luma frames, each with its own small shift and noise
    crefs = [np.roll(chroma_of(r, cdec, 8 + i), (i, 1 - i), axis=(1, 2)) for i, r in enumerate(refs)]
    return src, csrc, refs, crefs


def dev(cdec, pic=0):
    src, csrc, refs, crefs = planes(cdec, pic)
    return cuda(src)[0], cuda(csrc)[0], cuda(*refs), cuda(*crefs)


def yard_cands(cdec, pic, lg, c, metric, chroma=True):
    src, csrc, refs, crefs = planes(cdec, pic)
    pw, ph = PICS[pic]
    out = []
    for k in c:
        f, s = int(k["pic"]), int(k["slot"])
        out.append(C.cand_dist((src[f], csrc[f], csrc[F + f]), pw, ph, (refs[s][f], crefs[s][f], crefs[s][F + f]),
                               int(k["vx"]), int(k["vy"]), lg, int(k["mvx"]), int(k["mvy"]), cdec, metric, chroma))
    return [list(x) for x in out]


# ---- 1. costs against the recorded reference ----
@pytest.mark.parametrize("cdec", [1, 0], ids=["420", "444"])
def test_costs_equal_the_recorded_reference(D, cdec):
    g = load_golden()
    srcs, refs = C.golden_planes(g, cdec)
    src, plane = cuda(srcs[0][None], refs[0][None])
    csrc, cplane = cuda(np.stack(srcs[1:]), np.stack(refs[1:]))
    cases = g["cases"]
    seen = 0
    for pic, (pw, ph) in enumerate(g["pics"].tolist()):
        for lg in range(4):
            pick = (cases[:, 0] == cdec) & (cases[:, 1] == pic) & (cases[:, 4] == lg)
            c = np.zeros(int(pick.sum()), D.ME_CAND)
            c["vx"], c["vy"], c["mvx"], c["mvy"] = cases[pick, 2], cases[pick, 3], cases[pick, 5], cases[pick, 6]
            for metric, want in ((0, g["sad"]), (1, g["satd"])):
                got = D.me_costs2(src, [plane], pw, ph, lg, c, metric, D.ME_CHROMA, csrc, [cplane], cdec)
                assert np.array_equal(got, want[pick].astype(np.uint32)), (pic, lg, metric, got.tolist(),
                                                                           want[pick].tolist())
            seen += len(c)
    assert seen == int((cases[:, 0] == cdec).sum())


# ---- 2. costs against the yardstick ----
def yard_list(D, lg, cdec):
    """Every point of the frame's four edges (its corners with them), then every phase pair at random points; vectors
    up to 33 full pels either way."""
    rng = np.random.RandomState(30 + lg + 4*cdec)
    s = 1 << lg
    xs, ys = list(range(0, W//8 + 1, s)), list(range(0, H//8 + 1, s))
    pts = [(x, y) for x in xs for y in (ys[0], ys[-1])] + [(x, y) for y in ys for x in (xs[0], xs[-1])]
    pts += [(xs[rng.randint(len(xs))], ys[rng.randint(len(ys))]) for _ in range(64)]
    c = np.zeros(len(pts), D.ME_CAND)
    n0 = len(pts) - 64
    for i, (vx, vy) in enumerate(pts):
        fx, fy = ((i - n0) % 8, (i - n0)//8) if i >= n0 else (rng.randint(8), rng.randint(8))
        c[i] = (rng.randint(F), vx, vy, rng.randint(2), 8*rng.randint(-33, 33) + fx, 8*rng.randint(-33, 33) + fy)
    return c


@pytest.mark.parametrize("cdec", [1, 0], ids=["420", "444"])
@pytest.mark.parametrize("lg", [0, 1, 2, 3])
def test_costs_equal_the_yardstick(D, lg, cdec):
    pic = lg & 1
    pw, ph = PICS[pic]
    c = yard_list(D, lg, cdec)
    d_src, d_csrc, d_refs, d_crefs = dev(cdec, pic)
    for metric in (0, 1):
        got = D.me_costs2(d_src, d_refs, pw, ph, lg, c, metric, D.ME_CHROMA, d_csrc, d_crefs, cdec)
        assert got.tolist() == yard_cands(cdec, pic, lg, c, metric), metric
    # without the flag chroma is not read (no chroma planes are given) and reported as 0
    got = D.me_costs2(d_src, d_refs, pw, ph, lg, c[:16], 1, 0, None, None, cdec)
    assert got.tolist() == yard_cands(cdec, pic, lg, c[:16], 1, chroma=False)
    # a candidate that names nothing is flagged, not evaluated
    bad = c[:3].copy()
    bad["pic"][0], bad["slot"][1], bad["vx"][2] = F, 2, W//8 + 1
    got = D.me_costs2(d_src, d_refs, pw, ph, lg, bad, 1, D.ME_CHROMA, d_csrc, d_crefs, cdec)
    assert got.tolist() == [[0xffffffff]*3]*3


@pytest.mark.parametrize("lg", [0, 1, 2, 3])
def test_luma_costs_are_column_0_of_the_three_plane_costs(D, lg):
    """odhip_me_costs writes one value per candidate and nothing else: the candidates of
    test_costs_equal_the_yardstick, the three invalid ones behind them, into the middle of a pre-filled buffer."""
    import torch
    pic = lg & 1
    pw, ph = PICS[pic]
    c = yard_list(D, lg, 1)
    bad = c[:3].copy()
    bad["pic"][0], bad["slot"][1], bad["vx"][2] = F, 2, W//8 + 1
    both = np.concatenate([c, bad])
    d_src, _, d_refs, _ = dev(1, pic)
    got = D.me_costs(d_src, d_refs, pw, ph, lg, both)
    three = D.me_costs2(d_src, d_refs, pw, ph, lg, both, 0, 0, None, None)
    assert got.dtype == np.uint32 and got.shape == (len(both),) and np.array_equal(got, three[:, 0])
    assert not three[:len(c), 1:].any()
    assert got[:len(c)].tolist() == [d[0] for d in yard_cands(1, pic, lg, c, 0, chroma=False)]
    assert got[len(c):].tolist() == [0xffffffff]*3
    # the same call through the library, the output one element into a buffer of n + 2
    n = len(both)
    job = D.api._me_job(d_src, d_refs, pw, ph, lg, 0, 0, 0)
    d_c = torch.from_numpy(both.view(np.uint8)).cuda()
    buf = torch.full((n + 2,), 0x5a5a5a5a, dtype=torch.int32, device="cuda")
    rc = D.lib().odhip_me_costs(ctypes.byref(job), ctypes.c_void_p(d_c.data_ptr()), ctypes.c_long(n),
                                ctypes.c_void_p(buf.data_ptr() + 4), None)
    assert rc == 0
    torch.cuda.synchronize()
    out = buf.cpu().numpy().view(np.uint32)
    assert out[0] == 0x5a5a5a5a and out[n + 1] == 0x5a5a5a5a and np.array_equal(out[1:n + 1], got)


# ---- 3. the full search ----
def yard_search(cdec, pic, lg, rng_, res, lam, lam2, flags):
    src, csrc, refs, crefs = planes(cdec, pic)
    pw, ph = PICS[pic]
    return C.search(src, csrc, pw, ph, refs, crefs, lg, rng_, res, lam, lam2, flags, cdec)


def dev_search(D, cdec, pic, lg, rng_, res, lam, lam2, flags):
    d_src, d_csrc, d_refs, d_crefs = dev(cdec, pic)
    pw, ph = PICS[pic]
    return D.me_search2(d_src, d_refs, pw, ph, lg, rng_, res, lam, lam2, flags, d_csrc, d_crefs, cdec)


@pytest.mark.parametrize("cdec", [1, 0], ids=["420", "444"])
@pytest.mark.parametrize("flags", [0, 1, 2, 3], ids=["none", "chroma", "satd", "both"])
@pytest.mark.parametrize("lg", [0, 1, 2, 3])
def test_search_equals_the_yardstick(D, lg, flags, cdec):
    # range 7 at 16 x 16 blocks: at 4:2:0 both offset parities, every chroma phase plane and more chroma sample
    # offsets than one group of four; the other sizes alternate 0 (stage 1 has one candidate) and 3
    for res in (3, 0):
        rng_ = 7 if lg == 1 else (0, 3)[(lg + flags + res) & 1]
        lam, lam2 = ((0, 0), (5, 3))[(lg + flags + cdec + (res == 0)) & 1]
        pic = (lg + res) & 1
        got = dev_search(D, cdec, pic, lg, rng_, res, lam, lam2, flags)
        want = yard_search(cdec, pic, lg, rng_, res, lam, lam2, flags)
        same_search(got, want, (res, rng_, lam, lam2, pic))
        check_shape(D, got[0], got[1], lg, W, H)
        if not flags and not res and lam != lam2:
            # the search without flags has a lambda_subpel of its own: stage 2 under stage 1's lambda is another
            # result on this content, at every size, so a search that ignored lambda_subpel would not have passed
            other = yard_search(cdec, pic, lg, rng_, res, lam, lam, flags)
            assert want[0].tobytes() != other[0].tobytes() or not np.array_equal(want[1], other[1])


@pytest.mark.parametrize("cdec", [1, 0], ids=["420", "444"])
def test_a_wide_search_takes_every_lane_more_than_once(D, cdec):
    # range 16 at 64 x 64 blocks: 33 x 33 offsets, more luma and key tasks than lanes; both lambdas at work
    got = dev_search(D, cdec, 1, 3, 16, 1, 5, 3, 3)
    want = yard_search(cdec, 1, 3, 16, 1, 5, 3, 3)
    same_search(got, want, "range 16")
    assert np.abs(got[0]["mvx"]).max() > 8 and got[0]["ref"].any()


# ---- 4. no flags: the luma search ----
@pytest.mark.parametrize("lg", [0, 2])
def test_without_flags_it_is_the_luma_search(D, lg):
    d_src, d_csrc, d_refs, d_crefs = dev(1)
    pw, ph = PICS[0]
    for res, lam in ((0, 5), (3, 0), (1, 2)):
        want = D.me_search(d_src, d_refs, pw, ph, lg, 3, res, lam)
        got = D.me_search2(d_src, d_refs, pw, ph, lg, 3, res, lam, lam, 0, d_csrc, d_crefs, 1)
        assert got[0].tobytes() == want[0].tobytes() and got[1].tobytes() == want[1].tobytes()
        got = D.me_search2(d_src, d_refs, pw, ph, lg, 3, res, lam, lam, 0, None, None, 0)
        assert got[0].tobytes() == want[0].tobytes() and got[1].tobytes() == want[1].tobytes()


# ---- 5. not vacuous ----
@pytest.mark.parametrize("cdec", [1, 0], ids=["420", "444"])
def test_chroma_decides_between_slots_with_identical_luma(D, cdec):
    # flat luma everywhere: every luma distortion is the same, so without chroma the tie-break gives the zero vector
    # in slot 0; slot 1's chroma holds the pictures' chroma at a planted vector, slot 0's is unrelated
    pw, ph = PICS[0]
    cmv = (10, -4) if cdec else (20, -8)        # the planted vector, in eighths of a chroma sample
    # the shortest luma vector that scales to it wins the lambda term and the tie-break: (19, -7) at 4:2:0
    planted = tuple(min((v for v in range(-40, 41) if R.scale_mv(v, cdec) == c), key=abs) for c in cmv)
    assert planted == ((19, -7) if cdec else (20, -8))
    rng = np.random.RandomState(77)
    src = np.full((F, ph, pw), 100, np.uint8)
    refs = [np.full((F, H, W), 97, np.uint8)]*2
    hc, wc = H >> cdec, W >> cdec
    good = np.stack([M.smooth_noise(rng, hc, wc) for _ in range(2*F)])
    other = np.stack([M.smooth_noise(rng, hc, wc) for _ in range(2*F)])
    csrc = np.stack([M.displaced(p, *cmv)[:C.plane_sz(ph, cdec), :C.plane_sz(pw, cdec)] for p in good])
    crefs = [other, good]
    lg = 1
    d = cuda(src)[0], cuda(*refs), cuda(csrc)[0], cuda(*crefs)
    for flags in (0, D.ME_CHROMA):
        got = D.me_search2(d[0], d[1], pw, ph, lg, 3, 0, 2, 2, flags, d[2], d[3], cdec)
        want = C.search(src, csrc, pw, ph, refs, crefs, lg, 3, 0, 2, 2, flags, cdec)
        same_search(got, want, flags)
        # the points whose blocks are whole in every plane
        inner = got[0][:, 2:-2:2, 2:-2:2]
        assert inner.size
        if flags:
            assert np.all(inner["ref"] == 1) and np.all(inner["mvx"] == planted[0]) and np.all(inner["mvy"] == planted[1])
            assert np.all(got[1][:, 2:-2:2, 2:-2:2] == 8*3*16*16 + 2*(abs(planted[0]) + abs(planted[1])))
        else:
            assert not inner["ref"].any() and not inner["mvx"].any() and not inner["mvy"].any()
            assert np.all(got[1][:, 2:-2:2, 2:-2:2] == 8*3*16*16)


def test_satd_picks_other_vectors_than_sad(D):
    picks = {}
    for flags in (1, 3):
        want = yard_search(1, 0, 1, 3, 0, 2, 2, flags)
        same_search(dev_search(D, 1, 0, 1, 3, 0, 2, 2, flags), want, flags)
        picks[flags] = want[0]
    differ = (picks[1]["mvx"] != picks[3]["mvx"]) | (picks[1]["mvy"] != picks[3]["mvy"])
    share = differ[:, ::2, ::2].mean()
    print("SATD winners differ from SAD winners at %.0f%% of the points" % (100*share))
    assert share > 0


# ---- 6. layouts ----
@pytest.mark.parametrize("cdec", [1, 0], ids=["420", "444"])
def test_odd_strides_bases_and_larger_plane_strides_change_nothing(D, cdec):
    import torch
    pw, ph = PICS[1]
    want = dev_search(D, cdec, 1, 1, 3, 0, 5, 3, 3)

    def widened(t, dx, dy, fill):
        n, h, w = t.shape
        big = torch.full((n, h + dy + 2, w + dx), fill, dtype=torch.uint8, device="cuda")
        big[:, 1:1 + h, 1:1 + w] = t
        return big[:, 1:1 + h, 1:1 + w]

    d_src, d_csrc, d_refs, d_crefs = dev(cdec, 1)
    v_csrc = widened(d_csrc, 7 if d_csrc.shape[2] % 2 == 0 else 8, 3, 77)
    v_crefs = [widened(t, 5, 1, 99) for t in d_crefs]
    v_src = widened(d_src, 8, 2, 55)
    v_refs = [widened(t, 3, 1, 11) for t in d_refs]
    assert v_csrc.stride(1) % 2 == 1 and v_crefs[0].stride(1) % 2 == 1 and v_csrc.data_ptr() % 2 == 0
    assert v_csrc.stride(0) > v_csrc.shape[1]*v_csrc.stride(1)
    assert (v_csrc.data_ptr() - v_csrc.stride(1) - 1) % 2 == 0 and v_crefs[0].data_ptr() % 4 != 0
    got = D.me_search2(v_src, v_refs, pw, ph, 1, 3, 0, 5, 3, 3, v_csrc, v_crefs, cdec)
    same_search(got, want, "strides")
    c = np.zeros(8, D.ME_CAND)
    c["vx"], c["vy"], c["mvx"], c["mvy"], c["pic"] = [0, 2, 14, 16, 8, 6, 4, 2], [0, 6, 2, 6, 4, 0, 6, 2], \
        [3, -20, 9, 0, 41, -7, 12, 5], [-5, 4, 0, 13, -22, 6, 1, 8], [0, 1, 0, 1, 0, 1, 0, 1]
    for metric in (0, 1):
        a = D.me_costs2(v_src, v_refs, pw, ph, 1, c, metric, 1, v_csrc, v_crefs, cdec)
        b = D.me_costs2(d_src, d_refs, pw, ph, 1, c, metric, 1, d_csrc, d_crefs, cdec)
        assert np.array_equal(a, b) and a.tolist() == yard_cands(cdec, 1, 1, c, metric)


# ---- 7. refusals ----
def test_refused_jobs_launch_nothing(D):
    import torch
    d_src, d_csrc, d_refs, d_crefs = dev(1)
    pw, ph = PICS[0]
    L = D.lib()
    shape = (F, H//8 + 1, W//8 + 1)
    grid = torch.full(shape + (D.MV_POINT.itemsize,), 0xab, dtype=torch.uint8, device="cuda")
    cost = torch.full(shape, 0x5a5a5a5a, dtype=torch.int32, device="cuda")
    cands = torch.zeros(D.ME_CAND.itemsize, dtype=torch.uint8, device="cuda")
    out = torch.full((3,), 0x5a5a5a5a, dtype=torch.int32, device="cuda")

    def job(**kw):
        j = D.api._me_job2(d_src, d_refs, pw, ph, 1, 3, 0, 5, 3, 3, d_csrc, d_crefs, 1)
        j.luma.grid, j.luma.cost = grid.data_ptr(), cost.data_ptr()
        for k, v in kw.items():
            setattr(j, k, v)
        return j

    def search(j):
        return L.odhip_me_search2(ctypes.byref(j), None)

    def costs(j, metric=0):
        return L.odhip_me_costs2(ctypes.byref(j), ctypes.c_void_p(cands.data_ptr()), ctypes.c_long(1), metric,
                                 ctypes.c_void_p(out.data_ptr()), None)

    cw, ch = pw >> 1, ph >> 1
    no_cref1 = (ctypes.c_void_p * 3)(d_crefs[0].data_ptr(), None, None)
    for kw in (dict(flags=4), dict(flags=7), dict(cdec=2), dict(cdec=-1), dict(lambda_subpel=-1),
               dict(lambda_subpel=(1 << 20) + 1), dict(csrc=None), dict(cref=no_cref1), dict(csrc_stride=cw - 1),
               dict(cref_stride=W//2 - 1), dict(csrc_plane_stride=cw*ch - 1), dict(cref_plane_stride=W*H//4 - 1),
               dict(cdec=0)):
        assert search(job(**kw)) == EINVAL, kw
        assert costs(job(**kw)) == EINVAL, kw
    j = job()
    j.luma.range = 33
    assert search(j) == EINVAL and costs(job(), metric=2) == EINVAL
    with D.Context(0) as ctx:
        ctx.set_fpr(True)
        assert search(job()) == EIMPL and costs(job()) == EIMPL
    torch.cuda.synchronize()
    assert bool((grid == 0xab).all()) and bool((cost == 0x5a5a5a5a).all()) and bool((out == 0x5a5a5a5a).all())
    # ... and the same job, unchanged, runs
    assert search(job()) == 0 and costs(job()) == 0
    torch.cuda.synchronize()
    assert not bool((grid == 0xab).all()) and not bool((out == 0x5a5a5a5a).any())
