"""The deringing cache (daala_amd/csrc/dering_cache.hip: odhip_dering_cache_*) called directly,
every answer bit-exact against the CPU oracle's od_dering / od_compute_dist of the same call.

The cache keys on host addresses, decides per frame what is stale, keeps buffers across frames,
regrows on geometry changes and falls back to the per-call path; the drop-in encoder tests drive
one call order only (the encoder's) and can only say "packets differ".  Here each state
transition has its own case.  dir[][] is handled as the reference does: luma writes it, chroma
reads it."""
import ctypes
import os
import sys

import numpy as np
import pytest

from _caches import EINVAL, Pinned, addr, pair
from _libs import P, oracle

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tools"))

vp = ctypes.c_void_p
SENT = -31000            # no filter output of these planes (|x| <= 2048) comes near it
DIR_SENT = 99
THR = [19, 27, 38, 54, 77]      # one base threshold times the five level gains


def xdec_of(pli):
    return 0 if pli == 0 else 1


class Frame:
    """Three planes (4:2:0) and their skip maps at fixed host addresses."""

    def __init__(self, keep, nhsb, nvsb, seed):
        self.nhsb, self.nvsb = nhsb, nvsb
        self.ss = nhsb * 16 + 3
        self.x = [keep.array(((nvsb * 64) >> d, (nhsb * 64) >> d), np.int16) for d in (0, 1, 1)]
        self.skip = [keep.array(((nvsb * 16) >> d, self.ss), np.uint8) for d in (0, 1, 1)]
        self.fill(seed)

    def fill(self, seed):
        """New contents, IN PLACE."""
        from make_golden_dering import dering_input
        rng = np.random.RandomState(seed)
        for pli in range(3):
            self.x[pli][...] = dering_input(self.x[pli].shape[0], self.x[pli].shape[1], 10 * seed + pli)
            self.skip[pli][...] = rng.rand(*self.skip[pli].shape) < 0.3

    def xptr(self, pli, sbx, sby):
        n = 64 >> xdec_of(pli)
        return addr(self.x[pli], sby * n, sbx * n)

    def sptr(self, pli, sbx, sby):
        f = 16 >> xdec_of(pli)
        return addr(self.skip[pli], sby * f, sbx * f)

    def sbs(self):
        return [(sbx, sby) for sby in range(self.nvsb) for sbx in range(self.nhsb)]

    def want(self, pli, sbx, sby, thr, dirs_in, overlap=1, nhb=8, nvb=8):
        """odo_dering of this call: (y [n][n] with SENT where nothing is written, dir[8][8])."""
        xdec = xdec_of(pli)
        n = 64 >> xdec
        y = np.full((n, n), SENT, np.int16)
        d = (ctypes.c_int * 64)(*np.asarray(dirs_in).ravel().tolist())
        oracle().odo_dering(P(y), n, vp(self.xptr(pli, sbx, sby)), self.x[pli].shape[1], nhb, nvb, sbx, sby,
                            self.nhsb, self.nvsb, xdec, d, pli, vp(self.sptr(pli, sbx, sby)), self.ss,
                            int(thr), overlap, 4)
        return y, np.array(d[:]).reshape(8, 8)

    def luma_dirs(self):
        """The oracle's directions of every luma superblock (they do not depend on the threshold)."""
        return {sb: self.want(0, sb[0], sb[1], THR[0], np.full((8, 8), DIR_SENT))[1] for sb in self.sbs()}


@pytest.fixture(scope="module")
def L():
    import torch
    import daala_amd
    assert torch.cuda.is_available()
    daala_amd.init(0)
    return daala_amd.lib()


@pytest.fixture
def cache(L):
    c = L.odhip_dering_cache_create()
    assert c
    yield c
    L.odhip_dering_cache_destroy(c)


def call(L, c, fr, pli, sbx, sby, thr, dirs_in, overlap=1, nhb=8, nvb=8, rc_want=0):
    """odhip_dering_cache_call with y inside a sentinel-filled buffer (ystride > n): the block it
    wrote ([n][n], SENT where it wrote nothing) and dir[][] afterwards.  Every sample outside the
    nvb x nhb blocks must still be the sentinel."""
    xdec = xdec_of(pli)
    n = 64 >> xdec
    ys = n + 7
    buf = np.full((n + 2, ys), SENT, np.int16)
    d = (ctypes.c_int * 64)(*np.asarray(dirs_in).ravel().tolist())
    rc = L.odhip_dering_cache_call(c, addr(buf, 1, 3), ys, fr.xptr(pli, sbx, sby), fr.x[pli].shape[1], nhb, nvb,
                                   sbx, sby, fr.nhsb, fr.nvsb, xdec, d, pli, fr.sptr(pli, sbx, sby), fr.ss,
                                   int(thr), overlap, 4)
    assert rc == rc_want, (rc, pli, sbx, sby, thr)
    bh, bw = nvb * (n // 8), nhb * (n // 8)
    outside = np.ones(buf.shape, bool)
    outside[1:1 + bh, 3:3 + bw] = False
    assert (buf[outside] == SENT).all(), "wrote outside its block"
    return buf[1:1 + n, 3:3 + n].copy(), np.array(d[:]).reshape(8, 8)


def check(L, c, fr, pli, sbx, sby, thr, dirs_in, **kw):
    """One cache call against the oracle's: output block and dir[][]."""
    got, gd = call(L, c, fr, pli, sbx, sby, thr, dirs_in, **kw)
    want, wd = fr.want(pli, sbx, sby, thr, dirs_in, **kw)
    assert np.array_equal(got, want), (pli, sbx, sby, thr, kw)
    assert np.array_equal(gd, wd), (pli, sbx, sby, thr, kw)
    return got


def luma_in():
    return np.full((8, 8), DIR_SENT)


def stats(L, c):
    return pair(L.odhip_dering_cache_stats, c)


def search(L, c, fr, thrs, chroma_choice):
    """The level search in the encoder's order: per superblock the luma calls at `thrs`, then
    pli 1 and 2 at thrs[chroma_choice[sb]].  Returns (calls, the distinct pass keys)."""
    dirs = fr.luma_dirs()
    keys = set()
    calls = 0
    for i, (sbx, sby) in enumerate(fr.sbs()):
        for t in thrs:
            check(L, c, fr, 0, sbx, sby, t, luma_in())
            keys.add((0, t, 1, 4))
            calls += 1
        for pli in (1, 2):
            t = thrs[chroma_choice[i % len(chroma_choice)]]
            check(L, c, fr, pli, sbx, sby, t, dirs[(sbx, sby)])
            keys.add((pli, t, 1, 4))
            calls += 1
    return calls, keys


def test_frame_search_in_encoder_order(L, cache):
    """Every call of a frame's level search equals the oracle's; one launch per distinct (plane,
    threshold, overlap, coeff_shift), every full-superblock call served from a batched pass."""
    fr = Frame(Pinned(), 3, 2, 1)
    assert 0.2 < fr.skip[0].mean() < 0.4
    L.odhip_dering_cache_begin(cache)
    choice = [0, 2, 2, 4, 0, 2]           # per superblock: chroma passes are shared
    calls, keys = search(L, cache, fr, THR, choice)
    assert len(keys) == 5 + 2 * 3 and calls == 6 * 7
    assert stats(L, cache) == (len(keys), calls)


def test_overlap_is_part_of_the_key(L, cache):
    fr = Frame(Pinned(), 3, 2, 2)
    L.odhip_dering_cache_begin(cache)
    differ = 0
    for sb in ((1, 0), (2, 1), (0, 1)):
        a = check(L, cache, fr, 0, sb[0], sb[1], THR[2], luma_in(), overlap=0)
        b = check(L, cache, fr, 0, sb[0], sb[1], THR[2], luma_in(), overlap=1)
        differ += not np.array_equal(a, b)      # a and b are the oracle's values (check() passed)
    assert differ > 0, "overlap does not change these superblocks: the case proves nothing"
    assert stats(L, cache) == (2, 6)


def test_next_frame_at_the_same_addresses(L, cache):
    """begin, then the planes and the skip map rewritten in place: the new contents are filtered."""
    fr = Frame(Pinned(), 3, 2, 3)
    L.odhip_dering_cache_begin(cache)
    search(L, cache, fr, THR[1:3], [0, 1])
    before = {(pli, sb): fr.want(pli, sb[0], sb[1], THR[1], fr.luma_dirs()[sb])[0]
              for pli in range(3) for sb in fr.sbs()}
    L.odhip_dering_cache_begin(cache)
    fr.fill(4)
    dirs = fr.luma_dirs()
    for key, old in before.items():
        assert not np.array_equal(fr.want(key[0], key[1][0], key[1][1], THR[1], dirs[key[1]])[0], old)
    calls, keys = search(L, cache, fr, THR[1:3], [0, 1])
    assert stats(L, cache) == (2 * len(keys), 2 * calls)


def test_luma_reload_inside_a_frame_stales_the_chroma_passes(L, cache):
    """A luma plane arriving under another buffer inside a frame brings new directions: the chroma
    passes filtered along the old ones must not be served any more."""
    keep = Pinned()
    fa = Frame(keep, 3, 2, 5)
    fb = Frame(keep, 3, 2, 6)
    da, db = fa.luma_dirs(), fb.luma_dirs()
    tc = THR[3]
    sbs = [(1, 1), (2, 0)]
    for sb in sbs:
        assert not np.array_equal(da[sb], db[sb])
        for pli in (1, 2):
            assert not np.array_equal(fa.want(pli, sb[0], sb[1], tc, da[sb])[0],
                                      fa.want(pli, sb[0], sb[1], tc, db[sb])[0]), \
                "the directions do not matter here: the case proves nothing"
    L.odhip_dering_cache_begin(cache)
    for sb in fa.sbs():
        check(L, cache, fa, 0, sb[0], sb[1], THR[0], luma_in())
    for sb in sbs:
        for pli in (1, 2):
            check(L, cache, fa, pli, sb[0], sb[1], tc, da[sb])
    assert stats(L, cache)[0] == 3
    check(L, cache, fb, 0, 1, 1, THR[0], luma_in())            # the second luma buffer
    for sb in sbs:
        for pli in (1, 2):                                      # same chroma buffers, cached threshold
            check(L, cache, fa, pli, sb[0], sb[1], tc, db[sb])
    assert stats(L, cache)[0] == 6


def test_chroma_before_any_luma_call(L, cache):
    """Served per call with the directions passed in; after the luma calls the same call comes from
    a batched pass."""
    fr = Frame(Pinned(), 3, 2, 7)
    rng = np.random.RandomState(1)
    L.odhip_dering_cache_begin(cache)
    for pli, sb in ((1, (1, 0)), (2, (2, 1))):
        check(L, cache, fr, pli, sb[0], sb[1], THR[2], rng.randint(0, 8, size=(8, 8)))
    assert stats(L, cache) == (0, 0)
    for sb in fr.sbs():
        check(L, cache, fr, 0, sb[0], sb[1], THR[2], luma_in())
    dirs = fr.luma_dirs()
    for pli, sb in ((1, (1, 0)), (2, (2, 1))):
        check(L, cache, fr, pli, sb[0], sb[1], THR[2], dirs[sb])
    assert stats(L, cache) == (3, 8)


def test_partial_superblock(L, cache):
    """nhb = 5, nvb = 3 at the last superblock: the per-call path, od_dering's result, nothing
    written beyond the 3 x 5 blocks of y (call() checks the sentinels) or of dir[][]."""
    fr = Frame(Pinned(), 3, 2, 8)
    L.odhip_dering_cache_begin(cache)
    for sb in fr.sbs():
        check(L, cache, fr, 0, sb[0], sb[1], THR[4], luma_in())
    served = stats(L, cache)
    dirs = fr.luma_dirs()
    for overlap in (0, 1):
        got = check(L, cache, fr, 0, 2, 1, THR[4], luma_in(), overlap=overlap, nhb=5, nvb=3)
        assert (got[:24, :40] != SENT).all() and (got[24:] == SENT).all() and (got[:, 40:] == SENT).all()
        assert not np.array_equal(got[:24, :40], fr.x[0][64:88, 128:168])      # it did filter
        # chroma reads dir[][] of the 3 x 5 blocks only: the reference's caller fills no other entry
        # (its luma call was partial too), so the rest holds whatever was there - here a value
        # that is no direction, and the result and dir[][] are those of valid ones all over
        part = np.full((8, 8), 1 << 20)
        part[:3, :5] = dirs[(2, 1)][:3, :5]
        for pli in (1, 2):
            got = check(L, cache, fr, pli, 2, 1, THR[4], part, overlap=overlap, nhb=5, nvb=3)
            assert np.array_equal(got, fr.want(pli, 2, 1, THR[4], dirs[(2, 1)], overlap=overlap, nhb=5, nvb=3)[0])
            assert (got[:12, :20] != SENT).all() and (got[12:] == SENT).all() and (got[:, 20:] == SENT).all()
    assert stats(L, cache) == served


def test_geometry_across_frames(L, cache):
    """Smaller (buffers kept), then larger (everything regrown, the directions included)."""
    keep = Pinned()
    launches = calls = 0
    for i, (nhsb, nvsb) in enumerate(((3, 2), (2, 1), (4, 3))):
        fr = Frame(keep, nhsb, nvsb, 20 + i)
        L.odhip_dering_cache_begin(cache)
        n, keys = search(L, cache, fr, THR[2:4], [1])
        launches += len(keys)
        calls += n
        assert stats(L, cache) == (launches, calls)


def test_one_cache_across_frame_sizes(L, cache):
    """One superblock, then 3 x 2, then one again (new contents at the first frame's addresses), three
    thresholds each: the result list grows past its first entries while those are reused, every buffer is
    regrown once and then kept.  Each frame equals the oracle's superblock by superblock (search), and costs
    the launches and serves the calls it costs a cache that has seen nothing else."""
    keep = Pinned()
    one, six = Frame(keep, 1, 1, 40), Frame(keep, 3, 2, 41)
    thrs = [THR[0], THR[2], THR[4]]
    total = (0, 0)
    for i, fr in enumerate((one, six, one)):
        if i == 2:
            fr.fill(42)
        fresh = L.odhip_dering_cache_create()
        assert fresh
        try:
            counts = []
            for c in (cache, fresh):
                L.odhip_dering_cache_begin(c)
                calls, keys = search(L, c, fr, thrs, [0, 2, 1])
                counts.append(stats(L, c))
        finally:
            L.odhip_dering_cache_destroy(fresh)
        assert counts[1] == (len(keys), calls) and len(keys) >= 3 + 2
        total = (total[0] + counts[1][0], total[1] + counts[1][1])
        assert counts[0] == total, i


@pytest.mark.parametrize("seen_big_before", [False, True])
def test_another_chroma_geometry_inside_a_frame_is_refused(L, cache, seen_big_before):
    """After a luma pass the directions of the frame exist at the frame's geometry: a chroma call
    of a larger frame, or of one with as many superblocks in rows of another length, cannot be
    served from them and is an error, not a wrong answer - also on a cache whose buffers are
    large enough because an earlier frame had the larger geometry."""
    keep = Pinned()
    small, big, turned = Frame(keep, 3, 2, 30), Frame(keep, 4, 3, 31), Frame(keep, 2, 3, 32)
    if seen_big_before:
        L.odhip_dering_cache_begin(cache)
        search(L, cache, big, THR[:1], [0])
    before = stats(L, cache)
    L.odhip_dering_cache_begin(cache)
    for sb in small.sbs():
        check(L, cache, small, 0, sb[0], sb[1], THR[0], luma_in())
    for other, sb in ((big, (3, 2)), (big, (0, 0)), (turned, (1, 2)), (turned, (0, 0))):
        for pli in (1, 2):
            call(L, cache, other, pli, sb[0], sb[1], THR[0], np.zeros((8, 8), int), rc_want=EINVAL)
    assert stats(L, cache) == (before[0] + 1, before[1] + 6)
    # the frame's own chroma is still served, exact
    dirs = small.luma_dirs()
    for pli in (1, 2):
        check(L, cache, small, pli, 2, 1, THR[0], dirs[(2, 1)])
    assert stats(L, cache) == (before[0] + 3, before[1] + 8)


def test_argument_validation(L, cache):
    fr = Frame(Pinned(), 3, 2, 9)
    L.odhip_dering_cache_begin(cache)
    y = np.full((64, 64), SENT, np.int16)
    d = (ctypes.c_int * 64)()

    def rc(c=cache, yp=y.ctypes.data, xp=fr.xptr(0, 0, 0), dp=d, sp=fr.sptr(0, 0, 0), pli=0, xdec=0, sbx=0,
           sby=0):
        return L.odhip_dering_cache_call(c, yp, 64, xp, fr.x[pli if 0 <= pli < 3 else 0].shape[1], 8, 8, sbx, sby,
                                         fr.nhsb, fr.nvsb, xdec, dp, pli, sp, fr.ss, THR[0], 1, 4)

    assert rc(c=None) == EINVAL
    assert rc(yp=None) == EINVAL
    assert rc(xp=None) == EINVAL
    assert rc(dp=None) == EINVAL
    assert rc(sp=None) == EINVAL
    for pli in (-1, 3):
        assert rc(pli=pli, xdec=1) == EINVAL
    for xdec in (-1, 2):
        assert rc(pli=1, xdec=xdec, xp=fr.xptr(1, 0, 0), sp=fr.sptr(1, 0, 0)) == EINVAL
    assert rc(pli=0, xdec=1) == EINVAL
    assert rc(sbx=fr.nhsb) == EINVAL and rc(sby=fr.nvsb) == EINVAL and rc(sbx=-1) == EINVAL
    assert stats(L, cache) == (0, 0)
    assert (y == SENT).all()
    assert rc() == 0 and stats(L, cache) == (1, 1)


# ---- the level search's distortions ----------------------------------------------------

def _bits(v):
    return np.float64(v).view(np.int64)


class Source:
    """The 8-bit luma source picture, stride = w + 16: a host array and a device copy."""

    def __init__(self, keep, fr, seed):
        import torch
        h, w = fr.x[0].shape
        self.stride = w + 16
        rng = np.random.RandomState(seed)
        self.h = keep.array((h, self.stride), np.uint8, 7)
        self.h[:, :w] = np.clip((fr.x[0].astype(int) >> 4) + 128 + rng.randint(-6, 7, size=(h, w)), 0, 255)
        self.d = torch.from_numpy(self.h).cuda()

    def block(self, sbx, sby):
        """(src - 128) << 4 of a superblock: what the encoder passes as x."""
        b = self.h[sby * 64:(sby + 1) * 64, sbx * 64:(sbx + 1) * 64].astype(np.int32)
        return np.ascontiguousarray((b - 128) << 4)

    def set(self, L, c, masking, flat):
        assert L.odhip_dering_cache_set_source(c, self.h.ctypes.data, self.d.data_ptr(), self.stride, masking,
                                               flat) == 0


def _dist(L, c, x, y, sb, thr, masking, flat, cq, n=64):
    out = ctypes.c_double(-7.25)
    rc = L.odhip_dering_cache_dist(c, x.ctypes.data, y.ctypes.data, n, sb[0], sb[1], thr, masking, flat, cq,
                                   ctypes.byref(out))
    return rc, out.value


@pytest.mark.parametrize("masking,flat", [(1, 0), (0, 0), (1, 1)])
def test_distortions_served_from_the_luma_passes(L, cache, masking, flat):
    """od_compute_dist(source superblock, filtered superblock) for every superblock and threshold,
    at the three branches of the quantiser factor: the oracle's bits."""
    o = oracle()
    o.odo_compute_dist.restype = ctypes.c_double
    keep = Pinned()
    fr = Frame(keep, 3, 2, 11)
    src = Source(keep, fr, 12)
    L.odhip_dering_cache_begin(cache)
    src.set(L, cache, masking, flat)
    served = 0
    distinct = set()
    for sb in fr.sbs():
        x = src.block(*sb)
        for t in THR:
            y = check(L, cache, fr, 0, sb[0], sb[1], t, luma_in()).astype(np.int32)
            assert max(np.abs(x).max(), np.abs(y).max()) <= 11000     # od_compute_var_4x4 stays inside int
            vals = []
            for cq in (30, 41, 50):
                rc, got = _dist(L, cache, x, y, sb, t, masking, flat, cq)
                want = o.odo_compute_dist(P(x), P(y), 64, flat, masking, cq)
                assert rc == 1 and _bits(got) == _bits(want), (sb, t, cq, got, want)
                served += 1
                vals.append(want)
            assert flat or len(set(vals)) == 3      # the quantiser changes the answer: a reused finish would show
            distinct.add(vals[0])
    assert len(distinct) > 20
    assert L.odhip_dering_cache_dist_served(cache) == served
    # what the cache cannot vouch for: 0, *dist left alone
    sb, t = (1, 1), THR[1]
    x = src.block(*sb)
    y = check(L, cache, fr, 0, sb[0], sb[1], t, luma_in()).astype(np.int32)
    assert _dist(L, cache, x, y, sb, t, masking, flat, 41)[0] == 1
    served += 1
    for what, args in {
        "one sample of y differs": dict(y=np.where(np.arange(4096).reshape(64, 64) == 64 * 63 + 63, y + 1, y)
                                        .astype(np.int32)),
        "one sample of x differs": dict(x=np.where(np.arange(4096).reshape(64, 64) == 64 * 17 + 5, x - 16, x)
                                        .astype(np.int32)),
        "a threshold without a pass": dict(thr=t + 1),
        "another masking": dict(masking=1 - masking),
        "another flat": dict(flat=1 - flat),
        "n = 32": dict(n=32),
        "the superblock beside it": dict(sb=(2, 1)),
    }.items():
        kw = dict(x=x, y=y, sb=sb, thr=t, masking=masking, flat=flat, cq=41)
        kw.update(args)
        assert _dist(L, cache, **kw) == (0, -7.25), what
    assert L.odhip_dering_cache_dist_served(cache) == served


def test_distortions_need_the_source_before_the_pass(L, cache):
    keep = Pinned()
    fr = Frame(keep, 3, 2, 13)
    src = Source(keep, fr, 14)
    sb, t = (0, 1), THR[2]
    x = src.block(*sb)
    # no set_source since begin (the one of the frame before does not count)
    L.odhip_dering_cache_begin(cache)
    src.set(L, cache, 1, 0)
    L.odhip_dering_cache_begin(cache)
    y = check(L, cache, fr, 0, sb[0], sb[1], t, luma_in()).astype(np.int32)
    assert _dist(L, cache, x, y, sb, t, 1, 0, 41) == (0, -7.25)
    # set_source after the pass: that pass has no parts; a later pass has
    src.set(L, cache, 1, 0)
    assert _dist(L, cache, x, y, sb, t, 1, 0, 41) == (0, -7.25)
    y2 = check(L, cache, fr, 0, sb[0], sb[1], THR[3], luma_in()).astype(np.int32)
    assert _dist(L, cache, x, y2, sb, THR[3], 1, 0, 41)[0] == 1
    assert L.odhip_dering_cache_dist_served(cache) == 1
    assert L.odhip_dering_cache_set_source(cache, None, src.d.data_ptr(), src.stride, 1, 0) == EINVAL
    assert L.odhip_dering_cache_set_source(cache, src.h.ctypes.data, None, src.stride, 1, 0) == EINVAL
    assert L.odhip_dering_cache_set_source(cache, src.h.ctypes.data, src.d.data_ptr(), 0, 1, 0) == EINVAL
