"""The frame cache (daala_amd/csrc/frame_cache.hip: odhip_cache_*) called directly: the batched
pyramid behind every fdct_2d call and the batched band stage behind pvq_theta, bit-exact against
the CPU oracle (odo_forward_pyramid_plane, odo_fdct_2d, odo_pvq_theta), and the bookkeeping that
decides which result a call gets: address keys, reload rules, the key of the cached band stage."""
import ctypes

import numpy as np
import pytest

from _band_oracle import band_trace, block_vector
from _caches import DCT_TABLE, EINVAL, BandCands, Pinned, addr, pair, pulses
from _libs import P, oracle, synth_frame

pytestmark = pytest.mark.gpu
vp = ctypes.c_void_p
SENT = 0x5a5a5a5a
PIC = (120, 60)                    # the picture: smaller than the 128x64 / 64x32 planes
DIMS = {0: (128, 64, 0), 1: (64, 32, 1)}      # plane slot -> (w, h, dec)
MARGIN = 128                       # od_coeffs around each plane: addresses next to it belong to nobody


def pixels(seed):
    """Textured planes, so that gains above 1 and multi-pulse searches occur."""
    planes = synth_frame(128, 64, seed=seed)
    rng = np.random.RandomState(seed + 12)
    return {pli: np.clip(planes[pli].astype(int) + rng.randint(-60, 61, size=planes[pli].shape), 0, 255)
            .astype(np.uint8) for pli in (0, 1)}


def oracle_pyramid(px, dec, pic):
    h, w = px.shape
    lv = [np.zeros((h, w), np.int32) for _ in range(5 - dec)]
    arr = (ctypes.c_void_p * 5)(*[l.ctypes.data for l in lv])
    c = np.zeros((h, w), np.int32)
    oracle().odo_forward_pyramid_plane(arr, P(c), P(px), w, w, h, dec, pic[0], pic[1])
    return lv


def oracle_fdct(bs, block):
    n = 4 << bs
    x = np.ascontiguousarray(block, np.int32)
    y = np.zeros((n, n), np.int32)
    oracle().odo_fdct_2d(bs, P(y), n, P(x), n)
    return y


class Planes:
    """The encoder's coefficient planes ((p - 128) << 4, stride == w) at fixed host addresses, each
    inside a buffer of its own with a margin on both sides."""

    def __init__(self, seed=5):
        self.keep = Pinned()
        self.buf = {}
        self.coef = {}
        for pli, (w, h, _) in DIMS.items():
            self.buf[pli] = self.keep.array(w * h + 2 * MARGIN, np.int32, 0)
            self.coef[pli] = self.buf[pli][MARGIN:MARGIN + w * h].reshape(h, w)
        self.fill(seed)

    def fill(self, seed):
        self.px = pixels(seed)
        for pli in DIMS:
            self.coef[pli][...] = (self.px[pli].astype(np.int32) - 128) << 4

    def load(self, L, c, pli):
        w, h, dec = DIMS[pli]
        return L.odhip_cache_load_plane(c, pli, self.coef[pli].ctypes.data, w, w, h, dec)


@pytest.fixture(scope="module")
def D():
    import torch
    import daala_amd
    assert torch.cuda.is_available()
    daala_amd.init(0)
    return daala_amd


@pytest.fixture(scope="module")
def L(D):
    return D.lib()


@pytest.fixture
def cache(L):
    c = L.odhip_cache_create()
    assert c
    L.odhip_cache_set_picture(c, *PIC)
    yield c
    L.odhip_cache_make_current(None)
    L.odhip_cache_destroy(c)


def lookup(L, c, ptr, in_stride, bs):
    """odhip_cache_lookup into a sentinel-filled buffer with out_stride > n: (rc, the block)."""
    n = 4 << bs
    out = np.full((n + 2, n + 5), SENT, np.int32)
    rc = L.odhip_cache_lookup(c, ptr, in_stride, bs, addr(out, 1, 2), n + 5)
    blk = out[1:1 + n, 2:2 + n].copy()
    out[1:1 + n, 2:2 + n] = SENT
    assert (out == SENT).all(), "wrote outside its block"
    return rc, blk


def check_pyramid(L, c, pl, pli, want):
    """Every aligned block of every level of a plane, against the oracle's levels; returns the
    number of lookups."""
    w, h, dec = DIMS[pli]
    count = 0
    for bs in range(5 - dec):
        n = 4 << bs
        for by in range(h // n):
            for bx in range(w // n):
                rc, blk = lookup(L, c, addr(pl.coef[pli], by * n, bx * n), w, bs)
                assert rc == 1, (pli, bs, bx, by)
                assert np.array_equal(blk, want[bs][by * n:(by + 1) * n, bx * n:(bx + 1) * n]), (pli, bs, bx, by)
                count += 1
    return count


def test_lookups_serve_the_pixels_of_the_load(L, cache):
    """The encoder laps the plane in place after the load: the cache serves the pyramid of the
    pixels it was given, whatever the caller's buffer holds afterwards."""
    pl = Planes()
    want = {pli: oracle_pyramid(pl.px[pli], DIMS[pli][2], PIC) for pli in DIMS}
    for pli in DIMS:
        assert pl.load(L, cache, pli) == 0
    rng = np.random.RandomState(1)
    for pli in DIMS:
        pl.coef[pli][...] = rng.randint(-30000, 30000, size=pl.coef[pli].shape)
    total = sum(check_pyramid(L, cache, pl, pli, want[pli]) for pli in DIMS)
    assert total == 682 + 170
    assert pair(L.odhip_cache_stats, cache) == (total, 0)


def test_lookup_misses(L, cache):
    pl = Planes()
    for pli in DIMS:
        assert pl.load(L, cache, pli) == 0
    luma, chroma = pl.coef[0], pl.coef[1]
    cases = {
        "x not a multiple of n": (addr(luma, 0, 4), 128, 1),
        "y not a multiple of n": (addr(luma, 8, 0), 128, 2),
        "in_stride != w": (addr(luma, 0, 0), 129, 1),
        "in_stride of the other plane": (addr(luma, 0, 0), 64, 1),
        "one element before the plane": (addr(luma, 0, 0) - 4, 128, 0),
        "one element past the plane": (addr(luma, 63, 127) + 4, 128, 0),
        "one element before the chroma plane": (addr(chroma, 0, 0) - 4, 64, 0),
        "one element past the chroma plane": (addr(chroma, 31, 63) + 4, 64, 0),
        "bs above 4 - dec": (addr(chroma, 0, 0), 64, 4),
        # a block reaching over an edge: in a plane of whole tiles such a position is never aligned,
        # so these are refused as unaligned before the edge test is reached
        "unaligned, over the right edge": (addr(luma, 0, 96), 128, 4),
        "unaligned, over the bottom edge": (addr(luma, 48, 0), 128, 3),
        "unaligned, over the bottom edge of chroma": (addr(chroma, 16, 32), 64, 3),
    }
    for i, (what, (ptr, stride, bs)) in enumerate(cases.items()):
        rc, blk = lookup(L, cache, ptr, stride, bs)
        assert rc == 0 and (blk == SENT).all(), what
        assert pair(L.odhip_cache_stats, cache) == (0, i + 1), what
    # the control: the same calls, put right, hit
    assert lookup(L, cache, addr(luma, 0, 8), 128, 1)[0] == 1
    assert lookup(L, cache, addr(chroma, 0, 0), 64, 3)[0] == 1


def test_function_table(L, cache):
    """odhip_install_cached_dct_vtbl: fdct_2d[bs] serves the (lapped) pyramid block for a pointer
    into a loaded plane of the thread's current cache, and is the plain transform otherwise."""
    pl = Planes()
    want = oracle_pyramid(pl.px[0], 0, PIC)
    assert pl.load(L, cache, 0) == 0
    fd, idt = DCT_TABLE(), DCT_TABLE()
    L.odhip_install_cached_dct_vtbl(fd, idt)
    rng = np.random.RandomState(2)
    w = 128
    for bs in range(5):
        n = 4 << bs
        by, bx = (64 // n) - 1, (128 // n) // 2
        inp = addr(pl.coef[0], by * n, bx * n)
        block = pl.coef[0][by * n:(by + 1) * n, bx * n:(bx + 1) * n]
        cached = want[bs][by * n:(by + 1) * n, bx * n:(bx + 1) * n]
        plain = oracle_fdct(bs, block)
        assert not np.array_equal(cached, plain), "lapping does not show here: the case proves nothing"
        foreign = np.ascontiguousarray(rng.randint(-2048, 2048, size=(n, n)).astype(np.int32))

        def run(src_ptr, src_stride):
            out = np.full((n, n + 3), SENT, np.int32)
            fd[bs](out.ctypes.data, n + 3, src_ptr, src_stride)
            assert (out[:, n:] == SENT).all()
            return out[:, :n]

        L.odhip_cache_make_current(cache)
        assert np.array_equal(run(inp, w), cached), bs
        assert np.array_equal(run(foreign.ctypes.data, n), oracle_fdct(bs, foreign)), bs
        L.odhip_cache_make_current(None)
        assert np.array_equal(run(inp, w), plain), bs
    assert pair(L.odhip_cache_stats, cache) == (5, 5)


# ---- the band stage ----------------------------------------------------------------------

_TRACES = {}


def oracle_block(D, qt, level, pli, dec, bs, bx, by, lam):
    """The oracle's records of every band of block (bx, by) of `level` (block size bs of a plane in slot pli,
    decimation dec), keyed and shaped as oracle_bands' are."""
    n = 4 << bs
    off = int(qt.qm_offset[bs][dec])
    ln = min(n * n, 512)
    qm, qmi = np.ascontiguousarray(qt.qm[off:off + ln]), np.ascontiguousarray(qt.qm_inv[off:off + ln])
    qb, bb = qt.q_band(pli, bs), qt.beta_band(pli, bs)
    nb, offs, _ = D.pvq_band_layout(bs)
    vec = block_vector(level, n, bx, by)
    out = {}
    for band in range(nb):
        a, b = offs[band], offs[band + 1]
        tr, nr = band_trace(vec[a:b], qb[band], bb[band], qm[a:b], qmi[a:b], lam)
        cands = [(c.gain, c.k, c.searched, c.dist if c.searched else None,
                  tuple(c.y[:b - a]) if c.searched else None) for c in nr]
        out[(pli, bs, bx, by, band)] = (b - a, qb[band], bb[band], tr.cg, tr.dist0, cands)
    return out


def oracle_bands(D, px_seed, quality, lam, masking):
    """The oracle's no-reference pvq_theta record of every band of every block of every level of
    both planes: {(pli, bs, bx, by, band): (n, q, beta, cg, dist0, [(gain, k, searched, dist, y)])}.
    Computed once per setting."""
    key = (px_seed, quality, lam, masking)
    if key in _TRACES:
        return _TRACES[key]
    qt = D.QuantTables.for_quality(quality, use_masking=masking)
    px = pixels(px_seed)
    out = {}
    for pli, (w, h, dec) in DIMS.items():
        levels = oracle_pyramid(px[pli], dec, PIC)
        for bs in range(5 - dec):
            n = 4 << bs
            for by in range(h // n):
                for bx in range(w // n):
                    out.update(oracle_block(D, qt, levels[bs], pli, dec, bs, bx, by, lam))
    _TRACES[key] = out
    return out


def check_bands(L, c, want):
    """odhip_cache_band of every record in `want` against it; returns the number of searched
    candidates."""
    nsearched = 0
    multi = 0
    out = BandCands()
    for (pli, bs, bx, by, band), (n, q, beta, cg, dist0, cands) in want.items():
        where = (pli, bs, bx, by, band)
        assert L.odhip_cache_band(c, pli, bs, bx, by, band, None, ctypes.byref(out)) == 1, where
        assert (out.n, out.q, out.beta, out.cg) == (n, q, beta, cg), where
        assert out.dist0 == dist0, where
        for slot in range(2):
            if slot >= len(cands):
                assert out.gain[slot] == 0 and out.flags[slot] == 0, where
                continue
            gain, k, searched, dist, y = cands[slot]
            assert (out.gain[slot], out.k[slot], out.flags[slot]) == (gain, k, searched), where
            if searched:
                nsearched += 1
                multi += gain > 1 and k > 1
                assert out.dist[slot] == dist, where
                assert pulses(out, slot, n) == y, where
    assert nsearched > 0 and multi > 0
    return nsearched


def load_bands(L, c, D, pli, quality, lam, masking):
    qt = D.QuantTables.for_quality(quality, use_masking=masking)
    return L.odhip_cache_load_bands(c, pli, ctypes.byref(qt.c), lam)


def test_band_stage_and_its_key(L, D, cache):
    """Every record of both planes at the default quality; then quality, lambda and masking changed
    ONE at a time, from the default and back to it: each load serves the records of ITS setting, so
    each of the three is part of the key in both directions."""
    pl = Planes()
    lam = D.OD_PVQ_LAMBDA
    for pli in DIMS:
        assert pl.load(L, cache, pli) == 0
    base = oracle_bands(D, 5, 20, lam, 1)
    assert len(base) == 1338 + 330
    default = (20, lam, 1)
    settings = [default, (40, lam, 1), default, (20, 0.3, 1), default, (20, lam, 0), default]
    hits = 0
    for quality, lm, masking in settings:
        want = oracle_bands(D, 5, quality, lm, masking)
        if (quality, lm, masking) != default:
            assert sum(want[k] != base[k] for k in want) > 100, "this change changes no record: the case proves nothing"
        for pli in DIMS:
            assert load_bands(L, cache, D, pli, quality, lm, masking) == 0
        check_bands(L, cache, want)
        hits += len(want)
    assert pair(L.odhip_cache_band_stats, cache) == (hits, 0)
    # out of range: 0 and a miss
    out = BandCands()
    bad = [(0, 5, 0, 0, 0), (0, -1, 0, 0, 0), (1, 4, 0, 0, 0), (0, 1, 16, 0, 0), (0, 1, 0, 8, 0), (0, 1, -1, 0, 0),
           (0, 1, 0, -1, 0), (0, 1, 0, 0, 4), (0, 1, 0, 0, -1), (1, 3, 2, 0, 0), (1, 3, 0, 1, 0), (0, 4, 0, 0, 9)]
    for i, (pli, bs, bx, by, band) in enumerate(bad):
        assert L.odhip_cache_band(cache, pli, bs, bx, by, band, None, ctypes.byref(out)) == 0, bad[i]
        assert pair(L.odhip_cache_band_stats, cache) == (hits, i + 1), bad[i]
    assert L.odhip_cache_band(cache, 2, 0, 0, 0, 0, None, ctypes.byref(out)) == 0      # a slot never loaded
    assert load_bands(L, cache, D, 2, 20, lam, 1) == EINVAL


def test_plane_pixels(L, cache):
    """odhip_cache_plane_pixels: the samples of the load, on the host and on the device (the device
    copy read the way its consumer reads it: odhip_dist_parts_px16 against the same samples as
    int16 coefficients gives a zero squared error in every 8x8 block, and not with one changed)."""
    import torch
    pl = Planes()
    hp, dp, w, h = vp(), vp(), ctypes.c_int(), ctypes.c_int()
    args = (ctypes.byref(hp), ctypes.byref(dp), ctypes.byref(w), ctypes.byref(h))
    assert L.odhip_cache_plane_pixels(cache, 0, *args) == EINVAL
    for pli in DIMS:
        assert pl.load(L, cache, pli) == 0
    for pli, (pw, ph, _) in DIMS.items():
        assert L.odhip_cache_plane_pixels(cache, pli, *args) == 0
        assert (w.value, h.value) == (pw, ph)
        host = np.frombuffer(ctypes.string_at(hp.value, pw * ph), np.uint8).reshape(ph, pw)
        assert np.array_equal(host, pl.px[pli])
        for poke in (0, 1):
            y16 = pl.coef[pli].astype(np.int16)
            y16[ph - 1, pw - 1] += poke
            ty = torch.from_numpy(y16).cuda()
            parts = torch.full((ph // 8, pw // 8, 3), -1.0, dtype=torch.float64, device="cuda")
            assert L.odhip_dist_parts_px16(vp(parts.data_ptr()), dp, pw, vp(ty.data_ptr()), pw, 1, pw, ph, 1, 0, 1,
                                           None) == 0
            torch.cuda.synchronize()
            sq = parts.cpu().numpy()[:, :, 0]
            assert (sq != 0).sum() == poke and sq[-1, -1] == poke
    assert L.odhip_cache_plane_pixels(cache, 4, *args) == EINVAL
    assert L.odhip_cache_plane_pixels(cache, 2, *args) == EINVAL


# ---- reload rules ------------------------------------------------------------------------

def band_hit(L, c, pli=0):
    out = BandCands()
    return L.odhip_cache_band(c, pli, 1, 1, 1, 2, None, ctypes.byref(out))


def test_reload_rules(L, D, cache):
    lam = D.OD_PVQ_LAMBDA
    pl = Planes(5)
    want5 = oracle_pyramid(pl.px[0], 0, PIC)
    assert pl.load(L, cache, 0) == 0
    assert load_bands(L, cache, D, 0, 20, lam, 1) == 0
    assert band_hit(L, cache) == 1
    # the same pixels at the same address (the encoder's second RDO pass): everything survives
    assert pl.load(L, cache, 0) == 0
    assert band_hit(L, cache) == 1
    check_pyramid(L, cache, pl, 0, want5)
    # other pixels at the same address: a new pyramid, no band stage until it is loaded
    pl.fill(6)
    want6 = oracle_pyramid(pl.px[0], 0, PIC)
    assert not np.array_equal(want5[1], want6[1])
    assert pl.load(L, cache, 0) == 0
    check_pyramid(L, cache, pl, 0, want6)
    misses = pair(L.odhip_cache_band_stats, cache)[1]
    assert band_hit(L, cache) == 0
    assert pair(L.odhip_cache_band_stats, cache)[1] == misses + 1
    assert load_bands(L, cache, D, 0, 20, lam, 1) == 0
    check_bands(L, cache, {k: v for k, v in oracle_bands(D, 6, 20, lam, 1).items() if k[0] == 0})
    # the same pixels, another picture size: a new pyramid, and no band stage of the old one
    pic2 = (100, 44)
    want6b = oracle_pyramid(pl.px[0], 0, pic2)
    assert any(not np.array_equal(a, b) for a, b in zip(want6, want6b))
    L.odhip_cache_set_picture(cache, *pic2)
    assert pl.load(L, cache, 0) == 0
    check_pyramid(L, cache, pl, 0, want6b)
    assert band_hit(L, cache) == 0
    L.odhip_cache_set_picture(cache, *PIC)
    assert pl.load(L, cache, 0) == 0
    check_pyramid(L, cache, pl, 0, want6)
    # not a fresh 8-bit plane: refused, and nothing is served from the slot afterwards
    for y, x, v in ((3, 5, ((77 - 128) << 4) | 1), (60, 127, (256 - 128) << 4), (0, 0, (-1 - 128) << 4)):
        assert pl.load(L, cache, 0) == 0
        assert lookup(L, cache, addr(pl.coef[0], 0, 0), 128, 1)[0] == 1
        old = pl.coef[0][y, x]
        pl.coef[0][y, x] = v
        assert pl.load(L, cache, 0) == EINVAL, (y, x, v)
        pl.coef[0][y, x] = old
        assert lookup(L, cache, addr(pl.coef[0], 0, 0), 128, 1)[0] == 0
        assert band_hit(L, cache) == 0
    # the geometry the cache takes: stride == w, whole tiles
    p0 = pl.coef[0].ctypes.data
    assert L.odhip_cache_load_plane(cache, 0, p0, 129, 128, 64, 0) == EINVAL
    assert L.odhip_cache_load_plane(cache, 0, p0, 96, 96, 64, 0) == EINVAL
    assert L.odhip_cache_load_plane(cache, 0, p0, 128, 128, 32, 0) == EINVAL
    assert L.odhip_cache_load_plane(cache, 1, p0, 48, 48, 32, 1) == EINVAL
    assert L.odhip_cache_load_plane(cache, 0, p0, 128, 128, 64, 2) == EINVAL
    assert L.odhip_cache_load_plane(cache, 4, p0, 128, 128, 64, 0) == EINVAL
    assert L.odhip_cache_load_plane(cache, 0, None, 128, 128, 64, 0) == EINVAL
    assert pl.load(L, cache, 0) == 0
    check_pyramid(L, cache, pl, 0, want6)


# ---- one cache across shapes --------------------------------------------------------------

SLOT = 1                                              # chroma: decimated or, in 4:4:4, not
SHAPES = [(64, 64, 0), (128, 192, 0), (64, 64, 1)]    # w, h, dec of the loads, in this order


def band_record(L, c, key):
    """What odhip_cache_band answers for key = (pli, bs, bx, by, band), as plain values (distortion and pulses
    of the searched candidates only: nothing else is defined)."""
    out = BandCands()
    assert L.odhip_cache_band(c, *key, None, ctypes.byref(out)) == 1, key
    cands = [(out.gain[s], out.k[s], out.flags[s], out.dist[s] if out.flags[s] else None,
              pulses(out, s, out.n) if out.flags[s] else None) for s in range(2)]
    return out.n, out.q, out.beta, out.cg, out.dist0, cands


def test_one_cache_across_shapes(L, D):
    """A small plane, a larger one, then the small size again at another decimation, all in one slot of one
    cache: after each load every lookup of every level and a sample of the band records equal the oracle's and
    those of a cache that has seen this load only.  The buffers of the slot are replaced at every step (the
    third load needs fewer levels of fewer samples than the second left behind)."""
    lam = D.OD_PVQ_LAMBDA
    qt = D.QuantTables.for_quality(20, use_masking=1)
    keep = Pinned()
    old = L.odhip_cache_create()
    assert old
    try:
        for step, (w, h, dec) in enumerate(SHAPES):
            pic = ((w << dec) - 6, (h << dec) - 10)
            rng = np.random.RandomState(40 + step)
            px = synth_frame(w << dec, h << dec, seed=30 + step)[1 if dec else 0]
            px = np.clip(px.astype(int) + rng.randint(-60, 61, size=px.shape), 0, 255).astype(np.uint8)
            assert px.shape == (h, w)
            coef = keep.like((px.astype(np.int32) - 128) << 4)
            want = oracle_pyramid(px, dec, pic)
            sample = {}
            for bs in range(5 - dec):
                n = 4 << bs
                for bx, by in {(0, 0), (w // n - 1, h // n - 1), (w // n // 2, h // n // 2), (0, h // n - 1)}:
                    sample.update(oracle_block(D, qt, want[bs], SLOT, dec, bs, bx, by, lam))
            fresh = L.odhip_cache_create()
            assert fresh
            try:
                answers = []
                for c in (old, fresh):
                    before = pair(L.odhip_cache_stats, c), pair(L.odhip_cache_band_stats, c)
                    L.odhip_cache_set_picture(c, *pic)
                    assert L.odhip_cache_load_plane(c, SLOT, coef.ctypes.data, w, w, h, dec) == 0
                    assert L.odhip_cache_load_bands(c, SLOT, ctypes.byref(qt.c), lam) == 0
                    got = []
                    for bs in range(5):
                        n = 4 << bs
                        for by in range(h // n):
                            for bx in range(w // n):
                                rc, blk = lookup(L, c, addr(coef, by * n, bx * n), w, bs)
                                assert rc == (bs <= 4 - dec), (step, bs, bx, by)
                                if rc:
                                    assert np.array_equal(blk, want[bs][by * n:(by + 1) * n, bx * n:(bx + 1) * n]), \
                                        (step, bs, bx, by)
                                got.append((rc, blk.tobytes()))
                    check_bands(L, c, sample)
                    got += [band_record(L, c, key) for key in sample]
                    after = pair(L.odhip_cache_stats, c), pair(L.odhip_cache_band_stats, c)
                    answers.append((got, [(a[0] - b[0], a[1] - b[1]) for a, b in zip(after, before)]))
                assert answers[0] == answers[1], step
            finally:
                L.odhip_cache_destroy(fresh)
    finally:
        L.odhip_cache_destroy(old)
