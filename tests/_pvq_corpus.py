"""The directed corpus of the PVQ band stages: named bands (name, n, x0, r0) for n = 8, 15, 32 and
128 whose QM-scaled int16 vectors - pvq_theta's x16[i] = shr_round(x0[i]*qm[i], 11 + xshift) and
r16 likewise - are tied, degenerate or extreme in a way random Laplacian bands almost never are:
null vectors, collinear and orthogonal pairs, pairs one LSB off either, several equal maxima of
|r16| (the Householder axis), equal |x16| (the greedy search's ties), single spikes, gain ladders,
all of them from max |x0| = 1 to the peak of the frame pipeline.  numpy only: the checkers that
read it (tests/test_pvq_corpus_host.py, tests/test_gpu_pvq_corpus.py,
tools/make_golden_pvq_corpus.py) bring the oracle.

A case is built from integer SHAPES vx, vr and one-LSB offsets ex, er: x16 = vx*mx + ex and
r16 = vr*mr + er, with the multipliers taken from the amplitude, and x0 / r0 the integers of
smallest magnitude that the band's own qm slice maps to those targets (every matrix entry is
<= 2048 = 2^11, so every target is reachable at every shift).  Proportions, ties, zeros of the dot
product and the LSB offsets therefore hold exactly where pvq_theta looks at them."""
import zlib

import numpy as np

SIZES = (8, 15, 32, 128)
AMPLITUDES = (1, 20, 400, 8000, 270000)      # max |x0|; the last: the frame pipeline's peak (od_lift.cuh)
QUANTIZERS = (12, 37, 243, 1264)
K_BOUND = 3000                               # max|x0|*sqrt(n)/q0 below which K stays inside ODHIP_PVQ_MAX_K
Q_QM_SHIFT = 11
BAND_OFFSETS = (1, 16, 24, 32, 64, 96, 128, 256, 384, 512)
NBANDS = (1, 4, 7, 9, 9)
# where a band of n coefficients starts in a 16x16 block's coding order (band-level checks)
BAND_START = {15: 1, 8: 16, 32: 32, 128: 128}
CLASSES = ("nulls", "collinear", "anti", "gate", "near1", "axis", "ties", "spikes", "ladder")


def _ilog(v):
    return int(v).bit_length()


def vector_log_mag(x):
    """od_vector_log_mag (src/pvq.c:472-484) of an int32 vector."""
    t = (np.asarray(x, np.int64) >> 8).astype(np.int16).astype(np.int64)
    return 8 + 1 + _ilog(len(x) + int((t * t).sum())) // 2


def band_shift(x, headroom):
    """pvq_theta's xshift (headroom 15) / rshift (headroom 14) of the band x."""
    return max(0, vector_log_mag(x) - headroom)


def scale16(x, qm, shift):
    """shr_round(x*qm, 11 + shift) as int16: pvq_theta's x16 / r16."""
    s = Q_QM_SHIFT + shift
    v = (np.asarray(x, np.int64) * np.asarray(qm, np.int64) + (1 << (s - 1))) >> s
    return v.astype(np.int16)


def _preimage(t, qm, shift):
    """Per coefficient the integer of smallest magnitude that scale16 maps to the target t."""
    s = Q_QM_SHIFT + shift
    t = np.asarray(t, np.int64)
    q = np.asarray(qm, np.int64)
    half = 1 << (s - 1)
    lo = (t << s) - half                      # lo <= x*qm < lo + 2^s
    pos = -((-lo) // q)                       # ceil(lo/q)
    neg = (lo + (1 << s) - 1) // q            # floor((lo + 2^s - 1)/q)
    x = np.where(t > 0, pos, np.where(t < 0, neg, 0))
    assert np.array_equal(scale16(x, qm, shift), t.astype(np.int16))
    return x.astype(np.int32)


def lift(v, e, qm, amp, headroom, scale=None):
    """The int32 band whose int16 image is v*mult + e at the shift pvq_theta derives from the band
    itself, with mult such that max |x0| is about amp (or mult*2^shift about `scale` when given).
    Returns (x0, target16)."""
    v = np.asarray(v, np.int64)
    e = np.asarray(e, np.int64)
    if not v.any() and not e.any():
        return np.zeros(len(v), np.int32), np.zeros(len(v), np.int16)
    vm = max(1, int(np.abs(v).max()))
    qmin = int(np.asarray(qm)[(v != 0) | (e != 0)].min())
    if scale is None:
        scale = amp * qmin / 2048. / vm
    for attempt in range(8):
        for shift in range(0, 12):
            mult = max(1, int(round(scale / (1 << shift))))
            t = v * mult + e
            if np.abs(t).max() > 32767:
                continue
            x0 = _preimage(t, qm, shift)
            if band_shift(x0, headroom) == shift:
                return x0, t.astype(np.int16)
        scale *= 0.93                          # on a shift boundary: a little smaller
    raise AssertionError("no self-consistent shift for this shape")


def _e(n, *pos_val):
    a = np.zeros(n, np.int64)
    for p, val in pos_val:
        a[p] = val
    return a


def _shapes(n):
    """(class, variant, vx, vr, ex, er, core): the shapes of one band size.  core shapes are built at
    every amplitude, the others at two (rotating, so that every class meets every amplitude)."""
    z = np.zeros(n, np.int64)
    one = np.ones(n, np.int64)
    idx = np.arange(n)
    ramp = idx + 1
    alt = np.where(idx % 2 == 0, 1, -1)
    first, mid, last = 0, n // 2, n - 1
    out = []

    def add(cls, variant, vx, vr, ex=z, er=z, core=False):
        out.append((cls, variant, np.asarray(vx, np.int64), np.asarray(vr, np.int64),
                    np.asarray(ex, np.int64), np.asarray(er, np.int64), core))

    # ---- nulls
    add("nulls", "x0_r0", z, z)
    add("nulls", "x0_rramp", z, ramp)
    add("nulls", "xramp_r0", ramp, z, core=True)
    add("nulls", "xalt_r0", alt * (1 + idx % 3), z)
    # ---- collinear
    add("collinear", "ramp", ramp, ramp, core=True)
    add("collinear", "const", one, one, core=True)
    add("collinear", "alt", alt, alt)
    # a square number of ones: the norm is an integer, so that g*gr is the dot product exactly
    square = (idx < int(np.sqrt(n / 2. + 1)) ** 2).astype(np.int64)
    add("collinear", "square", square, square, core=True)
    add("collinear", "x2r_ramp", 2 * ramp, ramp)
    add("collinear", "r2x_const", one, 2 * one)
    add("anti", "ramp", ramp, -ramp, core=True)
    add("anti", "square", square, -square)
    add("anti", "const", one, -one)
    add("anti", "alt", alt, -alt)
    # ---- the corr > 0 gate: integer-orthogonal pairs, and one LSB to either side
    for tag, p in (("p0", first), ("pmid", mid - 1)):
        vx, vr = _e(n, (p, 1), (p + 1, 1)), _e(n, (p, 1), (p + 1, -1))
        add("gate", "narrow_%s" % tag, vx, vr, core=(tag == "p0"))
        add("gate", "narrow_%s_plus" % tag, vx, vr, ex=_e(n, (p, 1)))
        add("gate", "narrow_%s_minus" % tag, vx, vr, ex=_e(n, (p + 1, 1)))
    halves = np.where(idx < n // 2, 1, -1)
    if n % 2:
        halves[mid] = 0
    add("gate", "wide", one, halves, core=True)
    add("gate", "wide_plus", one, halves, ex=_e(n, (first, 1)))
    add("gate", "wide_minus", one, halves, ex=_e(n, (last, 1)))
    # ---- near corr = 1: x = r plus one LSB
    for tag, p in (("first", first), ("mid", mid), ("last", last)):
        add("near1", "ramp_%s" % tag, ramp, ramp, ex=_e(n, (p, 1)), core=(tag == "mid"))
        add("near1", "const_%s" % tag, one, one, ex=_e(n, (p, -1 if tag == "mid" else 1)))
    # ---- Householder axis: equal maxima of |r16|
    base = 1 + idx % 3
    near = base + alt                          # correlated with base, not collinear
    for variant, peaks in (("first_last", ((first, 5), (last, 5))),
                           ("adjacent", ((mid, 5), (mid + 1, 5))),
                           ("opposite", ((1, -5), (last - 1, 5))),
                           ("three", ((1, 5), (mid, -5), (last, 5))),
                           ("max_at_0", ((first, 5),)),
                           ("max_at_last", ((last, -5),))):
        vr = base.copy()
        for p, val in peaks:
            vr[p] = val
        vx = near.copy()
        for p, val in peaks:
            vx[p] = val - (1 if val > 0 else -1)
        add("axis", variant, vx, vr, core=variant in ("first_last", "opposite"))
    add("axis", "all_equal", ramp, one, core=True)
    add("axis", "all_equal_neg", -ramp, -one)
    add("axis", "all_equal_signs", ramp * alt, alt)
    vr = base.copy()
    vr[mid] = 7
    add("axis", "unique_on_spike", _e(n, (mid, 3)), vr)
    # ---- greedy ties: equal |x16|, without a reference and with a reference of one unique maximum
    def along(vx, p):
        """A reference of +-1 with the signs of vx and one unique maximum, at p."""
        vr = np.where(vx < 0, -1, 1)
        vr[p] *= 3
        return vr

    def refs(vx, core_first=False):
        yield "r0", z, core_first
        yield "rmax_mid", along(vx, mid), False
        yield "rmax_first", along(vx, first), False

    flats = (("flat_pos", one), ("flat_alt", alt), ("flat_neg", -one),
             ("flat_one_neg", one - 2 * _e(n, (mid, 1))), ("flat_halves", np.where(idx < n // 2, 1, -1)))
    for variant, vx in flats:
        for rtag, vr, core in refs(vx, variant in ("flat_pos", "flat_alt")):
            if rtag == "rmax_first" and variant not in ("flat_pos", "flat_alt"):
                continue
            add("ties", "%s_%s" % (variant, rtag), vx, vr, core=core or (variant == "flat_pos" and rtag == "rmax_mid"))
    two = 1 + idx % 2
    add("ties", "two_level_r0", two * alt, z)
    add("ties", "two_level_rmax_mid", two, along(two, mid))
    add("ties", "two_level_blocks_r0", np.where(idx < n // 2, 2, 1), z)
    perm = np.random.RandomState(n).permutation(n)
    add("ties", "pairs_shuffled_r0", (1 + np.arange(n) // 2)[perm], z)
    vx = (1 + np.arange(n) // 2)[perm] * alt
    add("ties", "pairs_shuffled_rmax_last", vx, along(vx, last))
    for j in (1, 2, 4, 8, 16, 32, 64):
        if j >= n:
            continue
        p0 = (n - j) // 2
        vx = idx % 3
        vx[p0] = vx[p0 + j] = 5
        add("ties", "apart%d_r0" % j, vx, z, core=(j == n // 2 or j == 1))
        vx = vx * np.where(idx < mid, 1, -1)
        # the axis between the two (on the second when j = 1)
        add("ties", "apart%d_rmax_between" % j, vx, along(vx, min(p0 + (j + 1) // 2, last)))
        vx = idx % 3
        vx[first] = vx[j] = -5
        add("ties", "apart%d_from0_neg_r0" % j, vx, z)
    # ---- spikes
    for tag, p in (("first", first), ("mid", mid), ("last", last)):
        add("spikes", "%s_match" % tag, _e(n, (p, 1)), _e(n, (p, 1)), core=(tag == "mid"))
    add("spikes", "first_orth", _e(n, (first, 1)), _e(n, (last, 1)))
    add("spikes", "last_const", _e(n, (last, -1)), -one)
    add("spikes", "mid_r0", _e(n, (mid, -1)), z)
    add("spikes", "floor_mid_r0", alt + _e(n, (mid, 9 - alt[mid])), z, core=True)
    add("spikes", "floor_first_const", alt + _e(n, (first, 9 - alt[first])), one)
    return out


def _ladder(n, a):
    """The ladder's shape at peak a (int16 domain): norm about 1.2*a."""
    vx = np.zeros(n, np.int64)
    vx[:4] = (a, -(a // 2), a // 3, a // 4)
    vr = vx.copy()
    vr[4] = a // 2 + 1
    return vx, vr


def cases(n, qm, quantizers=QUANTIZERS):
    """The corpus of one band of n coefficients whose slice of the quantisation matrix is qm:
    a list of (name, n, x0, r0), name = class/variant/aAMPLITUDE (a ladder's: its int16 peak)."""
    qm = np.asarray(qm, np.int16)
    assert len(qm) == n
    key = (n, qm.tobytes(), tuple(quantizers))
    if key not in _case_cache:
        _case_cache[key] = _build_cases(n, qm, quantizers)
    return _case_cache[key]


_case_cache = {}


def _build_cases(n, qm, quantizers):
    out = []
    for si, (cls, variant, vx, vr, ex, er, core) in enumerate(_shapes(n)):
        amps = AMPLITUDES if core else (AMPLITUDES[si % 5], AMPLITUDES[(si + 2) % 5])
        for amp in amps:
            x0, _ = lift(vx, ex, qm, amp, 15)
            r0, _ = lift(vr, er, qm, amp, 14)
            out.append(("%s/%s/a%d" % (cls, variant, amp), n, x0, r0))
    # one shape at 16 consecutive amplitudes across the gain-index boundaries of each quantiser
    # (|x16| runs geometrically from 1/25 of the step - gain index 0 also where beta = 1.5 compands
    # small gains upwards - to four steps)
    z = np.zeros(n, np.int64)
    for q0 in quantizers:
        for step in range(16):
            a = max(2, int(round(q0 * 0.04 * 100. ** (step / 15.) / 1.2)))
            vx, vr = _ladder(n, a)
            x0, _ = lift(vx, z, qm, 0, 15, scale=1.)
            r0, _ = lift(vr, z, qm, 0, 14, scale=1.)
            out.append(("ladder/q%d_step%02d/p%d" % (q0, step, a), n, x0, r0))
    return out


def quantizers_for(n, x0, quantizers=QUANTIZERS):
    """The quantisers a case is compared at: those that keep every K of pvq_theta inside
    ODHIP_PVQ_MAX_K.  A bound on the INPUTS (never on what the code under test returns); every case
    keeps at least the coarsest quantiser."""
    m = int(np.abs(x0).max()) if len(x0) else 0
    return [q for q in quantizers if m * np.sqrt(n) / q < K_BOUND]


def digest(case_list):
    """CRC-32 over the names and the inputs of a case list."""
    c = 0
    for name, n, x0, r0 in case_list:
        c = zlib.crc32(name.encode(), c)
        c = zlib.crc32(np.ascontiguousarray(x0, "<i4").tobytes(), c)
        c = zlib.crc32(np.ascontiguousarray(r0, "<i4").tobytes(), c)
    return c


def plane_blocks(bs, qm, q_band=None):
    """How many blocks per plane hold every case of the band size at home at level bs (15 at 4x4, 8
    at 8x8, 32 at 16x16, 128 at 32x32 and above)."""
    home = (15, 8, 32, 128, 128)[bs]
    bands = [b for b in range(NBANDS[bs]) if BAND_OFFSETS[b + 1] - BAND_OFFSETS[b] == home]
    need = 0
    for b in bands:
        a = BAND_OFFSETS[b]
        cs = cases(home, qm[a:a + home])
        fine = sum(1 for c in cs if q_band is None or _inside(c, q_band[b]))
        need = max(need, fine, len(cs) - fine)
    return -(-need // len(bands)) + 1


def _inside(case, q0):
    name, n, x0, _ = case
    return int(np.abs(x0).max(initial=0)) * np.sqrt(n) / q0 < K_BOUND


def plane_width(bs, qm, rows=64, q_band=None):
    """The width at which a plane of `rows` rows holds plane_blocks() blocks, a multiple of 32 and of the
    block size."""
    blk = 4 << bs
    cols = -(-plane_blocks(bs, qm, q_band) // (rows // blk))
    unit = max(blk, 32)
    return -(-cols * blk // unit) * unit


def corpus_planes(bs, qm, to_raster, w=None, rows=64, seed=0, rotate=0, q_band=None, q_coarse=None):
    """Coefficient and reference planes [nplanes][rows][w] of blocks of side 4 << bs that hold the
    corpus: the cases of every band size n are dealt over the bands of n coefficients, block after
    block (starting at case `rotate`), each built from that band's own slice of qm (the block's
    matrix in coding order).  DC and the bands left over keep mild random values.
    to_raster(block_vector, n) -> [n][n] is the oracle's odo_coding_order_to_raster.

    q_band None: one plane with every case.  With the per-band quantisers q_band and q_coarse: two
    planes, the first with the cases that keep K inside ODHIP_PVQ_MAX_K at the band's own step (K_BOUND),
    the second - to be coded at q_coarse, which keeps every case inside - with the others, so that no
    case is dropped.  Returns (x, r, names) with names[(blk, band)] the case name, blk counting through
    the planes."""
    blk = 4 << bs
    if w is None:
        w = plane_width(bs, qm, rows, q_band)
    assert rows % blk == 0 and w % blk == 0
    bh, bw = rows // blk, w // blk
    nblocks = bh * bw
    nplanes = 1 if q_band is None else 2
    ln = min(blk * blk, 512)
    rng = np.random.RandomState(1000 + 10 * bs + seed)
    vx = rng.randint(-30, 31, size=(nplanes * nblocks, blk * blk)).astype(np.int32)
    vr = rng.randint(-30, 31, size=(nplanes * nblocks, blk * blk)).astype(np.int32)
    vx[:, ln:] = 0
    vr[:, ln:] = 0
    names = {}
    by_size = {}
    for b in range(NBANDS[bs]):
        by_size.setdefault(BAND_OFFSETS[b + 1] - BAND_OFFSETS[b], []).append(b)
    for n, bands in by_size.items():
        count = [0] * nplanes
        lists = {b: cases(n, qm[BAND_OFFSETS[b]:BAND_OFFSETS[b] + n]) for b in bands}
        ncases = len(lists[bands[0]])
        for i in range(ncases):
            j = (i + rotate) % ncases
            # the same case goes to the same plane whichever band of this size holds it
            p = 0
            if q_band is not None and not all(_inside(lists[b][j], q_band[b]) for b in bands):
                assert all(_inside(lists[b][j], q_coarse) for b in bands), lists[bands[0]][j][0]
                p = 1
            k, b = divmod(count[p], len(bands))
            if k >= nblocks:
                continue                        # a level narrower than this size's home level
            count[p] += 1
            b = bands[b]
            name, _, x0, r0 = lists[b][j]
            a = BAND_OFFSETS[b]
            vx[p * nblocks + k, a:a + n] = x0
            vr[p * nblocks + k, a:a + n] = r0
            names[(p * nblocks + k, b)] = name
    x = np.zeros((nplanes, rows, w), np.int32)
    r = np.zeros((nplanes, rows, w), np.int32)
    for k in range(nplanes * nblocks):
        p, rem = divmod(k, nblocks)
        by, bx = divmod(rem, bw)
        x[p, by * blk:(by + 1) * blk, bx * blk:(bx + 1) * blk] = to_raster(vx[k], blk)
        r[p, by * blk:(by + 1) * blk, bx * blk:(bx + 1) * blk] = to_raster(vr[k], blk)
    return x, r, names


def search_vectors(n):
    """int16 tie and spike vectors of ANY length n for the stand-alone search: the shapes of the two
    classes at three magnitudes (1, 37 and near the int16 limit)."""
    out = []
    for cls, variant, vx, _, ex, _, _ in _shapes(n):
        if cls not in ("ties", "spikes") or not variant.endswith(("_r0", "_match")):
            continue
        top = 32767 // max(1, int(np.abs(vx).max()))
        for mult in (1, min(37, top), top):
            out.append(("%s/%s/x%d" % (cls, variant, mult), (vx * mult + ex).astype(np.int16)))
    return out
