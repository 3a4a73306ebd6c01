"""GPU: every entry point that takes or produces a picture plane, called through ctypes with strides,
plane pitches and base offsets OFF the packed layout, on sentinel-surrounded buffers (tests/_strided.py),
bit-exact against the CPU oracle - and at the plane widths where the inverse walkers have a joint
between two segments and a partial last segment.

Layouts, in samples of the plane's type (`base` = offset from a 256-byte aligned address):

    name     stride   base   plane_stride    what it reaches
    packed   w        0      stride*h        control: what daala_amd.api passes
    gap16    w+16     16     stride*h+16     the 16-byte `wide` stores of the walkers next to gaps
    min4     w+4      4      stride*h+4      `wide` off through all three conditions; minimal alignment
    pitch4   w+16     0      stride*h+4      `wide` off through the plane pitch alone

Every case asserts np.array_equal with the oracle AND that nothing outside the [p][y < h][x < w]
windows was touched; nothing is compared with another call of the library.  odhip_inverse_route
(host arithmetic of the launch code itself) says which kernel a case reaches; the table is asserted
in test_route_table and per case."""
import ctypes
import functools

import numpy as np
import pytest

import _mc_ref as R
import _partition_ref as PR
from _libs import GOLDEN, P, oracle, synth_frame
from _strided import LAYOUTS, PlaneSet

pytestmark = pytest.mark.gpu

EINVAL = -10
(WALK_HI, TOP2, SB_TOP, SB_REF, SB_ALL, WALK_LO, SB_LO, PART) = range(8)    # ODHIP_ROUTE_*
SRC_PLANE, SRC_PVQ, SRC_PVQ_REF, SRC_PART = range(4)

# (dec, w, h) of the plane, two planes per set so that the pitch matters:
#   luma 448x128    7 superblocks: segments of 6 + 1, one joint, a one-group last segment, one horizontal strip
#   luma 128x64     one k_inverse_sb_top2 pair, no horizontal edge
#   luma 192x128    an odd count: k_inverse_sb at levels 3 and 4
#   chroma 256x64   4 pairs: segments of 3 + 1, one joint
#   chroma 96x64    3 tiles: the k_inverse_sb<32> / <32, true> fallbacks
SIZES = [(0, 448, 128), (0, 128, 64), (0, 192, 128), (1, 256, 64), (1, 96, 64)]
SIZE_IDS = ["%s%dx%d" % ("c" if d else "y", w, h) for d, w, h in SIZES]
NPLANES = 2
LAYOUT_NAMES = list(LAYOUTS)


@pytest.fixture(scope="module")
def hip():
    import torch
    import daala_amd
    assert torch.cuda.is_available()
    daala_amd.init(0)
    return daala_amd


@pytest.fixture(params=[False, True], ids=["u8", "fpr"])
def depth(request, hip):
    """The calling thread in an 8-bit or a full-precision-references context."""
    fpr = request.param
    ctx = hip.Context(0).set_fpr(fpr)
    try:
        with ctx:
            yield fpr
    finally:
        ctx.destroy()


def _cuda(a):
    import torch
    return torch.from_numpy(np.array(a, order="C")).cuda()      # (a copy: the shared oracle data is read-only)


def _sync():
    import torch
    torch.cuda.synchronize()


def _px_dtype(fpr):
    return np.int16 if fpr else np.uint8


def _pic(dec, w, h):
    """A cropped picture size in luma units: the split filters are gated by it."""
    return (w << dec) - 6, (h << dec) - 10


def _route(hip, dec, src, leaf_bs, w, aligned16):
    route, nedges = ctypes.c_int(-1), ctypes.c_int(-1)
    wide = hip.lib().odhip_inverse_route(dec, src, leaf_bs, w, int(aligned16), ctypes.byref(route),
                                         ctypes.byref(nedges))
    assert wide in (0, 1), wide
    return route.value, nedges.value, wide


def _aligned16(ps):
    return ps.stride % 16 == 0 and ps.plane_stride % 16 == 0 and ps.ptr.value % 16 == 0


def _expected_route(dec, src, leaf_bs, w):
    """The table of the issue, written out: (route, nedges)."""
    nsb = w // (64 >> dec)
    if dec:
        if nsb % 2 == 0:
            return (WALK_LO if leaf_bs <= 2 else WALK_HI), (nsb // 2 + 2) // 3 - 1
        return (SB_REF if src == SRC_PVQ_REF else SB_ALL), nsb - 1
    if leaf_bs <= 2:
        return WALK_LO, (nsb + 5) // 6 - 1
    if src == SRC_PVQ_REF:
        return SB_REF, nsb - 1
    if src == SRC_PVQ and nsb % 2 == 0:
        return TOP2, (nsb - 1) // 2
    return SB_TOP, nsb - 1


def _check_route(hip, fpr, dec, src, leaf_bs, ps):
    """The case reaches the kernel it is meant to reach, through the store path its layout selects."""
    route, nedges, wide = _route(hip, dec, src, leaf_bs, ps.w, _aligned16(ps))
    assert (route, nedges) == _expected_route(dec, src, leaf_bs, ps.w), (dec, src, leaf_bs, ps.w)
    assert wide == int(not fpr and _aligned16(ps))


# ---- oracle-side data, computed once per (size, depth) -------------------------------------------

def _oracle_inverse(d, dec, bs, fpr):
    """odo_inverse_level_plane of every plane of d [nplanes][h][w], 8-bit or full-precision samples."""
    o = oracle()
    nplanes, h, w = d.shape
    pw, ph = _pic(dec, w, h)
    out = np.zeros(d.shape, np.uint16 if fpr else np.uint8)
    o.odo_set_fpr(int(fpr))
    try:
        for p in range(nplanes):
            cc = np.zeros((h, w), np.int32)
            o.odo_inverse_level_plane(P(out[p]), w, P(cc), P(np.ascontiguousarray(d[p])), w, h, dec, bs, pw, ph)
    finally:
        o.odo_set_fpr(0)
    return out.view(np.int16) if fpr else out


@functools.lru_cache(maxsize=None)
def _plane_data(dec, w, h, fpr):
    """Noisy pixels with saturated patches, the oracle's pyramid of them, a quantised and perturbed copy of
    the pyramid (the output clamps are reached), and the oracle's inverse of both at every leaf level."""
    o = oracle()
    rng = np.random.RandomState(1000 * dec + w + 7 * int(fpr))
    base = synth_frame(w << dec, h << dec, seed=61)[1 if dec else 0]
    px = np.stack([base, base[::-1, ::-1]]).astype(np.int32)
    px = np.clip(px + rng.randint(-60, 61, size=px.shape), 0, 255)
    px[:, :8, :8] = 255
    px[:, 8:16, :8] = 0
    px[:, -8:, -8:] = 255
    if fpr:
        px = np.clip((px << 4) + rng.randint(0, 16, size=px.shape), 0, 4095)
        px[:, :8, :8] = 4095
    px = px.astype(_px_dtype(fpr))
    top = 4 - dec
    pw, ph = _pic(dec, w, h)
    levels = [np.zeros((NPLANES, h, w), np.int32) for _ in range(5)]
    o.odo_set_fpr(int(fpr))
    try:
        for p in range(NPLANES):
            arr = (ctypes.c_void_p * 5)(*[lv[p].ctypes.data for lv in levels])
            c = np.zeros((h, w), np.int32)
            o.odo_forward_pyramid_plane(arr, P(c), P(np.ascontiguousarray(px[p])), w, w, h, dec, pw, ph)
    finally:
        o.odo_set_fpr(0)
    levels = levels[:top + 1]
    rough = [np.ascontiguousarray(((lv + 32) // 64) * 64 + rng.randint(-700, 701, size=lv.shape).astype(np.int32))
             for lv in levels]
    want = [_oracle_inverse(levels[bs], dec, bs, fpr) for bs in range(top + 1)]
    want_rough = [_oracle_inverse(rough[bs], dec, bs, fpr) for bs in range(top + 1)]
    lim = 4095 if fpr else 255
    assert any((wr == 0).any() for wr in want_rough) and any((wr == lim).any() for wr in want_rough)
    for a in [px] + levels + rough + want + want_rough:
        a.setflags(write=False)
    return dict(px=px, levels=levels, rough=rough, want=want, want_rough=want_rough)


def _out_sets(layout, n, h, w, fpr):
    return [PlaneSet.in_layout(layout, NPLANES, h, w, _px_dtype(fpr)) for _ in range(n)]


def _ptrs(sets):
    return (ctypes.c_void_p * len(sets))(*[s.ptr.value for s in sets])


# ---- forward pyramid and the plane-fed inverse ---------------------------------------------------

@pytest.mark.parametrize("layout", LAYOUT_NAMES)
@pytest.mark.parametrize("dec,w,h", SIZES, ids=SIZE_IDS)
def test_forward_pyramid_reads_strided_pixels(hip, depth, dec, w, h, layout):
    import torch
    fpr = depth
    data = _plane_data(dec, w, h, fpr)
    px = PlaneSet.in_layout(layout, NPLANES, h, w, _px_dtype(fpr)).write(data["px"])
    top = 4 - dec
    levels = [torch.full((NPLANES, h, w), 0x5AA55AA5, dtype=torch.int32, device="cuda") for _ in range(top + 1)]
    arr = (ctypes.c_void_p * 5)(*([t.data_ptr() for t in levels] + [None] * (4 - top)))
    pw, ph = _pic(dec, w, h)
    rc = hip.lib().odhip_forward_pyramid(arr, px.ptr, px.stride, px.pitch, NPLANES, w, h, dec, pw, ph, None)
    assert rc == 0
    _sync()
    for bs in range(top + 1):
        assert np.array_equal(levels[bs].cpu().numpy(), data["levels"][bs]), (layout, bs)
    assert px.intact() and np.array_equal(px.read(), data["px"])


@pytest.mark.parametrize("layout", LAYOUT_NAMES)
@pytest.mark.parametrize("dec,w,h", SIZES, ids=SIZE_IDS)
def test_inverse_level_and_levels_write_strided_pixels(hip, depth, dec, w, h, layout):
    """odhip_inverse_level of the oracle's pyramid, level by level, and odhip_inverse_levels of the quantised
    and perturbed copy, all levels in one call."""
    fpr = depth
    data = _plane_data(dec, w, h, fpr)
    L = hip.lib()
    top = 4 - dec
    pw, ph = _pic(dec, w, h)
    for bs in range(top + 1):
        out = _out_sets(layout, 1, h, w, fpr)[0]
        _check_route(hip, fpr, dec, SRC_PLANE, bs, out)
        coef = _cuda(data["levels"][bs])
        rc = L.odhip_inverse_level(out.ptr, out.stride, out.pitch, ctypes.c_void_p(coef.data_ptr()), NPLANES, w, h,
                                   dec, bs, pw, ph, None)
        assert rc == 0
        _sync()
        assert np.array_equal(out.read(), data["want"][bs]), (layout, bs)
        assert out.intact(), (layout, bs)
    outs = _out_sets(layout, top + 1, h, w, fpr)
    coefs = [_cuda(c) for c in data["rough"]]
    cf = (ctypes.c_void_p * (top + 1))(*[c.data_ptr() for c in coefs])
    lv = (ctypes.c_int * (top + 1))(*range(top + 1))
    rc = L.odhip_inverse_levels(_ptrs(outs), outs[0].stride, outs[0].pitch, cf, lv, top + 1, NPLANES, w, h, dec,
                                pw, ph, None)
    assert rc == 0
    _sync()
    for bs in range(top + 1):
        assert np.array_equal(outs[bs].read(), data["want_rough"][bs]), (layout, bs)
        assert outs[bs].intact(), (layout, bs)


# ---- pulse-fed inverses --------------------------------------------------------------------------

_jobs_cache = {}


def _noref_jobs(hip, dec, w, h):
    """PvqJobs of every level (as test_gpu_pvq_bands.py builds them) on the oracle's 8-bit pyramid, searched,
    chosen and dequantised; job.dq (pinned to the oracle by that file) is what the fused inverse must
    reconstruct."""
    import torch
    key = ("noref", dec, w, h)
    if key not in _jobs_cache:
        levels = _plane_data(dec, w, h, False)["levels"]
        qt = hip.QuantTables.load()
        pli = 1 if dec else 0
        jobs = []
        for bs in range(5 - dec):
            qm, qmi = qt.qm_slices(pli, bs)
            coef = _cuda(levels[bs])
            jobs.append(hip.PvqJob(coef, bs, _cuda(qm), _cuda(qmi), qt.q_band(pli, bs), qt.beta_band(pli, bs),
                                   dq=torch.empty_like(coef)))
        hip.pvq_noref_bands_multi(jobs, hip.OD_PVQ_LAMBDA)
        hip.pvq_select_synth_noref_multi(jobs, hip.OD_PVQ_LAMBDA)
        hip.pvq_choose_multi(jobs, hip.OD_PVQ_LAMBDA)
        _sync()
        _jobs_cache[key] = (jobs, [j.dq.cpu().numpy() for j in jobs], {})
    return _jobs_cache[key]


def _ref_jobs(hip, dec, w, h):
    """Jobs of the with-reference stage, built as test_gpu_pvq_refbands.py builds them (_job): keyframe chroma
    predicted from luma for the chroma sizes, an inter frame for the luma sizes."""
    from test_gpu_pvq_refbands import _job
    key = ("ref", dec, w, h)
    if key not in _jobs_cache:
        is_keyframe, pli = (1, 1) if dec else (0, 0)
        rng = np.random.RandomState(70 + 2 * is_keyframe + pli + w)
        jobs = [_job(hip, rng, bs, is_keyframe, pli, h=h, w=w, nplanes=NPLANES)[0] for bs in range(5 - dec)]
        hip.pvq_ref_bands_multi(jobs, hip.OD_PVQ_LAMBDA)
        hip.pvq_ref_select_synth_multi(jobs, hip.OD_PVQ_LAMBDA)
        _sync()
        dq = [j.dq.cpu().numpy() for j in jobs]
        for j in jobs:
            j.choice.fill_(0x5a5a5a5a)  # no mode: a record the choice left unwritten shows in the count below
            j.dq.fill_(12345)          # the fused path must not need it
        hip.pvq_ref_choose_multi(jobs, hip.OD_PVQ_LAMBDA)
        _sync()
        # what the shared with-reference chunk (od_ref_chunk) is fed on this size: word 8 of a choice record is
        # its synthesis mode - 0 zero, 1 / 4 copy of the reference / of its negative, 2 without reference, 3 with
        modes = {}
        for j in jobs:
            m, c = np.unique(j.choice.cpu().numpy()[:, :, 8], return_counts=True)
            for mi, ci in zip(m.tolist(), c.tolist()):
                modes[mi] = modes.get(mi, 0) + ci
        assert set(modes) <= {0, 1, 2, 3, 4}, (dec, w, h, modes)
        assert {0, 2, 3} <= set(modes), (dec, w, h, modes)
        if not is_keyframe:         # skip-copy bands only exist on inter frames
            assert set(modes) & {1, 4}, (dec, w, h, modes)
        _jobs_cache[key] = (jobs, dq, {})
    return _jobs_cache[key]


def _want_of(entry, dec, fpr):
    """The oracle's inverse of the dequantised planes, once per depth."""
    _, dq, wants = entry
    if fpr not in wants:
        wants[fpr] = [_oracle_inverse(d, dec, bs, fpr) for bs, d in enumerate(dq)]
    return wants[fpr]


@pytest.mark.parametrize("layout", LAYOUT_NAMES)
@pytest.mark.parametrize("dec,w,h", SIZES, ids=SIZE_IDS)
def test_inverse_levels_pvq_writes_strided_pixels(hip, depth, dec, w, h, layout):
    """Every source at 448x128 / 256x64 in the packed layout is the joint coverage against the oracle that the
    kernel-level tests (256 wide at most, against the plane-fed inverse of the same build) do not have."""
    from daala_amd import api
    fpr = depth
    entry = _noref_jobs(hip, dec, w, h)
    jobs = entry[0]
    want = _want_of(entry, dec, fpr)
    pw, ph = _pic(dec, w, h)
    outs = _out_sets(layout, len(jobs), h, w, fpr)
    for j in jobs:
        _check_route(hip, fpr, dec, SRC_PVQ, j.bs, outs[0])
    rc = hip.lib().odhip_inverse_levels_pvq(_ptrs(outs), outs[0].stride, outs[0].pitch, api._jobs_array(jobs),
                                            len(jobs), dec, pw, ph, None)
    assert rc == 0
    _sync()
    for bs in range(len(jobs)):
        assert np.array_equal(outs[bs].read(), want[bs]), (layout, bs)
        assert outs[bs].intact(), (layout, bs)


@pytest.mark.parametrize("layout", LAYOUT_NAMES)
@pytest.mark.parametrize("dec,w,h", SIZES, ids=SIZE_IDS)
def test_inverse_levels_pvq_ref_writes_strided_pixels(hip, depth, dec, w, h, layout):
    from daala_amd import api
    fpr = depth
    entry = _ref_jobs(hip, dec, w, h)
    jobs = entry[0]
    want = _want_of(entry, dec, fpr)
    pw, ph = _pic(dec, w, h)
    outs = _out_sets(layout, len(jobs), h, w, fpr)
    for j in jobs:
        _check_route(hip, fpr, dec, SRC_PVQ_REF, j.bs, outs[0])
    rc = hip.lib().odhip_inverse_levels_pvq_ref(_ptrs(outs), outs[0].stride, outs[0].pitch,
                                                api._refjobs_array(jobs), len(jobs), dec, pw, ph, None)
    assert rc == 0
    _sync()
    for bs in range(len(jobs)):
        assert np.array_equal(outs[bs].read(), want[bs]), (layout, bs)
        assert outs[bs].intact(), (layout, bs)
        assert int(jobs[bs].dq[0, 0, 1]) == 12345


# ---- the decoder's inverse at a block-size map ---------------------------------------------------

@pytest.mark.parametrize("layout", LAYOUT_NAMES)
@pytest.mark.parametrize("w,h", [(192, 128), (448, 128)], ids=["y192x128", "y448x128"])
def test_inverse_partition_writes_strided_pixels(hip, depth, w, h, layout):
    """A uniform map of every level equals the oracle's odo_inverse_level_plane everywhere, and the mixed map of
    test_gpu_fpr.py (superblock (sx, sy) at level (sx + sy) % 5) equals tests/_partition_ref.py's inverse() over
    the whole plane - and so, inside every superblock, away from the 2 samples the superblock-edge post-filter
    mixes with the neighbours, the oracle's uniform reconstruction of that superblock's level.  (Maps that vary
    inside a superblock: tests/test_gpu_partition.py.)"""
    fpr = depth
    data = _plane_data(0, w, h, fpr)
    L = hip.lib()
    bstride = (w // 64) * 8
    rows = (h // 64) * 8
    pw, ph = _pic(0, w, h)

    def run(bsize, coef):
        out = _out_sets(layout, 1, h, w, fpr)[0]
        tb, tc = _cuda(bsize), _cuda(coef)
        rc = L.odhip_inverse_partition(out.ptr, out.stride, out.pitch, ctypes.c_void_p(tc.data_ptr()), NPLANES, w, h,
                                       0, ctypes.c_void_p(tb.data_ptr()), bstride, ctypes.c_long(rows * bstride), 1,
                                       pw, ph, None)
        assert rc == 0
        _sync()
        assert out.intact(), layout
        return out.read()

    route, _, _ = _route(hip, 0, SRC_PART, 0, w, True)
    assert route == PART
    for lv in range(5):
        got = run(np.full((NPLANES, rows, bstride), lv, np.uint8), data["rough"][lv])
        assert np.array_equal(got, data["want_rough"][lv]), (layout, lv)
    mix = np.zeros((NPLANES, rows, bstride), np.uint8)
    coef_mix = np.zeros((NPLANES, h, w), np.int32)
    for sy in range(h // 64):
        for sx in range(w // 64):
            lv = (sx + sy) % 5
            mix[:, sy * 8:(sy + 1) * 8, sx * 8:(sx + 1) * 8] = lv
            coef_mix[:, sy * 64:(sy + 1) * 64, sx * 64:(sx + 1) * 64] = \
                data["rough"][lv][:, sy * 64:(sy + 1) * 64, sx * 64:(sx + 1) * 64]
    got = run(mix, coef_mix)
    for p in range(NPLANES):
        assert np.array_equal(got[p], PR.inverse(coef_mix[p], mix[p][:, :w // 8], 0, pw, ph, fpr)), (layout, p)
    for sy in range(h // 64):
        for sx in range(w // 64):
            lv = (sx + sy) % 5
            ys, xs = slice(sy * 64 + 2, sy * 64 + 62), slice(sx * 64 + 2, sx * 64 + 62)
            assert np.array_equal(got[:, ys, xs], data["want_rough"][lv][:, ys, xs]), (layout, sx, sy, lv)


# ---- which kernel a case reaches -----------------------------------------------------------------

def test_route_table(hip, depth):
    """odhip_inverse_route is the launch code's own decision (inverse_shape, inverse_plan, inverse_wide).
    ODHIP_ROUTE_SB_LO is not in the table: a luma plane is always a whole number of one-superblock groups
    wide, so in a default build its leaf levels up to 16x16 always walk."""
    fpr = depth
    for src in (SRC_PLANE, SRC_PVQ, SRC_PVQ_REF):
        for bs in range(3):
            assert _route(hip, 0, src, bs, 448, True)[:2] == (WALK_LO, 1)      # segments of 6 + 1 superblocks
            assert _route(hip, 0, src, bs, 192, True)[:2] == (WALK_LO, 0)
        for bs in range(4):
            assert _route(hip, 1, src, bs, 256, True)[:2] == (WALK_HI if bs == 3 else WALK_LO, 1)   # 3 + 1 pairs
    for bs in (3, 4):
        assert _route(hip, 0, SRC_PVQ, bs, 128, True)[:2] == (TOP2, 0)         # the one edge is inside the pair
        assert _route(hip, 0, SRC_PVQ, bs, 448, True)[:2] == (SB_TOP, 6)       # odd counts: one workgroup
        assert _route(hip, 0, SRC_PVQ, bs, 192, True)[:2] == (SB_TOP, 2)       # per superblock
        assert _route(hip, 0, SRC_PLANE, bs, 192, True)[:2] == (SB_TOP, 2)
        assert _route(hip, 0, SRC_PLANE, bs, 128, True)[:2] == (SB_TOP, 1)
        assert _route(hip, 0, SRC_PVQ_REF, bs, 192, True)[:2] == (SB_REF, 2)
    for bs in range(4):
        assert _route(hip, 1, SRC_PLANE, bs, 96, True)[:2] == (SB_ALL, 2)
        assert _route(hip, 1, SRC_PVQ, bs, 96, True)[:2] == (SB_ALL, 2)
        assert _route(hip, 1, SRC_PVQ_REF, bs, 96, True)[:2] == (SB_REF, 2)
    # the store path of the walkers: whole 16-byte pieces for packed and gap16, 4-sample groups otherwise
    for name in LAYOUT_NAMES:
        ps = PlaneSet.in_layout(name, NPLANES, 64, 448, _px_dtype(fpr), device=None)
        al = ps.stride % 16 == 0 and ps.plane_stride % 16 == 0 and ps.base % 16 == 0
        assert al == (name in ("packed", "gap16"))
        assert _route(hip, 0, SRC_PLANE, 0, 448, al)[2] == int(al and not fpr), name
    L = hip.lib()
    r, n = ctypes.c_int(), ctypes.c_int()
    assert L.odhip_inverse_route(0, 0, 0, 100, 1, ctypes.byref(r), ctypes.byref(n)) == EINVAL
    assert L.odhip_inverse_route(1, 0, 4, 64, 1, ctypes.byref(r), ctypes.byref(n)) == EINVAL
    assert L.odhip_inverse_route(0, 0, 0, 64, 1, None, ctypes.byref(n)) == EINVAL


# ---- the other plane surfaces --------------------------------------------------------------------

@pytest.mark.parametrize("layout", ["gap16", "min4"])
@pytest.mark.parametrize("pic,plane", [((70, 50), (128, 64)), ((33, 17), (64, 64))], ids=["70x50", "33x17"])
@pytest.mark.parametrize("bitdepth", [8, 10, 12, "u8"])
def test_copy_pad_strided_both_sides(hip, bitdepth, pic, plane, layout):
    """odhip_image_planes_copy_pad ("u8") and _copy_pad16 (a source of 8, 10 or 12 bits): the source at an odd
    stride and an odd base offset (it has no alignment rule), the destination in a gapped layout."""
    o = oracle()
    L = hip.lib()
    pw, ph = pic
    plane_w, plane_h = plane
    rng = np.random.RandomState(pw + (0 if bitdepth == "u8" else bitdepth))
    sdt = np.uint8 if bitdepth in ("u8", 8) else np.int16
    top = 256 if sdt == np.uint8 else 1 << bitdepth
    src = rng.randint(0, top, size=(3, ph, pw)).astype(sdt)
    s = PlaneSet(3, ph, pw, sdt, stride=pw + 3, base=5, plane_stride=(pw + 3) * ph + 1).write(src)
    ddt = np.uint8 if bitdepth == "u8" else np.int16
    d = PlaneSet.in_layout(layout, 3, plane_h, plane_w, ddt)
    if bitdepth == "u8":
        rc = L.odhip_image_planes_copy_pad(d.ptr, d.stride, d.pitch, plane_w, plane_h, s.ptr, s.stride, s.pitch,
                                           pw, ph, 3, None)
    else:
        rc = L.odhip_image_planes_copy_pad16(d.ptr, d.stride, d.pitch, plane_w, plane_h, s.ptr, bitdepth, s.stride,
                                             s.pitch, pw, ph, 3, None)
    assert rc == 0
    _sync()
    got = d.read()
    for p in range(3):
        if bitdepth == "u8":
            want = np.zeros((plane_h, plane_w), np.uint8)
            o.odo_img_plane_copy_pad(P(want), plane_w, plane_w, plane_h, P(np.ascontiguousarray(src[p])), pw, pw, ph)
        else:
            want = np.zeros((plane_h, plane_w), np.uint16)
            o.odo_img_plane_copy_pad16(P(want), plane_w, plane_w, plane_h, P(np.ascontiguousarray(src[p])), bitdepth,
                                       pw, pw, ph)
            want = want.view(np.int16)
        assert np.array_equal(got[p], want), (bitdepth, p)
    assert d.intact()
    assert s.intact() and np.array_equal(s.read(), src)


@pytest.mark.parametrize("inverse", [False, True], ids=["fdct", "idct"])
@pytest.mark.parametrize("ln", [0, 2, 4])
def test_dct_plane_with_different_strides(hip, ln, inverse):
    """in_stride and out_stride differ from each other and from w (multiples of 4; bases 16-byte aligned as
    the entry points require); the oracle transforms block by block."""
    o = oracle()
    L = hip.lib()
    w, h, n = 128, 64, 4 << ln
    rng = np.random.RandomState(3 + ln)
    x = rng.randint(-500, 501, size=(1, h, w)).astype(np.int32)
    src = PlaneSet(1, h, w, np.int32, stride=w + 8, base=4).write(x)
    dst = PlaneSet(1, h, w, np.int32, stride=w + 20, base=8)
    fn = L.odhip_idct2d_plane if inverse else L.odhip_fdct2d_plane
    assert fn(ln, dst.ptr, dst.stride, src.ptr, src.stride, w, h, 0, None) == 0
    _sync()
    want = np.zeros((h, w), np.int32)
    for by in range(h // n):
        for bx in range(w // n):
            blk = np.ascontiguousarray(x[0, by * n:(by + 1) * n, bx * n:(bx + 1) * n])
            out = np.zeros((n, n), np.int32)
            if inverse:
                o.odo_idct_2d(ln, P(out), n, P(blk), n)
            else:
                o.odo_fdct_2d(ln, P(out), n, P(blk), n)
            want[by * n:(by + 1) * n, bx * n:(bx + 1) * n] = out
    assert np.array_equal(dst.read()[0], want)
    assert dst.intact() and src.intact() and np.array_equal(src.read(), x)


MC_CASES = R.load_cases(GOLDEN + "/mc.npz")


@pytest.mark.parametrize("fpr", [0, 1], ids=["u8", "i16"])
@pytest.mark.parametrize("dec", [0, 1])
def test_mc_predict_planes_with_odd_strides(hip, fpr, dec):
    """ref_stride = w + 3, dst_stride = w + 5, plane pitches that are no multiples of the strides; the three
    192x128 grid patterns of tests/golden/mc.npz with random vectors, against tests/_mc_ref.py."""
    from daala_amd import api
    from test_gpu_mc import random_planes
    rng = np.random.RandomState(140 + 2 * fpr + dec)
    pats = [c["grid"]["valid"] for c in MC_CASES if (c["w"], c["h"]) == (192, 128)][:3]
    assert len(pats) == 3
    grids = np.stack([R.random_grid(v, rng, (dec,), nrefs=3) for v in pats])
    h, w = 128 >> dec, 192 >> dec
    nplanes = 6 if dec else 3
    dt = np.int16 if fpr else np.uint8
    data = [random_planes(rng, nplanes, h, w, fpr) for _ in range(3)]
    refs = [PlaneSet(nplanes, h, w, dt, stride=w + 3, base=1, plane_stride=(w + 3) * h + 7).write(r) for r in data]
    dst = PlaneSet(nplanes, h, w, dt, stride=w + 5, base=3, plane_stride=(w + 5) * h + 11)
    g = np.ascontiguousarray(grids, api.MV_POINT)
    job = api._McJob(192, 128, dec, api.SAMPLE_I16_12 if fpr else api.SAMPLE_U8, 3, nplanes, 3, 0, refs[0].stride,
                     dst.stride, refs[0].plane_stride, dst.plane_stride,
                     (ctypes.c_void_p * 3)(*[r.ptr.value for r in refs]), dst.ptr, g.ctypes.data)
    assert hip.lib().odhip_mc_predict_planes(ctypes.byref(job), None) == 0
    _sync()
    got = dst.read()
    for p in range(nplanes):
        want = R.mc_predict_plane([r[p] for r in data], grids[p % 3], dec, fpr)
        assert np.array_equal(got[p], want), p
    assert dst.intact()
    for r, d in zip(refs, data):
        assert r.intact() and np.array_equal(r.read(), d)


# ---- the contract of include/daala_hip.h, as return codes ----------------------------------------

def test_layouts_outside_the_contract_are_refused(hip, depth):
    """ODHIP_EINVAL before anything is launched: the buffers are sentinel-filled and stay so."""
    import torch
    fpr = depth
    L = hip.lib()
    w, h = 64, 64
    dt = _px_dtype(fpr)
    px = PlaneSet(2, h, w, dt, stride=w + 16, base=16, plane_stride=(w + 16) * h + 16)
    coef = torch.zeros((2, h, w), dtype=torch.int32, device="cuda")
    cp = ctypes.c_void_p(coef.data_ptr())
    bsize = torch.zeros((2, 8, 8), dtype=torch.uint8, device="cuda")
    item = np.dtype(dt).itemsize
    off = lambda k: ctypes.c_void_p(px.ptr.value + k * item)  # noqa: E731
    good = (px.ptr, px.stride, px.plane_stride)
    bad = [(px.ptr, w - 4, px.plane_stride),                 # rows overlap
           (px.ptr, px.stride, px.stride * h - 4),           # planes overlap
           (px.ptr, px.stride, w * h),                       # a pitch counted for the wrong stride
           (px.ptr, w + 2, (w + 2) * h),                     # stride no multiple of 4
           (px.ptr, px.stride, px.stride * h + 2),           # pitch no multiple of 4
           (off(1), px.stride, px.plane_stride),             # base off the sample group
           (off(2), px.stride, px.plane_stride)]           # (full precision: 4- but not 8-byte aligned)
    levels = (ctypes.c_void_p * 5)(*[coef.data_ptr()] * 5)
    one_px = (ctypes.c_void_p * 1)(px.ptr.value)
    one_cf = (ctypes.c_void_p * 1)(coef.data_ptr())
    one_lv = (ctypes.c_int * 1)(1)

    def calls(ptr, stride, pitch):
        pitch = ctypes.c_long(pitch)
        yield L.odhip_forward_pyramid(levels, ptr, stride, pitch, 2, w, h, 0, w, h, None)
        yield L.odhip_inverse_level(ptr, stride, pitch, cp, 2, w, h, 0, 1, w, h, None)
        yield L.odhip_inverse_levels((ctypes.c_void_p * 1)(ptr.value), stride, pitch, one_cf, one_lv, 1, 2, w, h, 0,
                                     w, h, None)
        yield L.odhip_inverse_partition(ptr, stride, pitch, cp, 2, w, h, 0, ctypes.c_void_p(bsize.data_ptr()), 8,
                                        ctypes.c_long(64), 1, w, h, None)

    for b in bad:
        assert list(calls(*b)) == [EINVAL] * 4, b[1:]
    _sync()
    assert px.intact(0, 0)          # nothing was written anywhere
    assert list(calls(*good)) == [0] * 4
    assert L.odhip_inverse_levels(one_px, px.stride, px.pitch, one_cf, one_lv, 1, 2, w, h, 0, w, h, None) == 0
    _sync()
    assert px.intact()
    # copy-pad: rows and planes that overlap, on either side
    d = PlaneSet(2, 64, 64, dt)
    s = PlaneSet(2, 17, 33, dt)
    if fpr:
        cp16 = lambda ds, dp, ss, sp: L.odhip_image_planes_copy_pad16(  # noqa: E731
            d.ptr, ds, ctypes.c_long(dp), 64, 64, s.ptr, 12, ss, ctypes.c_long(sp), 33, 17, 2, None)
    else:
        cp16 = lambda ds, dp, ss, sp: L.odhip_image_planes_copy_pad(  # noqa: E731
            d.ptr, ds, ctypes.c_long(dp), 64, 64, s.ptr, ss, ctypes.c_long(sp), 33, 17, 2, None)
    assert cp16(60, 64 * 64, 33, 33 * 17) == EINVAL
    assert cp16(64, 64 * 64 - 1, 33, 33 * 17) == EINVAL
    assert cp16(64, 64 * 64, 32, 33 * 17) == EINVAL
    assert cp16(64, 64 * 64, 33, 33 * 17 - 1) == EINVAL
    _sync()
    assert d.intact(0, 0)
    assert cp16(64, 64 * 64, 33, 33 * 17) == 0
    # DCT planes: a stride shorter than the plane is wide
    x = torch.zeros((64, 128), dtype=torch.int32, device="cuda")
    y = torch.zeros((64, 128), dtype=torch.int32, device="cuda")
    xp, yp = ctypes.c_void_p(x.data_ptr()), ctypes.c_void_p(y.data_ptr())
    for fn in (L.odhip_fdct2d_plane, L.odhip_idct2d_plane):
        assert fn(1, yp, 124, xp, 128, 128, 64, 0, None) == EINVAL
        assert fn(1, yp, 128, xp, 64, 128, 64, 0, None) == EINVAL
        assert fn(1, yp, 128, xp, 128, 128, 64, 0, None) == 0
    _sync()
