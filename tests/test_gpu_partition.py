"""GPU: odhip_inverse_partition (k_inverse_part<64/32>, daala_amd/csrc/lapped_kernels.hip) at block-size maps
that vary INSIDE a superblock, bit-exact over the whole plane - edge strips included - against
tests/_partition_ref.py (the decoder's recursion composed from the oracle's primitives, pinned to the real
decoder by tests/golden/partition.npz and tests/test_partition_ref.py).

What each family is there to reach in the kernel:
  lossless / rough / hot   PartIsLeaf per level, the split predicate `node.at(bx, by) < LN`, the picture gate of
                           split_filter_rows_if / split_filter_cols_if per node (the picture sizes below flip it
                           inside the last superblock at every node size), the 24-bit multiplies at the largest
                           coefficients pixels can give, both output clamps
  batch geometry           the map address `bsize + (plane / planes_per_frame)*bsize_frame_stride + row*bstride`
  4:2:0 derivation         `max(v, 1) - 1`, and PartLeaf::at's u == 0 branch for 4x4 luma
  contexts and layouts     the uchar4 / short4 stores of inverse_store and the stores of k_edge_rows / k_edge_cols
  one superblock           no edge kernel at all
  golden                   the real decoder's own maps and coefficients, device form and host form
  refusals                 the argument checks in front of every launch
"""
import ctypes
import functools

import numpy as np
import pytest

import _partition_ref as R
from _libs import GOLDEN, P, oracle, synth_frame
from _strided import PlaneSet

pytestmark = pytest.mark.gpu

EINVAL, EIMPL = -10, -23
# the smallest frames with interior superblock edges both ways (luma 192x128, its 4:2:0 chroma 96x64), and one
# superblock.  The LUMA picture size per plane kind flips the split filters' gate inside the last superblock at
# every node size; its width lands ON node borders (160 = 5*32, 80 = 5*16, 48 = 3*16: `<=`, not `<`), its height
# (106, 44, 44) between them.  A 4:2:0 plane is compared with the luma size all the same, so 80 < 96 flips it too.
NSBX, NSBY = 3, 2
PIC = {(0, NSBX): (160, 106), (1, NSBX): (80, 44), (0, 1): (48, 44)}
MAP_NAMES = ["corners", "extremes", "units01", "nodes16", "random0", "random1"]
GAP = 9                                  # what the bytes between map rows and frames hold: no block size
LAYOUTS = ["packed", "min4"]


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
    return torch.from_numpy(np.array(a, order="C")).cuda()


def _sync():
    import torch
    torch.cuda.synchronize()


def _px_dtype(fpr):
    return np.int16 if fpr else np.uint8


# ---- CPU side: maps, pixels, coefficients and expectations, once per module -----------------------

@functools.lru_cache(maxsize=None)
def _maps(nsbx=NSBX):
    nsby = NSBY if nsbx == NSBX else 1
    rng = np.random.RandomState(4 + nsbx)
    maps = {"corners": R.corners(nsbx, nsby), "extremes": R.extremes(nsbx, nsby), "units01": R.units01(nsbx, nsby),
            "nodes16": R.nodes16(rng, nsbx, nsby)}
    if nsbx == 1:
        maps = {"corner%d" % k: R.deep_corner(k) for k in range(4)}
    for k in range(2):
        # every leaf size in each random map (one superblock cannot hold a 64x64 leaf beside others)
        want = [0, 1, 2, 3, 4] if nsbx > 1 else [0, 1, 2, 3]
        for _ in range(200):
            m = R.random_map(rng, nsbx, nsby, 0.55 + 0.2 * k)
            if R.leaf_sizes(m) == want:
                break
        assert R.leaf_sizes(m) == want, (k, R.leaf_sizes(m))
        maps["random%d" % k] = m
    for m in maps.values():
        assert R.is_quadtree(m)
        m.setflags(write=False)
    return maps


def _leaf_pitch(bmap, dec):
    """Per sample of the plane, the side of the leaf that holds it."""
    lv = np.maximum(bmap.astype(np.int32), dec) - dec
    return np.kron(4 << lv, np.ones((8 >> dec, 8 >> dec), np.int32))


@functools.lru_cache(maxsize=None)
def _plane(dec, fpr, nsbx, name, variant):
    """One plane at one map: noisy pixels with saturated patches and their forward() (lossless); that quantised
    and perturbed as _plane_data of test_gpu_plane_layouts.py does, with its inverse() (rough); saturated
    checkerboards at the pitch of the leaf each sample lies in, forward() of them quantised, and its inverse()
    (hot).  `variant` tells the planes of one frame (Cb / Cr, or the three of a 4:4:4 frame) apart."""
    bmap = _maps(nsbx)[name]
    h, w = (bmap.shape[0] * 8) >> dec, (bmap.shape[1] * 8) >> dec
    pw, ph = PIC[dec, nsbx]
    top = 4095 if fpr else 255
    rng = np.random.RandomState(1000 * dec + 100 * variant + 7 * int(fpr) + len(name) + ord(name[-1]))
    base = synth_frame(w << dec, h << dec, seed=61 + variant)[1 if dec else 0].astype(np.int32)
    if variant & 1:
        base = base[::-1, ::-1]
    px = np.clip(base + rng.randint(-60, 61, size=base.shape), 0, 255)
    px[:8, :8] = 255
    px[8:16, :8] = 0
    px[-8:, -8:] = 255
    if fpr:
        px = np.clip((px << 4) + rng.randint(0, 16, size=px.shape), 0, 4095)
        px[:8, :8] = 4095
    px = px.astype(_px_dtype(fpr))
    coef = R.forward(px, bmap, dec, pw, ph, fpr)
    rough = np.ascontiguousarray(((coef + 32) // 64) * 64 + rng.randint(-700, 701, size=coef.shape).astype(np.int32))
    n = _leaf_pitch(bmap, dec)
    yy, xx = np.mgrid[0:h, 0:w]
    hot_px = (top * (((yy // n + xx // n + variant) & 1))).astype(_px_dtype(fpr))
    hot = np.ascontiguousarray(((R.forward(hot_px, bmap, dec, pw, ph, fpr) + 32) // 64) * 64)
    d = dict(px=px, coef=coef, rough=rough, want_rough=R.inverse(rough, bmap, dec, pw, ph, fpr),
             hot=hot, want_hot=R.inverse(hot, bmap, dec, pw, ph, fpr))
    for a in d.values():
        a.setflags(write=False)
    return d


def _frames(dec, fpr, nsbx, names, ppf, key):
    """[len(names)*ppf][h][w]: plane `variant` of every frame, frames in the order of `names`."""
    return np.stack([_plane(dec, fpr, nsbx, name, v)[key] for name in names for v in range(ppf)])


def _map_buffer(maps, bstride, frame_stride):
    rows, cols = maps[0].shape
    assert bstride >= cols and frame_stride >= (rows - 1) * bstride + cols
    buf = np.full(len(maps) * frame_stride + 64, GAP, np.uint8)
    for f, m in enumerate(maps):
        for r in range(rows):
            buf[f * frame_stride + r * bstride:f * frame_stride + r * bstride + cols] = m[r]
    return buf


def _inverse(hip, fpr, layout, dec, coefs, maps, ppf, pic, bstride=None, frame_stride=None):
    """odhip_inverse_partition of coefs [nplanes][h][w] at `maps` (one per frame of ppf planes) into a
    sentinel-surrounded plane set; every map read stays inside the map buffer (asserted by _map_buffer)."""
    nplanes, h, w = coefs.shape
    rows, cols = maps[0].shape
    assert nplanes == len(maps) * ppf and (rows, cols) == ((h << dec) // 8, (w << dec) // 8)
    bstride = cols if bstride is None else bstride
    frame_stride = rows * bstride if frame_stride is None else frame_stride
    out = PlaneSet.in_layout(layout, nplanes, h, w, _px_dtype(fpr))
    tb, tc = _cuda(_map_buffer(maps, bstride, frame_stride)), _cuda(coefs)
    assert tc.data_ptr() % 16 == 0
    rc = hip.lib().odhip_inverse_partition(out.ptr, out.stride, out.pitch, ctypes.c_void_p(tc.data_ptr()), nplanes, w, h,
                                           dec, ctypes.c_void_p(tb.data_ptr()), bstride, ctypes.c_long(frame_stride), ppf,
                                           pic[0], pic[1], None)
    assert rc == 0
    _sync()
    assert out.intact(), layout
    return out.read()


def _assert_planes(got, want, names, ppf):
    for i in range(got.shape[0]):
        bad = int((got[i] != want[i]).sum())
        assert bad == 0, "map %s plane %d: %d samples differ" % (names[i // ppf], i % ppf, bad)


# ---- lossless, rough, hot: every map in one call, luma and 4:2:0 chroma ---------------------------

@pytest.mark.parametrize("layout", LAYOUTS)
@pytest.mark.parametrize("dec", [0, 1], ids=["y192x128", "c96x64"])
def test_lossless_gives_the_pixels_back(hip, depth, dec, layout):
    """forward() of pixels at each map, then the GPU inverse: the pixels, whatever inverse() says."""
    fpr, ppf = depth, 1 + dec
    maps = [_maps()[n] for n in MAP_NAMES]
    got = _inverse(hip, fpr, layout, dec, _frames(dec, fpr, NSBX, MAP_NAMES, ppf, "coef"), maps, ppf, PIC[dec, NSBX])
    _assert_planes(got, _frames(dec, fpr, NSBX, MAP_NAMES, ppf, "px"), MAP_NAMES, ppf)


@pytest.mark.parametrize("layout", LAYOUTS)
@pytest.mark.parametrize("dec", [0, 1], ids=["y192x128", "c96x64"])
@pytest.mark.parametrize("kind", ["rough", "hot"])
def test_quantised_coefficients_equal_the_restated_recursion(hip, depth, kind, dec, layout):
    fpr, ppf = depth, 1 + dec
    maps = [_maps()[n] for n in MAP_NAMES]
    want = _frames(dec, fpr, NSBX, MAP_NAMES, ppf, "want_" + kind)
    lim = 4095 if fpr else 255
    assert (want == 0).any() and (want == lim).any()              # both clamps, on the expectation
    if kind == "hot":
        # the largest coefficients that data from pixels gives: inside the range the 24-bit multiplies are
        # documented for (od_lift.cuh: the frame pipeline's values stay below 2^19)
        assert int(np.abs(_frames(dec, fpr, NSBX, MAP_NAMES, ppf, "hot")).max()) < 1 << 19
    got = _inverse(hip, fpr, layout, dec, _frames(dec, fpr, NSBX, MAP_NAMES, ppf, kind), maps, ppf, PIC[dec, NSBX])
    _assert_planes(got, want, MAP_NAMES, ppf)


@pytest.mark.parametrize("layout", LAYOUTS)
def test_one_superblock_has_no_edge_kernel(hip, depth, layout):
    """A 64x64 luma plane per frame: the four corner paths and two random quadtrees."""
    fpr = depth
    names = list(_maps(1))
    maps = [_maps(1)[n] for n in names]
    for kind in ("rough", "hot"):
        got = _inverse(hip, fpr, layout, 0, _frames(0, fpr, 1, names, 1, kind), maps, 1, PIC[0, 1])
        _assert_planes(got, _frames(0, fpr, 1, names, 1, "want_" + kind), names, 1)
    got = _inverse(hip, fpr, layout, 0, _frames(0, fpr, 1, names, 1, "coef"), maps, 1, PIC[0, 1])
    _assert_planes(got, _frames(0, fpr, 1, names, 1, "px"), names, 1)


# ---- batch geometry ------------------------------------------------------------------------------

@pytest.mark.parametrize("dec,ppf", [(0, 1), (1, 2), (0, 3)], ids=["luma", "cbcr420", "yuv444"])
def test_three_frames_three_maps_in_one_call(hip, depth, dec, ppf):
    """bstride above the compact width, a frame stride that is no multiple of the row, and every byte in
    between holding no block size: a misaddressed read leaves a tile untransformed."""
    fpr = depth
    names = ["random1", "corners", "units01"]
    maps = [_maps()[n] for n in names]
    rows, cols = maps[0].shape
    bstride = cols + 5
    frame_stride = rows * bstride + 13
    assert frame_stride % bstride
    got = _inverse(hip, fpr, "min4", dec, _frames(dec, fpr, NSBX, names, ppf, "rough"), maps, ppf, PIC[dec, NSBX],
                   bstride, frame_stride)
    _assert_planes(got, _frames(dec, fpr, NSBX, names, ppf, "want_rough"), names, ppf)


# ---- the 4:2:0 derivation ------------------------------------------------------------------------

def test_chroma_of_4x4_and_8x8_luma_is_a_4x4_leaf(hip, depth):
    """The same chroma coefficients under `units01`, a random 0 / 1 map, all-8x8 and all-4x4 luma: four times the
    planes of inverse(), which are the oracle's uniform level 0 - no chroma split below 8x8."""
    fpr = depth
    o = oracle()
    names = ["units01", "nodes16", "uniform1", "uniform0"]
    maps = [_maps()["units01"], _maps()["nodes16"], R.uniform(1, NSBX, NSBY), R.uniform(0, NSBX, NSBY)]
    pw, ph = PIC[1, NSBX]
    one = _frames(1, fpr, NSBX, ["units01"], 2, "rough")
    h, w = one.shape[1:]
    want = np.zeros(one.shape, np.uint16 if fpr else np.uint8)
    o.odo_set_fpr(int(fpr))
    try:
        for p in range(2):
            o.odo_inverse_level_plane(P(want[p]), w, P(np.zeros((h, w), np.int32)), P(np.ascontiguousarray(one[p])), w, h,
                                      1, 0, pw, ph)
    finally:
        o.odo_set_fpr(0)
    want = want.view(_px_dtype(fpr))
    for p in range(2):
        for m in maps:
            assert np.array_equal(R.inverse(one[p], m, 1, pw, ph, fpr), want[p])
    got = _inverse(hip, fpr, "packed", 1, np.concatenate([one] * 4), maps, 2, (pw, ph))
    _assert_planes(got, np.concatenate([want] * 4), names, 2)


# ---- the real decoder's planes -------------------------------------------------------------------

CASES = R.load_cases(GOLDEN + "/partition.npz")
CASE_IDS = ["c%df%dp%d" % (r["clip"], r["frame"], r["pli"]) for r in CASES]


@pytest.mark.parametrize("i", range(len(CASES)), ids=CASE_IDS)
def test_golden_planes_device_form_and_host_form(hip, i):
    """8-bit, as recorded.  The host form with px_stride > w and bstride above the compact width."""
    r = CASES[i]
    L = hip.lib()
    h, w = r["coef"].shape
    pic = (r["pic_w"], r["pic_h"])
    for layout in LAYOUTS:
        got = _inverse(hip, False, layout, r["dec"], r["coef"][None], [r["bmap"]], 1, pic)
        assert np.array_equal(got[0], r["recon"]), layout
    rows, cols = r["bmap"].shape
    bstride = cols + 3
    bmap = _map_buffer([r["bmap"]], bstride, rows * bstride)
    px = PlaneSet(1, h, w, np.uint8, stride=w + 7, base=3, device=None)
    coef = np.ascontiguousarray(r["coef"])
    rc = L.odhip_inverse_partition_host(px.ptr, px.stride, P(coef), w, h, r["dec"], P(bmap), bstride, pic[0], pic[1])
    assert rc == 0
    assert np.array_equal(px.read()[0], r["recon"]) and px.intact()


def test_host_form_is_refused_with_full_precision_references(hip, depth):
    """It stages w*h BYTES of pixels; a full-precision context's inverse stores int16 samples."""
    fpr = depth
    r = CASES[0]
    h, w = r["coef"].shape
    px = PlaneSet(1, h, w, np.uint8, device=None)
    coef = np.ascontiguousarray(r["coef"])
    bmap = np.ascontiguousarray(r["bmap"])
    rc = hip.lib().odhip_inverse_partition_host(px.ptr, px.stride, P(coef), w, h, r["dec"], P(bmap), bmap.shape[1],
                                                r["pic_w"], r["pic_h"])
    if fpr:
        assert rc == EIMPL
        assert px.intact(0, 0)                  # the host buffer is untouched
    else:
        assert rc == 0 and np.array_equal(px.read()[0], r["recon"]) and px.intact()


# ---- refusals before any launch ------------------------------------------------------------------

def test_arguments_outside_the_contract_are_refused(hip, depth):
    fpr = depth
    L = hip.lib()
    dec, ppf = 0, 1
    names = ["corners"]
    maps = [_maps()[n] for n in names]
    coefs = _frames(dec, fpr, NSBX, names, ppf, "rough")
    nplanes, h, w = coefs.shape
    rows, cols = maps[0].shape
    out = PlaneSet.in_layout("min4", nplanes, h, w, _px_dtype(fpr))
    tb = _cuda(_map_buffer(maps, cols, rows * cols))
    tc = _cuda(np.concatenate([coefs.ravel(), np.zeros(4, np.int32)]))
    assert tc.data_ptr() % 16 == 0
    pw, ph = PIC[dec, NSBX]

    def call(coef_off=0, bsize=tb.data_ptr(), bstride=cols, planes_per_frame=ppf):
        return L.odhip_inverse_partition(out.ptr, out.stride, out.pitch, ctypes.c_void_p(tc.data_ptr() + coef_off), nplanes,
                                         w, h, dec, ctypes.c_void_p(bsize), bstride, ctypes.c_long(rows * cols),
                                         planes_per_frame, pw, ph, None)

    assert call(bsize=None) == EINVAL                   # no map
    assert call(planes_per_frame=0) == EINVAL
    assert call(planes_per_frame=-1) == EINVAL
    assert call(bstride=cols - 1) == EINVAL             # rows of the map overlap
    assert call(coef_off=4) == EINVAL                   # coefficients off 16 bytes
    assert call(coef_off=8) == EINVAL
    _sync()
    assert out.intact(0, 0)                             # nothing was written anywhere
    assert call() == 0
    _sync()
    assert out.intact()
    _assert_planes(out.read(), _frames(dec, fpr, NSBX, names, ppf, "want_rough"), names, ppf)
