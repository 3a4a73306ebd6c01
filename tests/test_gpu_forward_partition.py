"""GPU: odhip_forward_partition (k_forward_part<64/32>, daala_amd/csrc/lapped_kernels.hip) - the coefficients the
encoder codes at a block-size map that varies INSIDE a superblock - bit-exact against tests/_partition_ref.py::forward
(the encoder's recursion composed from the oracle's primitives, tests/test_partition_ref.py).  The shapes, picture
sizes and map families are those of tests/test_gpu_partition.py, which checks the inverse.

What each family is there to reach in the kernel:
  map families      PartIsLeaf per level, the split predicate `node.at(bx, by) < LN`, sb_load's 8-bit and int16 paths,
                    the superblock-edge lapping at edges that couple unlike partitions
  picture gates     `(bx + 1)*N <= pic_w` of split_filter_cols_if / `(by + 1)*N <= pic_h` of split_filter_rows_if at
                    every node size, counted in luma units for 4:2:0 too
  uniform maps      the one case where a level of odhip_forward_pyramid is the answer
  round trip        odhip_inverse_partition undoes it on the device
  batch geometry    the map address `bsize + (plane / planes_per_frame)*bsize_frame_stride + row*bstride`
  one superblock    no superblock edge at all, a picture smaller than the tile
  golden            the real decoder's own maps, device form and host form
  refusals          the argument checks in front of the launch
"""
import ctypes
import functools

import numpy as np
import pytest

import _partition_ref as R
from _libs import GOLDEN, P, synth_frame
from _strided import PlaneSet

pytestmark = pytest.mark.gpu

EINVAL, EIMPL = -10, -23
# 3 x 2 superblocks: the smallest frame with interior superblock edges both ways (luma 192x128, 4:2:0 chroma 96x64);
# the LUMA picture sizes put the width ON a node border (160 = 5*32, 80 = 5*16, 48 = 3*16) and the height between
# borders, so that the split filters' gate flips inside the last superblock
NSBX, NSBY = 3, 2
PIC = {(0, NSBX): (160, 106), (1, NSBX): (80, 44), (0, 1): (48, 44), (1, 1): (24, 22)}
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


# ---- CPU side: maps, pixels and expectations, once per module -------------------------------------

@functools.lru_cache(maxsize=None)
def _maps(nsbx=NSBX):
    nsby = NSBY if nsbx == NSBX else 1
    rng = np.random.RandomState(4 + nsbx)
    maps = {"corners": R.corners(nsbx, nsby), "extremes": R.extremes(nsbx, nsby), "units01": R.units01(nsbx, nsby),
            "nodes16": R.nodes16(rng, nsbx, nsby)}
    if nsbx == 1:
        maps = {"corner%d" % k: R.deep_corner(k) for k in range(4)}
    for k in range(2):
        want = [0, 1, 2, 3, 4] if nsbx > 1 else [0, 1, 2, 3]
        for _ in range(200):
            m = R.random_map(rng, nsbx, nsby, 0.55 + 0.2 * k)
            if R.leaf_sizes(m) == want:
                break
        assert R.leaf_sizes(m) == want, (k, R.leaf_sizes(m))
        maps["random%d" % k] = m
    for level in range(5):
        maps["uniform%d" % level] = R.uniform(level, nsbx, nsby)
    for m in maps.values():
        assert R.is_quadtree(m)
        m.setflags(write=False)
    return maps


@functools.lru_cache(maxsize=None)
def _px(dec, fpr, nsbx, variant):
    """One plane of noisy pixels with saturated patches at both ends of the range (0..255, or int16 in 0..4095);
    `variant` tells the planes of one frame apart."""
    nsby = NSBY if nsbx == NSBX else 1
    h, w = (nsby * 64) >> dec, (nsbx * 64) >> dec
    rng = np.random.RandomState(1000 * dec + 100 * variant + 7 * int(fpr) + nsbx)
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
    px = np.ascontiguousarray(px.astype(_px_dtype(fpr)))
    px.setflags(write=False)
    return px


@functools.lru_cache(maxsize=None)
def _want(dec, fpr, nsbx, name, variant, pic=None):
    pw, ph = PIC[dec, nsbx] if pic is None else pic
    c = R.forward(_px(dec, fpr, nsbx, variant), _maps(nsbx)[name], dec, pw, ph, fpr)
    c.setflags(write=False)
    return c


def _pixels(dec, fpr, nsbx, names, ppf):
    """[len(names)*ppf][h][w]: plane `variant` of every frame, frames in the order of `names`."""
    return np.stack([_px(dec, fpr, nsbx, v) for _ in names for v in range(ppf)])


def _wanted(dec, fpr, nsbx, names, ppf, pic=None):
    return np.stack([_want(dec, fpr, nsbx, name, v, pic) for name in names for v in range(ppf)])


def _map_buffer(maps, bstride, frame_stride):
    rows, cols = maps[0].shape
    assert bstride >= cols and frame_stride >= (rows - 1) * bstride + cols
    buf = np.full(len(maps) * frame_stride + 64, GAP, np.uint8)
    for f, m in enumerate(maps):
        for r in range(rows):
            buf[f * frame_stride + r * bstride:f * frame_stride + r * bstride + cols] = m[r]
    return buf


def _forward(hip, fpr, layout, dec, px, maps, ppf, pic, bstride=None, frame_stride=None):
    """odhip_forward_partition of px [nplanes][h][w], handed over in `layout`, at `maps` (one per frame of ppf
    planes) into sentinel-surrounded coefficient planes; every map read stays inside the map buffer (asserted by
    _map_buffer)."""
    nplanes, h, w = px.shape
    rows, cols = maps[0].shape
    assert nplanes == len(maps) * ppf and (rows, cols) == ((h << dec) // 8, (w << dec) // 8)
    bstride = cols if bstride is None else bstride
    frame_stride = rows * bstride if frame_stride is None else frame_stride
    src = PlaneSet.in_layout(layout, nplanes, h, w, _px_dtype(fpr)).write(px)
    out = PlaneSet(nplanes, h, w, np.int32)
    tb = _cuda(_map_buffer(maps, bstride, frame_stride))
    rc = hip.lib().odhip_forward_partition(out.ptr, src.ptr, src.stride, src.pitch, nplanes, w, h, dec,
                                           ctypes.c_void_p(tb.data_ptr()), bstride, ctypes.c_long(frame_stride), ppf,
                                           pic[0], pic[1], None)
    assert rc == 0
    _sync()
    assert out.intact() and src.intact(), layout
    assert np.array_equal(src.read(), px)                   # the source is only read
    return out.read()


def _inverse(hip, fpr, dec, coefs, maps, ppf, pic):
    nplanes, h, w = coefs.shape
    rows, cols = maps[0].shape
    out = PlaneSet(nplanes, h, w, _px_dtype(fpr))
    tb, tc = _cuda(_map_buffer(maps, cols, rows * cols)), _cuda(coefs)
    assert tc.data_ptr() % 16 == 0
    rc = hip.lib().odhip_inverse_partition(out.ptr, out.stride, out.pitch, ctypes.c_void_p(tc.data_ptr()), nplanes, w, h,
                                           dec, ctypes.c_void_p(tb.data_ptr()), cols, ctypes.c_long(rows * cols), ppf,
                                           pic[0], pic[1], None)
    assert rc == 0
    _sync()
    assert out.intact()
    return out.read()


def _assert_planes(got, want, names, ppf):
    assert got.shape == want.shape and got.dtype == want.dtype
    for i in range(got.shape[0]):
        bad = int((got[i] != want[i]).sum())
        assert bad == 0, "map %s plane %d: %d coefficients differ" % (names[i // ppf], i % ppf, bad)


# ---- every map family in one call, luma and 4:2:0 chroma ------------------------------------------

@pytest.mark.parametrize("layout", LAYOUTS)
@pytest.mark.parametrize("dec", [0, 1], ids=["y192x128", "c96x64"])
def test_mixed_maps_equal_the_restated_recursion(hip, depth, dec, layout):
    fpr, ppf = depth, 1 + dec
    maps = [_maps()[n] for n in MAP_NAMES]
    got = _forward(hip, fpr, layout, dec, _pixels(dec, fpr, NSBX, MAP_NAMES, ppf), maps, ppf, PIC[dec, NSBX])
    want = _wanted(dec, fpr, NSBX, MAP_NAMES, ppf)
    _assert_planes(got, want, MAP_NAMES, ppf)
    # the families are not the pyramid's business: a mixed map differs from every uniform one somewhere
    for level in range(5 - dec):
        assert not np.array_equal(want[0], _want(dec, fpr, NSBX, "uniform%d" % level, 0))


# ---- the picture gate of the split filters --------------------------------------------------------

@pytest.mark.parametrize("dec", [0, 1], ids=["y192x128", "c96x64"])
def test_gate_flips_at_every_node_size(hip, depth, dec):
    """A split node of side N = 8 .. TILE samples of the plane, the first of its size in the last superblock
    column: filtered when its right border (bx + 1)*N is inside the LUMA picture width, also for a 4:2:0 plane
    (whose own width the border is counted in); one sample narrower it is not.  The height lies between borders
    of every node size.  An all-4x4 map splits every node, `corners` only some."""
    fpr = depth
    tile = 64 >> dec
    w = NSBX * tile
    names = ["uniform0", "corners"]
    maps = [_maps()[n] for n in names]
    px = _pixels(dec, fpr, NSBX, names, 1)
    pic_h = PIC[dec, NSBX][1]
    for lv in range(1, 5 - dec):
        n = 4 << lv
        on = w - tile + n
        assert on % n == 0 and w - tile < on <= w and pic_h % n
        res = {}
        for pic_w in (on, on - 1):
            got = _forward(hip, fpr, "packed", dec, px, maps, 1, (pic_w, pic_h))
            _assert_planes(got, _wanted(dec, fpr, NSBX, names, 1, (pic_w, pic_h)), names, 1)
            res[pic_w] = got
        assert not np.array_equal(res[on][0], res[on - 1][0]), n


@pytest.mark.parametrize("dec", [0, 1], ids=["y192x128", "c96x64"])
def test_height_gate_flips_too(hip, depth, dec):
    """The same for `(by + 1)*N <= pic_h`, at the 16-sample nodes: height ON a border, width between."""
    fpr = depth
    tile = 64 >> dec
    w, h = NSBX * tile, NSBY * tile
    names = ["uniform0", "random1"]
    maps = [_maps()[n] for n in names]
    px = _pixels(dec, fpr, NSBX, names, 1)
    on = h - tile + 16
    res = {}
    for pic_h in (on, on - 1):
        pic = (w - 11, pic_h)
        got = _forward(hip, fpr, "packed", dec, px, maps, 1, pic)
        _assert_planes(got, _wanted(dec, fpr, NSBX, names, 1, pic), names, 1)
        res[pic_h] = got
    assert not np.array_equal(res[on][0], res[on - 1][0])


# ---- uniform maps: the pyramid's levels -----------------------------------------------------------

@pytest.mark.parametrize("dec", [0, 1], ids=["y192x128", "c96x64"])
def test_uniform_maps_are_the_pyramid_levels(hip, depth, dec):
    """Five frames of the same pixels at luma maps 0..4: each is the pyramid's level of that size, byte for byte;
    a 4:2:0 plane at luma map L is chroma level max(L - 1, 0)."""
    import torch
    fpr = depth
    names = ["uniform%d" % level for level in range(5)]
    maps = [_maps()[n] for n in names]
    px = _pixels(dec, fpr, NSBX, names, 1)
    pic = PIC[dec, NSBX]
    got = _forward(hip, fpr, "packed", dec, px, maps, 1, pic)
    _assert_planes(got, _wanted(dec, fpr, NSBX, names, 1), names, 1)
    levels = hip.forward_pyramid(torch.from_numpy(px[:1].copy()).cuda(), dec, pic[0], pic[1])
    _sync()
    for level in range(5):
        lv = levels[max(level - dec, 0)][0].cpu().numpy()
        assert lv.tobytes() == got[level].tobytes(), level
    # and through the package's wrapper, the map as a tensor
    bm = torch.from_numpy(np.stack(maps)).cuda()
    out = hip.forward_partition(torch.from_numpy(px.copy()).cuda(), bm, dec, pic[0], pic[1])
    _sync()
    assert np.array_equal(out.cpu().numpy(), got)


# ---- round trip on the device ---------------------------------------------------------------------

@pytest.mark.parametrize("dec", [0, 1], ids=["y192x128", "c96x64"])
def test_inverse_partition_gives_the_pixels_back(hip, depth, dec):
    fpr, ppf = depth, 1 + dec
    maps = [_maps()[n] for n in MAP_NAMES]
    px = _pixels(dec, fpr, NSBX, MAP_NAMES, ppf)
    coef = _forward(hip, fpr, "min4", dec, px, maps, ppf, PIC[dec, NSBX])
    back = _inverse(hip, fpr, dec, coef, maps, ppf, PIC[dec, NSBX])
    assert back.dtype == px.dtype
    for i in range(px.shape[0]):
        assert np.array_equal(back[i], px[i]), (MAP_NAMES[i // ppf], i % ppf)


# ---- batch geometry -------------------------------------------------------------------------------

@pytest.mark.parametrize("dec,ppf", [(0, 1), (1, 2), (0, 3)], ids=["luma", "cbcr420", "yuv444"])
def test_three_frames_three_maps_in_one_call(hip, depth, dec, ppf):
    """bstride above the compact width, a frame stride that is no multiple of the row, every byte in between
    holding no block size, and pixel planes at strides and an offset: a misaddressed read of the map leaves a tile
    without leaves."""
    fpr = depth
    names = ["random1", "corners", "units01"]
    maps = [_maps()[n] for n in names]
    rows, cols = maps[0].shape
    bstride = cols + 5
    frame_stride = rows * bstride + 13
    assert frame_stride % bstride
    got = _forward(hip, fpr, "min4", dec, _pixels(dec, fpr, NSBX, names, ppf), maps, ppf, PIC[dec, NSBX], bstride,
                   frame_stride)
    _assert_planes(got, _wanted(dec, fpr, NSBX, names, ppf), names, ppf)


# ---- one superblock -------------------------------------------------------------------------------

@pytest.mark.parametrize("layout", LAYOUTS)
@pytest.mark.parametrize("dec", [0, 1], ids=["y64x64", "c32x32"])
def test_one_superblock_has_no_edge(hip, depth, dec, layout):
    """One tile per frame, the picture smaller than it: the four corner paths, two random quadtrees, and the
    uniform maps."""
    fpr = depth
    names = list(_maps(1))
    maps = [_maps(1)[n] for n in names]
    got = _forward(hip, fpr, layout, dec, _pixels(dec, fpr, 1, names, 1), maps, 1, PIC[dec, 1])
    _assert_planes(got, _wanted(dec, fpr, 1, names, 1), names, 1)


# ---- the real decoder's maps ----------------------------------------------------------------------

CASES = R.load_cases(GOLDEN + "/partition.npz")
CASE_IDS = ["c%df%dp%d" % (r["clip"], r["frame"], r["pli"]) for r in CASES]


@functools.lru_cache(maxsize=None)
def _golden_want(i):
    r = CASES[i]
    return R.forward(r["recon"], r["bmap"], r["dec"], r["pic_w"], r["pic_h"], False)


@pytest.mark.parametrize("i", range(len(CASES)), ids=CASE_IDS)
def test_golden_maps_device_form_and_host_form(hip, i):
    """8-bit, as recorded: the decoder's reconstruction forward at the decoder's map.  The host form with
    px_stride > w and bstride above the compact width."""
    r = CASES[i]
    h, w = r["recon"].shape
    pic = (r["pic_w"], r["pic_h"])
    want = _golden_want(i)
    for layout in LAYOUTS:
        got = _forward(hip, False, layout, r["dec"], r["recon"][None], [r["bmap"]], 1, pic)
        assert np.array_equal(got[0], want), layout
    rows, cols = r["bmap"].shape
    bstride = cols + 3
    bmap = _map_buffer([r["bmap"]], bstride, rows * bstride)
    px = PlaneSet(1, h, w, np.uint8, stride=w + 7, base=3, device=None).write(r["recon"][None])
    out = PlaneSet(1, h, w, np.int32, device=None)
    rc = hip.lib().odhip_forward_partition_host(out.ptr, px.ptr, px.stride, w, h, r["dec"], P(bmap), bstride, pic[0],
                                                pic[1])
    assert rc == 0
    assert np.array_equal(out.read()[0], want) and out.intact() and px.intact()
    if i == 0:
        assert np.array_equal(hip.forward_partition_host(r["recon"], r["bmap"], r["dec"], pic[0], pic[1]), want)


def test_host_form_is_refused_with_full_precision_references(hip, depth):
    """Its px is 8-bit; a full-precision context's forward reads int16 samples."""
    fpr = depth
    r = CASES[0]
    h, w = r["recon"].shape
    px = np.ascontiguousarray(r["recon"])
    bmap = np.ascontiguousarray(r["bmap"])
    out = PlaneSet(1, h, w, np.int32, device=None)
    rc = hip.lib().odhip_forward_partition_host(out.ptr, P(px), w, w, h, r["dec"], P(bmap), bmap.shape[1], r["pic_w"],
                                                r["pic_h"])
    if fpr:
        assert rc == EIMPL
        assert out.intact(0, 0)                 # the host buffer is untouched
    else:
        assert rc == 0 and np.array_equal(out.read()[0], _golden_want(0)) and out.intact()


# ---- refusals before the launch -------------------------------------------------------------------

def test_arguments_outside_the_contract_are_refused(hip, depth):
    fpr = depth
    L = hip.lib()
    dec, ppf = 0, 1
    names = ["corners"]
    maps = [_maps()[n] for n in names]
    px = _pixels(dec, fpr, NSBX, names, ppf)
    nplanes, h, w = px.shape
    rows, cols = maps[0].shape
    src = PlaneSet.in_layout("gap16", nplanes, h, w, _px_dtype(fpr)).write(px)
    out = PlaneSet(nplanes, h, w, np.int32)
    tb = _cuda(_map_buffer(maps, cols, rows * cols))
    pw, ph = PIC[dec, NSBX]
    item = src.dtype.itemsize

    def call(coef_off=0, px_off=0, stride=src.stride, pitch=src.plane_stride, w=w, h=h, bsize=tb.data_ptr(),
             bstride=cols, planes_per_frame=ppf, coef=True, pixels=True, nplanes=nplanes, dec=dec):
        return L.odhip_forward_partition(ctypes.c_void_p(out.ptr.value + coef_off if coef else None),
                                         ctypes.c_void_p(src.ptr.value + px_off if pixels else None), stride,
                                         ctypes.c_long(pitch), nplanes, w, h, dec, ctypes.c_void_p(bsize), bstride,
                                         ctypes.c_long(rows * cols), planes_per_frame, pw, ph, None)

    assert call(bsize=None) == EINVAL                   # no map
    assert call(coef=False) == EINVAL
    assert call(pixels=False) == EINVAL
    assert call(planes_per_frame=0) == EINVAL
    assert call(planes_per_frame=-1) == EINVAL
    assert call(nplanes=0) == EINVAL
    assert call(dec=2) == EINVAL
    assert call(bstride=cols - 1) == EINVAL             # rows of the map overlap
    assert call(coef_off=4) == EINVAL                   # coefficients off 16 bytes
    assert call(coef_off=8) == EINVAL
    assert call(w=w - 32) == EINVAL                     # no whole superblocks
    assert call(h=h - 32) == EINVAL
    assert call(stride=w - 4) == EINVAL                 # rows overlap
    assert call(stride=src.stride + 2, pitch=(src.stride + 2) * h) == EINVAL
    assert call(pitch=src.stride * h - 4) == EINVAL     # planes overlap
    assert call(pitch=src.plane_stride + 2) == EINVAL
    assert call(px_off=2 * item) == EINVAL              # the base off a group of four samples
    _sync()
    assert out.intact(0, 0)                             # nothing was written anywhere
    assert call() == 0
    _sync()
    assert out.intact() and src.intact()
    _assert_planes(out.read(), _wanted(dec, fpr, NSBX, names, ppf), names, ppf)
