"""GPU: the Haar-wavelet / lossless coefficient path (k_haar_forward, k_haar_dc, k_haar_inverse, k_haar_planes;
daala_amd/csrc/haar_kernels.hip) bit-exact against tests/_haar_ref.py, the reference's loops restated
(tests/test_haar_ref.py pins its transforms to the compiled reference and shows that the inputs of
tests/_haar_cases.py reach ties, every DC-predictor case, both sides of the dead zone, both clamps).

  bare transforms   od_haar / od_haar_inv of ln = 2..6 on values up to +-2^17
  encode            q, tree, dc_rec, rec of every case: keyframe and inter, 8-bit and the three depths of a
                    full-precision-references context, lossless and three quantisers, 3 x 2 superblocks and one
  decode            odhip_haar_decode_planes of the encoder's symbols alone, queued on another stream once the
                    encoder has finished, gives the encoder's rec and dc_rec, keyframe and inter
  padding           inter: coefficients whose support lies outside the picture are zero
  round trip        lossless: rec == source, the property no other path of the library has
  tree invariant    on the device's own planes
  DC walk           a plane of more superblocks than k_haar_dc stages in LDS
  refusals          with real buffers, where a good job runs: one bad argument at a time
"""
import contextlib
import ctypes

import numpy as np
import pytest

import _haar_cases as C
import _haar_ref as R

pytestmark = pytest.mark.gpu

EINVAL = -10


@pytest.fixture(scope="module")
def hip():
    import torch
    import daala_amd
    assert torch.cuda.is_available()
    daala_amd.init(0)
    return daala_amd


@contextlib.contextmanager
def _context(hip, fpr):
    """The calling thread in an 8-bit or a full-precision-references context."""
    ctx = hip.Context(0).set_fpr(fpr)
    try:
        with ctx:
            yield
    finally:
        ctx.destroy()


def _cuda(a):
    import torch
    return None if a is None else torch.from_numpy(np.array(a, order="C")).cuda()


def _sync():
    import torch
    torch.cuda.synchronize()


def _encode(hip, px, pred, dec, pic, depth, quant, dcq, split, want_rec=True):
    import torch
    nplanes, h, w = px.shape
    tile = 64 >> dec
    dc_rec = torch.full((nplanes, (h // tile) * (w // tile)), -77, dtype=torch.int32, device="cuda")
    q, tree, rec = hip.haar_encode(_cuda(px), _cuda(pred), dec=dec, pic_w=pic[0], pic_h=pic[1], depth=depth,
                                   quant=quant, dc_quant=dcq, plane_split=split, want_rec=want_rec, dc_rec=dc_rec)
    _sync()
    return q, tree, dc_rec, rec


def _decode_on_second_stream(hip, q, pred, dec, depth, quant, dcq, split):
    """(rec, dc_rec) of odhip_haar_decode_planes, queued on a stream that is not the encoder's, after the encoder has
    finished: the decoder takes nothing from the encoder's call but the symbols.  (Nothing here overlaps: keyframe jobs
    of one context share a scratch buffer and must not, include/daala_hip.h.)"""
    import torch
    nplanes, h, w = q.shape
    tile = 64 >> dec
    dc_rec = torch.full((nplanes, (h // tile) * (w // tile)), -77, dtype=torch.int32, device="cuda")
    side = torch.cuda.Stream()
    with torch.cuda.stream(side):
        rec = hip.haar_decode(q, _cuda(pred), dec=dec, depth=depth, quant=quant, dc_quant=dcq, plane_split=split,
                              dc_rec=dc_rec)
    side.synchronize()
    return rec.cpu().numpy(), dc_rec.cpu().numpy()


# ---- the bare transforms ---------------------------------------------------------------------------

@pytest.mark.parametrize("inverse", [False, True], ids=["od_haar", "od_haar_inv"])
@pytest.mark.parametrize("ln", [2, 3, 4, 5, 6])
def test_bare_transforms_equal_the_restatement(hip, ln, inverse):
    n = 1 << ln
    x = C.transform_inputs(ln)
    got = hip.haar_planes(_cuda(x), ln, inverse=inverse).cpu().numpy()
    fn = R.haar_inv if inverse else R.haar
    for p in range(x.shape[0]):
        for by in range(x.shape[1] // n):
            for bx in range(x.shape[2] // n):
                ys, xs = slice(by * n, (by + 1) * n), slice(bx * n, (bx + 1) * n)
                assert np.array_equal(got[p, ys, xs], np.array(fn(x[p, ys, xs], ln), np.int64)), (p, by, bx)
    if not inverse:
        # reversible, and in place
        t = _cuda(x)
        hip.haar_planes(t, ln, out=t)
        hip.haar_planes(t, ln, inverse=True, out=t)
        assert np.array_equal(t.cpu().numpy(), x)


# ---- encoder and decoder against the restatement ------------------------------------------------------

def _padding_support(h, w, pic_w, pic_h, ln):
    """True where a coefficient's support lies wholly outside the picture: sub-band entry (i, j) of the level with
    np x np entries covers the square of side n/np at (i*n/np, j*n/np) of its block."""
    n = 1 << ln
    out = np.zeros((h, w), bool)
    for by in range(h // n):
        for bx in range(w // n):
            for level in range(ln):
                npairs = n >> (level + 1)
                side = n // npairs
                i, j = np.mgrid[0:npairs, 0:npairs]
                outside = (bx * n + j * side >= pic_w) | (by * n + i * side >= pic_h)
                for dy, dx in ((0, 1), (1, 0), (1, 1)):
                    out[by * n + dy * npairs: by * n + (dy + 1) * npairs,
                        bx * n + dx * npairs: bx * n + (dx + 1) * npairs] = outside
    return out


@pytest.mark.parametrize("name", C.CASE_IDS)
def test_encode_and_decode_equal_the_restatement(hip, name):
    c = C.BY_NAME[name]
    with _context(hip, c.fpr):
        for dec in (0, 1):
            px, pred, want = C.source(name, dec), C.prediction(name, dec), C.want(name, dec)
            pic, dcq, split = C.picture(name, dec), C.dc_quants(c, dec), C.plane_split(dec)
            q, tree, dc_rec, rec = _encode(hip, px, pred, dec, pic, c.depth, c.quant, dcq, split)
            gq, gt = q.cpu().numpy(), tree.cpu().numpy()
            for what, got, exp in (("q", gq, want.q), ("tree", gt, want.tree), ("dc_rec", dc_rec.cpu().numpy(), want.dc_rec),
                                   ("rec", rec.cpu().numpy(), want.rec)):
                assert got.dtype == exp.dtype and got.shape == exp.shape, (what, dec)
                bad = np.argwhere(got != exp)
                assert len(bad) == 0, (what, dec, len(bad), bad[:4].tolist())
            assert C.tree_violations(gq, gt, 6 - dec) == 0
            # the decoder's half, alone, on a stream of its own
            back, back_dc = _decode_on_second_stream(hip, q, pred, dec, c.depth, c.quant, dcq, split)
            assert np.array_equal(back, want.rec), dec
            assert np.array_equal(back_dc, want.dc_rec), dec          # keyframe: k_haar_dc; inter: k_haar_inverse
            # without d_rec and d_dc_rec the symbols are the same
            import torch
            q2, tree2, _ = hip.haar_encode(_cuda(px), _cuda(pred), dec=dec, pic_w=pic[0], pic_h=pic[1], depth=c.depth,
                                           quant=c.quant, dc_quant=dcq, plane_split=split, want_rec=False)
            _sync()
            assert torch.equal(q2, q) and torch.equal(tree2, tree)
            if c.inter:
                # outside the picture the source IS the prediction: every coefficient whose support lies there codes
                # zero at any quantiser; the samples there come back as the prediction when nothing else in their
                # block is quantised away, i.e. lossless (8-bit: the conversion is reversible too)
                _, h, w = px.shape
                dead = _padding_support(h, w, pic[0], pic[1], 6 - dec)
                assert dead.any() and not gq[:, dead].any()
                if c.quant == 0 and not c.fpr:
                    assert np.array_equal(want.rec[:, :, pic[0]:], pred[:, :, pic[0]:])
                    assert np.array_equal(want.rec[:, pic[1]:, :], pred[:, pic[1]:, :])
            if c.quant == 0 and not c.fpr:
                inside = np.s_[:, :pic[1], :pic[0]]
                assert np.array_equal(rec.cpu().numpy()[inside], px[inside])


# ---- the lossless round trip -------------------------------------------------------------------------

@pytest.mark.parametrize("depth", [8, 10, 12])
@pytest.mark.parametrize("inter", [False, True], ids=["key", "inter"])
def test_lossless_round_trip_in_a_full_precision_context(hip, depth, inter):
    """od_ref_buf_to_coeff drops the low OD_COEFF_SHIFT - (depth - 8) bits of an int16 sample (src/state.c:1243-1249),
    so the path is exact for sources that are multiples of 1 << that shift: 16, 4, 1 at depths 8, 10, 12."""
    shift = 4 - (depth - 8)
    name = "inter-fpr10-lossless" if inter else "key-fpr10-lossless"
    with _context(hip, True):
        for dec in (0, 1):
            px = (C.source(name, dec) >> shift << shift).astype(np.int16)
            pred = C.prediction(name, dec) if inter else None
            if inter:
                pred = (pred >> shift << shift).astype(np.int16)
            _, h, w = px.shape
            q, _, _, rec = _encode(hip, px, pred, dec, (w, h), depth, 0, (1, 1), C.plane_split(dec))
            assert np.array_equal(rec.cpu().numpy(), px), dec
            back, _ = _decode_on_second_stream(hip, q, pred, dec, depth, 0, (1, 1), C.plane_split(dec))
            assert np.array_equal(back, px), dec


@pytest.mark.parametrize("inter", [False, True], ids=["key", "inter"])
def test_lossless_round_trip_at_eight_bits(hip, inter):
    name = "inter-u8-lossless" if inter else "key-u8-lossless"
    with _context(hip, False):
        for dec in (0, 1):
            px = C.source(name, dec)
            pred = C.prediction(name, dec)
            _, h, w = px.shape
            q, _, _, rec = _encode(hip, px, pred, dec, (w, h), 8, 0, (1, 1), C.plane_split(dec))
            assert np.array_equal(rec.cpu().numpy(), px), dec
            assert np.array_equal(_decode_on_second_stream(hip, q, pred, dec, 8, 0, (1, 1), C.plane_split(dec))[0], px)


# ---- a DC walk beyond the LDS budget -------------------------------------------------------------------

def test_dc_walk_of_more_superblocks_than_fit_lds(hip):
    """65 x 32 blocks of 32 x 32, above the 2048 superblock DCs k_haar_dc stages in LDS: the walk runs in global memory.
    Every block is flat, so that its Haar transform is DC = (value - 128) << 4 << 5 and nothing else
    (tests/test_haar_ref.py::test_flat_block_transforms_to_its_dc_alone) and the expectation is the DC walk alone."""
    nhsb, nvsb, n, dcq = 65, 32, 32, 37
    rng = np.random.RandomState(9)
    vals = rng.randint(0, 256, size=(nvsb, nhsb))
    vals[:, :4] = 0                                   # negative DCs and predictor sums
    px = np.repeat(np.repeat(vals, n, axis=0), n, axis=1).astype(np.uint8)[None]
    sb_dc_mem = [0] * (nvsb * nhsb)
    syms = np.zeros((nvsb, nhsb), np.int32)
    for by in range(nvsb):
        for bx in range(nhsb):
            dc = (int(vals[by, bx]) - 128) << 4 << 5
            syms[by, bx], _ = R.quantize_haar_dc_sb(sb_dc_mem, nhsb, bx, by, dc, dcq, by > 0 and bx < nhsb - 1)
    with _context(hip, False):
        q, tree, dc_rec, rec = _encode(hip, px, None, 1, (nhsb * n, nvsb * n), 8, 16, (dcq, dcq), 1)
        gq = q.cpu().numpy()[0]
        assert np.array_equal(gq[::n, ::n], syms)
        assert np.array_equal(dc_rec.cpu().numpy()[0], np.array(sb_dc_mem, np.int32))
        assert np.count_nonzero(gq) == np.count_nonzero(syms) and not tree.cpu().numpy().any()
        got = rec.cpu().numpy()[0]
        for by, bx in ((0, 0), (17, 40), (nvsb - 1, nhsb - 1)):
            blk = [[0] * n for _ in range(n)]
            blk[0][0] = sb_dc_mem[by * nhsb + bx]
            exp = R.coeff_to_ref_buf(R.haar_inv(blk, 5), np.uint8, False, 8)
            assert np.array_equal(got[by * n:(by + 1) * n, bx * n:(bx + 1) * n], exp), (by, bx)
        back, back_dc = _decode_on_second_stream(hip, q, None, 1, 8, 16, (dcq, dcq), 1)
        assert np.array_equal(back[0], got)
        assert np.array_equal(back_dc[0], np.array(sb_dc_mem, np.int32))


# ---- refusals where a good job runs -----------------------------------------------------------------------

def test_refusals_in_front_of_the_launch(hip):
    import torch
    name, dec = "inter-u8-q16", 1
    c = C.BY_NAME[name]
    with _context(hip, False):
        px, pred = _cuda(C.source(name, dec)), _cuda(C.prediction(name, dec))
        nplanes, h, w = px.shape
        q = torch.full((nplanes, h, w), 123, dtype=torch.int32, device="cuda")
        tree = torch.full_like(q, 123)
        rec = torch.full_like(px, 9)

        def call(fn="odhip_haar_encode_planes", **kw):
            j = hip.HaarJob()
            j.d_px, j.d_pred, j.d_rec, j.d_q, j.d_tree = (px.data_ptr(), pred.data_ptr(), rec.data_ptr(), q.data_ptr(),
                                                        tree.data_ptr())
            j.px_stride, j.px_plane_stride, j.nplanes, j.w, j.h, j.dec = w, h * w, nplanes, w, h, dec
            j.pic_w, j.pic_h, j.lossless, j.depth, j.quant = 80, 53, 0, 8, 16
            j.dc_quant[0], j.dc_quant[1] = C.dc_quants(c, dec)
            j.plane_split = 2
            for k, v in kw.items():
                if k == "dc_quant":
                    j.dc_quant[0], j.dc_quant[1] = v
                else:
                    setattr(j, k, v)
            return getattr(hip.lib(), fn)(ctypes.byref(j), None)

        bads = [dict(d_px=None), dict(d_q=None), dict(d_tree=None), dict(w=w - 16), dict(h=h - 8), dict(dec=2),
                dict(depth=9), dict(lossless=1), dict(quant=0), dict(quant=-4), dict(dc_quant=(0, 5)),
                dict(dc_quant=(5, -1)), dict(pic_w=w + 1), dict(pic_h=0), dict(plane_split=5), dict(plane_split=-1),
                dict(px_stride=w - 4), dict(px_plane_stride=h * w - 4), dict(d_px=px.data_ptr() + 2),
                dict(d_q=q.data_ptr() + 4), dict(d_tree=tree.data_ptr() + 8), dict(nplanes=0)]
        for bad in bads:
            assert call(**bad) == EINVAL, bad
        assert call("odhip_haar_decode_planes", d_rec=None) == EINVAL
        assert call("odhip_haar_decode_planes", d_q=None) == EINVAL
        _sync()
        assert (q == 123).all() and (tree == 123).all() and (rec == 9).all()       # nothing was launched
        assert call() == 0
        _sync()
        assert np.array_equal(q.cpu().numpy(), C.want(name, dec).q)
        assert np.array_equal(rec.cpu().numpy(), C.want(name, dec).rec)
