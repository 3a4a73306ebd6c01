"""The host path of the block-size decision (odhip_bsize_decide_host / odhip_bsize_terms_host: what
odhip_bsize_resolve runs on the cells it is handed) against od_split_superblock - the recorded fixture everywhere, the
compiled reference itself where it is built - and the argument refusals of every entry point.  No GPU."""
import ctypes

import numpy as np
import pytest

import daala_amd as D
import _bsize_cases as B
from _libs import P, ref

EINVAL = -10
CASES = B.cases()


def _compare(got, want, what):
    gmap, gnoise, gpsy = got
    wmap, wnoise, wpsy = want
    assert np.array_equal(gmap, wmap), what
    assert np.array_equal(gnoise, wnoise), what
    assert B.same_bits(gpsy[..., :B.PSY], wpsy), what


@pytest.mark.parametrize("name,q", B.case_ids())
def test_host_equals_the_reference_function(name, q):
    px, pred, _ = CASES[name]
    bmap, noise, psy, _ = D.bsize_terms_host(px, q, pred)
    _compare((bmap, noise, psy), B.expected(name, q), "fixture")
    if ref() is not None:
        _compare((bmap, noise, psy), B.ref_decide(ref(), px, pred, q), "compiled reference")
    assert np.array_equal(D.bsize_decide_host(px, q, pred), bmap)
    # the five od_psy_var8x8 values the reference does not keep: what psy16 / psy32 were raised to at least
    assert np.all(psy[..., 80:84] >= .5 * psy[..., 85:89]) and np.all(psy[..., 84] >= .5 * psy[..., 89])


def test_host_takes_strides():
    px, pred, _ = CASES["tex_inter"]
    big = np.full((100, 150), 0x5A, np.uint8)
    big[:96, :128] = px
    bigp = np.full((97, 190), 0xC3, np.uint8)
    bigp[:96, :128] = pred
    got = D.bsize_terms_host(big[:96, :128], 800, bigp[:96, :128])
    _compare(got[:3], B.expected("tex_inter", 800), "strided views")


def _legal_quadtree(bmap):
    assert bmap.max() <= 3
    h8, w8 = bmap.shape
    for y in range(0, h8, 4):
        for x in range(0, w8, 4):
            cell = bmap[y:y + 4, x:x + 4]
            if (cell == 3).any():
                assert (cell == 3).all()
            for qy in (0, 2):
                for qx in (0, 2):
                    quad = cell[qy:qy + 2, qx:qx + 2]
                    if (quad == 2).any():
                        assert (quad == 2).all()


@pytest.mark.parametrize("name,q", B.case_ids())
def test_decided_maps_are_quadtrees(name, q):
    """partition_leaves_host of the decided map covers the plane exactly.  The leaf walk takes whole 64x64
    superblocks: the map is completed with 32x32 entries where the plane is no multiple of 64."""
    px, pred, _ = CASES[name]
    bmap = D.bsize_decide_host(px, q, pred)
    _legal_quadtree(bmap)
    h, w = px.shape
    H, W = -(-h // 64) * 64, -(-w // 64) * 64
    full = np.full((H // 8, W // 8), 3, np.uint8)
    full[:h // 8, :w // 8] = bmap
    leaves = D.partition_leaves_host(full, 1, H, W, 0)
    area = sum(int(leaves.counts[s, 0]) * (4 << s) ** 2 for s in range(D.api.NBSIZES))
    assert area == W * H
    assert int(leaves.counts[4, 0]) == 0
    pad_cells = (W * H - w * h) // (32 * 32)
    for s in range(4):
        want = int((bmap == s).sum()) * 64 // (4 << s) ** 2 + (pad_cells if s == 3 else 0)
        assert int(leaves.counts[s, 0]) == want, s


def test_refusals_make_no_hip_call(capfd):
    L = D.lib()
    px = np.zeros((64, 64), np.uint8)
    bmap = np.zeros((8, 8), np.uint8)
    q = np.array([800, 800], np.int32)
    neg = np.array([800, -1], np.int32)
    n = ctypes.c_int(-7)
    terms = np.zeros(2 * 4 * 90, np.int32)
    long_ = ctypes.c_long

    def device(bsize=P(bmap), bstride=8, d_px=P(px), px_stride=64, d_pred=None, pred_stride=64, nframes=1, w=64,
               h=64, quant=P(q)):
        a = (bsize, bstride, long_(64), d_px, px_stride, long_(4096), d_pred, pred_stride, long_(4096), nframes, w, h,
             quant, None)
        rcs = {L.odhip_bsize_decide(*a), L.odhip_bsize_resolve(*(a + (ctypes.byref(n),))),
               L.odhip_bsize_terms(*((P(terms), P(terms)) + a + (ctypes.byref(n),)))}
        assert len(rcs) == 1
        return rcs.pop()

    def host(bsize=P(bmap), bstride=8, p=P(px), px_stride=64, pred=None, pred_stride=64, w=64, h=64, quant=800):
        rcs = {L.odhip_bsize_decide_host(bsize, bstride, p, px_stride, pred, pred_stride, w, h, quant),
               L.odhip_bsize_terms_host(None, None, bsize, bstride, p, px_stride, pred, pred_stride, w, h, quant, 1.0,
                                        None)}
        assert len(rcs) == 1
        return rcs.pop()

    for fn in (device, host):
        assert fn(w=48) == EINVAL and fn(h=40) == EINVAL and fn(w=0) == EINVAL and fn(h=-32) == EINVAL
        assert fn(w=8192 + 32, bstride=2000, px_stride=9000) == EINVAL
        assert fn(h=8192 + 32) == EINVAL
        assert fn(bstride=7) == EINVAL
        assert fn(px_stride=63) == EINVAL
        assert fn(**{"d_pred" if fn is device else "pred": P(px)}, pred_stride=63) == EINVAL
        assert fn(bsize=None) == EINVAL
        assert fn(**{"d_px" if fn is device else "p": None}) == EINVAL
    assert device(quant=None) == EINVAL
    assert device(nframes=0) == EINVAL and device(nframes=-1) == EINVAL
    assert device(nframes=2, quant=P(neg)) == EINVAL
    assert host(quant=-1) == EINVAL
    a = (P(bmap), 8, long_(64), P(px), 64, long_(4096), None, 64, long_(4096), 1, 64, 64, P(q), None)
    assert L.odhip_bsize_resolve(*(a + (None,))) == EINVAL
    assert L.odhip_bsize_terms(*((None, P(terms)) + a + (ctypes.byref(n),))) == EINVAL
    assert L.odhip_bsize_terms_host(P(terms), None, P(bmap), 8, P(px), 64, None, 64, 64, 64, 800, 1.0, None) == EINVAL
    assert n.value == -7 and not bmap.any()
    # a refusal that had looked for a device or a context would have said so on stderr
    assert "libdaalahip" not in capfd.readouterr().err
    # and the same arguments, legal, are served on the host
    assert host() == 0


def test_pred_equal_to_px_is_a_keyframe():
    """The reference's psy_img == pred branch: the SAME buffer is no prediction (a copy of it is one)."""
    px = CASES["tex"][0]
    key = D.bsize_terms_host(px, 4000)
    same = D.bsize_terms_host(px, 4000, px)
    for a, b in zip(key[:3], same[:3]):
        assert np.array_equal(a, b)
    copy = D.bsize_terms_host(px, 4000, px.copy())
    assert not np.array_equal(copy[1], key[1])      # the residual's variances, not the picture's
