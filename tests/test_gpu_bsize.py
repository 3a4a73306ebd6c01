"""odhip_bsize_decide / _resolve / _terms on the device against the recorded reference (tests/golden/bsize.npz,
pinned to the compiled od_split_superblock by test_bsize_ref.py): maps and all terms bit for bit on every named case,
strided buffers with poison around them, several frames and quantisers in one call, the psy_img == pred branch, the
host re-run of listed cells (everything listed; a deliberately wrong device result), the cap on what the default
margin lists, and the composition with the partition transforms."""
import ctypes

import numpy as np
import pytest

import _bsize_cases as B

pytestmark = pytest.mark.gpu

EIMPL = -23
CASES = B.cases()


@pytest.fixture(scope="module")
def hip():
    import torch
    import daala_amd as D
    assert torch.cuda.is_available()
    D.init(0)
    D.bsize_set_test_hooks()
    yield D
    D.bsize_set_test_hooks()


def _cuda(a):
    import torch
    return torch.from_numpy(np.ascontiguousarray(a)).cuda()


def _check(got, name, q, what=""):
    """got: (map, noise, psy) of ONE frame, numpy, against the fixture."""
    wmap, wnoise, wpsy = B.expected(name, q)
    assert np.array_equal(got[0], wmap), (name, q, what)
    assert np.array_equal(got[1], wnoise), (name, q, what)
    assert B.same_bits(got[2][..., :B.PSY], wpsy), (name, q, what)


def _terms(hip, name, q, **kw):
    px, pred, _ = CASES[name]
    bmap, noise, psy, relisted = hip.bsize_terms(_cuda(px), q, None if pred is None else _cuda(pred), **kw)
    return (bmap.cpu().numpy(), noise[0], psy[0]), relisted


@pytest.mark.parametrize("name,q", B.case_ids())
def test_device_equals_the_reference(hip, name, q):
    px, pred, _ = CASES[name]
    got, relisted = _terms(hip, name, q)
    _check(got, name, q)
    # all 90 psy values, the five the reference does not keep included, against the host path
    _, hnoise, hpsy, _ = hip.bsize_terms_host(px, q, pred)
    assert np.array_equal(got[1], hnoise) and B.same_bits(got[2], hpsy)
    # the product call gives the same map and the same count
    bmap, n = hip.bsize_decide(_cuda(px), q, None if pred is None else _cuda(pred))
    assert np.array_equal(bmap.cpu().numpy(), got[0]) and n == relisted
    assert 0 <= relisted <= got[1].shape[0] * got[1].shape[1]


@pytest.mark.parametrize("poison", [0x00, 0xA5])
def test_strides_and_poison(hip, poison):
    """px_stride, pred_stride and bstride wider than needed and all different; what lies around the planes does
    not reach the result and what lies around the map is not written."""
    import torch
    px, pred, _ = CASES["tex_inter"]
    h, w = px.shape
    bpx = np.full((2, h + 5, w + 24), poison, np.uint8)
    bpred = np.full((2, h + 3, w + 40), poison ^ 0xFF, np.uint8)
    bpx[:, :h, :w] = px
    bpred[:, :h, :w] = pred
    bpx[1, :h, :w] = px[::-1]
    out = torch.full((2, h // 8 + 2, w // 8 + 7), 0xEE, dtype=torch.uint8, device="cuda")
    tpx, tpred = _cuda(bpx), _cuda(bpred)
    bmap, noise, psy, _ = hip.bsize_terms(tpx, (800, 4000), tpred, out=out, w=w, h=h)
    assert bmap.data_ptr() == out.data_ptr()
    got = out.cpu().numpy()
    _check((got[0, :h // 8, :w // 8], noise[0], psy[0]), "tex_inter", 800, "strided")
    hmap, hnoise, hpsy, _ = hip.bsize_terms_host(np.ascontiguousarray(px[::-1]), 4000, pred)
    assert np.array_equal(got[1, :h // 8, :w // 8], hmap) and np.array_equal(noise[1], hnoise)
    assert B.same_bits(psy[1], hpsy)
    got[:, :h // 8, :w // 8] = 0xEE
    assert np.all(got == 0xEE)
    assert np.array_equal(tpx.cpu().numpy(), bpx) and np.array_equal(tpred.cpu().numpy(), bpred)


def test_three_frames_three_quantisers(hip):
    px = CASES["tex"][0]
    pred = CASES["tex_inter"][1]
    qs = (160, 800, 4000)
    stack = _cuda(np.stack([px] * 3))
    bmap, noise, psy, _ = hip.bsize_terms(stack, qs)
    for f, q in enumerate(qs):
        _check((bmap[f].cpu().numpy(), noise[f], psy[f]), "tex", q, "frame %d" % f)
        single, _ = _terms(hip, "tex", q)
        assert np.array_equal(single[0], bmap[f].cpu().numpy()) and B.same_bits(single[2], psy[f])
    qs = (4000, 800, 4000)
    bmap, noise, psy, _ = hip.bsize_terms(stack, qs, _cuda(np.stack([pred] * 3)))
    for f, q in enumerate(qs):
        _check((bmap[f].cpu().numpy(), noise[f], psy[f]), "tex_inter", q, "inter frame %d" % f)


def test_more_frames_than_one_launch_takes(hip):
    """17 frames: the second launch of a call numbers its cells and reads its quantisers from frame 16 on."""
    px = CASES["cell"][0]
    n = 17
    qs = [0 if f % 2 else 800 for f in range(n)]
    bmap, noise, psy, _ = hip.bsize_terms(_cuda(np.stack([px] * n)), qs)
    for f in (0, 1, 15, 16):
        _check((bmap[f].cpu().numpy(), noise[f], psy[f]), "cell", qs[f], "frame %d" % f)


def test_pred_is_px(hip):
    """d_pred == d_px with equal strides: the reference's psy_img == pred branch, a keyframe."""
    t = _cuda(CASES["tex"][0])
    bmap, noise, psy, _ = hip.bsize_terms(t, 4000, t)
    _check((bmap.cpu().numpy(), noise[0], psy[0]), "tex", 4000)


@pytest.mark.parametrize("name,q", [("tex", 800), ("tex_inter", 800), ("synth_inter", 4000), ("checker", 800),
                                    ("cell_inter", 800)])
def test_everything_relisted(hip, name, q):
    """A margin no step can clear: every cell goes through the host path.  (Every cell that has a term of the
    device's own log, that is: a flat cell, whose terms all come from the host libm's table, has no step to test -
    test_flat_cells_are_never_listed.)"""
    hip.bsize_set_test_hooks(margin_scale=1e12)
    try:
        got, relisted = _terms(hip, name, q)
    finally:
        hip.bsize_set_test_hooks()
    _check(got, name, q)
    assert relisted == got[1].shape[0] * got[1].shape[1]


@pytest.mark.parametrize("name", ["zeros", "lo_hi"])
def test_flat_cells_are_never_listed(hip, name):
    """noise*invVar == 16384 everywhere: every term is log2 of 2, taken from the table of the host libm's own
    values, so no margin applies - not even one no other step can clear."""
    hip.bsize_set_test_hooks(margin_scale=1e12, perturb=True)
    try:
        got, relisted = _terms(hip, name, 800)
    finally:
        hip.bsize_set_test_hooks()
    _check(got, name, 800)
    assert relisted == 0
    assert np.all(got[1] == 4)      # and invVar is 16384/4 throughout


def test_host_rerun_replaces_device_output(hip):
    """With the device's result of a listed cell deliberately wrong, only the re-run can give the reference's."""
    px = CASES["tex"][0]
    t = _cuda(px)
    want = B.expected("tex", 800)[0]
    relisted = 0
    try:
        for scale in (1., 1e3, 1e5, 1e6, 1e7, 1e8, 1e9):
            hip.bsize_set_test_hooks(margin_scale=scale, perturb=True)
            got, relisted = _terms(hip, "tex", 800)
            _check(got, "tex", 800, "perturbed, scale %g" % scale)
            if relisted > 0:
                break
        assert relisted > 0
        # the hook does what it says: without the resolve the listed cells are wrong
        hip.bsize_set_test_hooks(margin_scale=1e12, perturb=True)
        raw, none = hip.bsize_decide(t, 800, resolve=False)
        assert none is None
        assert np.all(raw.cpu().numpy() != want)
        fixed, n = hip.bsize_decide(t, 800)
        assert n == 12 and np.array_equal(fixed.cpu().numpy(), want)
    finally:
        hip.bsize_set_test_hooks()


@pytest.mark.parametrize("q", B.TEX_Q)
def test_default_margin_lists_few_cells(hip, q):
    """A condition, not a figure: "everything went to the host" must not pass for success.  libm's own terms list
    no cell of "tex" at the default margin (bsize_terms_host's count)."""
    got, relisted = _terms(hip, "tex", q)
    _check(got, "tex", q)
    assert relisted <= 12 // 4
    assert hip.bsize_terms_host(CASES["tex"][0], q)[3] <= 12 // 4


def test_decided_map_feeds_the_partition_transforms(hip):
    """picture -> map -> forward at the map -> inverse at the map gives the picture back, and the leaf lists
    cover it.  The partition transforms take whole 64x64 superblocks: "tex" is continued to 128 x 128."""
    px = np.pad(CASES["tex"][0], ((0, 32), (0, 0)), mode="edge")
    t = _cuda(px[None])
    bmap, _ = hip.bsize_decide(t, 800)
    assert tuple(bmap.shape) == (1, 16, 16)
    assert np.array_equal(bmap[0].cpu().numpy(), hip.bsize_decide_host(px, 800))
    assert sorted(np.unique(bmap.cpu().numpy()).tolist()) == [0, 1, 2, 3]
    coef = hip.forward_partition(t, bmap, 0, 128, 128)
    back = hip.inverse_partition(coef, bmap, 0, 128, 128)
    assert np.array_equal(back.cpu().numpy()[0], px)
    leaves = hip.partition_leaves(bmap, 1, 128, 128, 0)
    assert sum(int(leaves.counts[s, 0]) * (4 << s) ** 2 for s in range(5)) == 128 * 128


def test_full_precision_context_is_refused(hip):
    import torch
    ctx = hip.Context(0).set_fpr(True)
    t = _cuda(CASES["cell"][0][None])
    out = torch.full((1, 4, 4), 0xEE, dtype=torch.uint8, device="cuda")
    try:
        with ctx:
            q = np.array([800], np.int32)
            rc = hip.lib().odhip_bsize_decide(out.data_ptr(), 4, ctypes.c_long(16), t.data_ptr(), 32, ctypes.c_long(1024),
                                              None, 0, ctypes.c_long(0), 1, 32, 32, q.ctypes.data, None)
            assert rc == EIMPL
            with pytest.raises(hip.DaalaHipError):
                hip.bsize_decide(t, 800)
    finally:
        ctx.destroy()
    torch.cuda.synchronize()
    assert np.all(out.cpu().numpy() == 0xEE)
