"""tests/golden/bsize.npz (tools/gen_bsize_golden.py) is what the compiled reference's od_split_superblock gives for
the named cases of _bsize_cases.py, and those cases cover what they are there for."""
import numpy as np
import pytest

import _bsize_cases as B
from _libs import ref

CASES = B.cases()


@pytest.mark.skipif(ref() is None, reason="oracle/_ref (the compiled reference) not present")
@pytest.mark.parametrize("name,q", B.case_ids())
def test_fixture_is_the_compiled_reference(name, q):
    px, pred, _ = CASES[name]
    bmap, noise, psy = B.ref_decide(ref(), px, pred, q)
    wmap, wnoise, wpsy = B.expected(name, q)
    assert np.array_equal(bmap, wmap) and np.array_equal(noise, wnoise) and B.same_bits(psy, wpsy)


def _sizes(name, q):
    return np.bincount(B.expected(name, q)[0].ravel(), minlength=4).tolist()


def test_fixture_holds_every_case():
    for name, q in B.case_ids():
        bmap, noise, psy = B.expected(name, q)
        h, w = CASES[name][0].shape
        assert bmap.shape == (h // 8, w // 8) and bmap.dtype == np.uint8
        assert noise.shape == (h // 32, w // 32, B.NOISE) and noise.dtype == np.int32
        assert psy.shape == (h // 32, w // 32, B.PSY) and psy.dtype == np.float32


def test_tex_has_all_four_sizes():
    for q in B.TEX_Q:
        assert all(n > 0 for n in _sizes("tex", q)), q
    assert _sizes("tex", 800) == [11, 49, 68, 64]
    assert all(n > 0 for n in _sizes("tex_inter", 800))
    s = _sizes("tex_inter", 4000)
    assert s[0] == 0 and s[1] == 0 and s[2] > 0 and s[3] > 0


def test_inter_adjustment_is_engaged():
    """(q >> OD_COEFF_SHIFT) > 40 lowers OD_CG4 / OD_CG8 of an inter cell (src/block_size_enc.c:361-362)."""
    qs = CASES["synth_inter"][2]
    assert [(q >> 4) > 40 for q in qs] == [False, True, True]
    # the prediction matters: the inter maps are not the keyframe maps of the same pictures
    assert not np.array_equal(B.expected("tex_inter", 800)[0], B.expected("tex", 800)[0])
    assert not np.array_equal(B.expected("tex_inter", 800)[1], B.expected("tex", 800)[1])


def test_extremes_reach_the_floors_and_the_clamp():
    """Flat pictures sit on the variance floor (4 + the mean's share); the checkerboard has the largest sums; 255
    over 0 and 0 over 255 clamp the residual to 127 and -128, flat again."""
    assert np.all(B.expected("zeros", 800)[1] == 4)                 # Sx = -128 per sample: floor 4
    for name in ("full", "hi_lo"):                                  # residual +255 -> 127, flat like "full"
        assert np.all(B.expected(name, 800)[1][..., :85] == 4 + 15)     # Sx4 = 127*16, (2032 + 2048) >> 8 = 15
        assert np.all(B.expected(name, 800)[1][..., 85:] == 4 + 63)     # Sx8 = 127*64, (8128 + 8192) >> 8 = 63
    assert B.expected("checker", 800)[1].max() > 8000
    assert np.all(B.expected("lo_hi", 800)[1] == 4)                 # residual -255 -> -128
    assert np.all(B.expected("same_pred", 800)[1][..., :85] == 4 + 8)   # residual 0: Sx4 = 0, 2048 >> 8 = 8
