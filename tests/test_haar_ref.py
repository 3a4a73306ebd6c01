"""CPU: the yardstick of the Haar-wavelet path (tests/_haar_ref.py) and the inputs the GPU test runs on.

Pins        haar / haar_inv of the restatement equal od_haar / od_haar_inv of the COMPILED reference
            (oracle/_ref/libdaalaref.so), ln = 2..6, on the inputs tests/test_gpu_haar.py hands the device.
Conditions  the fixed inputs of tests/_haar_cases.py make the restatement meet what the device could get wrong, so that
            tests/test_gpu_haar.py cannot pass vacuously."""
import numpy as np
import pytest

import _haar_cases as C
import _haar_ref as R
from _libs import P, ref


def _compiled_reference():
    """The pin is the only link between the yardstick and the real reference: without the library it fails."""
    lib = ref()
    assert lib is not None, "oracle/_ref/libdaalaref.so is missing: the build compiles it from the reference tree"
    return lib


def _blocks(x, ln):
    n = 1 << ln
    for p in range(x.shape[0]):
        for by in range(x.shape[1] // n):
            for bx in range(x.shape[2] // n):
                yield np.ascontiguousarray(x[p, by * n:(by + 1) * n, bx * n:(bx + 1) * n])


@pytest.mark.parametrize("ln", [2, 3, 4, 5, 6])
def test_restated_transforms_equal_the_compiled_reference(ln):
    lib = _compiled_reference()
    n = 1 << ln
    x = C.transform_inputs(ln)
    assert x.max() == 1 << 17 and x.min() == -(1 << 17) and (x[2] & 1).all()
    for blk in _blocks(x, ln):
        y = np.zeros((n, n), np.int32)
        lib.od_haar(P(y), n, P(blk), n, ln)
        assert np.array_equal(np.array(R.haar(blk, ln), np.int64), y)
        back = np.zeros((n, n), np.int32)
        lib.od_haar_inv(P(back), n, P(y), n, ln)
        assert np.array_equal(back, blk)                                     # the transform is reversible
        assert np.array_equal(np.array(R.haar_inv(y, ln), np.int64), back)
        # the inverse on its own, of values that are no forward transform's
        z = np.zeros((n, n), np.int32)
        lib.od_haar_inv(P(z), n, P(blk), n, ln)
        assert np.array_equal(np.array(R.haar_inv(blk, ln), np.int64), z)


def test_div_r0_is_c_division():
    for y in (1, 2, 3, 16, 24, 183, 549):
        for x in range(-3 * y - 2, 3 * y + 3):
            off = ((y + 1) >> 1) - 1
            num = x - off if x < 0 else x + off
            assert R.div_r0(x, y) == int(num / y)                              # truncation towards zero
    assert R.div_r0(8, 16) == 0 and R.div_r0(-8, 16) == 0 and R.div_r0(9, 16) == 1 and R.div_r0(-24, 16) == -1


def test_flat_block_transforms_to_its_dc_alone():
    """What the large DC-walk case of the GPU test relies on: a constant block is DC = value << ln, every AC zero."""
    for ln in (5, 6):
        for v in (-128, -3, 0, 1, 127):
            y = np.array(R.haar([[v] * (1 << ln)] * (1 << ln), ln))
            assert y[0, 0] == v << ln and np.count_nonzero(y) == (v != 0)


def _stats(names):
    for name in names:
        for dec in (0, 1):
            yield name, dec, C.want(name, dec).stats


def test_inputs_reach_rounding_ties_of_each_sign():
    for name, dec, s in _stats(["key-u8-q16", "key-fpr12-q16"]):
        assert s["ties_pos"] >= 50 and s["ties_neg"] >= 50, (name, dec, s)
    tot = [sum(s[k] for _, _, s in _stats(["inter-u8-q16"])) for k in ("ties_pos", "ties_neg")]
    assert min(tot) >= 50, tot


def test_inputs_reach_every_dc_predictor_case_and_a_negative_sum():
    for c in C.CASES:
        if not c.inter and c.nsbx == C.NSBX:
            for _, dec, s in _stats([c.name]):
                assert s["dc_cases"] == {"none", "left", "up", "three", "four"}, (c.name, dec)
                assert s["neg_pred_sum"] >= 1, (c.name, dec)
    assert C.want("key-u8-q16-1x1", 0).stats["dc_cases"] == {"none"}


def test_inputs_put_inter_dcs_on_both_sides_of_the_dead_zone():
    for name, dec, s in _stats(["inter-u8-q16", "inter-u8-q183", "inter-fpr12-q16"]):
        assert s["dead_in"] >= 2 and s["dead_out"] >= 2, (name, dec, s)
    # Cb and Cr differ in their step, and it shows in the symbols
    w = C.want("inter-u8-q16", 1)
    n = 32
    assert not np.array_equal(w.q[:2, ::n, ::n] != 0, w.q[2:, ::n, ::n] != 0)


def test_inputs_reach_empty_and_heavy_trees():
    assert C.want("key-u8-qzero", 0).stats["zero_tree_blocks"] == 2 * C.NSBX * C.NSBY
    assert C.want("key-u8-qzero", 1).stats["zero_tree_blocks"] == 4 * C.NSBX * C.NSBY
    for name in ("key-u8-lossless", "key-u8-q16", "key-fpr12-lossless"):
        assert C.want(name, 0).stats["max_tree"] >= 1 << 15, name


def test_inputs_clamp_reconstructed_samples_at_both_ends():
    for name, dec, s in _stats(["key-u8-q16", "key-u8-q183", "key-fpr12-q16"]):
        assert s["clamp_lo"] >= 1 and s["clamp_hi"] >= 1, (name, dec, s)
    for name in ("inter-fpr12-q16",):                                         # luma and chroma together
        assert all(sum(s[k] for _, _, s in _stats([name])) >= 1 for k in ("clamp_lo", "clamp_hi")), name


def test_tree_sums_of_the_restatement_are_trees():
    w = C.want("key-u8-q16", 1)
    assert C.tree_violations(w.q, w.tree, 5) == 0
    broken = w.tree.copy()
    broken[1, 40, 9] += 1
    assert C.tree_violations(w.q, broken, 5) >= 1
