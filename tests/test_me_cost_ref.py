"""The numpy cost with chroma planes and SATD (tests/_me_cost_ref.py) against the compiled reference's recorded
per-plane distortions (tests/golden/me_cost.npz, tools/make_golden_me_cost.py) and against its own definition.
No GPU."""
import os

import numpy as np
import pytest

import _mc_ref as R
import _me_cost_ref as C
import _me_ref as M

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "me_cost.npz")


def load_golden():
    return C.load_golden(GOLDEN)


def test_golden_covers_what_it_claims():
    g = load_golden()
    assert g["pics"].tolist() == [[120, 104], [119, 103]] and g["ref_y"].shape == (128, 128)
    assert g["ref_cb_420"].shape == (64, 64) and g["src_cr_420"].shape == (52, 60) and g["src_cb_444"].shape == (104, 120)
    cases = g["cases"].tolist()
    for cdec in (0, 1):
        sel = [c for c in cases if c[0] == cdec]
        assert {(c[5] & 7, c[6] & 7) for c in sel} == {(a, b) for a in range(8) for b in range(8)}
        assert {c[4] for c in sel} == {0, 1, 2, 3} and {c[1] for c in sel} == {0, 1}
    # whole blocks of every size, luma clipped to a smaller square of 4, 8, 16 and 32, a non-square clip, an empty
    # one, a whole 4 x 4 chroma block and a chroma clip narrower than 4
    C.assert_classes(C.golden_classes(g))
    clipped = set()
    for cdec, pic, vx, vy, lg, _, _ in cases:
        bx, by, blk = M.block_of(vx, vy, lg)
        c = M.clip_of(bx, by, blk, *g["pics"][pic].tolist())
        clipped.add("empty" if c is None else (c[0] > bx, c[1] < bx + blk, c[2] > by, c[3] < by + blk))
    for want in ("empty", (False, False, False, False), (True, False, False, False), (False, True, False, False),
                 (False, False, True, False), (False, False, False, True), (True, False, True, False),
                 (False, True, True, False), (True, False, False, True), (False, True, False, True)):
        assert want in clipped, want
    # the two metrics differ where a transform applies and agree where od_enc_satd falls back to the SAD
    assert (g["sad"] != g["satd"]).any() and (g["sad"] == g["satd"]).all(axis=1).any()


def test_plane_dist_equals_the_recorded_reference():
    g = load_golden()
    for (cdec, pic, vx, vy, lg, mvx, mvy), sad, satd in zip(g["cases"].tolist(), g["sad"].tolist(), g["satd"].tolist()):
        pw, ph = g["pics"][pic].tolist()
        srcs, refs = C.golden_planes(g, cdec)
        for metric, want in ((C.SAD_METRIC, sad), (C.SATD_METRIC, satd)):
            got = C.cand_dist(srcs, pw, ph, refs, vx, vy, lg, mvx, mvy, cdec, metric)
            assert list(got) == want, (cdec, pic, vx, vy, lg, mvx, mvy, metric, got, want)


def test_halfpel_chroma_vectors_are_the_block_matchers():
    # od_mv_est_bma_sad hands the predictor mv*(1 << (2 - dec)) of its half-pel vector
    for half in range(-70, 71):
        for dec in (0, 1):
            assert R.scale_mv(4*half, dec) == half*(1 << (2 - dec))


def test_satd_is_the_sum_of_absolute_hadamard_coefficients():
    rng = np.random.RandomState(5)
    d = rng.randint(-255, 256, size=(16, 16))
    assert C.satd_of(np.zeros((8, 8), int)) == 0
    one = np.zeros((8, 8), int)
    one[3, 5] = 7                                   # every coefficient of an impulse is +-7
    assert C.satd_of(one) == (64*7 + 4) >> 3
    assert C.satd_of(one[:4, 4:8]) == (16*7 + 2) >> 2
    assert C.satd_of(d) == sum(C.satd_of(d[y:y + 8, x:x + 8]) for y in (0, 8) for x in (0, 8))
    assert C.satd_of(d[:8, :12]) == np.abs(d[:8, :12]).sum() and C.satd_of(d[:2, :2]) == np.abs(d[:2, :2]).sum()


@pytest.mark.parametrize("cdec", [0, 1])
def test_fullpel_chroma_table_is_plane_dist(cdec):
    g = load_golden()
    srcs, refs = C.golden_planes(g, cdec)
    for vx, vy, lg in ((0, 0, 1), (15, 13, 0), (8, 8, 3), (12, 12, 2), (16, 16, 1), (14, 0, 0)):
        for pw, ph in g["pics"].tolist():
            table = C.fullpel_chroma_sads(srcs[1], pw, ph, refs[1], vx, vy, lg, 3, cdec)
            for dy in range(-3, 4):
                for dx in range(-3, 4):
                    assert table[dy + 3, dx + 3] == C.plane_dist(srcs[1], pw, ph, refs[1], vx, vy, lg, 8*dx, 8*dy, cdec,
                                                                 C.SAD_METRIC), (vx, vy, lg, dx, dy)


def test_search_without_flags_is_the_luma_search():
    g = load_golden()
    srcs, refs = C.golden_planes(g, 1)
    src, csrc = srcs[0][None], np.stack(srcs[1:])
    ref, cref = refs[0][None], np.stack(refs[1:])
    for lg, rng_, res, lam in ((1, 2, 0, 3), (3, 1, 3, 0)):
        want = M.search(src, 120, 104, [ref], lg, rng_, res, lam)
        got = C.search(src, csrc, 120, 104, [ref], [cref], lg, rng_, res, lam, lam, 0, 1)
        assert np.array_equal(got[0], want[0]) and np.array_equal(got[1], want[1])
    # the sub-pel stage has its own lambda and the reported cost is its cost
    a = C.search(src, csrc, 120, 104, [ref], [cref], 2, 2, 0, 3, 0, 0, 1)
    for vy in range(0, 17, 4):
        for vx in range(0, 17, 4):
            p = a[0][0, vy, vx]
            assert a[1][0, vy, vx] == 8*M.bma_sad(src[0], 120, 104, ref[0], vx, vy, 2, int(p["mvx"]), int(p["mvy"]))
