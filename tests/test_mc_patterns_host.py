"""CPU: the `valid` patterns of tests/_mc_patterns.py keep the reference's rule for its grid, as the recorded grids of
tests/golden/mc.npz do, and together hold every kind of leaf; and odhip_mc_check_grid (host code) agrees with the numpy
rule to the eighth-pel where a filter window sits exactly on the 64-sample border."""
import os

import numpy as np

import _mc_patterns as MP
import _mc_ref as R
from _libs import GOLDEN

CASES = R.load_cases(os.path.join(GOLDEN, "mc.npz"))


def test_fixture_patterns_keep_the_rule():
    assert len(CASES) == 11
    for c in CASES:
        valid = c["grid"]["valid"]
        assert MP.rule_violations(valid) == [], c["name"]
        assert MP.unread_points(valid) == [], c["name"]


def test_generated_patterns_keep_the_rule():
    made = [(name, v) for name, _, _, v in MP.patterns()] + [("border", MP.border_pattern())]
    made += [("uniform%d" % lg, MP.uniform_pattern(128, 64, lg)) for lg in range(4)]
    for name, valid in made:
        assert MP.rule_violations(valid) == [], name
        assert MP.unread_points(valid) == [], name
    # the checker is not blind: a centre without a corner, a midpoint beside an unsplit cell, a missing multiple of 8
    v = MP.uniform_pattern(128, 64, 3)
    for (y, x), rule in (((0, 4), "C"), ((4, 0), "C"), ((2, 2), "B"), ((8, 8), "A")):
        w = v.copy()
        w[y, x] ^= 1
        assert [b[0] for b in MP.rule_violations(w)] == [rule], (x, y)
    # uniform patterns are what the name says
    for lg in range(4):
        assert MP.kinds(MP.uniform_pattern(128, 64, lg)) <= {(lg, oc, 3) for oc in range(4)}


def test_every_kind_of_leaf_occurs():
    """All 49 kinds (lg, oc, s) - 48 below 64 x 64 and (3, 0, 3) - occur in a pattern of coded size 128 x 128 or
    192 x 128; none is excluded."""
    where = {}
    for name, w, h, valid in MP.patterns():
        assert (w, h) in ((128, 128), (192, 128)) and valid.shape == (h//8 + 1, w//8 + 1)
        for k in MP.kinds(valid):
            where.setdefault(k, []).append(name)
    assert len(MP.ALL_KINDS) == 49
    assert set(where) == MP.ALL_KINDS, sorted(MP.ALL_KINDS - set(where))
    # the kinds no recorded grid holds, by name
    fixtures = set()
    for c in CASES:
        fixtures |= MP.kinds(c["grid"]["valid"])
    assert MP.ALL_KINDS - fixtures == {(1, 1, 1), (2, 0, 1), (2, 0, 3), (2, 1, 3), (2, 2, 3), (2, 3, 3)}
    # the patterns are deterministic
    for (_, _, _, a), (_, _, _, b) in zip(MP.patterns(), MP.patterns()):
        assert a.tobytes() == b.tobytes()


def test_border_pattern_has_every_size_along_every_side():
    sizes = MP.side_sizes(MP.border_pattern())
    assert all(sizes[axis, side] == {0, 1, 2, 3} for axis in (0, 1) for side in (0, 1)), sizes


def test_check_grid_boundary():
    """A uniform grid of every leaf size on a 128 x 128 frame; the points of the frame's first and last line of an axis,
    which only the leaves of the first / last cell read, pushed to either side.  At the largest legal component the
    window is exactly on the border and the grid passes; one step further it is ODHIP_ERANGE; _mc_ref.grid_in_range
    says the same."""
    from daala_amd import api, build
    build.build()
    w = h = 128
    n = w >> 3
    for lg in range(4):
        valid = MP.uniform_pattern(w, h, lg)
        assert MP.kinds(valid) <= {(lg, oc, 3) for oc in range(4)}
        for dec in (0, 1):
            pad, blk = R.BORDER >> dec, 8 << lg >> dec
            for axis, name in ((0, "mvx"), (1, "mvy")):
                for cell in (0, 1):                  # the leaf in the frame's first / last cell of the axis
                    v = 0 if cell == 0 else n - (1 << lg)
                    at = 0 if cell == 0 else n       # its corner that no leaf nearer to the side reads
                    for side in (0, 1):
                        mv = MP.axis_extreme(v, lg, dec, n, side)
                        x0 = MP.window_start(v, mv, dec)
                        assert x0 == -pad if side == 0 else x0 + blk + 5 == (n << 3 >> dec) + pad
                        step = -1 if side == 0 else 1
                        assert (R.scale_mv(mv + step, dec) >> 3) - (R.scale_mv(mv, dec) >> 3) == step
                        for other in (0, n - (1 << lg), n):         # where along the side
                            g = np.zeros(valid.shape, R.MV_POINT)
                            g["valid"] = valid
                            pt = (other, at) if axis == 0 else (at, other)
                            what = (lg, dec, axis, cell, side, other)
                            g[name][pt] = mv
                            assert R.grid_in_range(g, dec), what
                            assert api.mc_check_grid(g, w, h, dec, 1) == 0, what
                            g[name][pt] = mv + step
                            assert not R.grid_in_range(g, dec), what
                            assert api.mc_check_grid(g, w, h, dec, 1) == api.ERANGE, what
