"""GPU: the motion compensation (mc_kernels.hip) on every kind of leaf and with filter windows exactly on the 64-sample
border, against tests/_mc_ref.py.  All exact.

The recorded grids of tests/golden/mc.npz lack six of the 49 kinds (log size, outside corner, split flags) and their
random vectors hardly ever put a window on the border; the patterns of tests/_mc_patterns.py hold all kinds (asserted in
tests/test_mc_patterns_host.py), and push_to_side gives every leaf along one side of the frame the largest legal
component.  Three slots; about a third of the points share a neighbour's slot and vector, so corners that need one
prediction only (k_mc_predict's `same`) occur in twos and in fours."""
import functools

import numpy as np
import pytest

import _mc_patterns as MP
import _mc_ref as R
from test_gpu_mc import random_planes

pytestmark = pytest.mark.gpu

PATTERNS = MP.patterns()
NAMES = [p[0] for p in PATTERNS]


@pytest.fixture(scope="module")
def D():
    import torch
    import daala_amd
    assert torch.cuda.is_available()
    daala_amd.init(0)
    return daala_amd


def corner_keys(grid, leaf, dec):
    """(slot, vector at the plane's decimation) of the four corners of a leaf: what k_mc_predict compares."""
    vx, vy, lg, oc, s = leaf
    out = []
    for k in range(4):
        dx, dy = R.vertex(oc, s, k)
        pt = grid[vy + (dy << lg), vx + (dx << lg)]
        out.append((int(pt["ref"]), R.scale_mv(int(pt["mvx"]), dec), R.scale_mv(int(pt["mvy"]), dec)))
    return out


def legalise(grid, dec, rng):
    for _ in range(200):
        if R.grid_in_range(grid, dec):
            return grid
        R.shrink_offenders(grid, dec, rng)
    raise AssertionError("no legal grid found")


def shared_grid(valid, rng, dec):
    """_mc_ref.random_grid on three slots; then about a third of the valid points take the slot and vector of the valid
    point to their left (tools/make_golden_mc.py does this with the neighbouring point, which a sparse pattern seldom
    reads), and every fifth leaf gets one slot and vector at all four corners."""
    g = R.random_grid(valid, rng, (dec,), nrefs=3)
    while set(np.unique(g["ref"][valid != 0]).tolist()) != {0, 1, 2}:      # (a pattern of a few points)
        g = R.random_grid(valid, rng, (dec,), nrefs=3)
    for y in range(valid.shape[0]):
        xs = np.flatnonzero(valid[y])
        for a, b in zip(xs[:-1], xs[1:]):
            if rng.rand() < 0.33:
                for name in ("ref", "mvx", "mvy"):
                    g[name][y, b] = g[name][y, a]
    for vx, vy, lg, oc, s in R.leaves(valid)[::5]:
        pts = [(vy + (dy << lg), vx + (dx << lg)) for dx, dy in (R.vertex(oc, s, k) for k in range(4))]
        for pt in pts[1:]:
            for name in ("ref", "mvx", "mvy"):
                g[name][pt] = g[name][pts[0]]
    return legalise(g, dec, rng)


@pytest.mark.parametrize("name,w,h,valid", PATTERNS, ids=NAMES)
def test_leaves_of_every_kind_equal_the_walk(D, name, w, h, valid):
    g = np.zeros(valid.shape, R.MV_POINT)
    g["valid"] = valid
    got = D.mc_leaves(g, w, h)[0]
    want = np.array(sorted(R.leaf_desc(*leaf) for leaf in R.leaves(valid)), np.uint32)
    assert np.array_equal(got, want)


@pytest.mark.parametrize("fpr", [0, 1], ids=["u8", "i16"])
@pytest.mark.parametrize("dec", [0, 1])
@pytest.mark.parametrize("name,w,h,valid", PATTERNS, ids=NAMES)
def test_every_kind_of_leaf_is_predicted(D, name, w, h, valid, dec, fpr):
    import torch
    rng = np.random.RandomState(300 + 4*NAMES.index(name) + 2*fpr + dec)
    grid = shared_grid(valid, rng, dec)
    equal = [max(keys.count(k) for k in keys) for keys in (corner_keys(grid, leaf, dec) for leaf in R.leaves(valid))]
    distinct = [len(set(corner_keys(grid, leaf, dec))) for leaf in R.leaves(valid)]
    assert any(e == 2 and d == 3 for e, d in zip(equal, distinct)), "no leaf with exactly two equal corners"
    assert 4 in equal and 1 in equal
    slots = {k[0] for leaf in R.leaves(valid) for k in corner_keys(grid, leaf, dec)}
    assert len(slots) > 1 and slots <= {0, 1, 2}
    ph, pw = h >> dec, w >> dec
    refs = [random_planes(rng, 1, ph, pw, fpr) for _ in range(3)]
    got = D.mc_predict([torch.from_numpy(r).cuda() for r in refs], grid, dec=dec).cpu().numpy()
    want = R.mc_predict_plane([r[0] for r in refs], grid, dec, fpr)
    assert np.array_equal(got[0], want)


@functools.lru_cache(maxsize=None)
def border_grid(axis, side, dec):
    """(grid, {lg: the points at which a leaf of that size along the side has a window exactly on the border})."""
    rng = np.random.RandomState(500 + 4*axis + 2*side + dec)
    grid = R.random_grid(MP.border_pattern(), rng, (dec,), nrefs=3)
    hits = MP.push_to_side(grid, dec, axis, side)
    return grid, hits


@pytest.mark.parametrize("fpr", [0, 1], ids=["u8", "i16"])
@pytest.mark.parametrize("dec", [0, 1])
@pytest.mark.parametrize("axis,side", [(0, 0), (0, 1), (1, 0), (1, 1)], ids=["left", "right", "top", "bottom"])
def test_windows_on_the_border(D, axis, side, dec, fpr):
    """Where x0 == -pad or x0 + blk + 5 == w + pad the clamps of the LDS stager and od_mc_window_ok have to agree to
    the sample: the outermost window column is then the last one the reference's border holds."""
    import torch
    grid, hits = border_grid(axis, side, dec)
    assert R.grid_in_range(grid, dec)
    assert set(hits) == {0, 1, 2, 3}, hits
    # one step further out, at any of those points, is outside
    name, step = ("mvx", "mvy")[axis], (-1, 1)[side]
    for x, y in {pts[0] for pts in hits.values()}:
        out = grid.copy()
        out[name][y, x] += step
        assert not R.grid_in_range(out, dec), (x, y)
    rng = np.random.RandomState(600 + fpr)
    refs = [random_planes(rng, 1, 128 >> dec, 128 >> dec, fpr) for _ in range(3)]
    got = D.mc_predict([torch.from_numpy(r).cuda() for r in refs], grid, dec=dec).cpu().numpy()
    want = R.mc_predict_plane([r[0] for r in refs], grid, dec, fpr)
    assert np.array_equal(got[0], want)
