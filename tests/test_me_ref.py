"""The numpy motion search (tests/_me_ref.py) against the compiled reference's recorded costs
(tests/golden/me.npz, tools/make_golden_me.py) and against its own definition.  No GPU."""
import os

import numpy as np
import pytest

import _mc_ref as R
import _me_ref as M

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "me.npz")


def load_golden():
    z = np.load(GOLDEN)
    b = int(z["border"])
    bordered = z["bordered"]
    plane = np.ascontiguousarray(bordered[b:-b, b:-b])
    return dict(src=z["src"], plane=plane, bordered=bordered, border=b, pic_w=int(z["pic"][0]), pic_h=int(z["pic"][1]),
                cases=z["cases"].tolist(), sad=z["sad"].tolist())


def test_golden_covers_what_it_claims():
    g = load_golden()
    assert np.array_equal(np.pad(g["plane"], g["border"], mode="edge"), g["bordered"])
    assert {(c[3] & 7, c[4] & 7) for c in g["cases"]} == {(a, b) for a in range(8) for b in range(8)}
    assert {c[2] for c in g["cases"]} == {0, 1, 2, 3}
    nh, nv = g["plane"].shape[1] >> 3, g["plane"].shape[0] >> 3
    clipped = set()
    for vx, vy, lg, _, _ in g["cases"]:
        bx, by, blk = M.block_of(vx, vy, lg)
        c = M.clip_of(bx, by, blk, g["pic_w"], g["pic_h"])
        clipped.add("empty" if c is None else (c[0] > bx, c[1] < bx + blk, c[2] > by, c[3] < by + blk))
        assert 0 <= vx <= nh and 0 <= vy <= nv
    # whole blocks, nothing left, each edge alone and each corner
    for want in ("empty", (False, False, False, False), (True, False, False, False), (False, True, False, False),
                 (False, False, True, False), (False, False, False, True), (True, False, True, False),
                 (False, True, True, False), (True, False, False, True), (False, True, False, True)):
        assert want in clipped, want


def test_bma_sad_equals_the_recorded_reference():
    g = load_golden()
    for (vx, vy, lg, mvx, mvy), want in zip(g["cases"], g["sad"]):
        got = M.bma_sad(g["src"], g["pic_w"], g["pic_h"], g["plane"], vx, vy, lg, mvx, mvy)
        assert got == want, (vx, vy, lg, mvx, mvy, got, want)


def test_fullpel_table_is_bma_sad():
    g = load_golden()
    for vx, vy, lg in ((0, 0, 1), (15, 13, 0), (8, 8, 3), (12, 12, 2), (16, 16, 1)):
        table = M.fullpel_sads(g["src"], g["pic_w"], g["pic_h"], g["plane"], vx, vy, lg, 3)
        for dy in range(-3, 4):
            for dx in range(-3, 4):
                assert table[dy + 3, dx + 3] == M.bma_sad(g["src"], g["pic_w"], g["pic_h"], g["plane"], vx, vy, lg,
                                                          8*dx, 8*dy)


def test_legality_is_grid_in_range_of_the_uniform_grid():
    # a uniform grid with one point moved: in range exactly when the predicate says so
    for lg in range(4):
        for vx, vy in ((0, 0), (16, 8), (8, 8), (16, 0)):
            if vx % (1 << lg) or vy % (1 << lg):
                continue
            for mvx, mvy in ((0, 0), (-8*70, 0), (8*62, 8*62), (-8*62 - 1, 3), (8*61 + 7, -8*62), (499, -497), (0, 8*63)):
                grid = np.zeros((9, 17), R.MV_POINT)
                grid["valid"][::1 << lg, ::1 << lg] = 1
                grid[vy, vx]["mvx"], grid[vy, vx]["mvy"] = mvx, mvy
                want = R.grid_in_range(grid, 0) and R.grid_in_range(grid, 1)
                assert M.legal(128, 64, vx, vy, lg, mvx, mvy) == want, (lg, vx, vy, mvx, mvy)
            lim = M.limits(128, 64, lg, vx, vy)
            assert lim[0] <= 0 <= lim[1] and lim[2] <= 0 <= lim[3]
            assert not M.mv_ok(vx, 8*(lim[0] - 1), lg, 16) and not M.mv_ok(vy, 8*(lim[3] + 1), lg, 8)


@pytest.mark.parametrize("lg, shift", [(0, (19, -3)), (1, (-13, 22)), (2, (8, -16)), (3, (5, 7))])
def test_search_finds_a_planted_shift(lg, shift):
    rng = np.random.RandomState(40 + lg)
    ref = M.smooth_noise(rng, 128, 128)
    src = M.displaced(ref, *shift)
    grid, cost = M.search(src[None], 128, 128, [ref[None]], lg, 3, 0, 0)
    g, c = grid[0], cost[0]
    s = 1 << lg
    assert np.all(g["valid"][::s, ::s] == 1)
    # interior points: the planted vector is legal there and within the range
    inner = g[s:-s:s, s:-s:s] if lg < 3 else g[8:9, 8:9]
    assert inner.size and np.all(inner["mvx"] == shift[0]) and np.all(inner["mvy"] == shift[1])
    assert np.all((c[s:-s:s, s:-s:s] if lg < 3 else c[8:9, 8:9]) == 0)
    assert R.grid_in_range(g, 0) and R.grid_in_range(g, 1)


@pytest.mark.parametrize("lg, rng_, res", [(0, 2, 0), (1, 7, 1), (2, 32, 0), (3, 32, 2)])
def test_every_searched_grid_is_in_range(lg, rng_, res):
    rs = np.random.RandomState(60 + lg)
    w, h = (128, 64) if lg < 2 else (128, 128)
    big = M.smooth_noise(rs, h + 160, w + 160)
    # references far from the source in opposite directions: the best matches lie outside the frame
    src = big[80:80 + h, 80:80 + w]
    refs = [np.ascontiguousarray(big[80 - 70:80 - 70 + h, 80 + 75:80 + 75 + w])[None],
            np.ascontiguousarray(big[80 + 66:80 + 66 + h, 80 - 72:80 - 72 + w])[None]]
    grid, cost = M.search(src[None], w - 8, h - 8, refs, lg, rng_, res, 1)
    assert R.grid_in_range(grid[0], 0) and R.grid_in_range(grid[0], 1)
    s = 1 << lg
    assert [leaf[2] for leaf in R.leaves(grid[0]["valid"])] == [lg]*((w >> 3)*(h >> 3) >> 2*lg)
    mask = np.ones(grid[0].shape, bool)
    mask[::s, ::s] = False
    assert not grid[0][mask].tobytes().strip(b"\0") and not cost[0][mask].any()
