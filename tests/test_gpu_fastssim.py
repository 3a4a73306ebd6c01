"""FastSSIM on the device (k_fastssim_pyramid, k_fastssim: fastssim_kernels.hip; k_metric_tile_sum) against the CPU
restatement (tests/_fastssim_ref.py), which reproduces the reference tool's printed lines and return values
(tests/test_fastssim_host.py):

- odhip_fastssim_terms: the term map of every level equals the restatement's as int64 bit patterns - 16x16 (level 3 is
  one sample), 33x31 (every level odd somewhere: the clamps), 70x50 and 130x66 (level 0 crosses tile joints in both
  directions, with a one-sample-wide last tile), samples as uint8, uint16 and 12-bit int16 brought to the depth, at 8,
  10 and 12 bits, strides larger than w with the base off the row start; a 0 / max checkerboard at 12 bits (the largest
  gradients); identical planes (every term exactly 1.0, the score exactly 1); a pair whose muy wraps modulo 2^32 (the
  restatement counts the wrapped samples: the case is void without one);
- odhip_fastssim_planes: each of the four sums has |sum - fsum(terms)| <= N * 2^-53 * sum|term| (N doubles added in
  ANY order, each addition rounding by at most 2^-53 relative of a partial sum that never exceeds sum|term|: N - 1
  roundings - a derivation, not a tuned tolerance); two runs give identical bits; more pairs than one launch group
  takes, of mixed sizes and some sharing their source plane, equal the single-pair calls;
- the device sums through odhip_fastssim_score and the tool's formatting give the golden lines of all clips, dB and
  raw;
- refused arguments launch nothing."""
import ctypes
import math
import os
import sys

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def D():
    import daala_amd
    daala_amd.init(0)
    return daala_amd


def _planes(seed, w, h, depth):
    import _metrics_ref as M
    rng = np.random.RandomState(seed)
    top = (1 << depth) - 1
    src = M._content(("natural", "texture", "noise")[seed % 3], rng, w, h, depth)
    amp = max(2, top // 20)
    rec = np.clip(src + rng.randint(-amp, amp + 1, size=src.shape), 0, top)
    keep = rng.rand(h, w) < 0.2
    rec[keep] = src[keep]
    return src, rec


def _stored(src, rec, depth, fmt, seed=0):
    """(src, rec) as the metric sees them (int32 at the depth) and as stored (arrays in the sample format)."""
    import _metrics_ref as M
    if fmt == "i16":
        # 12-bit planes of arbitrary values, the reconstruction beyond the range: the output conversion rounds and clamps
        rng = np.random.RandomState(seed + 1000)
        sh = 12 - depth
        s12 = (src << sh) + (rng.randint(0, 1 << sh, size=src.shape) if sh else 0) - ((1 << sh) >> 1)
        r12 = np.clip((rec << sh) + rng.randint(-9, 10, size=rec.shape), -40, 4200)
        return M.to_depth(s12, depth), M.to_depth(r12, depth), s12.astype(np.int16), r12.astype(np.int16)
    dt = np.uint8 if fmt == "u8" else np.int16
    return src, rec, src.astype(dt), rec.astype(dt)


def _dev(a, pad):
    """[h][w] -> samples inside a CUDA tensor [h + 1][w + pad] that start `pad - 1` samples into its first row; the
    padding holds values the metric must not read.  Returns (tensor, offset of the first sample, stride)."""
    import torch
    h, w = a.shape
    buf = np.full((h + 1, w + pad), 77, a.dtype)
    flat = buf.reshape(-1)
    off = pad - 1
    for y in range(h):
        flat[off + y * (w + pad):off + y * (w + pad) + w] = a[y]
    return torch.from_numpy(buf).cuda(), off, w + pad


def _item(D, src, rec, depth, fmt, seed=0):
    """A pair on the device and what the metric sees of it."""
    src, rec, ssrc, srec = _stored(src, rec, depth, fmt, seed)
    ts, so, sstride = _dev(ssrc, 3)
    tr, ro, rstride = _dev(srec, 6)
    es = ts.element_size()
    h, w = src.shape
    it = dict(keep=(ts, tr), src=ts.data_ptr() + so * es, rec=tr.data_ptr() + ro * es, sstride=sstride, rstride=rstride,
              w=w, h=h, depth=depth, fmt={"u8": D.SAMPLE_U8, "u16": D.SAMPLE_U16, "i16": D.SAMPLE_I16_12}[fmt])
    return it, src, rec


def _pairs(D, items):
    from daala_amd.api import _MetricsPair
    arr = (_MetricsPair * max(1, len(items)))()
    for i, it in enumerate(items):
        arr[i] = _MetricsPair(it["src"], it["rec"], it["fmt"], it["fmt"], it["sstride"], it["rstride"], it["w"], it["h"],
                              it["depth"], 0)
    return arr


def _terms_call(D, it, level):
    import torch
    import _fastssim_ref as S
    wl, hl = S.level_size(max(it["w"], 16), max(it["h"], 16), min(max(level, 0), 3))
    out = torch.full((hl * wl,), -7.0, dtype=torch.float64, device="cuda")
    pair = _pairs(D, [it])
    rc = D.lib().odhip_fastssim_terms(ctypes.byref(pair[0]), level, ctypes.c_void_p(out.data_ptr()), None)
    torch.cuda.synchronize()
    return rc, out.cpu().numpy().reshape(hl, wl)


def _planes_call(D, items, fill=0.0):
    import torch
    n = len(items)
    out = torch.full((max(1, n), 4), fill, dtype=torch.float64, device="cuda")
    rc = D.lib().odhip_fastssim_planes(_pairs(D, items), n, ctypes.c_void_p(out.data_ptr()), None)
    torch.cuda.synchronize()
    return rc, out.cpu().numpy()[:n]


def _check_terms(D, it, src, rec, depth):
    import _fastssim_ref as S
    want = S.terms(src, rec, depth)
    got = []
    for level in range(4):
        rc, t = _terms_call(D, it, level)
        assert rc == 0
        ref = want[level]
        assert t.shape == ref.shape == S.level_size(it["w"], it["h"], level)[::-1]
        bad = np.argwhere(t.view(np.int64) != ref.view(np.int64))
        assert len(bad) == 0, (level, len(bad), bad[:4], t[tuple(bad[0])], ref[tuple(bad[0])])
        got.append(t)
    return got


TERM_CASES = [
    # w, h, depth, format
    (16, 16, 8, "u8"), (33, 31, 8, "u8"), (33, 31, 10, "i16"), (70, 50, 10, "u16"), (70, 50, 8, "i16"),
    (130, 66, 12, "i16"), (130, 66, 12, "u16"), (130, 66, 8, "u8"),
]


@pytest.mark.parametrize("w,h,depth,fmt", TERM_CASES)
def test_terms_are_bit_exact(D, w, h, depth, fmt):
    src, rec = _planes(w + depth, w, h, depth)
    it, src, rec = _item(D, src, rec, depth, fmt, w)
    _check_terms(D, it, src, rec, depth)


@pytest.mark.parametrize("fmt", ["u16", "i16"])
def test_checkerboard_has_the_largest_gradients(D, fmt):
    import _fastssim_ref as S
    src, rec = S.checkerboard(96, 80, 12)
    assert int(S.gradient(S.pyramid(src)[3]).max()) == 5 * 4095 * 256
    # 12-bit int16 planes hold the samples themselves: stored exactly, no noise below the depth
    it, s, r = _item(D, src, rec, 12, "u16")
    if fmt == "i16":
        it = dict(it, fmt=D.SAMPLE_I16_12)
    _check_terms(D, it, s, r, 12)


def test_identical_planes_give_exactly_one(D):
    import _fastssim_ref as S
    src, _ = _planes(9, 70, 50, 10)
    it, s, r = _item(D, src, src, 10, "u16")
    for t in _check_terms(D, it, s, r, 10):
        assert (t == 1.0).all()
    rc, sums = _planes_call(D, [it])
    assert rc == 0 and list(sums[0]) == [float(a * b) for a, b in (S.level_size(70, 50, l) for l in range(4))]
    assert D.fastssim_score(sums[0], 70, 50, raw=True) == 1.0


@pytest.mark.parametrize("fmt", ["u8", "i16"])
def test_wrapped_muy(D, fmt):
    import _fastssim_ref as S
    src, rec = S.wrap_pair()
    n = S.wrapped(src, rec)
    print("%d of %d level-3 samples have a wrapped muy" % (n, 4 * 3))
    assert n > 0                                        # otherwise the case is void
    it, s, r = _item(D, src, rec, 8, fmt)
    assert S.wrapped(s, r) > 0
    _check_terms(D, it, s, r, 8)
    # the wrap across a tile joint of level 3: 1056 x 64 has 66 columns there, x dark from the middle on
    src, rec = S.wrap_pair(1056, 64)
    assert S.wrapped(src, rec) > 0
    it, s, r = _item(D, src, rec, 8, "u8")
    rc, t = _terms_call(D, it, 3)
    assert rc == 0 and np.array_equal(t.view(np.int64), S.terms(s, r, 8)[3].view(np.int64))


@pytest.fixture(scope="module")
def batch(D):
    """Pairs of different sizes, depths and formats, with the restatement's terms (computed once); the last two share
    the source plane of the first."""
    import _fastssim_ref as S
    shapes = [(70, 50, 10, "u16"), (16, 16, 8, "u8"), (33, 31, 12, "i16"), (130, 66, 8, "u8"), (31, 47, 10, "i16"),
              (64, 48, 8, "i16"), (17, 31, 8, "u8")]
    items, terms = [], []
    for i, (w, h, depth, fmt) in enumerate(shapes):
        src, rec = _planes(40 + i, w, h, depth)
        it, src, rec = _item(D, src, rec, depth, fmt, i)
        items.append(it)
        terms.append(S.terms(src, rec, depth))
        if i == 0:
            first = (it, src)
    for k in (1, 2):
        it0, src = first
        rec = np.clip(src + np.random.RandomState(60 + k).randint(-30 * k, 30 * k + 1, size=src.shape), 0, 1023)
        tr, ro, rstride = _dev(rec.astype(np.int16), 6)
        items.append(dict(it0, rec=tr.data_ptr() + ro * tr.element_size(), rstride=rstride, keep=it0["keep"] + (tr,)))
        terms.append(S.terms(src, rec, 10))
    return items, terms


def test_planes_sums_within_the_bound_of_any_order(D, batch):
    import _fastssim_ref as S
    items, terms = batch
    rc, got = _planes_call(D, items)
    assert rc == 0
    for i, per_level in enumerate(terms):
        for l, t in enumerate(per_level):
            exact = math.fsum(t.ravel().tolist())
            bound = t.size * 2.0 ** -53 * math.fsum(np.abs(t).ravel().tolist())
            print("pair %d level %d: sum %.17g, off the exact sum by %.3g (bound %.3g)"
                  % (i, l, got[i][l], got[i][l] - exact, bound))
            assert abs(got[i][l] - exact) <= bound, (i, l, got[i][l], exact, bound)
    # the Python wrappers and the score
    import torch
    src, rec = _planes(40, 70, 50, 10)
    ts, tr = torch.from_numpy(src.astype(np.int16)).cuda(), torch.from_numpy(rec.astype(np.int16)).cuda()
    sums = D.fastssim_planes(ts[None], tr[None], depth=10)
    assert np.array_equal(sums[0].view(np.int64), got[0].view(np.int64))
    assert 0 < D.fastssim_score(sums[0], 70, 50, raw=True) == S.score(sums[0], 70, 50) < 1
    t = D.fastssim_terms(ts, tr, 1, depth=10)
    assert np.array_equal(t.view(np.int64), terms[0][1].view(np.int64))
    assert not D.fastssim_tool_exact(70, 50) and D.fastssim_tool_exact(31, 47)


def test_planes_repeat_and_batches_equal_single_calls(D, batch):
    items, _ = batch
    rc, a = _planes_call(D, items)
    rc2, b = _planes_call(D, items)
    assert rc == 0 and rc2 == 0
    assert np.array_equal(a.view(np.int64), b.view(np.int64))
    for i, it in enumerate(items):
        rc, one = _planes_call(D, [it])
        assert rc == 0 and np.array_equal(one.view(np.int64)[0], a.view(np.int64)[i]), i
    # more pairs than one launch group takes (32), sizes and shared sources interleaved
    many = [items[i % len(items)] for i in range(40)]
    rc, c = _planes_call(D, many)
    assert rc == 0
    assert np.array_equal(c.view(np.int64), np.stack([a.view(np.int64)[i % len(items)] for i in range(40)]))
    rc, none = _planes_call(D, [])
    assert rc == 0 and none.shape == (0, 4)


@pytest.mark.parametrize("raw", [False, True], ids=["db", "raw"])
def test_device_sums_print_the_golden_lines(D, raw):
    """%-8G keeps six digits; a sum is off the tool's running double by far less."""
    import torch
    import _fastssim_ref as S
    import _metrics_ref as M
    g = np.load(os.path.join(ROOT, "tests", "golden", "fastssim.npz"))
    for idx, case in enumerate(S.CASES):
        name, kind, w, h, c444, depth, nframes, seed = case
        assert str(g["names"][idx]) == name
        src, dst = M.make_case(case)
        dt = np.uint8 if depth == 8 else np.int16
        keep, items = [], []
        for fs, fd in zip(src, dst):
            for a, b in zip(fs, fd):
                assert D.fastssim_tool_exact(a.shape[1], a.shape[0])
                ta, tb = torch.from_numpy(a.astype(dt)).cuda(), torch.from_numpy(b.astype(dt)).cuda()
                keep.append((ta, tb))
                items.append(dict(src=ta.data_ptr(), rec=tb.data_ptr(), sstride=a.shape[1], rstride=a.shape[1],
                                  w=a.shape[1], h=a.shape[0], depth=depth,
                                  fmt=D.SAMPLE_U8 if depth == 8 else D.SAMPLE_U16))
        rc, sums = _planes_call(D, items)
        assert rc == 0
        values = [D.fastssim_score(sums[i], items[i]["w"], items[i]["h"], raw=True) for i in range(len(items))]
        frames = [values[3 * f:3 * f + 3] for f in range(nframes)]
        want = str(g["fastssim_raw" if raw else "fastssim"][idx]).splitlines()
        assert S.tool_lines(frames, c444, raw) == want, name


def test_refused_arguments_launch_nothing(D):
    import torch
    z = torch.zeros((64, 64), dtype=torch.uint8, device="cuda")
    ok = dict(src=z.data_ptr(), rec=z.data_ptr(), sstride=64, rstride=64, w=64, h=64, depth=8, fmt=D.SAMPLE_U8)
    for w, h in ((15, 64), (64, 15)):
        # the refused pair comes last: the pairs before it are not launched either
        rc, out = _planes_call(D, [ok, dict(ok, w=w, h=h)], fill=-7.0)
        assert rc == -10 and (out == -7.0).all()
        rc, t = _terms_call(D, dict(ok, w=w, h=h), 0)
        assert rc == -10 and (t == -7.0).all()
    for bad in (dict(ok, depth=9), dict(ok, depth=10), dict(ok, sstride=63), dict(ok, src=0)):
        rc, out = _planes_call(D, [bad], fill=-7.0)
        assert rc == -10 and (out == -7.0).all()
    for level in (-1, 4):
        rc, t = _terms_call(D, ok, level)
        assert rc == -10 and (t == -7.0).all()
    L = D.lib()
    out = torch.zeros(4, dtype=torch.float64, device="cuda")
    assert L.odhip_fastssim_planes(None, 1, ctypes.c_void_p(out.data_ptr()), None) == -10
    assert L.odhip_fastssim_planes(_pairs(D, [ok]), 1, None, None) == -10
    assert L.odhip_fastssim_planes(_pairs(D, [ok]), -1, ctypes.c_void_p(out.data_ptr()), None) == -10
    # 16 x 16 is taken
    rc, out = _planes_call(D, [dict(ok, w=16, h=16)])
    assert rc == 0 and list(out[0]) == [64.0, 16.0, 4.0, 1.0]                # identical planes: every term is 1
