"""MS-SSIM on the device (k_msssim_pyramid, k_msssim: msssim_kernels.hip; k_metric_tile_sum) against the CPU restatement
(tests/_msssim_ref.py), which reproduces the reference tool's printed lines (tests/test_msssim_host.py):

- odhip_msssim_terms: both term maps of all five scales equal the restatement's as int64 bit patterns - 16x16 (scale 4
  is one sample), 77x53, 45x39 at 10 bits, 49x35 at 12 bits, and sizes that straddle one, two and three tiles in each
  direction at scale 0 (33, 65) and at scale 1 (130x70); samples as uint8, uint16 and 12-bit int16 brought to the
  depth; strides larger than w with the base off the row start.  A bright 10-bit plane has a scale-4 moment above 2^53,
  which reaches the term through the rounding int64 -> double conversion (asserted);
- odhip_msssim_planes: each of the five sums has |sum - fsum(terms)| <= N * 2^-53 * sum|term| (N doubles added in ANY
  order, each addition rounding by at most 2^-53 relative of a partial sum that never exceeds sum|term|: N - 1
  roundings - a derivation, not a tuned tolerance); two runs give identical bits; more pairs than one launch group
  takes, of mixed sizes and some sharing their source plane, equal the single-pair calls;
- the device sums through odhip_msssim_score and the tool's formatting give the golden lines of all nine clips, dB and
  raw;
- planes below 16 in either direction are refused before any launch."""
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


def _planes(seed, w, h, depth, fmt, bright=False):
    """(src, rec) as the metric sees them (int32 at the depth) and as stored (arrays in the sample format)."""
    import _metrics_ref as M
    rng = np.random.RandomState(seed)
    kind = ("natural", "texture", "noise")[seed % 3]
    top = (1 << depth) - 1
    src = M._content(kind, rng, w, h, depth)
    if bright:
        src = top - src // 16
    amp = max(2, top // 20)
    rec = np.clip(src + rng.randint(-amp, amp + 1, size=src.shape), 0, top)
    keep = rng.rand(h, w) < 0.2
    rec[keep] = src[keep]
    if fmt == "i16":
        # 12-bit planes of arbitrary values, the reconstruction beyond the range: the output conversion rounds and clamps
        sh = 12 - depth
        s12 = (src << sh) + (rng.randint(0, 1 << sh, size=src.shape) if sh else 0) - ((1 << sh) >> 1)
        r12 = np.clip((rec << sh) + rng.randint(-9, 10, size=rec.shape), -40, 4200)
        return M.to_depth(s12, depth), M.to_depth(r12, depth), s12.astype(np.int16), r12.astype(np.int16)
    dt = np.uint8 if fmt == "u8" else np.int16
    return src, rec, src.astype(dt), rec.astype(dt)


def _dev(a, pad):
    """[h][w] -> a view [h][w] of a CUDA tensor [h + 1][w + pad] that starts `pad - 1` samples into its first row; the
    padding holds values the metric must not read.  Returns (tensor, offset of the first sample, stride)."""
    import torch
    h, w = a.shape
    buf = np.full((h + 1, w + pad), 77, a.dtype)
    flat = buf.reshape(-1)
    off = pad - 1
    for y in range(h):
        flat[off + y * (w + pad):off + y * (w + pad) + w] = a[y]
    t = torch.from_numpy(buf).cuda()
    return t, off, w + pad


def _fmt(D, name):
    return {"u8": D.SAMPLE_U8, "u16": D.SAMPLE_U16, "i16": D.SAMPLE_I16_12}[name]


def _item(D, seed, w, h, depth, fmt, bright=False):
    """A pair on the device: (keep-alive tensors, src pointer, rec pointer, strides, w, h, depth, format) and what the
    metric sees."""
    src, rec, ssrc, srec = _planes(seed, w, h, depth, fmt, bright)
    ts, so, sstride = _dev(ssrc, 3)
    tr, ro, rstride = _dev(srec, 6)
    es = ts.element_size()
    it = dict(keep=(ts, tr), src=ts.data_ptr() + so * es, rec=tr.data_ptr() + ro * es, sstride=sstride, rstride=rstride,
              w=w, h=h, depth=depth, fmt=_fmt(D, fmt))
    return it, src, rec


def _pairs(D, items):
    from daala_amd.api import _MetricsPair
    arr = (_MetricsPair * max(1, len(items)))()
    for i, it in enumerate(items):
        arr[i] = _MetricsPair(it["src"], it["rec"], it["fmt"], it["fmt"], it["sstride"], it["rstride"], it["w"], it["h"],
                              it["depth"], 0)
    return arr


def _terms_call(D, it, scale):
    import torch
    ws, hs = it["w"] >> scale, it["h"] >> scale
    cs = torch.full((hs * ws,), -7.0, dtype=torch.float64, device="cuda")
    ss = torch.full((hs * ws,), -7.0, dtype=torch.float64, device="cuda")
    pair = _pairs(D, [it])
    rc = D.lib().odhip_msssim_terms(ctypes.byref(pair[0]), scale, ctypes.c_void_p(cs.data_ptr()),
                                    ctypes.c_void_p(ss.data_ptr()), None)
    torch.cuda.synchronize()
    return rc, cs.cpu().numpy().reshape(hs, ws), ss.cpu().numpy().reshape(hs, ws)


def _planes_call(D, items, fill=0.0):
    import torch
    n = len(items)
    out = torch.full((max(1, n), 5), fill, dtype=torch.float64, device="cuda")
    wt = (ctypes.c_int64 * (5 * max(1, n)))()
    rc = D.lib().odhip_msssim_planes(_pairs(D, items), n, ctypes.c_void_p(out.data_ptr()), wt, None)
    torch.cuda.synchronize()
    return rc, out.cpu().numpy()[:n], np.array(wt[:5 * n], np.int64).reshape(n, 5)


TERM_CASES = [
    # w, h, depth, format, bright
    (16, 16, 8, "u8", False), (77, 53, 8, "u8", False), (77, 53, 8, "i16", False), (45, 39, 10, "u16", False),
    (45, 39, 10, "i16", False), (49, 35, 12, "i16", False), (49, 35, 12, "u16", False), (65, 33, 10, "u16", True),
    (33, 65, 8, "u8", False), (130, 70, 8, "u8", False),
]


@pytest.mark.parametrize("w,h,depth,fmt,bright", TERM_CASES)
def test_terms_are_bit_exact(D, w, h, depth, fmt, bright):
    import _msssim_ref as S
    it, src, rec = _item(D, w + depth, w, h, depth, fmt, bright)
    want = S.terms(src, rec, depth)
    if bright:
        # a moment above 2^53: it is not a double, the conversion rounds
        top = max(int(np.abs(m).max()) for m in S.moments(S.pyramid(src)[4], S.pyramid(rec)[4])[:5])
        print("largest scale-4 moment 2^%.2f" % math.log2(top))
        assert top > 1 << 53
    for scale in range(5):
        rc, cs, ss = _terms_call(D, it, scale)
        assert rc == 0
        for name, got, ref in (("cs", cs, want[scale][0]), ("ssim", ss, want[scale][1])):
            assert got.shape == ref.shape == (h >> scale, w >> scale)
            bad = np.argwhere(got.view(np.int64) != ref.view(np.int64))
            assert len(bad) == 0, (scale, name, len(bad), bad[:4], got[tuple(bad[0])], ref[tuple(bad[0])])


@pytest.fixture(scope="module")
def batch(D):
    """Pairs of different sizes, depths and formats, with the restatement's summed terms (computed once); the last two
    share the source plane of the first."""
    import _msssim_ref as S
    shapes = [(77, 53, 10, "u16"), (16, 16, 8, "u8"), (49, 35, 12, "i16"), (130, 70, 8, "u8"), (33, 65, 10, "i16"),
              (64, 48, 8, "i16"), (17, 31, 8, "u8")]
    items, terms = [], []
    for i, (w, h, depth, fmt) in enumerate(shapes):
        it, src, rec = _item(D, 40 + i, w, h, depth, fmt)
        items.append(it)
        t = S.terms(src, rec, depth)
        terms.append([t[sc][0 if sc < 4 else 1] for sc in range(5)])
        if i == 0:
            first = (it, src)
    for k in (1, 2):
        it0, src = first
        rec = np.clip(src + np.random.RandomState(60 + k).randint(-30 * k, 30 * k + 1, size=src.shape), 0, 1023)
        tr, ro, rstride = _dev(rec.astype(np.int16), 6)
        it = dict(it0, rec=tr.data_ptr() + ro * tr.element_size(), rstride=rstride, keep=it0["keep"] + (tr,))
        items.append(it)
        t = S.terms(src, rec, 10)
        terms.append([t[sc][0 if sc < 4 else 1] for sc in range(5)])
    return items, terms


def test_planes_sums_within_the_bound_of_any_order(D, batch):
    import _msssim_ref as S
    items, terms = batch
    rc, got, wt = _planes_call(D, items)
    assert rc == 0
    for i, per_scale in enumerate(terms):
        assert list(wt[i]) == S.weights(items[i]["w"], items[i]["h"])
        for sc, t in enumerate(per_scale):
            exact = math.fsum(t.ravel().tolist())
            bound = t.size * 2.0 ** -53 * math.fsum(np.abs(t).ravel().tolist())
            print("pair %d scale %d: sum %.17g, off the exact sum by %.3g (bound %.3g)"
                  % (i, sc, got[i][sc], got[i][sc] - exact, bound))
            assert abs(got[i][sc] - exact) <= bound, (i, sc, got[i][sc], exact, bound)
            assert 0 < got[i][sc] / wt[i][sc] <= 1
    # the Python wrapper and its score
    import torch
    src, rec, ssrc, srec = _planes(40, 77, 53, 10, "u16")
    sums, weights = D.msssim_planes(torch.from_numpy(ssrc).cuda()[None], torch.from_numpy(srec).cuda()[None], depth=10)
    assert np.array_equal(sums[0].view(np.int64), got[0].view(np.int64)) and list(weights[0]) == S.weights(77, 53)
    assert D.msssim_score(sums[0], weights[0], raw=True) == S.score(sums[0], weights[0]) > 0
    cs, ss = D.msssim_terms(torch.from_numpy(ssrc).cuda(), torch.from_numpy(srec).cuda(), 1, depth=10)
    assert np.array_equal(cs.view(np.int64), S.terms(src, rec, 10)[1][0].view(np.int64)) and ss.shape == cs.shape


def test_planes_repeat_and_batches_equal_single_calls(D, batch):
    items, _ = batch
    rc, a, _ = _planes_call(D, items)
    rc2, b, _ = _planes_call(D, items)
    assert rc == 0 and rc2 == 0
    assert np.array_equal(a.view(np.int64), b.view(np.int64))
    for i, it in enumerate(items):
        rc, one, _ = _planes_call(D, [it])
        assert rc == 0 and np.array_equal(one.view(np.int64)[0], a.view(np.int64)[i]), i
    # more pairs than one launch group takes (32), sizes and shared sources interleaved
    many = [items[i % len(items)] for i in range(40)]
    rc, c, _ = _planes_call(D, many)
    assert rc == 0
    assert np.array_equal(c.view(np.int64), np.stack([a.view(np.int64)[i % len(items)] for i in range(40)]))
    rc, none, _ = _planes_call(D, [])
    assert rc == 0 and none.shape == (0, 5)


@pytest.mark.parametrize("raw", [False, True], ids=["db", "raw"])
def test_device_sums_print_the_golden_lines(D, raw):
    """%-8G keeps six digits; a sum is off the tool's running double by far less."""
    import torch
    import _metrics_ref as M
    import _msssim_ref as S
    g = np.load(os.path.join(ROOT, "tests", "golden", "msssim.npz"))
    for idx, case in enumerate(S.CASES):
        name, kind, w, h, c444, depth, nframes, seed = case
        assert str(g["names"][idx]) == name
        src, dst = M.make_case(case)
        dt = np.uint8 if depth == 8 else np.int16
        keep, items = [], []
        for fs, fd in zip(src, dst):
            for a, b in zip(fs, fd):
                ta, tb = torch.from_numpy(a.astype(dt)).cuda(), torch.from_numpy(b.astype(dt)).cuda()
                keep.append((ta, tb))
                items.append(dict(src=ta.data_ptr(), rec=tb.data_ptr(), sstride=a.shape[1], rstride=a.shape[1],
                                  w=a.shape[1], h=a.shape[0], depth=depth,
                                  fmt=D.SAMPLE_U8 if depth == 8 else D.SAMPLE_U16))
        rc, sums, wt = _planes_call(D, items)
        assert rc == 0
        values = [D.msssim_score(sums[i], wt[i], raw=True) for i in range(len(items))]
        frames = [values[3 * f:3 * f + 3] for f in range(nframes)]
        want = str(g["msssim_raw" if raw else "msssim"][idx]).splitlines()
        assert S.tool_lines(frames, c444, raw) == want, name


def test_small_planes_are_refused_before_any_launch(D):
    import torch
    z = torch.zeros((64, 64), dtype=torch.uint8, device="cuda")
    ok = dict(src=z.data_ptr(), rec=z.data_ptr(), sstride=64, rstride=64, w=64, h=64, depth=8, fmt=D.SAMPLE_U8)
    for w, h in ((15, 64), (64, 15)):
        # the refused pair comes last: the pairs before it are not launched either
        rc, out, _ = _planes_call(D, [ok, dict(ok, w=w, h=h)], fill=-7.0)
        assert rc == -10 and (out == -7.0).all()
        rc, cs, ss = _terms_call(D, dict(ok, w=w, h=h), 0)
        assert rc == -10 and (cs == -7.0).all() and (ss == -7.0).all()
    rc, out, _ = _planes_call(D, [dict(ok, depth=9)], fill=-7.0)
    assert rc == -10 and (out == -7.0).all()
    rc, cs, _ = _terms_call(D, ok, 5)
    assert rc == -10 and (cs == -7.0).all()
    L = D.lib()
    out = torch.zeros(5, dtype=torch.float64, device="cuda")
    assert L.odhip_msssim_planes(None, 1, ctypes.c_void_p(out.data_ptr()), None, None) == -10
    assert L.odhip_msssim_planes(_pairs(D, [ok]), 1, None, None, None) == -10
    assert L.odhip_msssim_planes(_pairs(D, [ok]), -1, ctypes.c_void_p(out.data_ptr()), None, None) == -10
    # 16 x 16 is taken
    rc, out, wt = _planes_call(D, [dict(ok, w=16, h=16)])
    assert rc == 0 and np.allclose(out[0], wt[0], rtol=1e-12, atol=0)          # identical planes: every term is its weight
