"""SSIM on the device (k_ssim, metrics_kernels.hip) against the CPU restatement (tests/_ssim_ref.py), which reproduces the
reference tool's printed lines (tests/test_ssim_host.py):

- odhip_ssim_terms: every sample's term equals the restatement's as an int64 bit pattern - the tall, narrow golden
  shapes (radius 9 / 7 capped / 4 / 3 capped, both truncations at once) and a 77x53 plane, depths 8 / 10 / 12, samples
  as uint8, uint16 and 12-bit int16 brought to the depth, odd strides, par 1 and 4/3;
- odhip_ssim_planes: |sum - fsum(terms)| <= N * 2^-53 * sum|term| (N doubles added in ANY order, each addition rounding
  by at most 2^-53 relative of a partial sum that never exceeds sum|term|: N - 1 roundings - a derivation, not a tuned
  tolerance); two runs give identical bits; pairs of different sizes in one call equal the single-pair calls, also
  with more pairs than one launch takes;
- a radius above ODHIP_SSIM_MAX_RADIUS: ODHIP_EIMPL and nothing launched."""
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


def _planes(seed, w, h, depth, fmt):
    """(src, rec) as the metric sees them (int32 at the depth) and as stored (arrays in the sample format)."""
    import _metrics_ref as M
    rng = np.random.RandomState(seed)
    kind = ("natural", "texture", "noise")[seed % 3]
    top = (1 << depth) - 1
    src = M._content(kind, rng, w, h, depth)
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
    """[h][w] -> a CUDA tensor [h][w + pad], the padding filled with values the metric must not read."""
    import torch
    h, w = a.shape
    buf = np.full((h, w + pad), 77, a.dtype)
    buf[:, :w] = a
    return torch.from_numpy(buf).cuda()


def _fmt(D, name):
    return {"u8": D.SAMPLE_U8, "u16": D.SAMPLE_U16, "i16": D.SAMPLE_I16_12}[name]


def _odd(w, k):
    """a padding that makes the stride odd"""
    return k + ((w + k + 1) & 1)


TERM_CASES = [
    # w, h, depth, format, par
    (24, 544, 8, "u8", 1.0), (24, 544, 8, "i16", 4 / 3), (12, 272, 8, "u8", 1.0),
    (8, 544, 8, "u8", 1.0), (8, 544, 8, "u8", 4 / 3), (4, 272, 8, "i16", 1.0),
    (40, 256, 10, "u16", 1.0), (40, 256, 10, "i16", 4 / 3), (40, 256, 12, "u16", 1.0),
    (77, 53, 8, "u8", 1.0), (77, 53, 8, "i16", 4 / 3), (77, 53, 10, "u16", 4 / 3), (77, 53, 10, "i16", 1.0),
    (77, 53, 12, "u16", 1.0), (77, 53, 12, "i16", 4 / 3), (24, 544, 12, "i16", 1.0),
]


@pytest.mark.parametrize("w,h,depth,fmt,par", TERM_CASES)
def test_terms_are_bit_exact(D, w, h, depth, fmt, par):
    import _ssim_ref as S
    src, rec, ssrc, srec = _planes(w + depth, w, h, depth, fmt)
    f = _fmt(D, fmt)
    got = D.ssim_terms(_dev(ssrc, _odd(w, 1)), _dev(srec, _odd(w, 3)), w, h, depth, par, src_fmt=f, rec_fmt=f)
    want = S.terms(src, rec, depth, par)
    assert got.shape == want.shape == (h, w)
    bad = np.argwhere(got.view(np.int64) != want.view(np.int64))
    assert len(bad) == 0, (len(bad), bad[:4], got[tuple(bad[0])], want[tuple(bad[0])])


def _pairs(D, items):
    """items: [(src tensor, rec tensor, w, h, depth, fmt)] -> a ctypes array of odhip_metrics_pair."""
    from daala_amd.api import _MetricsPair
    arr = (_MetricsPair * len(items))()
    for i, (s, r, w, h, depth, f) in enumerate(items):
        arr[i] = _MetricsPair(s.data_ptr(), r.data_ptr(), f, f, s.shape[1], r.shape[1], w, h, depth, 0)
    return arr


def _planes_call(D, items, par=1.0, fill=0.0):
    import torch
    n = len(items)
    out = torch.full((n,), fill, dtype=torch.float64, device="cuda")
    wt = (ctypes.c_int64 * n)()
    rc = D.lib().odhip_ssim_planes(_pairs(D, items), n, ctypes.c_double(par), ctypes.c_void_p(out.data_ptr()), wt, None)
    torch.cuda.synchronize()
    return rc, out.cpu().numpy(), list(wt)


@pytest.fixture(scope="module")
def batch(D):
    """Pairs of different sizes, depths and formats, with the restatement's terms (computed once)."""
    import _ssim_ref as S
    shapes = [(24, 544, 8, "u8"), (77, 53, 10, "u16"), (40, 256, 12, "i16"), (8, 544, 8, "i16"), (130, 70, 8, "u8"),
              (33, 33, 10, "i16"), (4, 272, 8, "u8")]
    items, terms = [], []
    for i, (w, h, depth, fmt) in enumerate(shapes):
        src, rec, ssrc, srec = _planes(40 + i, w, h, depth, fmt)
        items.append((_dev(ssrc, _odd(w, 1)), _dev(srec, _odd(w, 3)), w, h, depth, _fmt(D, fmt)))
        terms.append(S.terms(src, rec, depth))
    return items, terms


def test_planes_sum_within_the_bound_of_any_order(D, batch):
    import _ssim_ref as S
    items, terms = batch
    rc, got, wt = _planes_call(D, items)
    assert rc == 0
    for i, t in enumerate(terms):
        exact = math.fsum(t.ravel().tolist())
        bound = t.size * 2.0 ** -53 * math.fsum(np.abs(t).ravel().tolist())
        print("pair %d: sum %.17g, off the exact sum by %.3g (bound %.3g)" % (i, got[i], got[i] - exact, bound))
        assert abs(got[i] - exact) <= bound, (i, got[i], exact, bound)
        assert wt[i] == S.weight(items[i][2], items[i][3])
        assert 0 < got[i] / wt[i] <= 1
    # the Python wrapper, and its scores
    s, r, w, h, depth, f = items[0]
    sums, weights = D.ssim_planes(s[None], r[None], w, h, depth, src_fmt=f, rec_fmt=f)
    assert sums.view(np.int64)[0] == got.view(np.int64)[0] and weights[0] == wt[0]
    assert D.ssim_score(sums, weights, raw=True)[0] == got[0] / wt[0]


def test_planes_repeat_and_batches_equal_single_calls(D, batch):
    items, _ = batch
    rc, a, _ = _planes_call(D, items)
    rc2, b, _ = _planes_call(D, items)
    assert rc == 0 and rc2 == 0
    assert np.array_equal(a.view(np.int64), b.view(np.int64))
    for i, it in enumerate(items):
        rc, one, _ = _planes_call(D, [it])
        assert rc == 0 and one.view(np.int64)[0] == a.view(np.int64)[i], i
    # more pairs than one launch takes (32), sizes interleaved
    many = [items[i % len(items)] for i in range(40)]
    rc, c, _ = _planes_call(D, many)
    assert rc == 0
    assert np.array_equal(c.view(np.int64), np.array([a.view(np.int64)[i % len(items)] for i in range(40)]))
    # par reaches the kernel: another horizontal table, another sum
    rc, p, _ = _planes_call(D, items[:1], par=4 / 3)
    assert rc == 0 and p[0] != a[0]


def test_radius_above_the_tiling_is_refused_before_any_launch(D):
    import torch
    import _ssim_ref as S
    w, h = 70, 6000
    assert len(S.plane_taps(w, h)[0]) // 2 == 65 > D.SSIM_MAX_RADIUS
    z = torch.zeros((h, w), dtype=torch.uint8, device="cuda")
    small = torch.zeros((64, 64), dtype=torch.uint8, device="cuda")
    # the refused pair comes last: the pairs before it are not launched either
    rc, out, _ = _planes_call(D, [(small, small, 64, 64, 8, D.SAMPLE_U8), (z, z, w, h, 8, D.SAMPLE_U8)], fill=-7.0)
    assert rc == -23
    assert (out == -7.0).all()
    terms = torch.full((w * h,), -7.0, dtype=torch.float64, device="cuda")
    pair = _pairs(D, [(z, z, w, h, 8, D.SAMPLE_U8)])
    assert D.lib().odhip_ssim_terms(ctypes.byref(pair[0]), ctypes.c_double(1.0), ctypes.c_void_p(terms.data_ptr()),
                                    None) == -23
    torch.cuda.synchronize()
    assert bool((terms == -7.0).all())
    # the widest radius the tiling takes still runs: 65 columns cap it to 64
    assert len(S.plane_taps(65, h)[0]) // 2 == D.SSIM_MAX_RADIUS
    src, rec, ssrc, srec = _planes(5, 65, h, 8, "u8")
    rc, out, wt = _planes_call(D, [(_dev(ssrc, 2), _dev(srec, 4), 65, h, 8, D.SAMPLE_U8)])
    t = S.terms(src, rec, 8)
    assert rc == 0 and wt[0] == S.weight(65, h)
    assert abs(out[0] - math.fsum(t.ravel().tolist())) <= t.size * 2.0 ** -53 * math.fsum(np.abs(t).ravel().tolist())
    # bad arguments
    rc, _, _ = _planes_call(D, [(small, small, 64, 64, 8, D.SAMPLE_U8)], par=0.0)
    assert rc == -10
    assert D.lib().odhip_metrics_planes(_pairs(D, [(small, small, 64, 64, 8, D.SAMPLE_U8)]), 1, 4, None, None, None,
                                        None, None) == -10       # no array for SSIM there
