"""od_compute_dist (src/encode.c:1082-1226): the oracle restatement
against golden values from the compiled reference and, when it is present, live; the GPU
split (device parts + host pow) against the oracle, bit for bit."""
import ctypes
import os

import numpy as np
import pytest

from _caches import EINVAL
from _libs import GOLDEN, P, ROOT, oracle

DIST_SO = os.path.join(ROOT, "oracle", "_ref", "libdaalaref_dist.so")


def _o():
    o = oracle()
    o.odo_compute_dist.restype = ctypes.c_double
    return o


def _bits(a):
    return np.asarray(a, np.float64).view(np.int64)


def test_oracle_dist_matches_reference_golden():
    g = np.load(os.path.join(GOLDEN, "dist.npz"))
    o = _o()
    for n in (8, 16, 32, 64):
        for x, y, (flat, masking, cq), want in zip(g["x%d" % n], g["y%d" % n], g["meta%d" % n],
                                                    g["dist%d" % n]):
            x, y = np.ascontiguousarray(x), np.ascontiguousarray(y)
            got = o.odo_compute_dist(P(x), P(y), n, int(flat), int(masking), int(cq))
            assert _bits(got) == _bits(want), (n, flat, masking, cq)
        assert len(set(np.round(g["dist%d" % n], 3))) > 40


@pytest.mark.skipif(not os.path.exists(DIST_SO), reason="oracle/_ref not built here")
def test_oracle_dist_matches_reference_live():
    r = ctypes.CDLL(DIST_SO)
    r.ref_compute_dist.restype = ctypes.c_double
    o = _o()
    rng = np.random.RandomState(5)
    for n in (8, 16, 32, 64):
        for _ in range(60):
            amp = rng.choice([20, 300, 5000, 60000])
            x = (rng.laplace(size=(n, n)) * amp).astype(np.int32)
            y = (x * rng.choice([0, 1]) + rng.laplace(size=(n, n)) * amp * rng.choice([0.02, 0.3, 2])) \
                .astype(np.int32)
            for flat in (0, 1):
                masking, cq = int(rng.randint(2)), int(rng.randint(1, 64))
                a = o.odo_compute_dist(P(x), P(y), n, flat, masking, cq)
                b = r.ref_compute_dist(P(x), P(y), n, flat, masking, cq)
                assert _bits(a) == _bits(b)


@pytest.mark.gpu
@pytest.mark.parametrize("bs", [1, 2, 3, 4])
def test_gpu_dist_matches_oracle(bs):
    import torch
    import daala_amd as D
    D.init(0)
    o = _o()
    n = 4 << bs
    rng = np.random.RandomState(40 + bs)
    nplanes, h, w = 2, 192, 320            # whole 64 x 64 tiles only (5 x 3 of them; 3 x 2 for n = 64):
    if n == 64:                            # the clipped tiles are test_gpu_dist_clipped_tiles'
        h, w = 128, 192
    amp = np.kron(rng.choice([30, 300, 4000], size=(nplanes, h // 8, w // 8)), np.ones((8, 8)))
    x = (rng.laplace(size=(nplanes, h, w)) * amp).astype(np.int32)
    y = (x + rng.laplace(size=(nplanes, h, w)) * amp * 0.2).astype(np.int32)
    y[0, :16] = x[0, :16]                  # identical blocks: zero error
    tx, ty = torch.from_numpy(x).cuda(), torch.from_numpy(y).cuda()
    for (masking, flat, cq) in ((1, 0, 41), (0, 0, 30), (1, 1, 50)):
        got, _ = D.compute_dist(tx, ty, bs, masking, flat, cq)
        for p in range(nplanes):
            for by in range(h // n):
                for bx in range(w // n):
                    xb = np.ascontiguousarray(x[p, by * n:(by + 1) * n, bx * n:(bx + 1) * n])
                    yb = np.ascontiguousarray(y[p, by * n:(by + 1) * n, bx * n:(bx + 1) * n])
                    want = o.odo_compute_dist(P(xb), P(yb), n, flat, masking, cq)
                    assert _bits(got[p, by, bx]) == _bits(want), (bs, masking, flat, p, by, bx)


SETTINGS = ((1, 0, 41), (0, 0, 30), (1, 1, 50))      # (use_masking, flat_qm, coded_quantizer)


def _planes(rng, nplanes, h, w):
    """Source / reconstruction pairs with every sample inside |v| <= 11000: od_compute_var_4x4
    squares a sum of sixteen v >> 2 in int, and beyond about 11584 the reference itself overflows."""
    amp = np.kron(rng.choice([30, 300, 3000], size=(nplanes, h // 8, w // 8)), np.ones((8, 8)))
    x = np.clip(rng.laplace(size=(nplanes, h, w)) * amp, -11000, 11000).astype(np.int32)
    y = np.clip(x + rng.laplace(size=(nplanes, h, w)) * amp * 0.2, -11000, 11000).astype(np.int32)
    y[0, :8] = x[0, :8]                    # identical blocks: zero error
    return x, y


def _check_blocks(o, got, x, y, n, masking, flat, cq):
    nplanes, h, w = x.shape
    for p in range(nplanes):
        for by in range(h // n):
            for bx in range(w // n):
                xb = np.ascontiguousarray(x[p, by * n:(by + 1) * n, bx * n:(bx + 1) * n])
                yb = np.ascontiguousarray(y[p, by * n:(by + 1) * n, bx * n:(bx + 1) * n])
                want = o.odo_compute_dist(P(xb), P(yb), n, flat, masking, cq)
                assert _bits(got[p, by, bx]) == _bits(want), (n, w, h, masking, flat, p, by, bx)


@pytest.mark.gpu
@pytest.mark.parametrize("n,w,h", [(8, 88, 72), (16, 80, 48), (16, 144, 80), (32, 96, 160)])
def test_gpu_dist_clipped_tiles(n, w, h):
    """Planes that are multiples of n but not of the kernel's 64 x 64 tile: the last tile of a row
    and of a column is clipped (tw, th < 64), alone (80 x 48) or after whole ones."""
    import torch
    import daala_amd as D
    D.init(0)
    o = _o()
    assert w % 64 and h % 64
    bs = {8: 1, 16: 2, 32: 3}[n]
    x, y = _planes(np.random.RandomState(60 + w), 2, h, w)
    tx, ty = torch.from_numpy(x).cuda(), torch.from_numpy(y).cuda()
    for (masking, flat, cq) in SETTINGS:
        got, _ = D.compute_dist(tx, ty, bs, masking, flat, cq)
        _check_blocks(o, got, x, y, n, masking, flat, cq)


@pytest.mark.gpu
@pytest.mark.parametrize("bs,w,h", [(1, 88, 72), (2, 144, 80), (3, 96, 160), (4, 192, 128)])
def test_gpu_dist_px16_matches_oracle(bs, w, h):
    """odhip_dist_parts_px16: x as 8-bit source samples, y as an int16 plane, each with a row stride
    of its own, two planes; equal to the oracle on x = (p - 128) << 4."""
    import torch
    import daala_amd as D
    D.init(0)
    L = D.lib()
    o = _o()
    n = 4 << bs
    nplanes = 2
    xs, ys = w + 5, w + 8
    rng = np.random.RandomState(70 + bs)
    px = np.zeros((nplanes, h, xs), np.uint8)
    px[:, :, :w] = np.clip(128 + np.cumsum(rng.randint(-9, 10, size=(nplanes, h, w)), axis=2)
                           + rng.randint(-20, 21, size=(nplanes, h, w)), 0, 255)
    px[:, :, w:] = 255                     # the padding must not be read
    x = (px[:, :, :w].astype(np.int32) - 128) << 4
    amp = np.kron(rng.choice([3, 40, 400], size=(nplanes, h // 8, w // 8)), np.ones((8, 8)))
    y = np.clip(x + rng.laplace(size=x.shape) * amp, -11000, 11000).astype(np.int32)
    y[1, -8:] = x[1, -8:]
    y16 = np.full((nplanes, h, ys), 32767, np.int16)
    y16[:, :, :w] = y
    tpx, ty = torch.from_numpy(px).cuda(), torch.from_numpy(y16).cuda()
    vp = ctypes.c_void_p
    for (masking, flat, cq) in SETTINGS:
        parts = torch.full((nplanes, h // 8, w // 8, 3), -1.0, dtype=torch.float64, device="cuda")
        assert L.odhip_dist_parts_px16(vp(parts.data_ptr()), vp(tpx.data_ptr()), xs, vp(ty.data_ptr()), ys, nplanes,
                                       w, h, bs, masking, flat, None) == 0
        torch.cuda.synchronize()
        hp = np.ascontiguousarray(parts.cpu().numpy())
        got = np.zeros((nplanes, h // n, w // n), np.float64)
        assert L.odhip_dist_finish(P(got), P(hp), nplanes, w, h, bs, masking, flat, cq) == 0
        _check_blocks(o, got, x, y, n, masking, flat, cq)
    parts = torch.zeros((nplanes, h // 8, w // 8, 3), dtype=torch.float64, device="cuda")
    for xstride, ystride in ((w - 1, ys), (xs, w - 1)):
        assert L.odhip_dist_parts_px16(vp(parts.data_ptr()), vp(tpx.data_ptr()), xstride, vp(ty.data_ptr()), ystride,
                                       nplanes, w, h, bs, 1, 0, None) == EINVAL
