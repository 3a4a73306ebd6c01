"""The seeded plane pairs whose tile sums tests/golden/metric_sums.npz records (tools/make_golden_metric_sums.py) and
tests/test_gpu_metric_sums.py compares: per metric one 8-bit pair with more than 256 tiles of 32x32 in its largest
level, so that a lane of the tile-sum kernel adds more than one partial, and one call of 40 small pairs of mixed
sizes, depths and formats, some sharing their source plane - more than one launch group takes."""
import ctypes

import numpy as np

import _metrics_ref as M

METRICS = ("ssim", "msssim", "fastssim")
COLUMNS = {"ssim": 1, "msssim": 5, "fastssim": 4}
# 544 x 512 is 17 x 16 = 272 tiles (SSIM, scale 0 of MS-SSIM); level 0 of FastSSIM halves the plane first
BIG = {"ssim": (544, 512), "msssim": (544, 512), "fastssim": (1088, 1024)}
# the shape lists of the `batch` fixtures of test_gpu_ssim.py, test_gpu_msssim.py and test_gpu_fastssim.py
SHAPES = {
    "ssim": [(24, 544, 8, "u8"), (77, 53, 10, "u16"), (40, 256, 12, "i16"), (8, 544, 8, "i16"), (130, 70, 8, "u8"),
             (33, 33, 10, "i16"), (4, 272, 8, "u8")],
    "msssim": [(77, 53, 10, "u16"), (16, 16, 8, "u8"), (49, 35, 12, "i16"), (130, 70, 8, "u8"), (33, 65, 10, "i16"),
               (64, 48, 8, "i16"), (17, 31, 8, "u8")],
    "fastssim": [(70, 50, 10, "u16"), (16, 16, 8, "u8"), (33, 31, 12, "i16"), (130, 66, 8, "u8"), (31, 47, 10, "i16"),
                 (64, 48, 8, "i16"), (17, 31, 8, "u8")],
}
MIXED = 40


def _pair(seed, w, h, depth):
    rng = np.random.RandomState(seed)
    top = (1 << depth) - 1
    src = M._content(("natural", "texture", "noise")[seed % 3], rng, w, h, depth)
    amp = max(2, top // 20)
    return src, np.clip(src + rng.randint(-amp, amp + 1, size=src.shape), 0, top)


def big_pair(metric):
    """[(src, rec, depth, format)]: the one large 8-bit pair, int32 planes at the depth."""
    w, h = BIG[metric]
    return [_pair(500 + METRICS.index(metric), w, h, 8) + (8, "u8")]


def mixed_pairs(metric):
    """The 40 pairs of the mixed call: the shape list, then two more reconstructions of the first shape's source; the
    nine go round.  A source that is the same array is the same plane on the device."""
    nine = []
    for i, (w, h, depth, fmt) in enumerate(SHAPES[metric]):
        nine.append(_pair(40 + i, w, h, depth) + (depth, fmt))
    src, _, depth, fmt = nine[0]
    for k in (1, 2):
        noise = np.random.RandomState(60 + k).randint(-30*k, 30*k + 1, size=src.shape)
        nine.append((src, np.clip(src + noise, 0, (1 << depth) - 1), depth, fmt))
    return [nine[i % len(nine)] for i in range(MIXED)]


class Device:
    """The pairs on the device, each distinct array uploaded once: .pairs is the odhip_metrics_pair array."""

    def __init__(self, D, host_pairs):
        import torch
        from daala_amd.api import _MetricsPair
        code = {"u8": D.SAMPLE_U8, "u16": D.SAMPLE_U16, "i16": D.SAMPLE_I16_12}
        self.keep = {}
        self.n = len(host_pairs)
        self.pairs = (_MetricsPair*max(1, self.n))()
        for i, (src, rec, depth, fmt) in enumerate(host_pairs):
            h, w = src.shape
            ptr = []
            for a in (src, rec):
                if id(a) not in self.keep:
                    # 12-bit int16 planes hold the samples shifted up: the output conversion gives them back
                    stored = a.astype(np.uint8) if fmt == "u8" else (a << (12 - depth if fmt == "i16" else 0)).astype(np.int16)
                    self.keep[id(a)] = (a, torch.from_numpy(np.ascontiguousarray(stored)).cuda())
                ptr.append(self.keep[id(a)][1].data_ptr())
            self.pairs[i] = _MetricsPair(ptr[0], ptr[1], code[fmt], code[fmt], w, w, w, h, depth, 0)


def planes(D, metric, dev):
    """The sums of odhip_*_planes over the pairs: float64 [n][columns]."""
    import torch
    out = torch.zeros((max(1, dev.n), COLUMNS[metric]), dtype=torch.float64, device="cuda")
    p = ctypes.c_void_p(out.data_ptr())
    L = D.lib()
    if metric == "ssim":
        rc = L.odhip_ssim_planes(dev.pairs, dev.n, ctypes.c_double(1.0), p, None, None)
    elif metric == "msssim":
        rc = L.odhip_msssim_planes(dev.pairs, dev.n, p, None, None)
    else:
        rc = L.odhip_fastssim_planes(dev.pairs, dev.n, p, None)
    torch.cuda.synchronize()
    assert rc == 0, (metric, rc)
    return out.cpu().numpy()[:dev.n]


def term_maps(D, metric, dev):
    """The device's term map of every column of pair 0 (odhip_*_terms): a list of float64 arrays.  MS-SSIM: the cs map
    of scales 0..3 and the ssim map of scale 4, the terms its sums add."""
    import torch
    q = dev.pairs[0]
    L = D.lib()
    maps = []
    for col in range(COLUMNS[metric]):
        if metric == "fastssim":
            wl, hl = D.fastssim_level_size(q.w, q.h, col)
        else:
            wl, hl = q.w >> col, q.h >> col
        a = torch.zeros(hl*wl, dtype=torch.float64, device="cuda")
        b = torch.zeros(hl*wl, dtype=torch.float64, device="cuda")
        pa, pb = ctypes.c_void_p(a.data_ptr()), ctypes.c_void_p(b.data_ptr())
        if metric == "ssim":
            rc = L.odhip_ssim_terms(ctypes.byref(q), ctypes.c_double(1.0), pa, None)
        elif metric == "msssim":
            rc = L.odhip_msssim_terms(ctypes.byref(q), col, pa, pb, None)
        else:
            rc = L.odhip_fastssim_terms(ctypes.byref(q), col, pa, None)
        torch.cuda.synchronize()
        assert rc == 0, (metric, col, rc)
        maps.append((b if metric == "msssim" and col == 4 else a).cpu().numpy())
    return maps
