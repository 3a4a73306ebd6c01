"""PSNR and PSNR-HVS-M on the device (metrics_kernels.hip) against the CPU restatement (tests/_metrics_ref.py) and
against what the reference's tools printed (tests/golden/metrics.npz):

- odhip_psnrhvs_windows: every window's float sum equals the restatement's EXACTLY, at depth 8, 10 and 12 (uint16
  and 12-bit int16 samples), with each of the three CSF tables;
- odhip_metrics_planes: SSE exact, the HVS sum within 1e-9 relative of the restatement's exact sum;
- the golden clips: PSNR the identical %-7G string, PSNR-HVS-M within 0.01 dB of the tool (whose running float
  accounts for the gap; the largest gap is printed);
- tools/y4m_metrics.py on two written Y4M files prints the tool's PSNR lines."""
import os
import subprocess
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


def _pair(rng, h, w, depth, kind):
    import _metrics_ref as M
    src = M._content(kind, rng, w, h, depth)
    top = (1 << depth) - 1
    amp = max(2, top // 20)
    rec = np.clip(src + rng.randint(-amp, amp + 1, size=src.shape), 0, top)
    keep = rng.rand(h, w) < 0.2
    rec[keep] = src[keep]
    return src.astype(np.int32), rec.astype(np.int32)


def _dev(D, a, depth, fmt):
    """a [h][w] samples at `depth` -> a CUDA tensor [1][h][w + pad] in the sample format fmt."""
    import torch
    h, w = a.shape
    buf = np.zeros((1, h, w + 3), np.uint8 if fmt == D.SAMPLE_U8 else np.int16)
    buf[0, :, :w] = a << (12 - depth) if fmt == D.SAMPLE_I16_12 else a
    return torch.from_numpy(buf).cuda()


@pytest.mark.parametrize("depth,fmt", [(8, "u8"), (8, "i16"), (10, "u16"), (10, "i16"), (12, "u16"), (12, "i16")])
def test_window_sums_are_bit_exact(D, depth, fmt):
    import _metrics_ref as M
    f = {"u8": D.SAMPLE_U8, "u16": D.SAMPLE_U16, "i16": D.SAMPLE_I16_12}[fmt]
    rng = np.random.RandomState(depth * 7 + len(fmt))
    for csf in (D.CSF_Y, D.CSF_CB, D.CSF_CR):
        for kind in ("natural", "texture", "noise"):
            h, w = 45 + csf * 8, 61 + csf * 5
            src, rec = _pair(rng, h, w, depth, kind)
            if f == D.SAMPLE_I16_12:
                # the reconstruction as a 12-bit plane of arbitrary values: the output conversion rounds it
                rec12 = np.clip((rec << (12 - depth)) + rng.randint(-9, 10, size=rec.shape), -40, 4200)
                import torch
                t = torch.from_numpy(np.pad(rec12, ((0, 0), (0, 3))).astype(np.int16)).cuda()
                rec = M.to_depth(rec12, depth)
            else:
                t = _dev(D, rec, depth, f)[0]
            got = D.psnrhvs_windows(_dev(D, src, depth, f)[0], t, w, h, depth, csf, src_fmt=f, rec_fmt=f)
            want = M.window_sums(src, rec, csf)
            assert got.shape == want.shape
            assert np.array_equal(got.view(np.uint32), want.view(np.uint32)), (csf, kind)


def test_metrics_planes_against_the_restatement(D):
    import torch
    import _metrics_ref as M
    rng = np.random.RandomState(11)
    for depth, f in ((8, D.SAMPLE_U8), (10, D.SAMPLE_U16), (12, D.SAMPLE_I16_12)):
        h, w, n = 83, 131, 5
        pairs = [_pair(rng, h, w, depth, ("natural", "texture", "noise")[i % 3]) for i in range(n)]
        src = torch.cat([_dev(D, s, depth, f) for s, _ in pairs])
        rec = torch.cat([_dev(D, r, depth, f) for _, r in pairs])
        csf = [i % 3 for i in range(n)]
        sse, hvs, npix, nwin = D.metrics_planes(src, rec, w, h, depth, csf, src_fmt=f, rec_fmt=f)
        for i, (s, r) in enumerate(pairs):
            assert sse[i] == M.sse(s, r)
            want = M.hvs_sum(s, r, csf[i])
            assert abs(hvs[i] - want) <= 1e-9 * want, (depth, i, hvs[i], want)
        assert list(npix) == [w * h] * n and list(nwin) == [18 * 11] * n
        # each metric alone
        sse2, hvs2, _, _ = D.metrics_planes(src, rec, w, h, depth, csf, psnrhvs=False, src_fmt=f, rec_fmt=f)
        assert np.array_equal(sse2, sse) and not hvs2.any()
        sse3, hvs3, _, _ = D.metrics_planes(src, rec, w, h, depth, csf, sse=False, src_fmt=f, rec_fmt=f)
        assert np.array_equal(hvs3, hvs) and not sse3.any()
    # more pairs than one launch takes (32)
    s, r = _pair(rng, 20, 30, 8, "noise")
    src = torch.cat([_dev(D, s, 8, D.SAMPLE_U8)] * 40)
    rec = torch.cat([_dev(D, r, 8, D.SAMPLE_U8)] * 40)
    sse, hvs, _, _ = D.metrics_planes(src, rec, 30, 20, 8, D.CSF_CB)
    assert (sse == M.sse(s, r)).all() and (hvs == hvs[0]).all()


def test_golden_tool_output(D):
    """PSNR identical to the tool's printed string; PSNR-HVS-M within 0.01 dB (the tool's running float)."""
    import torch
    import _metrics_ref as M
    g = np.load(os.path.join(ROOT, "tests", "golden", "metrics.npz"))
    worst = 0.0
    for idx, case in enumerate(M.CASES):
        name, _, w, h, c444, depth, _, _ = case
        srcs, dsts = M.make_case(case)
        pf, hf = [], []
        f = D.SAMPLE_U8 if depth == 8 else D.SAMPLE_U16
        for fs, fd in zip(srcs, dsts):
            se, hv = [], []
            for pli, (a, b) in enumerate(zip(fs, fd)):
                sse, hvs, npix, nwin = D.metrics_planes(_dev(D, a, depth, f), _dev(D, b, depth, f), a.shape[1],
                                                        a.shape[0], depth, pli, src_fmt=f, rec_fmt=f)
                se.append(int(sse[0]))
                hv.append(float(hvs[0] / (64.0 * nwin[0]) / float(((1 << depth) - 1) ** 2)))
            pf.append((se, [a.size for a in fs]))
            hf.append(hv)
        assert M.psnr_lines(pf, depth) == str(g["psnr"][idx]).splitlines(), name
        got = M.psnrhvs_lines(hf, c444)
        for gl, wl in zip(got, str(g["psnrhvs"][idx]).splitlines()):
            gv = [float(v) for v in gl.replace("(", " ").replace(")", " ").split()[1::2]]
            wv = [float(v) for v in wl.replace("(", " ").replace(")", " ").split()[1::2]]
            gap = max(abs(a - b) for a, b in zip(gv, wv))
            worst = max(worst, gap)
            assert gap < 0.01, (name, gl, wl)
    print("largest PSNR-HVS-M gap to the tool: %.3g dB" % worst)


def test_y4m_tool_prints_the_psnr_lines(D, tmp_path):
    import _metrics_ref as M
    g = np.load(os.path.join(ROOT, "tests", "golden", "metrics.npz"))
    for idx, case in enumerate(M.CASES):
        name, _, w, h, c444, depth, _, _ = case
        if depth != 8:
            continue
        srcs, dsts = M.make_case(case)
        a, b = tmp_path / ("%s_a.y4m" % name), tmp_path / ("%s_b.y4m" % name)
        a.write_bytes(M.y4m_bytes(srcs, w, h, c444, depth))
        b.write_bytes(M.y4m_bytes(dsts, w, h, c444, depth))
        r = subprocess.run([sys.executable, os.path.join(ROOT, "tools", "y4m_metrics.py"), str(a), str(b)],
                           capture_output=True, text=True, timeout=300)
        assert r.returncode == 0, r.stderr
        lines = r.stdout.splitlines()
        want = str(g["psnr"][idx]).splitlines()
        assert lines[:len(want)] == want, name
        assert len(lines) == 2 * len(want) and lines[-1].startswith("Total:")
