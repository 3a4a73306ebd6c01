"""The UNMODIFIED reference encoder_example (oracle/_ref) on 4:4:4 input (`C444`,
examples/encoder_example.c:232-260): chroma planes with xdec = ydec = 0.

CPU: the plain C run codes the clip (three header packets, one per frame).
GPU: the same binary with tests/interpose/libinterpose.so + libdaalahip.so in LD_PRELOAD - the
per-call surfaces, the frame cache and the dering cache serving chroma planes of the picture
size - writes the same Ogg packets as the plain C run."""
import os

import numpy as np
import pytest

from _libs import synth_frame
from test_encoder_example import EXE, HERE, ROOT, ogg_packets

needs_exe = pytest.mark.skipif(not os.path.exists(EXE), reason="oracle/_ref/encoder_example not present")


def write_y4m444(path, w, h, nframes, seed=7):
    with open(path, "wb") as f:
        f.write(b"YUV4MPEG2 W%d H%d F30:1 Ip A1:1 C444\n" % (w, h))
        for fr in range(nframes):
            f.write(b"FRAME\n")
            luma = synth_frame(w, h, seed=seed, phase=5 * fr)[0].astype(np.uint8)
            f.write(luma.tobytes())
            # full-size chroma: a gain of luma plus a pattern of its own
            yy, xx = np.mgrid[0:h, 0:w]
            for g, k in ((5, 0.21), (-3, 0.13)):
                c = 128 + g * (luma.astype(np.int32) - 128) / 10 + 20 * np.sin(xx * k + yy * 0.07 + fr)
                f.write(np.clip(c, 0, 255).astype(np.uint8).tobytes())


def run444(tmp_path, name, w, h, nframes, env=None):
    import subprocess
    y4m = str(tmp_path / "in444.y4m")
    write_y4m444(y4m, w, h, nframes)
    out = str(tmp_path / name)
    e = dict(os.environ)
    e.update(env or {})
    p = subprocess.run([EXE, "-v", "20", "-k", "1", "-z", "7", "-o", out, y4m], capture_output=True,
                       text=True, timeout=900, env=e)
    assert p.returncode == 0, p.stderr[-2000:]
    with open(out, "rb") as f:
        return f.read(), p.stderr


@needs_exe
def test_encoder_example_codes_444_on_the_cpu(tmp_path):
    ogv, _ = run444(tmp_path, "c.ogv", 64, 64, 2)
    packets, _ = ogg_packets(ogv)
    assert len(packets) == 3 + 2 and packets[0][:6] == b"\x80daala"


@needs_exe
@pytest.mark.gpu
@pytest.mark.parametrize("size", [(64, 64), (176, 120)])
def test_encoder_example_444_with_libdaalahip_is_byte_identical(tmp_path, size):
    import torch
    assert torch.cuda.is_available()
    w, h = size
    nframes = 2
    want, _ = run444(tmp_path, "c.ogv", w, h, nframes)
    ipo = os.path.join(HERE, "interpose", "libinterpose.so")
    hip = os.path.join(ROOT, "daala_amd", "lib", "libdaalahip.so")
    assert os.path.exists(ipo) and os.path.exists(hip)
    got, err = run444(tmp_path, "h.ogv", w, h, nframes,
                      env={"LD_PRELOAD": ipo + ":" + hip, "ODHIP_INTERPOSE_VTBL": "1",
                           "ODHIP_INTERPOSE_REPORT": "1"})
    line = [l for l in err.splitlines() if l.startswith("odhip_interposed_calls")]
    assert line, err[-1000:]
    calls = [int(v) for v in line[-1].split()[1:]]
    assert all(c > 0 for c in calls), calls
    assert ogg_packets(got) == ogg_packets(want), \
        "the 4:4:4 .ogv written through libdaalahip differs from the plain C one"
    assert len(ogg_packets(got)[0]) == 3 + nframes
