"""CPU: odhip_haar_planes, odhip_haar_encode_planes and odhip_haar_decode_planes (include/daala_hip.h) are exported by
both builds of the library, and every argument outside the contract is answered ODHIP_EINVAL by host-side checks in
front of any HIP call - there is no GPU here and the pointers are fake addresses, as in
tests/test_forward_partition_host.py."""
import ctypes
import subprocess

import pytest

EINVAL = -10
W, H = 192, 128
PX, PRED, REC, Q, TREE, DCREC = 0x10000, 0x90000, 0x110000, 0x200000, 0x400000, 0x600000
NAMES = {"odhip_haar_planes", "odhip_haar_encode_planes", "odhip_haar_decode_planes", "odhip_haar_sizeof"}


@pytest.fixture(scope="module")
def built():
    from daala_amd import build
    return build.build()


def _job(**kw):
    import daala_amd
    j = daala_amd.HaarJob()
    j.d_px, j.d_pred, j.d_rec, j.d_q, j.d_tree, j.d_dc_rec = PX, None, REC, Q, TREE, DCREC
    j.px_stride, j.px_plane_stride, j.nplanes, j.w, j.h, j.dec = W, W * H, 2, W, H, 0
    j.pic_w, j.pic_h, j.lossless, j.depth, j.quant = W, H, 1, 8, 0
    j.dc_quant[0] = j.dc_quant[1] = 1
    j.plane_split = 1
    for k, v in kw.items():
        if k == "dc_quant":
            j.dc_quant[0], j.dc_quant[1] = v
        else:
            setattr(j, k, v)
    return j


def _enc(L, **kw):
    return L.odhip_haar_encode_planes(ctypes.byref(_job(**kw)), None)


def _dec(L, **kw):
    return L.odhip_haar_decode_planes(ctypes.byref(_job(**kw)), None)


def test_both_builds_export_the_entry_points(built):
    import daala_amd
    for path in (built, daala_amd.EXPERIMENTS_LIB):
        out = subprocess.run(["nm", "-D", "--defined-only", path], capture_output=True, text=True, check=True).stdout
        names = {ln.split()[-1] for ln in out.splitlines() if " T " in ln}
        assert NAMES <= names, path


def test_package_exports_the_wrappers_and_the_job_matches(built):
    import daala_amd
    assert callable(daala_amd.haar_planes) and callable(daala_amd.haar_encode) and callable(daala_amd.haar_decode)
    assert ctypes.sizeof(daala_amd.HaarJob) == daala_amd.lib().odhip_haar_sizeof()


ENCODE_REFUSALS = [
    dict(d_px=None), dict(d_q=None), dict(d_tree=None),
    dict(w=W - 32), dict(h=H - 32), dict(w=W - 16, dec=1, px_stride=W), dict(h=H - 4, dec=1), dict(w=0), dict(h=-64),
    dict(dec=2), dict(dec=-1),
    dict(depth=9), dict(depth=0), dict(depth=16),
    dict(lossless=1, quant=16), dict(lossless=0, quant=0), dict(lossless=0, quant=-1), dict(lossless=1, quant=-1),
    dict(dc_quant=(0, 1)), dict(dc_quant=(1, 0)), dict(dc_quant=(-5, 1)),
    dict(pic_w=W + 1), dict(pic_h=H + 1), dict(pic_w=0), dict(pic_h=0), dict(pic_w=-3),
    dict(plane_split=-1), dict(plane_split=3),
    dict(nplanes=0),
    # what the launch grid cannot hold
    dict(nplanes=65536, plane_split=1), dict(h=65536 * 64, px_plane_stride=W * 65536 * 64),
    # the picture-plane layout rules: rows and planes that overlap, strides and bases off the 4-sample groups
    dict(px_stride=W - 4), dict(px_plane_stride=W * H - 4), dict(px_stride=W + 2, px_plane_stride=(W + 2) * H),
    dict(px_plane_stride=W * H + 2), dict(d_px=PX + 2), dict(d_rec=REC + 1), dict(d_pred=PRED + 2),
    # the coefficient planes off 16 bytes, the DCs off their words
    dict(d_q=Q + 4), dict(d_q=Q + 8), dict(d_tree=TREE + 4), dict(d_dc_rec=DCREC + 2),
]


@pytest.mark.parametrize("bad", ENCODE_REFUSALS, ids=lambda d: ",".join("%s=%s" % kv for kv in d.items()))
def test_encoder_refuses_bad_arguments_without_gpu(built, bad):
    import daala_amd
    assert _enc(daala_amd.lib(), **bad) == EINVAL


def test_encoder_refuses_a_null_job(built):
    import daala_amd
    L = daala_amd.lib()
    assert L.odhip_haar_encode_planes(None, None) == EINVAL and L.odhip_haar_decode_planes(None, None) == EINVAL


def test_decoder_refuses_bad_arguments_without_gpu(built):
    import daala_amd
    L = daala_amd.lib()
    for bad in (dict(d_q=None), dict(d_rec=None), dict(w=W - 32), dict(dec=2), dict(depth=11),
                dict(lossless=1, quant=3), dict(lossless=0, quant=0), dict(dc_quant=(0, 0)), dict(plane_split=5),
                dict(px_stride=W - 4), dict(d_q=Q + 4), dict(d_rec=REC + 2)):
        assert _dec(L, **bad) == EINVAL, bad


def test_bare_transforms_refuse_bad_arguments_without_gpu(built):
    import daala_amd
    L = daala_amd.lib()

    def call(out=Q, src=TREE, nplanes=1, w=64, h=64, ln=3, inverse=0):
        return L.odhip_haar_planes(ctypes.c_void_p(out), ctypes.c_void_p(src), nplanes, w, h, ln, inverse, None)

    for bad in (dict(out=0), dict(src=0), dict(nplanes=0), dict(ln=1), dict(ln=7), dict(w=60), dict(h=68, ln=3),
                dict(w=0), dict(out=Q + 4), dict(src=TREE + 8)):
        assert call(**bad) == EINVAL, bad
