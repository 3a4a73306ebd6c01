"""CPU: odhip_forward_partition and odhip_forward_partition_host (include/daala_hip.h) are exported by both
builds of the library, and every argument outside the contract is answered ODHIP_EINVAL by host-side
checks in front of any HIP call - there is no GPU here, and the pointers are fake addresses, as in
tests/test_abi_symbols.py::test_plane_layout_validation_without_gpu."""
import ctypes
import subprocess

import pytest

EINVAL = -10
W = H = 128                 # 2 x 2 luma superblocks, 4 x 4 of 4:2:0 chroma
PX, COEF, MAP = 0x10000, 0x200000, 0x300000


@pytest.fixture(scope="module")
def built():
    from daala_amd import build
    return build.build()


def _forward(L, coef=COEF, px=PX, stride=W, pitch=W * H, nplanes=2, w=W, h=H, dec=0, bsize=MAP, bstride=None,
             frame_stride=1024, ppf=1):
    if bstride is None:
        bstride = 8 * (w // (64 >> (dec & 1)))           # the compact width, so that only the argument under test is off
    return L.odhip_forward_partition(ctypes.c_void_p(coef), ctypes.c_void_p(px), stride, ctypes.c_long(pitch), nplanes, w,
                                     h, dec, ctypes.c_void_p(bsize), bstride, ctypes.c_long(frame_stride), ppf, w, h,
                                     None)


def test_both_builds_export_the_two_entry_points(built):
    import daala_amd
    L = daala_amd.lib()
    assert hasattr(L, "odhip_forward_partition") and hasattr(L, "odhip_forward_partition_host")
    for path in (built, daala_amd.EXPERIMENTS_LIB):
        out = subprocess.run(["nm", "-D", "--defined-only", path], capture_output=True, text=True, check=True).stdout
        names = {ln.split()[-1] for ln in out.splitlines() if " T " in ln}
        assert {"odhip_forward_partition", "odhip_forward_partition_host"} <= names, path


def test_package_exports_the_wrappers(built):
    import daala_amd
    assert callable(daala_amd.forward_partition) and callable(daala_amd.forward_partition_host)


def test_device_form_refuses_bad_arguments_without_gpu(built):
    import daala_amd
    L = daala_amd.lib()
    # NULL pointers, plane counts, decimations
    assert _forward(L, coef=0) == EINVAL
    assert _forward(L, px=0) == EINVAL
    assert _forward(L, bsize=0) == EINVAL
    assert _forward(L, ppf=0) == EINVAL
    assert _forward(L, ppf=-1) == EINVAL
    assert _forward(L, nplanes=0) == EINVAL
    assert _forward(L, dec=2) == EINVAL
    assert _forward(L, dec=-1) == EINVAL
    # sizes that are no multiple of 64 >> dec
    assert _forward(L, w=W - 32) == EINVAL              # a multiple of 32: fine for chroma only
    assert _forward(L, h=H - 32) == EINVAL
    assert _forward(L, w=W - 16, dec=1, bstride=64) == EINVAL
    assert _forward(L, h=H - 4, dec=1) == EINVAL
    assert _forward(L, w=0) == EINVAL
    assert _forward(L, h=-64) == EINVAL
    # the picture-plane layout rules
    for px, stride, pitch in ((PX, W - 4, W * H), (PX, W + 16, W * H), (PX, W + 2, (W + 2) * H), (PX, W, W * H + 2),
                              (PX + 2, W, W * H)):
        assert _forward(L, px=px, stride=stride, pitch=pitch) == EINVAL, (px, stride, pitch)
    # rows of the map that overlap: below 8 entries per superblock of the row
    assert _forward(L, bstride=8 * (W // 64) - 1) == EINVAL
    assert _forward(L, dec=1, bstride=8 * (W // 32) - 1) == EINVAL
    # the coefficient planes off 16 bytes
    assert _forward(L, coef=COEF + 4) == EINVAL
    assert _forward(L, coef=COEF + 8) == EINVAL


def test_host_form_refuses_bad_arguments_without_gpu(built):
    import daala_amd
    L = daala_amd.lib()

    def call(coef=COEF, px=PX, stride=W, w=W, h=H, dec=0, bsize=MAP, bstride=64):
        return L.odhip_forward_partition_host(ctypes.c_void_p(coef), ctypes.c_void_p(px), stride, w, h, dec,
                                              ctypes.c_void_p(bsize), bstride, w, h)

    assert call(coef=0) == EINVAL
    assert call(px=0) == EINVAL
    assert call(bsize=0) == EINVAL
    assert call(dec=2) == EINVAL
    assert call(stride=W - 1) == EINVAL
    assert call(w=W - 32) == EINVAL
    assert call(h=H - 32) == EINVAL
    assert call(w=W - 16, dec=1) == EINVAL
    assert call(bstride=8 * (W // 64) - 1) == EINVAL
    assert call(dec=1, bstride=8 * (W // 32) - 1) == EINVAL
