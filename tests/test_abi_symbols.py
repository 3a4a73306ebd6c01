"""CPU: the C-ABI library loads and exports every symbol include/daala_hip.h
declares (no compute calls: there is no GPU here), and it does NOT link or load
anything from oracle/."""
import os
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.fixture(scope="module")
def built():
    from daala_amd import build
    return build.build()


def test_library_exports_every_declared_symbol(built):
    import daala_amd
    L = daala_amd.lib()
    from daala_amd import _abi
    names = set(_abi.prototypes())
    assert len(names) >= 25
    out = subprocess.run(["nm", "-D", "--defined-only", built], capture_output=True, text=True, check=True).stdout
    exported = {ln.split()[-1] for ln in out.splitlines() if " T " in ln}
    missing = sorted(names - exported)
    assert not missing, missing
    assert b"gfx950" in L.odhip_version()


def test_product_does_not_depend_on_oracle(built):
    out = subprocess.run(["ldd", built], capture_output=True, text=True).stdout
    assert "oracle" not in out and "daalaref" not in out
    for root, _, files in os.walk(os.path.join(ROOT, "daala_amd")):
        for f in files:
            if f.endswith((".py", ".hip", ".cuh", ".h")):
                src = open(os.path.join(root, f)).read()
                assert "liboracle" not in src and "od_oracle" not in src, f


def test_argument_validation_without_gpu(built):
    """Pure host-side validation paths return OD_EINVAL before touching HIP."""
    import ctypes
    import daala_amd
    L = daala_amd.lib()
    assert L.odhip_fdct2d_batch(7, None, None, ctypes.c_long(1), 0, None) == -10
    assert L.odhip_fdct2d_batch(0, None, None, ctypes.c_long(0), 0, None) == 0
    assert L.odhip_pvq_search_batch(None, 16, None, None, None, ctypes.c_double(0.1), None,
                                    None, ctypes.c_long(1), None) == -10
    nb = ctypes.c_int()
    offs = (ctypes.c_int * 13)()
    ln = ctypes.c_int()
    assert L.odhip_pvq_band_layout(2, ctypes.byref(nb), offs, ctypes.byref(ln)) == 0
    assert nb.value == 7 and ln.value == 256
    assert [offs[i] for i in range(8)] == [1, 16, 24, 32, 64, 96, 128, 256]


def test_band_stage_and_reference_path_validation_without_gpu(built):
    """The multi-job and with-reference entry points reject bad arguments before
    any HIP call (no GPU in this container)."""
    import ctypes
    import daala_amd
    from daala_amd import api
    L = daala_amd.lib()
    EINVAL = -10
    assert L.odhip_pvq_noref_bands_multi(None, 1, ctypes.c_double(0.1), None) == EINVAL
    assert L.odhip_pvq_choose_multi(None, 0, ctypes.c_double(0.1), None) == EINVAL
    jobs = (api._Job * 17)()
    assert L.odhip_pvq_noref_bands_multi(jobs, 17, ctypes.c_double(0.1), None) == EINVAL  # > 16 jobs
    assert L.odhip_inverse_levels_pvq(None, 64, ctypes.c_long(4096), jobs, 1, 0, 64, 64, None) == EINVAL
    ptrs = (ctypes.c_void_p * 6)()
    assert L.odhip_inverse_levels_pvq(ptrs, 64, ctypes.c_long(4096), jobs, 6, 0, 64, 64, None) == EINVAL
    # with-reference blocks: empty batches succeed, bad sizes / null pointers are refused
    z = ctypes.c_long(0)
    one = ctypes.c_long(1)
    assert L.odhip_pvq_ref_prepare(None, None, 16, z, None, 1, 4096, 0, None, None, None, None, None) == 0
    assert L.odhip_pvq_ref_prepare(None, None, 16, one, None, 1, 4096, 0, None, None, None, None,
                                   None) == EINVAL
    assert L.odhip_pvq_ref_candidates(None, None, 16, one, 4096, None, None, None) == EINVAL
    assert L.odhip_pvq_synthesis(None, None, None, 16, one, None, None, None) == EINVAL
    assert L.odhip_pvq_synthesis(None, None, None, 16, z, None, None, None) == 0
    # record layouts the Python mirror relies on
    assert api.BAND_RECORD.itemsize == 64 and api.BAND_RECORD.fields["dist0"][1] == 24
    assert api.BAND_RECORD.fields["yy"][1] == 32 and api.BAND_RECORD.fields["dist"][1] == 40
    assert api.REFPREP_RECORD.fields["corr"][1] == 48


def test_plane_layout_validation_without_gpu(built):
    """The picture-plane contract of include/daala_hip.h (stride >= w, plane_stride >= stride*h, both
    multiples of 4, the base on a sample group) is refused before any HIP call; so are DCT planes and
    copy-pad planes whose rows or planes overlap."""
    import ctypes
    import daala_amd
    L = daala_amd.lib()
    EINVAL = -10
    px, coef = ctypes.c_void_p(0x10000), ctypes.c_void_p(0x20000)
    lv = (ctypes.c_void_p * 5)(*[0x20000] * 5)
    w = h = 64
    for ptr, stride, pitch in ((px, 60, 64 * 64), (px, 80, 64 * 64), (px, 66, 66 * 64), (px, 64, 64 * 64 + 2),
                               (ctypes.c_void_p(0x10002), 64, 64 * 64)):
        pitch = ctypes.c_long(pitch)
        assert L.odhip_forward_pyramid(lv, ptr, stride, pitch, 2, w, h, 0, w, h, None) == EINVAL
        assert L.odhip_inverse_level(ptr, stride, pitch, coef, 2, w, h, 0, 1, w, h, None) == EINVAL
        assert L.odhip_inverse_partition(ptr, stride, pitch, coef, 2, w, h, 0, coef, 8, ctypes.c_long(64), 1, w, h,
                                         None) == EINVAL
    r, n = ctypes.c_int(), ctypes.c_int()
    assert L.odhip_inverse_route(0, 0, 0, 100, 1, ctypes.byref(r), ctypes.byref(n)) == EINVAL
    assert L.odhip_inverse_route(0, 4, 0, 64, 1, ctypes.byref(r), ctypes.byref(n)) == EINVAL
    assert L.odhip_fdct2d_plane(1, px, 60, coef, 64, 64, 64, 0, None) == EINVAL
    assert L.odhip_idct2d_plane(1, px, 64, coef, 60, 64, 64, 0, None) == EINVAL
    one = ctypes.c_long(1)
    assert L.odhip_image_planes_copy_pad(px, 64, ctypes.c_long(64 * 64 - 1), 64, 64, coef, 33, ctypes.c_long(33 * 17),
                                         33, 17, 2, None) == EINVAL
    assert L.odhip_image_planes_copy_pad(px, 64, ctypes.c_long(64 * 64), 64, 64, coef, 33, one, 33, 17, 2,
                                         None) == EINVAL
    assert L.odhip_image_planes_copy_pad16(px, 64, ctypes.c_long(64 * 64), 64, 64, coef, 12, 33, one, 33, 17, 2,
                                           None) == EINVAL


def _default_build_source(text):
    """`text` as the DEFAULT build compiles it: `#ifdef ODHIP_EXPERIMENTS` ... (`#else`) ... `#endif`
    blocks resolved for an undefined ODHIP_EXPERIMENTS (other conditionals are kept whole)."""
    out = []
    stack = []          # per open conditional: None (not ours) or True / False = currently emitting
    for line in text.splitlines():
        t = line.strip()
        if t.startswith("#if"):
            if t.replace(" ", "") in ("#ifdefODHIP_EXPERIMENTS", "#ifdefined(ODHIP_EXPERIMENTS)"):
                stack.append(False)
                continue
            stack.append(None)
        elif t.startswith("#else") and stack and stack[-1] is not None:
            stack[-1] = not stack[-1]
            continue
        elif t.startswith("#endif"):
            ours = stack.pop() if stack else None
            if ours is not None:
                continue
        if all(s is not False for s in stack):
            out.append(line)
    return "\n".join(out)


def test_default_build_reads_at_most_six_environment_switches(built):
    """superseded kernel generations, ablations and tuning knobs live behind
    -DODHIP_EXPERIMENTS (lib/libdaalahip_exp.so); what the DEFAULT library still reads from the
    environment is counted here from the sources as that build compiles them: ODHIP_PVQ_SERIAL,
    ODHIP_PVQ_FORCE_SEQ (ctx.hip) and ODHIP_CACHE_CHECK (frame_cache.hip)."""
    import re
    names = set()
    calls = 0
    csrc = os.path.join(ROOT, "daala_amd", "csrc")
    for root, _, files in os.walk(csrc):
        for f in files:
            if f.endswith((".hip", ".cuh", ".h")):
                src = _default_build_source(open(os.path.join(root, f)).read())
                src = re.sub(r"/\*.*?\*/", "", src, flags=re.S)
                calls += len(re.findall(r"\bgetenv\s*\(", src))
                names.update(re.findall(r"\bgetenv\s*\(\s*\"([A-Z_0-9]+)\"", src))
    assert calls <= 6, (calls, sorted(names))
    assert names == {"ODHIP_PVQ_SERIAL", "ODHIP_PVQ_FORCE_SEQ", "ODHIP_CACHE_CHECK"}, sorted(names)
    # the ablation that removes loads / stores on purpose cannot be reached in the default build
    lap = _default_build_source(open(os.path.join(csrc, "lapped_kernels.hip")).read())
    assert "ODHIP_INVERSE_DBG\")" not in lap and "#define OD_INV_DBG(a, bit) false" in lap
    # both builds exist and export the same C ABI
    import daala_amd
    assert os.path.exists(daala_amd.EXPERIMENTS_LIB)
    def syms(p):
        out = subprocess.run(["nm", "-D", "--defined-only", p], capture_output=True, text=True).stdout
        return {ln.split()[-1] for ln in out.splitlines() if " T " in ln and ("odhip_" in ln or "od_" in ln)}
    # (odhip_exp_*: read-outs of counters only the experiments build keeps, e.g. odhip_exp_row_replay_stats)
    assert syms(built) == {s for s in syms(daala_amd.EXPERIMENTS_LIB) if not s.startswith("odhip_exp_")}
