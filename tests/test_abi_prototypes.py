"""CPU: the ctypes prototypes daala_amd/_abi.py reads from include/daala_hip.h - every declared
function is covered and bound on daala_amd.lib(), a hand-written sample of every type class,
what the parser refuses, and calls that only come out right with the right prototype."""
import os
import re
from ctypes import ArgumentError, c_char_p, c_double, c_int, c_int64, c_long, c_size_t, c_void_p

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
EINVAL = -10
P = c_void_p            # every pointer or array parameter, and odhip_stream


@pytest.fixture(scope="module")
def L():
    import daala_amd
    from daala_amd import build
    build.build()
    return daala_amd.lib()


@pytest.fixture(scope="module")
def protos():
    from daala_amd import _abi
    return _abi.prototypes()


def test_every_declared_function_is_covered_and_bound(L, protos):
    # the names as the symbol test used to find them: an identifier of the library's before a "("
    hdr = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "daala_hip.h")).read(), flags=re.S)
    names = set(re.findall(r"\b(od_[a-z0-9_]+_hip|odhip_[a-z0-9_]+)\s*\(", hdr))
    assert set(protos) == names and len(names) >= 229
    for name, (res, args) in protos.items():
        fn = getattr(L, name)
        assert fn.argtypes is not None and list(fn.argtypes) == args and fn.restype is res, name


PINNED = {
    "odhip_version": (c_char_p, []),
    "odhip_pipe_create": (c_void_p, [P]),
    "odhip_pipe_export_bytes": (c_size_t, [P]),
    "odhip_pipe_host_wait_ms": (c_double, [P]),
    "odhip_pipe_theta_listed": (c_long, [P]),
    "odhip_forward_partition": (c_int, [P, P, c_int, c_long, c_int, c_int, c_int, c_int, P, c_int, c_long,
                                        c_int, c_int, c_int, P]),
    "odhip_me_downsample": (c_int, [P, c_int, c_int64, P, c_int, c_int64, c_int, c_int, c_int, P]),
    "odhip_me_limits": (c_int, [c_int, c_int, c_int, c_int, c_int, P]),                 # int lim[4]
    "odhip_install_dct_vtbl": (None, [P, P]),                                            # function-pointer tables
    "od_pvq_search_rdo_double_hip": (c_double, [P, c_int, c_int, P, c_double, c_double, c_int]),
    "odhip_y4m_open2": (c_void_p, [P, c_int, P, P, P, P, P, P]),
    "odhip_copy_ceiling": (c_int, [c_size_t, c_int, c_int, P, P]),
    "odhip_pipe_export_release": (c_int, [P, c_long]),
    "odhip_cache_destroy": (None, [P]),
}


@pytest.mark.parametrize("name", sorted(PINNED))
def test_pinned_prototype(protos, name):
    assert protos[name] == PINNED[name]


@pytest.mark.parametrize("text", [
    "int odhip_x(float a);",
    "typedef struct { int a; } odhip_s;\nint odhip_x(odhip_s s);",
    "int odhip_x(struct odhip_s s);",
    "int odhip_x(int a, ...);",
    "float odhip_x(int a);",
    "int odhip_x(void (*cb)(int, long));",          # the header names its function-pointer types
    "#ifdef ODHIP_EXPERIMENTS\nint odhip_x(int a);\n#endif",
])
def test_parser_refuses_what_it_does_not_know(text):
    from daala_amd import _abi
    with pytest.raises(ValueError, match="odhip_x|ODHIP_EXPERIMENTS"):
        _abi.prototypes(text)


def test_parser_reads_a_small_header():
    from daala_amd import _abi
    text = """#ifndef X_H
    #define X_H
    #ifdef __cplusplus
    extern "C" {
    #endif
    /* int odhip_not_this(int a); */
    typedef struct odhip_t odhip_t;
    typedef void (*odhip_fn)(int *out, int n);
    typedef struct { int a; long b; } odhip_s;
    enum { ODHIP_A, ODHIP_B };
    odhip_t *odhip_make(void);
    void odhip_use(const odhip_t *t, const odhip_fn table[2], unsigned flags,
                   uint64_t n);
    #ifdef __cplusplus
    }
    #endif
    #endif"""
    from ctypes import c_uint, c_uint64
    assert _abi.prototypes(text) == {"odhip_make": (c_void_p, []), "odhip_use": (None, [P, P, c_uint, c_uint64])}


def test_calls_that_need_the_prototype(L):
    """Plain Python ints, no restype or argtypes set here."""
    # a long result above 2^32: ((w - 8) / 7 + 1) * ((h - 8) / 7 + 1) windows (metrics_kernels.hip)
    assert L.odhip_psnrhvs_window_count(700000, 700000, None, None) == 99999 * 99999
    # a by-value long above 2^32 whose low half is zero: cut to an int it is an empty batch (0), whole it
    # is a batch with null planes.  (No host-only entry point's result depends on a size_t that large:
    # odhip_copy_ceiling allocates it.)
    assert L.odhip_fdct2d_batch(0, None, None, 0, 0, None) == 0
    assert L.odhip_fdct2d_batch(0, None, None, 1 << 32, 0, None) == EINVAL
    with pytest.raises(TypeError):
        L.odhip_fdct2d_batch(0, None, None, 1, 0)                  # one argument too few
    with pytest.raises(ArgumentError):
        L.odhip_fdct2d_batch(0, None, None, c_size_t(1), 0, None)  # a size_t for a long
    assert b"gfx950" in L.odhip_version()


def test_bind_refuses_a_library_without_a_declared_function():
    import ctypes
    import daala_amd
    with pytest.raises(AttributeError, match="undefined symbol: od"):
        daala_amd.bind(ctypes.CDLL("libc.so.6"))
