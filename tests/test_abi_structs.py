"""CPU: the ctypes structs and integer constants daala_amd/_abi.py reads from include/daala_hip.h,
shim/daala_hip_glue.h and oracle/od_oracle.h - every struct's size and every field's offset against the host C
compiler, the numpy records made of them, what the reader refuses, what it reads, the constants, and the guard that
compares the loaded library's own sizeof answers with the header's structs."""
import ctypes
import os
import subprocess

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HEADERS = {"include/daala_hip.h": (28, 271), "shim/daala_hip_glue.h": (2, 29), "oracle/od_oracle.h": (2, 29)}


def _fields(cls):
    return [f[0] for f in cls._fields_]


def _c_name(field):
    """The header's spelling of a field: a Python keyword got one trailing underscore."""
    return field[:-1] if field.endswith("_") else field


@pytest.mark.parametrize("header", sorted(HEADERS))
def test_layouts_match_the_compiler(header, tmp_path):
    from daala_amd import _abi
    structs = _abi.structs(os.path.join(ROOT, header))
    lines = ["#include <stddef.h>", "#include <stdio.h>", '#include "%s"' % os.path.join(ROOT, header),
             "int main(void) {"]
    want = []
    for name, cls in structs.items():
        lines.append('printf("%s %%zu\\n", sizeof(%s));' % (name, name))
        want.append("%s %d" % (name, ctypes.sizeof(cls)))
        for f in _fields(cls):
            lines.append('printf("%s.%s %%zu %%zu\\n", offsetof(%s, %s), sizeof(((%s *)0)->%s));'
                         % (name, f, name, _c_name(f), name, _c_name(f)))
            want.append("%s.%s %d %d" % (name, f, getattr(cls, f).offset, getattr(cls, f).size))
    lines += ["return 0;", "}"]
    src, exe = tmp_path / "layout.c", tmp_path / "layout"
    src.write_text("\n".join(lines))
    # the host C compiler of oracle/Makefile
    subprocess.run([os.environ.get("CC", "gcc"), "-I", os.path.join(ROOT, "include"), "-o", str(exe), str(src)],
                   check=True)
    got = subprocess.run([str(exe)], check=True, capture_output=True, text=True).stdout.splitlines()
    assert got == want
    # nothing skipped: every struct and every field of the header was printed and compared
    nstructs = sum(1 for line in got if "." not in line.split()[0])
    assert (nstructs, len(got) - nstructs) == (len(structs), sum(len(c._fields_) for c in structs.values()))
    assert (nstructs, len(got) - nstructs) == HEADERS[header]


def test_one_class_per_struct():
    from daala_amd import _abi
    S = _abi.structs()
    assert _abi.structs() is S and S["odhip_me_job2"] is _abi.structs()["odhip_me_job2"]
    assert dict(S["odhip_me_job4"]._fields_)["base"] is S["odhip_me_job3"]          # nested by value: the same class
    assert dict(S["odhip_export_layout"]._fields_)["section"]._type_ is S["odhip_export_section"]
    assert list(S)[:3] == ["odhip_quant", "odhip_pvq_band", "odhip_pvq_cands"]         # declaration order
    assert "lambda_" in _fields(S["odhip_me_job"]) and "lambda" not in _fields(S["odhip_me_job"])
    # every pointer, and every array of pointers, is a c_void_p
    assert dict(S["odhip_pvq_job"]._fields_)["q_band"] is ctypes.c_void_p
    assert dict(S["odhip_band_cands"]._fields_)["y"] is ctypes.c_void_p * 2


RECORDS = {"BAND_RECORD": "odhip_pvq_band", "REFPREP_RECORD": "odhip_pvq_refprep", "REFCAND_RECORD": "odhip_pvq_refcand",
           "REFBAND_RECORD": "odhip_pvq_refband", "REFITEM_RECORD": "odhip_pvq_refitem", "MV_POINT": "odhip_mv_point",
           "ME_CAND": "odhip_me_cand"}


@pytest.mark.parametrize("record", sorted(RECORDS))
def test_numpy_records(record):
    from daala_amd import _abi, api
    cls, dt = _abi.structs()[RECORDS[record]], getattr(api, record)
    assert dt == np.dtype(cls) and dt.itemsize == ctypes.sizeof(cls)
    assert list(dt.names) == _fields(cls)
    for f in dt.names:
        assert dt.fields[f][1] == getattr(cls, f).offset and dt.fields[f][0].itemsize == getattr(cls, f).size, f


REFUSED = {
    "bit-field": ("typedef struct { int a; unsigned flags : 3; } odhip_s;", "flags"),
    "union": ("typedef struct { union { int a; double b; } u; } odhip_s;", "union"),
    "union typedef": ("typedef union { int a; double b; } odhip_s;", "union"),
    "anonymous nested struct": ("typedef struct { int a; struct { int b; } in; } odhip_s;", "struct { int b"),
    "function-pointer field": ("typedef struct { void (*cb)(int a, long b); } odhip_s;", "cb"),
    "unknown type": ("typedef struct { float a; } odhip_s;", "float"),
    "use before declaration": ("typedef struct { odhip_t t; } odhip_s;\ntypedef struct { int a; } odhip_t;", "odhip_t"),
    "undefined macro": ("typedef struct { int a[2*ODHIP_N]; } odhip_s;", "ODHIP_N"),
    "under #if": ("#if ODHIP_WIDE\ntypedef struct { long a; } odhip_s;\n#endif", "ODHIP_WIDE"),
    "packing pragma": ("#pragma pack(push, 1)\ntypedef struct { char a; } odhip_s;", "pragma"),
    "attribute": ("typedef struct { int a; } __attribute__((packed)) odhip_s;", "packed"),
    "no typedef": ("struct odhip_s { int a; };", "odhip_s"),
}


@pytest.mark.parametrize("what", sorted(REFUSED))
def test_reader_refuses_what_it_does_not_know(what, tmp_path):
    from daala_amd import _abi
    text, named = REFUSED[what]
    path = tmp_path / "refused.h"
    path.write_text(text)
    with pytest.raises(ValueError) as e:
        _abi.structs(str(path))
    assert named in str(e.value) and "refused.h" in str(e.value)


def test_reader_reads_a_small_header(tmp_path):
    from daala_amd import _abi
    path = tmp_path / "small.h"
    path.write_text("""#ifndef SMALL_H
    #define SMALL_H
    #include <stdint.h>
    #ifdef __cplusplus
    extern "C" {
    #endif
    #define ODHIP_ROWS 3        /* a comment */
    #define ODHIP_COLS (ODHIP_ROWS + 1)
    #define ODHIP_FLAG (1 << 4)
    #define ODHIP_MINUS (-10)
    #define ODHIP_HEX 0x1ff
    #define ODHIP_SCALE 0.5
    #define ODHIP_NAME "name"
    #define ODHIP_WORDS(fn) ((fn) & 0x1ff)
    typedef int32_t odhip_coeff;
    typedef struct odhip_opaque odhip_opaque;
    typedef void (*odhip_fn)(int *out, int n);
    typedef struct { int16_t x, y[2], *p; } odhip_point;
    typedef struct odhip_grid_s {
      odhip_coeff cell[ODHIP_ROWS][2*ODHIP_COLS];  /* a 2-D array, a macro product */
      odhip_point origin;                          /* an earlier struct by value */
      const struct odhip_grid_s *next;
      const uint8_t *plane[ODHIP_ROWS];            /* an array of pointers */
      int32_t lambda;
      size_t bytes;
    } odhip_grid;
    int odhip_use(const odhip_grid *g);
    #ifdef __cplusplus
    }
    #endif
    #endif""")
    S = _abi.structs(str(path))
    assert list(S) == ["odhip_point", "odhip_grid"]
    vp = ctypes.c_void_p
    assert S["odhip_point"]._fields_ == [("x", ctypes.c_int16), ("y", ctypes.c_int16 * 2), ("p", vp)]
    assert S["odhip_grid"]._fields_ == [("cell", (ctypes.c_int32 * 8) * 3), ("origin", S["odhip_point"]), ("next", vp),
                                        ("plane", vp * 3), ("lambda_", ctypes.c_int32), ("bytes", ctypes.c_size_t)]
    assert _abi.constants(str(path)) == {"ODHIP_ROWS": 3, "ODHIP_COLS": 4, "ODHIP_FLAG": 16, "ODHIP_MINUS": -10,
                                         "ODHIP_HEX": 511}


def test_constants_of_the_header():
    from daala_amd import _abi, api, quant
    C = _abi.constants()
    want = {"ODHIP_EINVAL": -10, "ODHIP_EIMPL": -23, "ODHIP_ERANGE": -24, "ODHIP_EBUSY": -101, "ODHIP_NBSIZES": 5,
            "ODHIP_QM_SIZE": 30, "ODHIP_QM_BUFFER_SIZE": 10912, "ODHIP_BSIZE_TERMS": 90, "ODHIP_PVQ_MAX_REFCANDS": 24,
            "ODHIP_PVQ_REF_SLOTS": 16, "ODHIP_REFBAND_UNCERTAIN": 16, "ODHIP_REFITEM_K_RANGE": 4,
            "ODHIP_REFITEM_MOMENT_SHIFT": 8, "ODHIP_Y4M_ALLOW_444": 1, "ODHIP_EXPORT_MAX_SECTIONS": 16,
            "ODHIP_METRIC_PSNRHVS": 2, "ODHIP_METRIC_SSIM": 4, "ODHIP_METRIC_MSSSIM": 8, "ODHIP_METRIC_FASTSSIM": 16,
            "ODHIP_METRIC_CIEDE": 32, "ODHIP_SAMPLE_I16_12": 2, "ODHIP_CSF_CR": 2, "ODHIP_SSIM_MAX_RADIUS": 64,
            "ODHIP_MSSSIM_SCALES": 5, "ODHIP_MSSSIM_MIN_SIZE": 16, "ODHIP_FASTSSIM_LEVELS": 4, "ODHIP_ME_CHROMA": 1,
            "ODHIP_ME_SATD": 2}
    assert {k: C.get(k) for k in want} == want
    # defines that are no integer constant: function-like macros, the include guard
    assert not {"ODHIP_EXPORT_NWORDS", "ODHIP_EXPORT_NOREF", "ODHIP_EXPORT_SKIP", "DAALA_HIP_H"} & set(C)
    assert all(isinstance(v, int) for v in C.values())
    # the Python names take these values
    assert (api.ERANGE, api.EBUSY, api.METRIC_CIEDE, api.REF_SLOTS, api.MAX_REFCANDS, api.NBSIZES, api.BSIZE_TERMS,
            api.ME_SATD, quant.QM_SIZE, quant.QM_BUFFER_SIZE) == (-24, -101, 32, 16, 24, 5, 90, 2, 30, 10912)


@pytest.mark.parametrize("expr, value", [("2*5*4", 40), ("14*7", 98), ("(1 << 5)", 32), ("-(3 + 2)*2 - 1", -11),
                                         ("0x10 << 1 + 1", 64), ("A*(B - 1)", 6)])
def test_constant_expressions(expr, value):
    from daala_amd import _abi
    assert _abi._eval(expr, {"A": 3, "B": 3}) == value


@pytest.mark.parametrize("expr", ["", "1 2", "(1", "1 +", "C", "1.5", "010", "sizeof(int)", "4/2", "__import__('os')"])
def test_constant_expressions_refused(expr):
    from daala_amd import _abi
    with pytest.raises(ValueError):
        _abi._eval(expr, {"A": 3})


def test_layout_guard():
    """lib() compares every odhip_*_sizeof answer of the library with the header's struct, once; a library compiled
    against another layout is refused by name, with both sizes."""
    from daala_amd import _abi, api
    S = _abi.structs()
    assert set(api._LAYOUT_GUARD.values()) == {"odhip_me_job", "odhip_me_cand", "odhip_me_job2", "odhip_me_job3",
                                               "odhip_me_job4", "odhip_mv_point", "odhip_mc_job", "odhip_haar_job"}

    class Fake:
        """A library that answers as the header does, but for one struct."""
        def __init__(self, wrong=None):
            self.wrong = wrong

        def __getattr__(self, fn):
            def sizeof(*index):
                name = api._LAYOUT_GUARD[(fn, index[0] if index else None)]
                return ctypes.sizeof(S[name]) + (8 if name == self.wrong else 0)
            return sizeof

    fake = Fake()
    assert api._check_layouts(fake) is fake
    for name in sorted(set(api._LAYOUT_GUARD.values())):
        with pytest.raises(api.DaalaHipError, match=r"%s is %d bytes .* %d bytes" % (
                name, ctypes.sizeof(S[name]) + 8, ctypes.sizeof(S[name]))):
            api._check_layouts(Fake(name))
    assert api._check_layouts(api.lib()) is api.lib()       # the real library agrees
