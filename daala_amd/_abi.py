"""ctypes prototypes of the C ABI, read from include/daala_hip.h (the declared boundary, DESIGN.md par. 1), so that a
`long`, a `size_t`, a `double` or a handle passes at its full width and a missing argument or a scalar of the wrong
ctypes type raises.  The mapping is deliberately plain: scalars by name, every pointer or array c_void_p (callers pass
byref(), arrays, numpy .ctypes, data_ptr() ints, bytes or None).  What it does not know it refuses, naming the
declaration."""
import ctypes
import os
import re

HEADER = os.path.join(os.path.dirname(os.path.abspath(__file__)), "..", "include", "daala_hip.h")
_SCALARS = {
    "int": ctypes.c_int, "long": ctypes.c_long, "size_t": ctypes.c_size_t, "double": ctypes.c_double,
    "int32_t": ctypes.c_int32, "int64_t": ctypes.c_int64, "unsigned": ctypes.c_uint, "uint32_t": ctypes.c_uint32,
    "uint64_t": ctypes.c_uint64, "odhip_stream": ctypes.c_void_p,
}


def _scalar(words, decl):
    """The ctypes type of a by-value type spelled `words` (a parameter's name, if any, already removed)."""
    t = " ".join(w for w in words if w != "const")
    if t not in _SCALARS:
        raise ValueError("daala_hip.h: no ctypes type for `%s` in `%s`" % (t, decl))
    return _SCALARS[t]


def prototypes(text=None):
    """{name: (restype, [argtypes])} of every function `text` (default: the header) declares."""
    if text is None:
        with open(HEADER) as f:
            text = f.read()
    text = re.sub(r"/\*.*?\*/|\\\n", " ", text, flags=re.S)
    # read as C: the C++ guards go; the include guard is the one other conditional a declaration may stand in
    text = re.sub(r"#ifdef __cplusplus\b.*?#endif", " ", text, flags=re.S)
    text = re.sub(r"\A\s*#ifndef (\w+)\s*#define \1\b", " ", text)
    cond = re.search(r"^[ \t]*#[ \t]*(if|el).*", text, flags=re.M)
    if cond:
        raise ValueError("daala_hip.h: a declaration under `%s` would be bound or skipped by accident"
                         % cond.group().strip())
    text = re.sub(r"^[ \t]*#.*", " ", text, flags=re.M)
    n = 1
    while n:                    # struct / enum bodies, innermost first
        text, n = re.subn(r"\{[^{}]*\}", " ", text)
    protos = {}
    for decl in (" ".join(s.split()) for s in text.split(";")):
        if "(" not in decl or decl.startswith("typedef"):
            continue            # typedefs, forward declarations, what is left of a struct / enum
        m = re.fullmatch(r"([^()]+?) ?(\w+) ?\(([^()]*)\)", decl)
        if not m:               # function-pointer parameters included: the header uses typedefs for them
            raise ValueError("daala_hip.h: cannot parse `%s`" % decl)
        ret, name, params = m.groups()
        if "*" in ret:
            res = ctypes.c_char_p if ret.replace(" ", "") == "constchar*" else ctypes.c_void_p
        else:
            res = None if ret == "void" else _scalar(ret.split(), decl)
        args = []
        for p in [] if params.strip() in ("", "void") else params.split(","):
            words = p.split()
            if len(words) > 1 and words[-1] not in _SCALARS and words[-2] not in ("struct", "enum", "union"):
                words.pop()     # the parameter's name
            args.append(ctypes.c_void_p if "*" in p or "[" in p else _scalar(words, decl))
        protos[name] = (res, args)
    return protos


_PROTOS = {}


def bind(L):
    """Set restype and argtypes of every declared function on the loaded library L and return it.  A declared function
    that L does not export raises: ctypes' AttributeError names the symbol."""
    if not _PROTOS:
        _PROTOS.update(prototypes())
    for name, (res, args) in _PROTOS.items():
        fn = getattr(L, name)
        fn.restype, fn.argtypes = res, args
    return L
