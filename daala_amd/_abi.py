"""The C ABI as ctypes, read from include/daala_hip.h (the declared boundary, DESIGN.md par. 1): prototypes() for every
function, structs() for every `typedef struct`, constants() for every integer `#define`, so that a `long`, a `size_t`,
a `double` or a handle passes at its full width, a struct field sits where the compiler puts it, and a missing argument
or a scalar of the wrong ctypes type raises.  The mapping is deliberately plain: scalars by name, every pointer or array
parameter and every pointer field c_void_p (callers pass byref(), arrays, numpy .ctypes, data_ptr() ints, bytes or
None; a c_void_p field keeps nothing alive, its owner does), array fields as ctypes arrays, earlier structs by value.
The grammar is what the project's headers use; what it does not know it refuses, naming the declaration."""
import ctypes
import functools
import keyword
import os
import re

HEADER = os.path.join(os.path.dirname(os.path.abspath(__file__)), "..", "include", "daala_hip.h")
_SCALARS = {
    "int": ctypes.c_int, "long": ctypes.c_long, "size_t": ctypes.c_size_t, "double": ctypes.c_double,
    "int32_t": ctypes.c_int32, "int64_t": ctypes.c_int64, "unsigned": ctypes.c_uint, "uint32_t": ctypes.c_uint32,
    "uint64_t": ctypes.c_uint64, "odhip_stream": ctypes.c_void_p,
    "int8_t": ctypes.c_int8, "uint8_t": ctypes.c_uint8, "int16_t": ctypes.c_int16, "uint16_t": ctypes.c_uint16,
}


def _scalar(words, decl, types=_SCALARS, hdr="daala_hip.h"):
    """The ctypes type of a by-value type spelled `words` (a parameter's name, if any, already removed)."""
    t = " ".join(w for w in words if w != "const")
    if t not in types:
        raise ValueError("%s: no ctypes type for `%s` in `%s`" % (hdr, t, decl))
    return types[t]


def _front(text, hdr="daala_hip.h"):
    """`text` read as C with its comments and line splices gone, the C++ guards and the include guard removed and
    any other conditional refused; the other directives are still in it."""
    text = re.sub(r"/\*.*?\*/|\\\n", " ", text, flags=re.S)
    # read as C: the C++ guards go; the include guard is the one other conditional a declaration may stand in
    text = re.sub(r"#ifdef __cplusplus\b.*?#endif", " ", text, flags=re.S)
    text = re.sub(r"\A\s*#ifndef (\w+)\s*#define \1\b", " ", text)
    cond = re.search(r"^[ \t]*#[ \t]*(if|el).*", text, flags=re.M)
    if cond:
        raise ValueError("%s: a declaration under `%s` would be bound or skipped by accident"
                         % (hdr, cond.group().strip()))
    return text


def prototypes(text=None):
    """{name: (restype, [argtypes])} of every function `text` (default: the header) declares."""
    if text is None:
        with open(HEADER) as f:
            text = f.read()
    text = re.sub(r"^[ \t]*#.*", " ", _front(text), flags=re.M)
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


def _eval(expr, names):
    """The value of an integer constant expression over literals, `* + - << ( )` and `names`; ValueError otherwise."""
    toks = re.findall(r"0[xX][0-9a-fA-F]+|\w+|<<|\S", expr)[::-1]
    ops = [{"<<": int.__lshift__}, {"+": int.__add__, "-": int.__sub__}, {"*": int.__mul__}]    # loosest first

    def level(i):
        if i < len(ops):
            v = level(i + 1)
            while toks and toks[-1] in ops[i]:
                v = ops[i][toks.pop()](v, level(i + 1))
            return v
        t = toks.pop() if toks else ""
        if t in ("-", "+"):
            return -level(i) if t == "-" else level(i)
        if t == "(":
            v = level(0)
            if toks and toks.pop() == ")":
                return v
        elif t in names:
            return names[t]
        elif re.fullmatch(r"0[xX][0-9a-fA-F]+|0|[1-9][0-9]*", t):
            return int(t, 0)
        raise ValueError(expr)

    v = level(0)
    if toks:
        raise ValueError(expr)
    return v


_ITEM = (r"^[ \t]*#[ \t]*(\w+)[ \t]*(.*)$"                                               # a directive
         r"|\btypedef\b([^;{]*)(?:\{((?:[^{}]|\{[^{}]*\})*)\}([^;{}]*))?;"                # a typedef, with a body or not
         r"|\b(?:struct|union)\b[^;{()]*\{")                                              # a body without a typedef
_FIELD = r"([\w ]*?\w)\s*((?:\*[\s*]*)?\w+\s*(?:\[[^\[\]]*\]\s*)*)"                        # type, first declarator
_DECLARATOR = r"\s*([\s*]*)(\w+)\s*((?:\[[^\[\]]*\]\s*)*)"


def _struct(name, body, types, consts, hdr):
    """The ctypes class of `typedef struct { body } name;`."""
    fields = []
    for field in (" ".join(s.split()) for s in body.split(";")):
        if not field:
            continue
        first, *more = field.split(",")
        t = re.fullmatch(_FIELD, first)
        decls = [re.fullmatch(_DECLARATOR, d) for d in ([t.group(2)] + more if t else [])]
        if not t or None in decls:      # bit-fields, function pointers, nested bodies, attributes
            raise ValueError("%s: cannot parse the field `%s` of `%s`" % (hdr, field, name))
        for stars, fname, dims in (d.groups() for d in decls):
            ft = ctypes.c_void_p if stars else _scalar(t.group(1).split(), field, types, hdr)
            for dim in reversed(re.findall(r"\[([^\[\]]*)\]", dims)):
                try:
                    ft = ft * _eval(dim, consts)
                except ValueError:
                    raise ValueError("%s: no value for the dimension `%s` of `%s` in `%s`"
                                     % (hdr, dim, field, name)) from None
            fields.append((fname + "_" if keyword.iskeyword(fname) else fname, ft))
    return type(name, (ctypes.Structure,), {"_fields_": fields})


@functools.lru_cache(maxsize=None)
def _read(path):
    """(structs, constants) of the header at `path`, read once: the same class objects at every later call."""
    hdr = os.path.basename(path)
    with open(path) as f:
        text = _front(f.read(), hdr)
    types, structs, consts = dict(_SCALARS), {}, {}
    for m in re.finditer(_ITEM, text, flags=re.M):
        decl = " ".join(m.group().split())
        directive, rest, head, body, name = m.groups()
        if directive == "define":
            d = re.fullmatch(r"(\w+)\s+(\S.*)", rest)
            try:                # object-like defines with an integer value; the others are not constants
                consts[d.group(1)] = _eval(d.group(2), consts)
            except (AttributeError, ValueError):
                pass
        elif directive and directive not in ("include", "endif"):
            raise ValueError("%s: `%s` may change a layout" % (hdr, decl))
        elif body is not None:
            name = name.strip()
            if not re.fullmatch(r"\s*struct(\s+\w+)?\s*", head) or not name.isidentifier():
                raise ValueError("%s: `%s` is not `typedef struct [tag] { fields } name;`" % (hdr, decl))
            types[name] = structs[name] = _struct(name, body, types, consts, hdr)
        elif head is not None:
            words = head.split()
            if len(words) == 2 and words[0] in types and words[1].isidentifier():
                types[words[1]] = types[words[0]]           # typedef <scalar> name;
        elif not directive:
            raise ValueError("%s: `%s ...` is not `typedef struct [tag] { fields } name;`" % (hdr, decl))
    return structs, consts


def structs(path=None):
    """{typedef name: ctypes.Structure subclass} of every `typedef struct` of the header, in declaration order.  A
    field named like a Python keyword gets one trailing underscore (`lambda_`)."""
    return _read(os.path.abspath(path or HEADER))[0]


def constants(path=None):
    """{name: int} of every `#define` of the header whose value is an integer constant expression."""
    return _read(os.path.abspath(path or HEADER))[1]


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
