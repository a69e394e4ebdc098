"""include/sqair_hip.h, parsed: the header is the one statement of the C ABI, and the ctypes binding (sqair_amd/_capi.py) is made
from what this module reads in it.  Standard library only: no torch, no library, no GPU.

The header keeps to a small C subset, and the parser is strict about it: ``/* */`` comments, preprocessor lines (a ``#define
SQAIR_*`` with a value must be an integer literal), the ``extern "C"`` guard, ``typedef struct [Tag] { ... } Name;``, the opaque
``typedef struct Tag Tag;``, and prototypes.  Declarations take the base types of ``_SCALARS``, ``void`` and earlier structs,
``const``, ``*`` up to depth 2, several declarators per line, fixed arrays and nested struct values.  Anything else -- a bit-field, a
union, an enum, a function pointer, an unknown type name -- raises ``HeaderError`` naming the text, so an edit of the header that
leaves the subset fails at import and is never skipped."""
from __future__ import annotations

import collections
import ctypes
import functools
import os
import re

HEADER_PATH = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "include", "sqair_hip.h")

# ``const``: of the base type; ``pointer_const``: the pointer levels that are const themselves, (0,) in ``const float* const* p``
Field = collections.namedtuple("Field", "name base const pointer_depth array_len pointer_const", defaults=((),))
Param = collections.namedtuple("Param", "name base const pointer_depth pointer_const", defaults=((),))
Header = collections.namedtuple("Header", "constants structs functions")   # functions: name -> (return type as a Param, [Param])

_SCALARS = {"int": ctypes.c_int, "int32_t": ctypes.c_int32, "int64_t": ctypes.c_int64, "uint32_t": ctypes.c_uint32,
            "uint64_t": ctypes.c_uint64, "float": ctypes.c_float, "double": ctypes.c_double, "char": ctypes.c_char}
_DTYPES = {"float": "float32", "int32_t": "int32", "int64_t": "int64", "double": "float64"}
_TYPE = r"(const\s+)?(\w+)\s*((?:\*\s*(?:const\b\s*)?)*)"   # [const] base, then the '*'s, each of them const or not
_DECLARATION = re.compile(r"\s*" + _TYPE + r"(\w+)\s*(?:\[\s*(\d+)\s*\])?\s*$")
_DECLARATOR = re.compile(r"\s*(\w+)\s*(?:\[\s*(\d+)\s*\])?\s*$")
_SPACE = re.compile(r"\s*")
_OPAQUE = re.compile(r"typedef\s+struct\s+(\w+)\s+(\w+)\s*;")
_STRUCT = re.compile(r"typedef\s+struct\s*(\w*)\s*\{([^{}]*)\}\s*(\w+)\s*;")
_FUNCTION = re.compile(_TYPE + r"(\w+)\s*\(([^(){};]*)\)\s*;")


class HeaderError(ValueError):
    """The header holds something outside the subset the binding is read from."""


def parse_header(path):
    """``Header(constants, structs, functions)`` of the header at ``path``: {name: int} of every ``#define SQAIR_* <integer>[u]``;
    in declaration order name -> [Field] per struct and name -> (return type, [Param]) per function."""
    constants, structs, functions, opaque = {}, {}, {}, set()

    def bad(what):
        raise HeaderError("{}: outside the C subset the binding is read from: {!r}".format(path, " ".join(what.split())))
    with open(path) as f:
        text, *commented = f.read().split("/*")
    for c in commented:   # (plain string work: a regex over the header's prose is the slow part of an import)
        if "*/" not in c:
            bad("/*" + c[:200])
        text += " " + c.partition("*/")[2]

    def directive(m):
        define = re.match(r"\s*#\s*define\s+(SQAIR_\w+)(.*)", m.group(0))
        if define and define.group(2).strip():   # (the include guard has no value)
            value = re.fullmatch(r"(\d+)[uU]?", define.group(2).strip())
            if not value:
                bad(m.group(0))
            constants[define.group(1)] = int(value.group(1))
        return ""
    text = re.sub(r"^[ \t]*#.*$", directive, text, flags=re.M)
    text, closers = re.subn(r'extern\s+"C"\s*\{', "", text)

    def declared(text, const, base, stars):
        """(const, depth, const pointer levels) of a declaration's type, checked against what has been declared so far."""
        levels = ["const" in level for level in stars.split("*")[1:]]
        if len(levels) > 2 or not (base in _SCALARS or base in structs or (levels and (base == "void" or base in opaque))):
            bad(text)
        return bool(const), len(levels), tuple(i for i, c in enumerate(levels) if c)

    def fields(body):
        *lines, rest = body.split(";")
        if rest.strip():
            bad(rest)
        for line in lines:
            first, *more = line.split(",")
            m = _DECLARATION.match(first)
            if not m or (more and m.group(3)):   # (``int *a, b`` reads two ways: not in the subset)
                bad(line)
            const, depth, pconst = declared(line, *m.group(1, 2, 3))
            for name, n in [m.group(4, 5)] + [(_DECLARATOR.match(d) or bad(line)).groups() for d in more]:
                yield Field(name, m.group(2), const, depth, int(n) if n else None, pconst)

    def params(text):
        if text.strip() == "void":
            return
        for p in text.split(","):
            m = _DECLARATION.match(p)
            if not m or m.group(5):
                bad(p)
            yield Param(m.group(4), m.group(2), *declared(p, *m.group(1, 2, 3)))

    pos = 0
    while True:
        pos = _SPACE.match(text, pos).end()
        if pos == len(text):
            return Header(constants, structs, functions)
        if text[pos] == "}" and closers:   # the guard's closing brace
            closers, pos = closers - 1, pos + 1
            continue
        for kind in (_OPAQUE, _STRUCT, _FUNCTION):
            m = kind.match(text, pos)
            if m:
                break
        else:
            bad(text[pos:].split(";")[0][:200])
        if kind is _OPAQUE:
            if m.group(1) != m.group(2):
                bad(m.group(0))
            opaque.add(m.group(2))
        elif kind is _STRUCT:
            structs[m.group(3)] = list(fields(m.group(2)))
        else:
            ret = Param("", m.group(2), *declared(m.group(0), *m.group(1, 2, 3)))
            if ret.pointer_depth > 1 or not (ret.pointer_depth or ret.base in _SCALARS):
                bad(m.group(0))
            functions[m.group(4)] = (ret, list(params(m.group(5))))
        pos = m.end()


def spell(t):
    """The type of a Field or Param as C spells it: ``const float* const*``."""
    return ("const " if t.const else "") + t.base + "".join("* const" if i in t.pointer_const else "*" for i in range(t.pointer_depth))


@functools.lru_cache(maxsize=None)
def header():
    """The parse of the header beside the package, once per process."""
    try:
        return parse_header(HEADER_PATH)
    except OSError as e:
        raise ImportError("{}: the ctypes binding of libsqair_hip*.so is read from the C header, and the header ships with the "
                          "library (include/ beside the package, as in the source tree): {}".format(HEADER_PATH, e))


def bind(hdr, addresses=()):
    """The ctypes form of a parse: ({struct: Structure class}, {function: (restype, argtypes)}).  A scalar has its fixed-width type; a
    pointer to a struct of the header is POINTER(that struct) -- but as a field not for the (struct, field) pairs of ``addresses`` --, a
    ``char*`` argument or return c_char_p, and every other pointer c_void_p: a device address or an opaque handle, passed as an
    integer."""
    classes = {}

    def of(struct, t, param=True):
        if t.pointer_depth == 1 and t.base in classes and (struct, t.name) not in addresses:
            return ctypes.POINTER(classes[t.base])
        if t.pointer_depth:
            return ctypes.c_char_p if param and t.pointer_depth == 1 and t.base == "char" else ctypes.c_void_p
        return _SCALARS.get(t.base) or classes[t.base]
    for name, fields in hdr.structs.items():
        types = [(f.name, of(name, f, False) * f.array_len if f.array_len else of(name, f, False)) for f in fields]
        classes[name] = type(name, (ctypes.Structure,), {"_fields_": types, "__doc__": "include/sqair_hip.h: " + name})
    return classes, {name: (of(None, ret), [of(None, p) for p in ps]) for name, (ret, ps) in hdr.functions.items()}


def field_dtype(owner, name):
    """The element type (\"float32\", \"int32\", \"int64\", \"float64\") of the pointer field ``name`` of the struct ``owner``, or of the
    pointer parameter ``name`` of the function ``owner``: what a buffer handed over through it is allocated as."""
    hdr = header()
    t, = [t for t in (hdr.structs.get(owner) or hdr.functions[owner][1]) if t.name == name]
    if t.pointer_depth != 1 or t.base not in _DTYPES:
        raise KeyError("{}.{} is a {}: no array of a device element type".format(owner, name, spell(t)))
    return _DTYPES[t.base]
