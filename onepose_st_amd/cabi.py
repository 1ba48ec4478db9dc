"""Reader of the project's C headers (``include/onepose_hip.h``, ``include/onepose_pnp.h``, ``include/onepose_sfm.h``,
``include/onepose_sfm_tracks.h``, ``include/onepose_sfm_triangulate.h``, ``include/onepose_sfm_fine.h``,
``include/onepose_pnp_device.h``, ``include/onepose_track.h``) and the one rule that turns a C type
into a ctypes class.  The headers are the only place a C signature is written; ``hip.py`` and ``pnp.py`` bind from what this reads.

Not a C parser: it reads the regular subset those headers use and raises ``HeaderError`` (with the line) on anything else that looks
like an entry point.  Standard library only."""
from __future__ import annotations

import ctypes
import itertools
import re
from collections import namedtuple

SCALARS = {"int": ctypes.c_int, "unsigned": ctypes.c_uint, "long long": ctypes.c_longlong, "unsigned long long": ctypes.c_ulonglong,
           "float": ctypes.c_float, "double": ctypes.c_double, "size_t": ctypes.c_size_t}
RETURN_TYPES = (*SCALARS, "const char*", "void", "void*")
_POINTEES = (*SCALARS, "char", "unsigned char", "void")
_NAME = r"\b(?:ophip|oppnp|oppnpd|opsfm|opsft|opstr|opsff|optrk)_\w+"


class HeaderError(ValueError):
    pass


Prototype = namedtuple("Prototype", "name ret params")           # params: ((C type, parameter name), ...)
# prototypes: name -> Prototype in header order; defines: NAME -> int for every ``#define NAME <integer literal>``;
# structs: typedef name -> ((C type, field name, array length or None), ...)
Header = namedtuple("Header", "prototypes defines structs")


def _type(text: str) -> str:
    """``const  float *`` -> ``const float*``"""
    return re.sub(r"\s*\*", "*", " ".join(text.split()))


def _bare(ctype: str) -> str:
    return re.sub(r"\bconst\b", "", ctype).strip()


def _declarator(text: str, where: str, structs=()) -> tuple:
    """``const void* w_coarse[16]`` -> (``const void*``, ``w_coarse``, 16)"""
    m = re.fullmatch(r"\s*(.*?)(\w+)\s*(?:\[\s*(\d+)\s*\])?\s*", text, re.S)
    ctype = _type(m.group(1)) if m else ""
    bare = _bare(ctype)
    if bare not in SCALARS and not (bare.endswith("*") and bare.rstrip("*") in (*_POINTEES, *structs)):
        raise HeaderError(f"{where}: cannot read {' '.join(text.split())!r}")
    return ctype, m.group(2), int(m.group(3)) if m.group(3) else None


def parse(text: str) -> Header:
    text = re.sub(r"/\*.*?\*/", lambda m: "\n" * m.group().count("\n"), text, flags=re.S)      # comments go, line numbers stay
    text = re.sub(r"//[^\n]*", "", text)

    def line(pos):
        return f"line {text.count(chr(10), 0, pos) + 1}"

    defines = {n: int(v, 0) for n, v in re.findall(r"^[ \t]*#[ \t]*define[ \t]+(\w+)[ \t]+(0[xX][0-9a-fA-F]+|\d+)[ \t]*$", text, re.M)}
    structs = {}
    for m in re.finditer(r"\btypedef\s+struct\s*\w*\s*\{([^{}]*)\}\s*(\w+)\s*;", text):
        fields = []
        for decl in filter(str.strip, m.group(1).split(";")):
            first, *more = decl.split(",")
            ctype, name, length = _declarator(first, f"{line(m.start())}, struct {m.group(2)}", structs)
            fields.append((ctype, name, length))
            for d in more:          # ``int B, N, M;``: the stars of the first declarator are its own
                fields.append(_declarator(ctype.rstrip("*") + " " + d, f"{line(m.start())}, struct {m.group(2)}", structs))
        structs[m.group(2)] = tuple(fields)
    text = re.sub(r"^[ \t]*#.*$", "", text, flags=re.M)
    prototypes, read_at = {}, set()
    for m in re.finditer(rf"(?:\A|(?<=[;{{}}]))\s*([\w\s*]+?)\s*({_NAME})\s*\(", text):
        where, ret = f"{line(m.start(2))}, {m.group(2)}", _type(m.group(1))
        end = re.compile(r"([^();{}]*)\)\s*;").match(text, m.end())
        if ret not in RETURN_TYPES or end is None:
            raise HeaderError(f"{where}: not a prototype this reader knows (return types: {', '.join(RETURN_TYPES)})")
        params = end.group(1).strip()
        prototypes[m.group(2)] = Prototype(m.group(2), ret, tuple(
            _declarator(p, where, structs)[:2] for p in ([] if params in ("", "void") else params.split(","))))
        read_at.add(m.start(2))
    for m in re.finditer(rf"({_NAME})\s*\(", text):          # nothing that looks like an entry point may be left out silently
        if m.start() not in read_at:
            raise HeaderError(f"{line(m.start())}, {m.group(1)}: declared in a form this reader does not know")
    return Header(prototypes, defines, structs)


def ctype(c: str, mirrors: dict | None = None, ret: bool = False):
    """The rule: scalars one to one; ``char*`` -> ``c_char_p``; a pointer to a mirrored structure -> ``POINTER(mirror)``; ``void**`` ->
    ``POINTER(c_void_p)``; every other pointer -> ``c_void_p``; as a return type ``void`` -> ``None``."""
    c = _bare(c)
    if c in SCALARS:
        return SCALARS[c]
    if c == "void" and ret:
        return None
    if c == "char*":
        return ctypes.c_char_p
    if c == "void**":
        return ctypes.POINTER(ctypes.c_void_p)
    if c.endswith("*"):
        return ctypes.POINTER(mirrors[c[:-1]]) if mirrors and c[:-1] in mirrors else ctypes.c_void_p
    raise HeaderError(f"no ctypes class for {c!r}")


def signature(proto, mirrors: dict | None = None) -> tuple:
    """-> (restype, argtypes)"""
    return ctype(proto.ret, mirrors, ret=True), [ctype(t, mirrors) for t, _ in proto.params]


def check_mirror(mirror, struct_name: str, fields: tuple):
    """A hand-written ``ctypes.Structure`` against the header's fields: names in order, type class of each, array lengths."""
    def key(name, cls, length=None):
        return (name, cls._type_, cls._length_) if issubclass(cls, ctypes.Array) else (name, cls, length)
    want = [key(name, ctype(c), length) for c, name, length in fields]
    got = [key(*f) for f in mirror._fields_]
    for k, (w, g) in enumerate(itertools.zip_longest(want, got)):
        if w != g:
            raise HeaderError(f"{struct_name}.{(w or g)[0]}: field {k} is {w and w[1:]} in the header, {g and g[1:]} in {mirror.__name__}")
