"""Reader of the project's C headers (``include/onepose_*.h``: one per entry of ``LIBRARIES`` below, plus ``onepose_pnp.h`` of the host
library), the one rule that turns a C type into a ctypes class, and ``Binding``: the header, the signatures, the constants and the loaded
handle of one HIP library.  The headers are the only place a C signature or a constant is written; the modules ``LIBRARIES`` names and
``pnp.py`` bind from what this reads.  Every HIP library is an entry of ``LIBRARIES`` or, with its header under ``include/ext/``, of
``EXTENSIONS``, ``ADDONS``, ``TRAINING``, ``BACKWARD`` or ``ENCODER_BACKWARD``; the host library alone keeps a loader of its own (``pnp.py``).

Not a C parser: it reads the regular subset those headers use and raises ``HeaderError`` (with the line) on anything else that looks
like an entry point.  Standard library only."""
from __future__ import annotations

import ctypes
import itertools
import os
import re
from collections import namedtuple

# The HIP libraries, one line each: C prefix, header under include/, file under onepose_st_amd/lib/, the environment variable that names
# another build of it (A/B runs), the module that binds it (``Binding.of(__name__)``).  __graft_entry__.build() checks and loads every
# entry, the reader below knows an entry point by these prefixes (and the host library's ``oppnp``), tests/test_cabi_binding.py runs over
# every entry, and DESIGN.md section 1b says what else a new one needs.
Library = namedtuple("Library", "prefix header so env module")
LIBRARIES = (Library("ophip", "onepose_hip.h", "libonepose_hip.so", "OPHIP_LIB", "hip"),
             Library("opsfm", "onepose_sfm.h", "libonepose_sfm.so", "OPSFM_LIB", "sfm_objectblock"),
             Library("opsft", "onepose_sfm_tracks.h", "libonepose_sfm_tracks.so", "OPSFT_LIB", "sfm_tracks"),
             Library("opstr", "onepose_sfm_triangulate.h", "libonepose_sfm_triangulate.so", "OPSTR_LIB", "sfm_triangulate"),
             Library("opsff", "onepose_sfm_fine.h", "libonepose_sfm_fine.so", "OPSFF_LIB", "sfm_fine"),
             Library("oppnpd", "onepose_pnp_device.h", "libonepose_pnp_device.so", "OPPNPD_LIB", "pnp_device"),
             Library("optrk", "onepose_track.h", "libonepose_track.so", "OPTRK_LIB", "track_device"),
             Library("opdet", "onepose_detect.h", "libonepose_detect.so", "OPDET_LIB", "detect_device"),
             Library("oplm", "onepose_postopt_lm.h", "libonepose_postopt_lm.so", "OPLM_LIB", "postopt_lm"),
             Library("optmp", "onepose_temporal.h", "libonepose_temporal.so", "OPTMP_LIB", "temporal"),
             Library("opevl", "onepose_pose_eval.h", "libonepose_pose_eval.so", "OPEVL_LIB", "pose_eval"))

SCALARS = {"int": ctypes.c_int, "unsigned": ctypes.c_uint, "long long": ctypes.c_longlong, "unsigned long long": ctypes.c_ulonglong,
           "float": ctypes.c_float, "double": ctypes.c_double, "size_t": ctypes.c_size_t}
RETURN_TYPES = (*SCALARS, "const char*", "void", "void*")
_POINTEES = (*SCALARS, "char", "unsigned char", "void")
_NAME = rf"\b(?:{'|'.join([entry.prefix for entry in LIBRARIES] + ['oppnp'])})_\w+"          # oppnp: the host library (pnp.py)

# Libraries outside the table above: the same five columns, the header under include/ext/ (so the header path holds
# the directory).  Bound with ``Binding.of`` like an entry of ``LIBRARIES``, read with the library's own prefix (``names_of``), and checked
# and loaded by __graft_entry__.build() too.
EXTENSIONS = (Library("opfcx", "ext/onepose_fine_context.h", "libonepose_fine_context.so", "OPFCX_LIB", "fine_context"),)
# Libraries beside the inference path (training and validation signals): rows like those of ``EXTENSIONS`` in every respect, kept apart
# because that table is the LoFTR matcher's.
ADDONS = (Library("opsup", "ext/onepose_supervision.h", "libonepose_supervision.so", "OPSUP_LIB", "supervision"),)
# The training-mode forward's own step: a row like those of ``ADDONS``, in a table of its own because that one is held to its one row.
TRAINING = (Library("optrn", "ext/onepose_train_forward.h", "libonepose_train_forward.so", "OPTRN_LIB", "train_forward"),)
# The backward of the training loss down to the matcher's feature boundaries: a row like those of ``ADDONS`` and ``TRAINING``, in a table of
# its own because each of those two is held to its one row.
BACKWARD = (Library("opbwd", "ext/onepose_loss_backward.h", "libonepose_loss_backward.so", "OPBWD_LIB", "loss_backward"),)
# The backward of the coarse transformer's encoder layer: the next consumer of what ``BACKWARD``'s row writes, in a table of its own because
# that one too is held to its one row.
ENCODER_BACKWARD = (Library("openb", "ext/onepose_encoder_backward.h", "libonepose_encoder_backward.so", "OPENB_LIB", "encoder_backward"),)


def names_of(*prefixes: str) -> str:
    """The pattern of an entry point's name for libraries with these C prefixes: what ``parse`` and ``Binding`` take as ``names``"""
    return rf"\b(?:{'|'.join(prefixes)})_\w+"


class HeaderError(ValueError):
    pass


class HipLibraryError(RuntimeError):
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


def parse(text: str, names: str | None = None) -> Header:
    """``names``: the pattern of an entry point's name (``names_of``); ``None``: the table's prefixes and the host library's (``_NAME``)"""
    names = _NAME if names is None else names
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
    for m in re.finditer(rf"(?:\A|(?<=[;{{}}]))\s*([\w\s*]+?)\s*({names})\s*\(", text):
        where, ret = f"{line(m.start(2))}, {m.group(2)}", _type(m.group(1))
        end = re.compile(r"([^();{}]*)\)\s*;").match(text, m.end())
        if ret not in RETURN_TYPES or end is None:
            raise HeaderError(f"{where}: not a prototype this reader knows (return types: {', '.join(RETURN_TYPES)})")
        params = end.group(1).strip()
        prototypes[m.group(2)] = Prototype(m.group(2), ret, tuple(
            _declarator(p, where, structs)[:2] for p in ([] if params in ("", "void") else params.split(","))))
        read_at.add(m.start(2))
    for m in re.finditer(rf"({names})\s*\(", text):          # nothing that looks like an entry point may be left out silently
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


class Binding:
    """One HIP library bound from its header: ``header`` (an empty parse when the file is missing, and ``load()`` says so),
    ``signatures`` (name -> (restype, argtypes)), ``exported_symbols``, ``abi_version`` (``constant("ABI_VERSION")``), ``path``
    (the environment variable ``env``, read once here, or ``lib/<so>``) and ``handle`` (``None`` until ``load()``)."""

    def __init__(self, header: str, so: str, prefix: str, env: str, mirrors: dict | None = None, names: str | None = None):
        pkg = os.path.dirname(os.path.abspath(__file__))
        self.so, self.prefix = so, prefix
        self.path = os.environ.get(env) or os.path.join(pkg, "lib", so)
        self.header_path = os.path.join(os.path.dirname(pkg), "include", header)         # where csrc/Makefile finds it too
        self.header = parse(open(self.header_path).read() if os.path.exists(self.header_path) else "", names)
        self.signatures = {name: signature(proto, mirrors) for name, proto in self.header.prototypes.items()}
        self.exported_symbols = tuple(self.signatures)
        self.handle = None
        self._params = {name: proto.params for name, proto in self.header.prototypes.items()}
        self._names = {name: tuple(n for _, n in params) for name, params in self._params.items()}
        self._last_error = f"{prefix}_last_error"

    @classmethod
    def of(cls, module: str, mirrors: dict | None = None) -> "Binding":
        """The binding of the ``LIBRARIES`` (or ``EXTENSIONS``, ``ADDONS``, ``TRAINING``, ``BACKWARD``, ``ENCODER_BACKWARD``) entry whose module is ``module`` (a ``__name__``)"""
        entry, = [e for e in LIBRARIES + EXTENSIONS + ADDONS + TRAINING + BACKWARD + ENCODER_BACKWARD if e.module == module.rpartition(".")[2]]
        return cls(entry.header, entry.so, entry.prefix, entry.env, mirrors, None if entry in LIBRARIES else names_of(entry.prefix))

    @property
    def abi_version(self):
        return self.constant("ABI_VERSION")

    def constant(self, name: str):
        """The header's ``#define <PREFIX>_<name> <integer literal>``: ``None`` when the header file is missing (``load()`` says so),
        ``HeaderError`` when the header is there and has no such define"""
        macro = f"{self.prefix.upper()}_{name}"
        if macro in self.header.defines:
            return self.header.defines[macro]
        if os.path.exists(self.header_path):
            raise HeaderError(f"{self.header_path}: no #define {macro} <integer literal>")
        return None

    def library_path(self) -> str:
        return self.path

    def load(self):
        """Load (once) and return the ctypes handle; raises ``HipLibraryError`` when the library or its header is missing or their ABI
        versions differ -- build it with ``python -c 'import __graft_entry__ as g; g.build()'``."""
        if self.handle is not None:
            return self.handle
        if not os.path.exists(self.path):
            raise HipLibraryError(f"{self.path} not found: the HIP extension is not built (run __graft_entry__.build())")
        if not self.header.prototypes:
            raise HipLibraryError(f"{self.header_path} not found: the binding takes every C signature from that header")
        lib = ctypes.CDLL(self.path)
        for name, (res, args) in self.signatures.items():
            fn = getattr(lib, name)
            fn.restype, fn.argtypes = res, args
        built = getattr(lib, f"{self.prefix}_abi_version")()
        if built != self.abi_version:
            raise HipLibraryError(f"{self.so} ABI version {built}, this binding is written for {self.abi_version} "
                                  f"({self.header_path} {self.prefix.upper()}_ABI_VERSION): rebuild with __graft_entry__.build()")
        self.handle = lib
        return lib

    def check_arity(self, name: str, args) -> None:
        """ctypes accepts surplus arguments silently (a stream handle one slot late would reach C), so the count is checked against
        the header's prototype"""
        params = self._params[name]
        if len(args) != len(params):
            raise TypeError(f"{name} takes {len(params)} arguments ({', '.join(n for _, n in params)}), {len(args)} given")

    def order(self, name: str, **named) -> tuple:
        """The values of ``named`` in the order of the header's parameter names: two neighbouring ``float*`` cannot change places on the
        way to C.  ``TypeError`` names every missing and every unknown parameter.  Needs no loaded library."""
        names = self._names[name]
        if len(named) == len(names):
            try:
                return tuple([named[n] for n in names])
            except KeyError:
                pass
        missing, unknown = [n for n in names if n not in named], [n for n in named if n not in names]
        raise TypeError(f"{name}: missing {', '.join(missing) or 'nothing'}; unknown {', '.join(unknown) or 'nothing'}")

    def call_named(self, name: str, **named) -> None:
        self.call(name, *self.order(name, **named))

    def call(self, name: str, *args) -> None:
        """Call an entry point that returns a status and raise on failure: -1 (a rejected argument) -> ``ValueError``, any other
        non-zero status -> ``RuntimeError``, both with the library's ``<prefix>_last_error()``.  The arity check comes first."""
        if len(args) != len(self._params[name]):
            self.check_arity(name, args)
        lib = self.handle
        if lib is None:
            lib = self.load()
        rc = getattr(lib, name)(*args)
        if rc != 0:
            msg = getattr(lib, self._last_error)().decode(errors="replace")
            if rc == -1:
                raise ValueError(f"{name}: {msg}")
            raise RuntimeError(f"{name} failed (rc={rc}): {msg}")
