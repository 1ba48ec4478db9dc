"""The Python bindings take every C signature, constant and structure layout from ``include/*.h`` (``onepose_st_amd/cabi.py``).
CPU only: the reader on the real headers and on made-up ones, the structure mirrors, ``cabi.Binding`` (arity check, error mapping, load
errors, checked constants) on stand-in handles and on the built libraries for every row of ``cabi.LIBRARIES`` (the table-driven tests
below: one case per row, and per satellite library the symbols written out in ``SYMBOLS`` and one hand-written rejected call in
``REJECTED``), and three faults seeded into copies of the header that the prototypes written out below must catch."""
import ast
import ctypes
import glob
import importlib
import os
import re

import pytest

from onepose_st_amd import cabi, hip

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HIP_H = open(os.path.join(REPO, "include", "onepose_hip.h")).read()
PNP_H = open(os.path.join(REPO, "include", "onepose_pnp.h")).read()

BINDINGS = {entry.module: importlib.import_module(f"onepose_st_amd.{entry.module}")._BINDING for entry in cabi.LIBRARIES}

LL4 = "long long, long long, long long, long long"
# (name, return type, parameter types): written from the headers by hand, one of every type the headers use
WRITTEN_OUT = [
    ("ophip_coarse_match_masked", "int",
     "const float*, const float*, const float*, long long, int, int, int, int, double, float, int, float, "
     "float*, float*, long long*, long long*, long long*, float*, float*, float*, long long*, unsigned char*, "
     "int*, int, int, const unsigned char*, const float*, void*"),
    ("ophip_fine_refine_bf16_scaled", "int",
     f"const float*, {LL4}, int, int, const float*, long long, long long, "
     "const long long*, const long long*, const long long*, const int*, int, const float*, const void*, int, unsigned, int, int, "
     "int, int, float, float*, float*, float*, float*, const float*, void*"),
    ("ophip_frame_enqueue_object", "int",
     f"const ophip_frame_desc*, const ophip_frame_layout_t*, void*, const float*, const float*, {LL4}, "
     "const float*, long long, const float*, long long, const float*, long long, long long, const ophip_object_cache*, "
     "const unsigned char*, const float*, void*, size_t, void*, void*, void*, void*, int*"),
    ("ophip_postopt_refine", "int",
     "double*, const long long*, int, long long, const double*, const double*, const double*, const double*, const long long*, "
     "const long long*, const double*, int, const double*, int, double, double, double, double*, int*, double*, void*, size_t, void*"),
    ("ophip_sfm_points2d_rank", "int",
     "const float*, long long, int, int, void*, size_t, float*, float*, long long*, long long*, void*"),
    ("ophip_device_info", "int", "int*, int*, char*, int"),
    ("ophip_coarse_frag_planes", "int", "float*, int, int, int, void**, void**"),
    ("ophip_sample_features", "int", "const ophip_sample_job*, int, void*"),
    ("ophip_build_stamp", "const char*", ""),
    ("ophip_roctx_ranges", "long long", ""),
    ("ophip_postopt_workspace_bytes", "size_t", "long long, int, int"),
    ("oppnp_pool_result", "int", "void*, long long, double*, int*"),
    ("oppnp_pool_create", "void*", "int"),
    ("oppnp_p3p4", "void", "const double*, const double*, double*, int*"),
    ("oppnp_ransac", "int", "const double*, const float*, const float*, int, double, double, int, int, unsigned long long, int, double*, "
                            "unsigned char*, int*, int*"),
]


def check_written_out(*headers):
    protos = {}
    for h in headers:
        protos.update(h.prototypes)
    for name, ret, types in WRITTEN_OUT:
        if name in protos:
            p = protos[name]
            assert (p.name, p.ret, [t for t, _ in p.params]) == (name, ret, types.split(", ") if types else []), name


def test_reader_finds_every_prototype_of_both_headers():
    hh, ph = cabi.parse(HIP_H), cabi.parse(PNP_H)
    assert list(hh.prototypes) and set(hh.prototypes) == set(re.findall(r"\b(ophip_\w+)\s*\(", HIP_H))     # the expression of test_boundary_cpu
    assert len(hh.prototypes) == len(hip.EXPORTED_SYMBOLS) == 84
    assert set(ph.prototypes) == set(re.findall(r"\b(oppnp_\w+)\s*\(", PNP_H)) and len(ph.prototypes) == 10
    assert all(name in hh.prototypes or name in ph.prototypes for name, _, _ in WRITTEN_OUT)
    check_written_out(hh, ph)
    p = hh.prototypes["ophip_coarse_match_masked"]
    assert [n for _, n in p.params][3:8] == ["kpts_bstride", "B", "N", "M", "wc"] and p.params[-1] == ("void*", "stream")
    assert hh.defines == {"OPHIP_ABI_VERSION": 4, "OPHIP_COARSE_PLANES_READY": 0x100, "OPHIP_SAMPLE_MAX_JOBS": 4}
    assert (hip.ABI_VERSION, hip.COARSE_PLANES_READY, hip.SAMPLE_MAX_JOBS) == (4, 0x100, 4)
    assert ph.defines == {} and ph.structs == {}


def test_the_rule_from_c_types_to_ctypes_classes():
    vp, i = ctypes.c_void_p, ctypes.c_int
    sig = BINDINGS["hip"].signatures
    assert sig["ophip_device_info"] == (i, [vp, vp, ctypes.c_char_p, i])
    assert sig["ophip_build_stamp"] == (ctypes.c_char_p, [])
    assert sig["ophip_coarse_frag_planes"] == (i, [vp, i, i, i, ctypes.POINTER(vp), ctypes.POINTER(vp)])
    assert sig["ophip_postopt_workspace_bytes"] == (ctypes.c_size_t, [ctypes.c_longlong, i, i])
    res, args = sig["ophip_frame_enqueue_object"]
    assert args[0] is ctypes.POINTER(hip.FrameDesc) and args[1] is ctypes.POINTER(hip.FrameLayout) and args[16] is ctypes.POINTER(hip.ObjectCache)
    assert args[20] is ctypes.c_size_t and args[5] is ctypes.c_longlong and args[-1] is vp and len(args) == 26
    assert sig["ophip_sample_features"][1][0] is ctypes.POINTER(hip.SampleJob)
    res, args = sig["ophip_coarse_match_masked"]
    assert [args[k] for k in (3, 8, 9)] == [ctypes.c_longlong, ctypes.c_double, ctypes.c_float]
    res, args = sig["ophip_fine_refine_bf16_scaled"]
    assert args[18] is ctypes.c_uint and len(args) == 30
    pnp = cabi.parse(PNP_H).prototypes
    assert cabi.signature(pnp["oppnp_p3p4"]) == (None, [vp, vp, vp, vp])
    assert cabi.signature(pnp["oppnp_pool_create"]) == (vp, [i])
    assert cabi.signature(pnp["oppnp_ransac"])[1][8] is ctypes.c_ulonglong
    with pytest.raises(cabi.HeaderError):
        cabi.ctype("void")           # only a return type


MADE_UP = """
/* a block comment with a prototype inside: int ophip_not_this(int x); */
#ifndef X_H
#define X_H
#define OPHIP_SOME_FLAG 0x20   // trailing comment
#define OPHIP_COUNT 12
#define OPHIP_NOT_A_LITERAL ((1LL << 30) - 1)
typedef struct ophip_thing {
    int B, N, M;                 /* a declarator list */
    const float* pe; long long pe_bs;
    const void* w[16];           // an array field
    size_t total,
           used;
} ophip_thing;
int ophip_nothing(void);
const char*
ophip_several_lines(const float* a,     /* the first */
                    long long a_bstride,  // the second
                    const ophip_thing* thing,
                    /* nothing here */
                    unsigned bits, void** out,
                    void* stream);
size_t ophip_bytes(int n);   void ophip_two_on_a_line(double x);
#endif
"""


def test_reader_on_made_up_headers():
    h = cabi.parse(MADE_UP)
    assert list(h.prototypes) == ["ophip_nothing", "ophip_several_lines", "ophip_bytes", "ophip_two_on_a_line"]
    assert h.prototypes["ophip_nothing"] == ("ophip_nothing", "int", ())
    assert h.prototypes["ophip_several_lines"] == ("ophip_several_lines", "const char*", (
        ("const float*", "a"), ("long long", "a_bstride"), ("const ophip_thing*", "thing"), ("unsigned", "bits"), ("void**", "out"), ("void*", "stream")))
    assert h.prototypes["ophip_two_on_a_line"] == ("ophip_two_on_a_line", "void", (("double", "x"),))
    assert h.defines == {"OPHIP_SOME_FLAG": 0x20, "OPHIP_COUNT": 12}            # integer literals only
    assert h.structs == {"ophip_thing": (("int", "B", None), ("int", "N", None), ("int", "M", None), ("const float*", "pe", None),
                                         ("long long", "pe_bs", None), ("const void*", "w", 16), ("size_t", "total", None), ("size_t", "used", None))}


def test_constant_on_a_made_up_header(tmp_path):
    (tmp_path / "made_up.h").write_text(MADE_UP)
    binding = cabi.Binding(str(tmp_path / "made_up.h"), "libmade_up.so", "ophip", "OPHIP_LIB")       # an absolute path stands as it is
    assert binding.header_path == str(tmp_path / "made_up.h") and list(binding.header.prototypes)[0] == "ophip_nothing"
    assert (binding.constant("SOME_FLAG"), binding.constant("COUNT")) == (0x20, 12)
    for name in ("NO_SUCH", "NOT_A_LITERAL"):                      # absent, and present but no integer literal
        with pytest.raises(cabi.HeaderError) as e:
            binding.constant(name)
        assert binding.header_path in str(e.value) and f"OPHIP_{name}" in str(e.value)
    with pytest.raises(cabi.HeaderError, match="OPHIP_ABI_VERSION"):
        binding.abi_version
    absent = cabi.Binding("no_such_header.h", "libmade_up.so", "ophip", "OPHIP_LIB")
    assert absent.constant("COUNT") is None and absent.abi_version is None


def test_the_reader_knows_the_prefixes_of_the_table_and_of_the_host_library():
    prefixes = [e.prefix for e in cabi.LIBRARIES] + ["oppnp"]
    assert cabi._NAME == rf"\b(?:{'|'.join(prefixes)})_\w+"
    for prefix in prefixes:
        assert list(cabi.parse(f"int {prefix}_f(int x);").prototypes) == [f"{prefix}_f"]
    for text in ("int opzz_f(int x);", "int op_f(int x);", "int xophip_f(int x);"):
        assert cabi.parse(text).prototypes == {}


@pytest.mark.parametrize("text,line", [
    ("int ophip_a(int x);\n\nint ophip_fn_pointer(int (*cb)(int), void* stream);\n", 3),      # a parameter it cannot read
    ("/* two\n lines */\nint ophip_b(struct foo* x);\n", 3),                                   # a type it does not know
    ("int ophip_c(int);\n", 1),                                                                 # a parameter without a name
    ("int ophip_d(int x)\n{ return x; }\n", 1),                                                 # not a prototype
    ("short ophip_e(int x);\n", 1),                                                             # a return type outside the set
    ("int ophip_f(int x);\n__attribute__((visibility(\"default\"))) int ophip_g(int x);\n", 2),      # a declaration in another form
])
def test_reader_fails_loudly(text, line):
    with pytest.raises(cabi.HeaderError) as e:
        cabi.parse(text)
    assert f"line {line}," in str(e.value)
    assert re.search(r"ophip_[b-g]|ophip_fn_pointer", str(e.value))


def test_structure_mirrors_match_the_header():
    structs = cabi.parse(HIP_H).structs
    assert set(structs) == set(hip._MIRRORS) == {"ophip_frame_desc", "ophip_frame_layout_t", "ophip_object_cache", "ophip_sample_job"}
    for name, fields in structs.items():
        cabi.check_mirror(hip._MIRRORS[name], name, fields)
    assert len(structs["ophip_frame_layout_t"]) == 22 and ("const void*", "w_coarse", 16) in structs["ophip_frame_desc"]

    def mirror(fields):
        return type("Mirror", (ctypes.Structure,), {"_fields_": fields})

    good = list(hip.FrameDesc._fields_)
    cabi.check_mirror(mirror(good), "ophip_frame_desc", structs["ophip_frame_desc"])
    k = [n for n, _ in good].index("hc")
    swapped = good[:k] + [good[k + 1], good[k]] + good[k + 2:]                  # same classes, two names in the other order
    with pytest.raises(cabi.HeaderError, match=r"ophip_frame_desc\.hc"):
        cabi.check_mirror(mirror(swapped), "ophip_frame_desc", structs["ophip_frame_desc"])
    for bad, field in ((("temperature", ctypes.c_float), "temperature"), (("w_coarse", ctypes.c_void_p * 8), "w_coarse"),
                       (("n_fine", ctypes.c_longlong), "n_fine")):
        with pytest.raises(cabi.HeaderError, match=rf"ophip_frame_desc\.{field}"):
            cabi.check_mirror(mirror([bad if n == bad[0] else (n, c) for n, c in good]), "ophip_frame_desc", structs["ophip_frame_desc"])
    with pytest.raises(cabi.HeaderError):
        cabi.check_mirror(mirror(good[:-1]), "ophip_frame_desc", structs["ophip_frame_desc"])
    with pytest.raises(cabi.HeaderError):
        cabi.check_mirror(mirror(good + [("extra", ctypes.c_int)]), "ophip_frame_desc", structs["ophip_frame_desc"])


class _StandIn:
    """in place of the library handle: records what would have reached C; ``rc`` is what every entry point returns, ``<prefix>_last_error``
    and ``<prefix>_abi_version`` answer ``error`` and ``abi``"""

    def __init__(self, rc=0, error=b"", abi=None):
        self.entered, self.rc, self.error, self.abi = [], rc, error, abi

    def __getattr__(self, name):
        if name.endswith("_last_error"):
            return lambda: self.entered.append((name, ())) or self.error
        if name.endswith("_abi_version"):
            return lambda: self.abi
        return lambda *args: self.entered.append((name, args)) or self.rc


def test_call_checks_the_number_of_arguments(monkeypatch):
    lib = _StandIn()
    monkeypatch.setattr(BINDINGS["hip"], "handle", lib)
    args = (None, None, None, 1, 2, 3, None)                       # ophip_pe_add_transpose(feat_nchw, pe_nlc, out_nlc, B, C, M, stream)
    hip.call("ophip_pe_add_transpose", *args)
    assert lib.entered == [("ophip_pe_add_transpose", args)]
    for wrong in (args + (None,), args[:-1]):
        with pytest.raises(TypeError) as e:
            hip.call("ophip_pe_add_transpose", *wrong)
        msg = str(e.value)
        assert "ophip_pe_add_transpose" in msg and "7" in msg and str(len(wrong)) in msg and "feat_nchw, pe_nlc, out_nlc, B, C, M, stream" in msg
    with pytest.raises(TypeError):
        hip.call("ophip_frame_wait")
    spliced = "ophip_encoder_layer_x3w8_streams"                     # (called by name in layercall.py; here the positional check itself)
    with pytest.raises(TypeError):                                  # the spliced kind: an optional pointer too many pushes the stream one slot late
        hip.call(spliced, *([None] * 12), None)
    assert len(lib.entered) == 1                                    # nothing else reached the handle


def _status_entries(binding):
    """the entry points of a binding that return a status and take arguments"""
    return [p for p in binding.header.prototypes.values() if p.ret == "int" and p.params]


def _status_entry(binding):
    return _status_entries(binding)[0]


@pytest.mark.parametrize("module", BINDINGS)
def test_every_binding_checks_the_number_of_arguments(module, monkeypatch):
    """the same statement for each library and each of its entry points, through the names its module exports"""
    binding, mod = BINDINGS[module], importlib.import_module(f"onepose_st_amd.{module}")
    assert mod.check_arity == binding.check_arity
    for proto in _status_entries(binding):
        lib = _StandIn()
        monkeypatch.setattr(binding, "handle", lib)
        args = (None,) * len(proto.params)
        mod.call(proto.name, *args)
        assert lib.entered == [(proto.name, args)]
        for wrong in (args + (None,), args[:-1]):
            for check in ((lambda: mod.call(proto.name, *wrong)), (lambda: mod.check_arity(proto.name, wrong))):
                with pytest.raises(TypeError) as e:
                    check()
                msg = str(e.value)
                assert f"{proto.name} takes {len(args)} arguments" in msg and f"{len(wrong)} given" in msg
                assert ", ".join(n for _, n in proto.params) in msg
        mod.check_arity(proto.name, args)
        assert len(lib.entered) == 1                                # nothing else reached the handle


@pytest.mark.parametrize("module", BINDINGS)
def test_order_puts_named_arguments_into_header_order(module, monkeypatch):
    """``Binding.order`` for every prototype: shuffled keywords of sentinel values come back in header order without a loaded library;
    a missing and an unknown name raise ``TypeError`` naming them; ``call_named`` hands ``call`` that tuple"""
    import random
    binding, rng = BINDINGS[module], random.Random(5)
    monkeypatch.setattr(binding, "load", lambda: pytest.fail("order() must not load the library"))
    assert binding.header.prototypes
    for proto in binding.header.prototypes.values():
        names = [n for _, n in proto.params]
        assert len(set(names)) == len(names), f"{proto.name}: a parameter name twice"
        sentinels = {n: object() for n in names}
        shuffled = rng.sample(names, len(names))
        got = binding.order(proto.name, **{n: sentinels[n] for n in shuffled})
        assert len(got) == len(names) and all(g is sentinels[n] for g, n in zip(got, names)), proto.name
        if names:
            with pytest.raises(TypeError) as e:
                binding.order(proto.name, **{n: sentinels[n] for n in shuffled if n != names[-1]})
            assert proto.name in str(e.value) and f"missing {names[-1]}" in str(e.value)
        with pytest.raises(TypeError) as e:
            binding.order(proto.name, **sentinels, no_such_parameter=1)
        assert proto.name in str(e.value) and "unknown no_such_parameter" in str(e.value)
        if proto.ret == "int" and names:
            lib = _StandIn()
            monkeypatch.setattr(binding, "handle", lib)
            binding.call_named(proto.name, **{n: sentinels[n] for n in shuffled})
            assert lib.entered == [(proto.name, got)]
    if module == "hip":
        assert hip.order == binding.order
        with pytest.raises(TypeError, match="missing stream; unknown streem"):
            hip.call_named("ophip_pe_add_transpose", feat_nchw=None, pe_nlc=None, out_nlc=None, B=1, C=2, M=3, streem=None)


@pytest.mark.parametrize("module", BINDINGS)
def test_call_maps_the_status_to_an_exception(module, monkeypatch):
    binding, mod = BINDINGS[module], importlib.import_module(f"onepose_st_amd.{module}")
    proto = _status_entry(binding)
    args = (None,) * len(proto.params)
    last_error = (f"{binding.prefix}_last_error", ())
    ok = _StandIn(rc=0, error=b"never read")
    monkeypatch.setattr(binding, "handle", ok)
    assert mod.call(proto.name, *args) is None
    assert ok.entered == [(proto.name, args)]                       # the error text is read on failure only
    rejected = _StandIn(rc=-1, error=b"somewhere: null pointer")
    monkeypatch.setattr(binding, "handle", rejected)
    with pytest.raises(ValueError) as e:
        mod.call(proto.name, *args)
    assert str(e.value) == f"{proto.name}: somewhere: null pointer"
    assert rejected.entered == [(proto.name, args), last_error]
    failed = _StandIn(rc=7, error=b"somewhere: out of memory")
    monkeypatch.setattr(binding, "handle", failed)
    with pytest.raises(RuntimeError) as e:
        mod.call(proto.name, *args)
    assert "rc=7" in str(e.value) and "somewhere: out of memory" in str(e.value) and proto.name in str(e.value)
    assert not isinstance(e.value, cabi.HipLibraryError) and failed.entered == [(proto.name, args), last_error]


@pytest.mark.parametrize("module", BINDINGS)
def test_abi_mismatch_is_reported_by_load(module, monkeypatch):
    binding = BINDINGS[module]
    opened = []
    monkeypatch.setattr(binding, "handle", None)
    monkeypatch.setattr(cabi.ctypes, "CDLL", lambda path: opened.append(path) or _StandIn(abi=binding.abi_version + 1))
    for attempt in (1, 2):                                          # the handle is not kept: the second load() opens the file again
        with pytest.raises(cabi.HipLibraryError) as e:
            binding.load()
        msg = str(e.value)
        assert binding.so in msg and f"ABI version {binding.abi_version + 1}" in msg and f"written for {binding.abi_version}" in msg
        assert binding.header_path in msg and "__graft_entry__.build()" in msg
        assert binding.handle is None and opened == [binding.path] * attempt
    monkeypatch.setattr(cabi.ctypes, "CDLL", lambda path: _StandIn(abi=binding.abi_version))
    assert binding.load() is binding.handle is not None


def test_call_arity_with_the_real_library():
    hip.call("ophip_timing_every", 1)                              # host side only
    with pytest.raises(TypeError):
        hip.call("ophip_timing_every", 1, 1)
    with pytest.raises(TypeError):
        hip.call("ophip_timing_every")
    assert hip.load().ophip_encoder_workspace_floats(1, 7000, 4800) == (219 + 150 + 2) * 8448      # calls on the handle itself work as before


def _seed(old, new, text=HIP_H, count=1):
    assert text.count(old) >= 1
    return text.replace(old, new, count)


def test_seeded_fault_parameter_type():
    """``long long kpts_bstride`` -> ``int`` in a copy of the header: the binding would pass a 32-bit stride"""
    k = HIP_H.index("int ophip_coarse_match_masked(")
    bad = cabi.parse(HIP_H[:k] + _seed("long long kpts_bstride", "int kpts_bstride", HIP_H[k:]))
    assert cabi.signature(bad.prototypes["ophip_coarse_match_masked"])[1][3] is ctypes.c_int
    with pytest.raises(AssertionError, match="ophip_coarse_match_masked"):
        check_written_out(bad)
    check_written_out(cabi.parse(HIP_H))


def test_seeded_fault_parameter_removed():
    k = HIP_H.index("int ophip_fine_refine_bf16_scaled(")
    bad = cabi.parse(HIP_H[:k] + _seed("int encoder_enable, int nsplit,", "int encoder_enable,", HIP_H[k:]))
    assert len(bad.prototypes["ophip_fine_refine_bf16_scaled"].params) == 29
    with pytest.raises(AssertionError, match="ophip_fine_refine_bf16_scaled"):
        check_written_out(bad)


def test_seeded_fault_layout_field_moved():
    bad = cabi.parse(_seed("size_t total, result_bytes;\n    size_t x2d, ffcl,", "size_t total, x2d;\n    size_t result_bytes, ffcl,"))
    assert len(bad.structs["ophip_frame_layout_t"]) == 22
    with pytest.raises(cabi.HeaderError, match=r"ophip_frame_layout_t\.x2d"):
        cabi.check_mirror(hip.FrameLayout, "ophip_frame_layout_t", bad.structs["ophip_frame_layout_t"])


@pytest.mark.parametrize("entry", cabi.LIBRARIES, ids=lambda e: e.module)
def test_missing_header_is_reported_by_load(entry):
    binding = cabi.Binding("no_such_header.h", entry.so, entry.prefix, entry.env)
    assert binding.exported_symbols == () and binding.abi_version is None and binding.library_path() == BINDINGS[entry.module].path
    with pytest.raises(hip.HipLibraryError, match="no_such_header.h"):
        binding.load()
    assert binding.handle is None


@pytest.mark.parametrize("entry", cabi.LIBRARIES, ids=lambda e: e.module)
def test_missing_library_is_reported_by_load(entry, monkeypatch, tmp_path):
    absent = str(tmp_path / "libonepose_absent.so")
    monkeypatch.setenv(entry.env, absent)                           # read once, when the binding is made
    binding = cabi.Binding.of(f"onepose_st_amd.{entry.module}")
    with pytest.raises(cabi.HipLibraryError) as e:
        binding.load()
    assert str(e.value) == f"{absent} not found: the HIP extension is not built (run __graft_entry__.build())"
    monkeypatch.delenv(entry.env)
    assert binding.library_path() == absent and binding.handle is None
    assert cabi.Binding.of(f"onepose_st_amd.{entry.module}").library_path() == os.path.join(REPO, "onepose_st_amd", "lib", entry.so)


def test_the_table_of_libraries_is_complete():
    assert hip.HipLibraryError is cabi.HipLibraryError
    headers = sorted(os.path.basename(p) for p in glob.glob(os.path.join(REPO, "include", "onepose_*.h")))
    assert sorted(e.header for e in cabi.LIBRARIES) == [h for h in headers if h != "onepose_pnp.h"] and "onepose_pnp.h" in headers
    for column in zip(*cabi.LIBRARIES):
        assert len(set(column)) == len(cabi.LIBRARIES)              # no header, prefix, file, variable or module twice
    for entry in cabi.LIBRARIES:
        mod, binding = importlib.import_module(f"onepose_st_amd.{entry.module}"), BINDINGS[entry.module]
        assert (binding.so, binding.prefix, binding.header_path) == (entry.so, entry.prefix, os.path.join(REPO, "include", entry.header))
        assert (mod.library_path, mod.load, mod.check_arity, mod.call) == (binding.library_path, binding.load, binding.check_arity, binding.call)
        assert mod.EXPORTED_SYMBOLS is binding.exported_symbols and mod.ABI_VERSION == binding.abi_version and isinstance(mod.ABI_VERSION, int)
        assert mod.EXPORTED_SYMBOLS and all(s.startswith(entry.prefix + "_") for s in mod.EXPORTED_SYMBOLS)
        assert {f"{entry.prefix}_abi_version", f"{entry.prefix}_last_error"} <= set(mod.EXPORTED_SYMBOLS)
        text = open(binding.header_path).read()
        assert set(mod.EXPORTED_SYMBOLS) == set(re.findall(rf"\b({entry.prefix}_\w+)\s*\(", text))
        others = "|".join(e.prefix for e in cabi.LIBRARIES if e is not entry)                        # no other library's prefix in it
        assert not re.findall(rf"\b(?:{others})_\w+\s*\(", re.sub(r"/\*.*?\*/", "", text, flags=re.S))


# The symbols of every satellite library, written out by hand in header order
SYMBOLS = {
    "sfm_objectblock": ("opsfm_abi_version", "opsfm_last_error", "opsfm_workspace_bytes", "opsfm_aggregate", "opsfm_box_test", "opsfm_pair_count",
                        "opsfm_pair_emit", "opsfm_merge_resolve", "opsfm_group_emit", "opsfm_point_mean"),
    "sfm_tracks": ("opsft_abi_version", "opsft_last_error", "opsft_assign", "opsft_finish", "opsft_track_rows", "opsft_pair_keys", "opsft_pair_emit",
                   "opsft_fine_rows"),
    "sfm_triangulate": ("opstr_abi_version", "opstr_last_error", "opstr_workspace_bytes", "opstr_components", "opstr_prepare", "opstr_round"),
    "sfm_fine": ("opsff_abi_version", "opsff_last_error", "opsff_row_ids", "opsff_sample_rows"),
    "pnp_device": ("oppnpd_abi_version", "oppnpd_last_error", "oppnpd_workspace_bytes", "oppnpd_ranges", "oppnpd_prep", "oppnpd_sample", "oppnpd_p3p",
                   "oppnpd_score", "oppnpd_select", "oppnpd_refine", "oppnpd_solve"),
    "track_device": ("optrk_abi_version", "optrk_last_error", "optrk_box_set", "optrk_box_from_pose", "optrk_crop"),
    "detect_device": ("opdet_abi_version", "opdet_last_error", "opdet_workspace_bytes", "opdet_ranges", "opdet_score", "opdet_select",
                      "opdet_fit_box", "opdet_vote", "opdet_detect"),
    "postopt_lm": ("oplm_abi_version", "oplm_last_error", "oplm_workspace_bytes", "oplm_refine"),
    "temporal": ("optmp_abi_version", "optmp_last_error", "optmp_pyramid_bytes", "optmp_pyramid", "optmp_track", "optmp_collect", "optmp_inject"),
    "pose_eval": ("opevl_abi_version", "opevl_last_error", "opevl_errors", "opevl_add", "opevl_adds", "opevl_proj2d"),
}


def test_the_symbols_written_out_are_those_of_every_satellite_library():
    """against the module, the header text and the built file; every entry point returns a status and takes the stream last, but for the
    ABI number, the error text and the size helpers"""
    assert set(SYMBOLS) == set(BINDINGS) - {"hip"}
    for module, want in SYMBOLS.items():
        mod, binding = importlib.import_module(f"onepose_st_amd.{module}"), BINDINGS[module]
        assert mod.EXPORTED_SYMBOLS == want == tuple(binding.header.prototypes)
        assert set(re.findall(rf"\b({binding.prefix}_\w+)\s*\(", open(binding.header_path).read())) == set(want)
        lib = ctypes.CDLL(mod.library_path())
        assert all(hasattr(lib, s) for s in want)
        for name, proto in binding.header.prototypes.items():
            assert len(binding.signatures[name][1]) == len(cabi.signature(proto)[1]) == len(proto.params)
            if not name.endswith(("_abi_version", "_last_error", "_bytes")):
                assert proto.ret == "int" and proto.params[-1] == ("void*", "stream"), name


def _names_read_with_constant(mod):
    """the names a module assigns from ``_BINDING.constant``, in the form every module writes: ``A, B = map(_BINDING.constant, ("A", "B"))``"""
    names = []
    for node in ast.parse(open(mod.__file__).read()).body:
        if isinstance(node, ast.Assign) and "_BINDING.constant" in ast.unparse(node.value):
            targets, (fn, arg) = [t.id for t in node.targets[0].elts], node.value.args
            assert ast.unparse(node.value.func) == "map" and ast.unparse(fn) == "_BINDING.constant" and targets == list(ast.literal_eval(arg))
            names += targets
    return names


@pytest.mark.parametrize("entry", cabi.LIBRARIES, ids=lambda e: e.module)
def test_every_module_imports_and_reads_its_constants(entry):
    mod = importlib.import_module(f"onepose_st_amd.{entry.module}")
    names = _names_read_with_constant(mod)
    assert names and open(mod.__file__).read().count(".constant") == 1          # one assignment holds them all
    for name in names:
        assert type(getattr(mod, name)) is int and getattr(mod, name) == BINDINGS[entry.module].header.defines[f"{entry.prefix.upper()}_{name}"], name


_PTR = ctypes.c_void_p(8)        # not null and never followed: the entries below return before they launch anything
# One entry point per satellite library whose argument checks are its first statements, before any HIP call (read in its .hip file),
# the arguments that are not 0 / NULL, and the text the library itself writes.
REJECTED = {
    "sfm_objectblock": ("opsfm_box_test", {}, "opsfm_box_test: null pointer"),
    "sfm_tracks": ("opsft_finish", {}, "opsft_finish: table sizes"),
    "sfm_triangulate": ("opstr_components", {"T": -1, "U": 1}, "opstr_components: table sizes"),
    "sfm_fine": ("opsff_row_ids", {}, "opsff_row_ids: null pointer"),
    "pnp_device": ("oppnpd_ranges", {"cap": 1}, "oppnpd_ranges: table sizes"),
    "track_device": ("optrk_box_set", {"x1": 1, "y1": 1, "K": _PTR, "S": 0, "box": _PTR, "flag": _PTR, "K_crop": _PTR, "trans": _PTR},
                     "optrk_box_set: crop size S outside [1, OPTRK_MAX_CROP]"),
    "detect_device": ("opdet_ranges", {"cap": 1}, "opdet_ranges: table sizes"),
    "postopt_lm": ("oplm_refine", {}, "oplm_refine: null pointer"),
    "temporal": ("optmp_pyramid", {}, "optmp_pyramid: null pointer"),
    "pose_eval": ("opevl_errors", {}, "opevl_errors: null pointer"),
}


def test_the_built_libraries_answer_for_themselves():
    """No device: the ABI number of each built library, then one rejected call per satellite library.  Every library keeps its own error
    text, whatever is called in another one afterwards."""
    assert set(REJECTED) == set(BINDINGS) - {"hip"}
    for module, binding in BINDINGS.items():
        mod = importlib.import_module(f"onepose_st_amd.{module}")
        assert getattr(mod.load(), f"{binding.prefix}_abi_version")() == mod.ABI_VERSION == binding.abi_version
        assert mod.load() is binding.handle

    def last_error(module):
        return getattr(BINDINGS[module].load(), f"{BINDINGS[module].prefix}_last_error")().decode()

    def reject(module):
        name, given, text = REJECTED[module]
        mod, params = importlib.import_module(f"onepose_st_amd.{module}"), BINDINGS[module].header.prototypes[name].params
        assert set(given) <= {n for _, n in params}
        args = [given.get(n, None if c.endswith("*") else 0) for c, n in params]
        with pytest.raises(ValueError) as e:
            mod.call(name, *args)
        assert str(e.value) == f"{name}: {text}" and last_error(module) == text

    for module, (_, _, text) in REJECTED.items():
        reject(module)
        hip.call("ophip_timing_every", 1)                           # a correct call into another library (host side only)
        assert last_error(module) == text
    reject(next(iter(REJECTED)))                                    # so that the last row too has seen a rejection in another library
    for module, (_, _, text) in REJECTED.items():                   # and the rejections that followed in the other nine
        assert last_error(module) == text


def test_pnp_binds_from_its_header():
    from onepose_st_amd import pnp
    lib = pnp.load()
    for name, proto in cabi.parse(PNP_H).prototypes.items():
        fn = getattr(lib, name)
        assert (fn.restype, list(fn.argtypes)) == cabi.signature(proto), name
    assert lib.oppnp_pool_destroy.restype is None and lib.oppnp_pool_submit.argtypes[9] is ctypes.c_ulonglong
