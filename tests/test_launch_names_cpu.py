"""The launch step (``hip.launcher``): every stream-taking entry point of every library is called by the header's parameter names, each
value converted by the header's C type of that parameter.  CPU only: the converter table against all the headers and a made-up one, the
names and the values of a launch with ``<module>.call`` replaced by a recorder, and an ``ast`` walk that finds no positional call left."""
import ast
import ctypes
import glob
import importlib
import os
import re
import types

import numpy as np
import pytest
import torch

from onepose_st_amd import cabi, hip

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
ENTRIES = cabi.LIBRARIES + cabi.EXTENSIONS + cabi.ADDONS
MODULES = {e.module: importlib.import_module(f"onepose_st_amd.{e.module}") for e in ENTRIES}
SEED = 2 ** 64 + 5
STREAM = types.SimpleNamespace(cuda_stream=0x5150)          # in place of a ``torch.cuda.Stream``: the launch step reads its handle only
# One prototype per library for the value test: the first stream-taking one, but where another has an ``unsigned`` or a seed
CHOSEN = {"hip": "ophip_fine_refine_bf16_scaled", "pnp_device": "oppnpd_solve", "detect_device": "opdet_detect"}


def stream_taking(binding):
    return [p for p in binding.header.prototypes.values() if any(n == "stream" for _, n in p.params)]


def names_of(proto):
    return [n for _, n in proto.params if n != "stream"]


def test_the_converter_table_is_total(tmp_path):
    from_the_text = 0
    for entry in ENTRIES:
        text = re.sub(r"/\*.*?\*/|//[^\n]*", "", open(os.path.join(REPO, "include", entry.header)).read(), flags=re.S)
        from_the_text += len(re.findall(rf"\b{entry.prefix}_\w+\s*\([^()]*\bvoid\s*\*\s*stream\b[^()]*\)\s*;", text))
    seen = 0
    for module, mod in MODULES.items():
        protos = stream_taking(mod._BINDING)
        assert protos, module
        for proto in protos:
            conv = mod.launch.converters(proto.name)
            assert list(conv) == names_of(proto) and all(callable(c) for c in conv.values()), proto.name
            seen += 1
    assert seen == from_the_text > 0                        # every stream-taking prototype of the 13 headers, counted from them
    assert hip.converters is hip.launch.converters and hip.launch is MODULES["hip"].launch
    made_up = tmp_path / "made_up.h"
    made_up.write_text("int ophip_fine(const double* a, size_t n, unsigned long long seed, void** out, void* stream);\n"
                       "int ophip_odd(const float* a, char* label, void* stream);\n")
    launch = hip.launcher(cabi.Binding(str(made_up), "libmade_up.so", "ophip", "OPHIP_LIB"), {})
    assert list(launch.converters("ophip_fine")) == ["a", "n", "seed", "out"]
    with pytest.raises(cabi.HeaderError) as e:
        launch.converters("ophip_odd")
    assert all(word in str(e.value) for word in ("ophip_odd", "label", "char*"))
    with pytest.raises(cabi.HeaderError, match="ophip_frame_wait takes no stream"):          # stream-less entries stay on call / call_named
        hip.converters("ophip_frame_wait")


@pytest.mark.parametrize("module", MODULES)
def test_a_launch_names_the_missing_and_the_unknown_parameter(module, monkeypatch):
    mod = MODULES[module]
    monkeypatch.setattr(mod._BINDING, "load", lambda: pytest.fail("the names are checked without the library"))
    monkeypatch.setattr(mod, "call", lambda *a: pytest.fail("nothing may be called"))
    for proto in stream_taking(mod._BINDING):
        names = names_of(proto)
        named = dict.fromkeys(names[:-1], None)
        with pytest.raises(TypeError) as e:
            mod.launch(proto.name, dict(named, no_such_parameter=1), STREAM)
        assert proto.name in str(e.value) and f"missing {names[-1]}" in str(e.value) and "unknown no_such_parameter" in str(e.value)


def _value(ctype, k):
    """a CPU-free value for a parameter of C type ``ctype`` (numpy scalars: what reaches C must be the plain Python number)"""
    bare = ctype.replace("const ", "")
    if bare.endswith("*"):
        return None
    return {"int": np.int32(k + 1), "long long": np.int64(2 ** 40 + k), "size_t": np.int64(k + 1), "unsigned": np.uint32(k + 1),
            "unsigned long long": SEED, "float": np.float32(k + 0.5), "double": np.float64(k + 0.25)}[bare]


@pytest.mark.parametrize("module", MODULES)
def test_a_launch_puts_every_value_into_the_headers_slot(module, monkeypatch):
    mod = MODULES[module]
    proto = mod._BINDING.header.prototypes[CHOSEN[module]] if module in CHOSEN else stream_taking(mod._BINDING)[0]
    entered = []
    monkeypatch.setattr(mod, "call", lambda name, *args: entered.append((name, args)))
    named = {n: _value(c, k) for k, (c, n) in enumerate(proto.params) if n != "stream"}
    mod.launch(proto.name, named, STREAM)
    (name, args), = entered
    assert name == proto.name and len(args) == len(proto.params)
    seen = set()
    for k, ((c, n), a) in enumerate(zip(proto.params, args)):
        bare = c.replace("const ", "")
        seen.add(bare)
        if n == "stream":
            assert type(a) is ctypes.c_void_p and a.value == STREAM.cuda_stream
        elif bare.endswith("*"):
            assert a is None, n
        elif bare in ("int", "long long", "size_t"):
            assert type(a) is int and a == int(named[n]), n
        elif bare in ("float", "double"):
            assert type(a) is float and a == float(named[n]), n
        elif bare == "unsigned":
            assert type(a) is ctypes.c_uint and a.value == k + 1, n
        else:
            assert bare == "unsigned long long" and type(a) is ctypes.c_ulonglong and a.value == 5, n
    if module in CHOSEN:
        assert {"hip": "unsigned", "pnp_device": "unsigned long long", "detect_device": "unsigned long long"}[module] in seen
    # a CPU tensor reaches no kernel, whichever pointer it is given to; a ctypes object passes as it is
    del entered[:]
    pointers = [n for c, n in proto.params if c.endswith("*") and n != "stream"]
    assert pointers
    for n in pointers:
        with pytest.raises(hip.HipLibraryError) as e:
            mod.launch(proto.name, dict(named, **{n: torch.zeros(4)}), STREAM)
        assert n in str(e.value) and proto.name in str(e.value)
    assert entered == []
    address = ctypes.c_void_p(64)
    mod.launch(proto.name, dict(named, **{pointers[0]: address}), STREAM)
    assert entered[0][1][[n for _, n in proto.params].index(pointers[0])] is address


def test_a_wrong_dtype_is_a_type_error_that_names_the_parameter(monkeypatch):
    """the dtype check comes after the device check (``hip.ptr``), so without a device it is shown on the converters themselves"""
    conv = MODULES["pnp_device"].launch.converters("oppnpd_ranges")

    class OnDevice:                                          # what ``hip.ptr`` reads of a tensor
        is_cuda = True

        def __init__(self, dtype):
            self.dtype = dtype

        def data_ptr(self):
            return 4096
    assert conv["b_ids"](OnDevice(torch.int64)).value == conv["count"](OnDevice(torch.int32)).value == 4096
    for name, dtype in (("b_ids", torch.int32), ("count", torch.int64), ("ranges", torch.float32)):
        with pytest.raises(TypeError):
            conv[name](OnDevice(dtype))
    double = MODULES["pose_eval"].launch.converters("opevl_errors")["pose_pred"]
    assert double(OnDevice(torch.float64)).value == 4096
    with pytest.raises(TypeError):
        double(OnDevice(torch.float32))
    entered = []
    monkeypatch.setattr(MODULES["pnp_device"], "call", lambda *a: entered.append(a))
    with pytest.raises(TypeError, match="oppnpd_ranges, b_ids: expected torch.int64, got torch.int32"):
        MODULES["pnp_device"].launch("oppnpd_ranges", dict(b_ids=OnDevice(torch.int32), count=None, cap=4, F=1, ranges=None), STREAM)
    assert entered == []


def test_no_positional_call_of_a_stream_taking_entry_is_left():
    """A call whose first argument is the literal name of a stream-taking prototype hands C nothing by position: it is a ``launch`` of
    ``(entry, {name: value}[, stream])``, or it has no further positional argument (``call_named``).  An entry chosen at run time is
    written as one such call per branch, so that this walk sees every name."""
    stream_entries = {p.name for mod in MODULES.values() for p in stream_taking(mod._BINDING)}
    found, launches = [], 0
    for path in sorted(glob.glob(os.path.join(REPO, "onepose_st_amd", "*.py"))):
        for node in ast.walk(ast.parse(open(path).read())):
            if not (isinstance(node, ast.Call) and node.args and isinstance(node.args[0], ast.Constant) and node.args[0].value in stream_entries):
                continue
            callee = node.func.attr if isinstance(node.func, ast.Attribute) else getattr(node.func, "id", "")
            if callee == "launch" and len(node.args) in (2, 3) and not any(isinstance(a, ast.Starred) for a in node.args):
                launches += 1
            elif len(node.args) > 1:
                found.append(f"{os.path.relpath(path, REPO)}:{node.lineno}: {node.args[0].value}")
    assert not found, "positional calls of stream-taking entries:\n" + "\n".join(found)
    assert launches >= 70                                    # the walk does see the launches (77 when this was written)
