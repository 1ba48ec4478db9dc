"""ctypes binding of ``libonepose_hip.so`` (include/onepose_hip.h).

The product path has no CPU fallback: if the shared library cannot be loaded, or a
tensor is not a contiguous float32/int64 CUDA(HIP) tensor, this module raises.
PyTorch is used for device memory and streams only; every kernel is reached through
the C ABI with raw device pointers.
"""
from __future__ import annotations

import contextlib
import ctypes

import torch

from . import cabi
from .cabi import HipLibraryError  # noqa: F401  (its old name: hip.HipLibraryError)

c_i = ctypes.c_int
c_ll = ctypes.c_longlong


class SampleJob(ctypes.Structure):
    """``ophip_sample_job`` (include/onepose_hip.h): one map / keypoint set of ``ophip_sample_features``"""
    _fields_ = [("map", ctypes.c_void_p), ("keypoints", ctypes.c_void_p), ("scale", ctypes.c_void_p), ("out", ctypes.c_void_p),
                ("h", c_i), ("w", c_i), ("C", c_i), ("K", c_i), ("H", c_i), ("W", c_i), ("keypoints_double", c_i), ("nearest", c_i)]


class FrameDesc(ctypes.Structure):
    """``ophip_frame_desc`` (include/onepose_hip.h)"""
    _fields_ = [("B", c_i), ("N", c_i), ("M", c_i), ("hc", c_i), ("wc", c_i), ("hf", c_i), ("wf", c_i), ("cf", c_i),
                ("lazy_conf", c_i), ("n_coarse", c_i), ("coarse_cross_bits", ctypes.c_uint),
                ("n_fine", c_i), ("fine_cross_bits", ctypes.c_uint), ("fine_encoder_enable", c_i),
                ("border_rm", c_i),
                ("thr", ctypes.c_float), ("scale_c", ctypes.c_float), ("fine_scale", ctypes.c_float),
                ("temperature", ctypes.c_double),
                ("pe", ctypes.c_void_p), ("w_kpt", ctypes.c_void_p), ("w_coarse", ctypes.c_void_p * 16), ("w_fine", ctypes.c_void_p)]


class FrameLayout(ctypes.Structure):
    """``ophip_frame_layout_t``: byte offsets inside the frame's device block"""
    _fields_ = [(n, ctypes.c_size_t) for n in ("total", "result_bytes", "x2d", "ffcl", "x3d", "y3d", "y2d", "z3d", "stats", "enc_ws", "conf", "cws",
                                               "result", "i_ids", "j_ids", "m_bids", "gt_mask", "mconf", "mkc", "expec", "feat3d_out", "feat2d_out")]


class ObjectCache(ctypes.Structure):
    """``ophip_object_cache``: per-object buffers of the frame-invariant encoder work (keypoint encoding, first layer's 3D rows, layer 1's
    K^T V | Ksum block of the 3D source) + the event behind the kernels that wrote them"""
    _fields_ = [("x3d", ctypes.c_void_p), ("x3d_bs", c_ll), ("y3d0", ctypes.c_void_p), ("y3d0_bs", c_ll),
                ("kv1", ctypes.c_void_p), ("kv1_bs", c_ll), ("ready", ctypes.c_void_p)]


_MIRRORS = {"ophip_sample_job": SampleJob, "ophip_frame_desc": FrameDesc, "ophip_frame_layout_t": FrameLayout, "ophip_object_cache": ObjectCache}
# The header is the one place a signature, a structure or a constant of the C ABI is written: an entry point is added there and in its
# .hip file, nothing here.  (A missing header leaves the tables empty and load() says so.)
_BINDING = cabi.Binding.of(__name__, _MIRRORS)
for _name, _fields in _BINDING.header.structs.items():
    cabi.check_mirror(_MIRRORS[_name], _name, _fields)
library_path, load, check_arity, call, order = _BINDING.library_path, _BINDING.load, _BINDING.check_arity, _BINDING.call, _BINDING.order
EXPORTED_SYMBOLS, PROTOTYPES = _BINDING.exported_symbols, _BINDING.header.prototypes
ABI_VERSION = _BINDING.abi_version                                      # what the FrameDesc / FrameLayout mirrors above are written for
# COARSE_PLANES_READY is or-ed into ophip_coarse_match's nsplit
SAMPLE_MAX_JOBS, COARSE_PLANES_READY = map(_BINDING.constant, ("SAMPLE_MAX_JOBS", "COARSE_PLANES_READY"))
NO_CPU_FALLBACK = "the HIP path needs device tensors (no CPU fallback)"     # what every device-loop module says of a CPU tensor


def call_named(name: str, **named) -> None:
    """``call`` with every argument bound by its name in the header (``cabi.Binding.order``)"""
    call(name, *order(name, **named))          # this module's ``call``: whoever replaces it (a test's spy) sees these calls too


def ptr(t: torch.Tensor | None, dtype=torch.float32):
    """Device pointer of a tensor of the given dtype (``dtype=None``: any, e.g. packed byte blocks)."""
    if t is None:
        return None
    if not t.is_cuda:
        raise HipLibraryError(NO_CPU_FALLBACK)
    if dtype is not None and t.dtype != dtype:
        raise TypeError(f"expected {dtype}, got {t.dtype}")
    return ctypes.c_void_p(t.data_ptr())


def bstride(t: torch.Tensor) -> int:
    """Batch stride in elements; an object block that the batch shares (batch 1, or a stride-0 expand) gives 0."""
    return 0 if t.shape[0] == 1 or t.stride(0) == 0 else t.stride(0)


def stream_handle():
    return ctypes.c_void_p(torch.cuda.current_stream().cuda_stream)


def stream_arg(stream):
    """The handle of ``stream`` (a ``torch.cuda.Stream``); ``None``: the current stream"""
    return ctypes.c_void_p(stream.cuda_stream) if stream is not None else stream_handle()


def seed_arg(seed):
    """An ``unsigned long long`` seed: ``seed`` mod 2^64"""
    return ctypes.c_ulonglong(int(seed) & (2 ** 64 - 1))


_CDATA = (ctypes.c_int.__mro__[-2], type(ctypes.byref(ctypes.c_int())))      # every ctypes object, and what ``ctypes.byref`` returns


def _pointer(dtype):
    """The converter of a pointer: ``None`` -> NULL; a ctypes object as it is (an address C handed out, a ``ctypes.byref`` out-parameter);
    else ``ptr`` of a device tensor of ``dtype`` (``None``: any, e.g. packed byte blocks and bf16 planes)"""
    return lambda t: t if isinstance(t, _CDATA) else ptr(t, dtype)


def _byte_ptr(t):
    """``unsigned char*`` (masks, gt_mask, images): bytes, as ``torch.bool`` or ``torch.uint8``"""
    return t if isinstance(t, _CDATA) else ptr(t, torch.bool if t is not None and t.dtype == torch.bool else torch.uint8)


def _ctypes_object(t):
    """``void**`` and a pointer to a mirrored structure: a ctypes object (or ``None``) as it is"""
    if t is None or isinstance(t, _CDATA):
        return t
    if isinstance(t, torch.Tensor) and not t.is_cuda:
        raise HipLibraryError(NO_CPU_FALLBACK)
    raise TypeError(f"expected a ctypes object, got {type(t).__name__}")


# The one table from a parameter's C type (``const`` set aside) to what turns a Python value into it.  A new C parameter type is one row here.
_CONVERTER = {"int": int, "long long": int, "size_t": int, "float": float, "double": float, "unsigned": lambda v: ctypes.c_uint(int(v)),
              "unsigned long long": seed_arg, "float*": _pointer(torch.float32), "double*": _pointer(torch.float64),
              "long long*": _pointer(torch.int64), "int*": _pointer(torch.int32), "unsigned char*": _byte_ptr, "void*": _pointer(None),
              "void**": _ctypes_object}


def launcher(binding: cabi.Binding, module: dict):
    """The launch step of one library: ``launch`` (and ``launch.converters``) of ``binding``, calling through ``module["call"]`` (the
    binding module's ``globals()``: whoever replaces ``<module>.call``, a test's spy, sees these calls too)."""
    made = {}

    def converters(entry: str) -> dict:
        """``{parameter name: converter}`` of ``entry`` without ``stream``, in the header's order and each from the header's C type of
        that parameter (``const`` set aside); made on first use.  ``HeaderError`` for a type the table has no row for."""
        if entry not in made:
            conv = {}
            for c, n in binding.header.prototypes[entry].params:
                bare = c.replace("const ", "")
                if n != "stream" and bare not in _CONVERTER and bare[:-1] not in binding.header.structs:
                    raise cabi.HeaderError(f"{entry}, {n}: no converter for {c!r} (hip._CONVERTER)")
                conv[n] = _CONVERTER.get(bare, _ctypes_object)
            if "stream" not in conv:
                raise cabi.HeaderError(f"{entry} takes no stream: it is called with call / call_named")
            made[entry] = (conv, list(conv).index("stream"))
            del conv["stream"]
        return made[entry][0]

    def launch(entry: str, named: dict, stream=None) -> None:
        """``call`` of ``entry`` on ``stream`` (a ``torch.cuda.Stream``; ``None``: the current one), every argument bound by its name in
        the header and turned into what the header's C type of that parameter asks for.  A refused value raises what ``ptr`` raises, with
        the entry and the parameter in front."""
        conv = converters(entry)
        if named.keys() != conv.keys():
            binding.order(entry, **named, stream=None)          # TypeError: names every missing and every unknown parameter
        try:
            args = [c(named[n]) for n, c in conv.items()]
        except (HipLibraryError, TypeError, ValueError):
            for n, c in conv.items():                           # again, one at a time, for the name
                try:
                    c(named[n])
                except (HipLibraryError, TypeError, ValueError) as e:
                    raise type(e)(f"{entry}, {n}: {e}") from None
            raise
        args.insert(made[entry][1], stream_arg(stream))
        module["call"](entry, *args)

    launch.converters = converters
    return launch


launch = launcher(_BINDING, globals())
converters = launch.converters


@contextlib.contextmanager
def enqueue_on(dev, stream=None):
    """Where a device-loop call allocates and enqueues: the device ``dev`` current and, given one, ``stream`` (a ``torch.cuda.Stream``)"""
    with torch.cuda.device(dev), torch.cuda.stream(stream):         # torch.cuda.stream(None) changes nothing
        yield


def need_tensors(named) -> None:
    """``named``: (name, value) pairs.  Every value is a tensor."""
    for name, t in named:
        if not isinstance(t, torch.Tensor):
            raise TypeError(f"{name}: expected a tensor")


def on_device(tensors) -> None:
    """Every one of ``tensors`` lies on the device."""
    if not all(t.is_cuda for t in tensors):
        raise HipLibraryError(NO_CPU_FALLBACK)


def need_device(named) -> None:
    """:func:`need_tensors`, and then every one of them lies on the device."""
    named = list(named)
    need_tensors(named)
    on_device(t for _, t in named)


def exclusive(counts: torch.Tensor) -> torch.Tensor:
    """``[n]`` counts -> ``[n + 1]`` int64 offsets from 0"""
    return torch.cat([torch.zeros(1, dtype=torch.int64, device=counts.device), torch.cumsum(counts, 0)])


def build_stamp() -> str:
    """16 hex digits identifying the sources ``libonepose_hip.so`` was built from (``ophip_build_stamp``)."""
    return load().ophip_build_stamp().decode()


def device_info() -> dict:
    cu, lds = c_i(0), c_i(0)
    buf = ctypes.create_string_buffer(64)
    call("ophip_device_info", ctypes.byref(cu), ctypes.byref(lds), buf, 64)
    return {"cu_count": cu.value, "lds_per_block": lds.value, "arch": buf.value.decode()}


def timing_select(kernel_name: str, every: int = 1):
    """Bracket every ``every``-th launch of ``kernel_name`` with HIP events ("" switches timing off)."""
    call("ophip_timing_every", int(every))
    call("ophip_timing_select", kernel_name.encode())


def timing_read():
    """-> (launches, total device milliseconds) since the last select/read."""
    n, ms = c_i(0), ctypes.c_double(0.0)
    call("ophip_timing_read", ctypes.byref(n), ctypes.byref(ms))
    return n.value, ms.value
