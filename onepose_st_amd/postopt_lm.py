"""Binding of ``libonepose_postopt_lm.so`` (``csrc/postopt_lm.hip``, ``include/postopt_lm.h``): the second-order
(Levenberg-Marquardt) solver of the SfM depth refinement.  The public call is ``postopt.refine_depths_lm``; this module is the
library's handle only.  The library sits outside ``cabi.LIBRARIES``, so the binding is written out here."""
from __future__ import annotations

from . import cabi

_BINDING = cabi.Binding("postopt_lm.h", "libonepose_postopt_lm.so", "oplm", "OPLM_LIB")
library_path, load, check_arity, call = _BINDING.library_path, _BINDING.load, _BINDING.check_arity, _BINDING.call
EXPORTED_SYMBOLS = _BINDING.exported_symbols
ABI_VERSION = _BINDING.abi_version
_DEFINES = _BINDING.header.defines
CONVERGED, MAX_ITERS, STALLED, DEGENERATE = (_DEFINES.get(f"OPLM_{n}") for n in ("CONVERGED", "MAX_ITERS", "STALLED", "DEGENERATE"))
