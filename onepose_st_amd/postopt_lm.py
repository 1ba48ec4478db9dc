"""Binding of ``libonepose_postopt_lm.so`` (``csrc/postopt_lm.hip``, ``include/onepose_postopt_lm.h``): the second-order
(Levenberg-Marquardt) solver of the SfM depth refinement.  The public call is ``postopt.refine_depths_lm``; this module is the
library's handle only."""
from __future__ import annotations

from . import cabi, hip

_BINDING = cabi.Binding.of(__name__)                # the header is the one place a signature or a constant is written
library_path, load, check_arity, call = _BINDING.library_path, _BINDING.load, _BINDING.check_arity, _BINDING.call
launch = hip.launcher(_BINDING, globals())          # every stream-taking entry is called through it, by the header's parameter names
EXPORTED_SYMBOLS = _BINDING.exported_symbols
ABI_VERSION = _BINDING.abi_version
CONVERGED, MAX_ITERS, STALLED, DEGENERATE = map(_BINDING.constant, ("CONVERGED", "MAX_ITERS", "STALLED", "DEGENERATE"))
