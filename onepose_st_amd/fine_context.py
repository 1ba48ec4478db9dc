"""The coarse context of the LoFTR matcher's fine windows (``fine_concat_coarse_feat``): ctypes binding of
``libonepose_fine_context.so`` (``include/ext/onepose_fine_context.h``, ``csrc/fine_context.hip``), the row of ``cabi.EXTENSIONS``.

The published ``FinePreprocess`` with the switch set: ``win'[k, r] = merge_feat(cat[win[k, r], down_proj(coarse[b_k, id_k])])`` for both
images, computed as ``Wm[:, :128] . win[k, r] + u_k`` with ``u_k = Wm[:, 128:] . down_proj(...) + bm`` once per match: one entry point,
two launches, split-bf16 products (the arithmetic of ``ophip_rows_linear_x3``).  CPU tensors raise :class:`hip.HipLibraryError` (no CPU
fallback)."""
from __future__ import annotations

import torch

from . import cabi, hip

_BINDING = cabi.Binding.of(__name__)                # the header is the one place a signature or a constant is written
library_path, load, check_arity, call, order = _BINDING.library_path, _BINDING.load, _BINDING.check_arity, _BINDING.call, _BINDING.order
launch = hip.launcher(_BINDING, globals())          # every stream-taking entry is called through it, by the header's parameter names
EXPORTED_SYMBOLS = _BINDING.exported_symbols
ABI_VERSION = _BINDING.abi_version
TILE_ROWS, MAX_ROWS = map(_BINDING.constant, ("TILE_ROWS", "MAX_ROWS"))


def wpack_bytes() -> int:
    """``opfcx_wpack_bytes()``: the length of ``packing.pack_fine_context``'s block"""
    return int(load().opfcx_wpack_bytes())


def merge(win0, win1, x0, x1, b_ids, i_ids, j_ids, W, wpack, out=None):
    """``win0, win1 [K, W * W, 128]`` (float32, contiguous) with the coarse rows ``x0 [V, L0, 256]``, ``x1 [V or 1, L1, 256]`` of the
    matches' cells ``(b_ids, i_ids)`` / ``(b_ids, j_ids)`` (int64 ``[K]``) -> ``(win0', win1')``.  ``out``: ``None`` -- in place, the
    inputs are overwritten and returned -- or a pair of tensors like ``win0, win1`` that share no memory with them.  A coarse tensor of
    batch 1 (or a stride-0 expand) is one image for every match.  ``wpack``: ``packing.pack_fine_context`` on the device.  On the
    current stream; nothing is synchronised."""
    named = [("win0", win0), ("win1", win1), ("x0", x0), ("x1", x1), ("b_ids", b_ids), ("i_ids", i_ids), ("j_ids", j_ids), ("wpack", wpack)]
    out0, out1 = (win0, win1) if out is None else out
    hip.need_device(named + [("out0", out0), ("out1", out1)])
    K, WW = win0.shape[0], int(W) * int(W)
    for name, t in (("win0", win0), ("win1", win1), ("out0", out0), ("out1", out1)):
        if t.dim() != 3 or tuple(t.shape) != (K, WW, 128) or not t.is_contiguous():
            raise ValueError(f"{name}: a contiguous tensor [{K}, {WW}, 128], got {list(t.shape)}")
    for name, t in (("x0", x0), ("x1", x1)):
        if t.dim() != 3 or t.shape[2] != 256 or t.stride(2) != 1 or t.stride(1) != 256:
            raise ValueError(f"{name}: coarse rows [V, L, 256] with contiguous images, got {list(t.shape)}")
    B = max(x0.shape[0], x1.shape[0])
    if x0.shape[0] not in (1, B) or x1.shape[0] not in (1, B):
        raise ValueError(f"x0 and x1: batches {x0.shape[0]} and {x1.shape[0]} (expected equal, or 1 for an image every match shares)")
    for name, t in (("b_ids", b_ids), ("i_ids", i_ids), ("j_ids", j_ids)):
        if tuple(t.shape) != (K,) or not t.is_contiguous():
            raise ValueError(f"{name}: a contiguous tensor [{K}], got {list(t.shape)}")
    if K == 0:                                          # nothing to launch (and empty tensors have no address to hand over)
        return out0, out1
    context = torch.empty(2 * K * 128, device=win0.device)
    launch("opfcx_merge", dict(win0=win0, win1=win1, coarse0=x0, coarse0_bstride=hip.bstride(x0), coarse1=x1, coarse1_bstride=hip.bstride(x1),
                               b_ids=b_ids, i_ids=i_ids, j_ids=j_ids, K=K, B=B, L0=x0.shape[1], L1=x1.shape[1], W=W, wpack=wpack, context=context,
                               out0=out0, out1=out1))
    return out0, out1
