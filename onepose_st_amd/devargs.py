"""What the device-loop modules (``pnp_device``, ``detect_device``, ``track_device``, ``temporal``, ``pose_eval``, ``frameloop``) ask of
their arguments, and the codec of their one packed read-back.  The tensor and device checks themselves are
``hip.need_tensors`` / ``hip.on_device`` / ``hip.need_device``; a module keeps only the checks that no other module makes."""
from __future__ import annotations

import numpy as np
import torch


def count_arg(count, dev, default=None):
    """``None`` (then ``default`` rows, or ``None``), a host integer, or one int32 on the device -> ``None`` or int32 ``[1]`` on ``dev``"""
    count = default if count is None else count
    if count is None or isinstance(count, torch.Tensor):
        if count is not None and (count.dtype != torch.int32 or count.numel() != 1):
            raise ValueError("count: one int32 on the device")
        return count
    return torch.full((1,), int(count), dtype=torch.int32, device=dev)


def mat64(name, m, shapes, dev, wording=None):
    """A small matrix (``K``, ``trans``, a pose table) as float64, contiguous: a tensor where it lies, host numbers uploaded to ``dev``.
    Its shape is one of ``shapes`` (``None`` in one: any extent; ``shapes=None``: any shape), else ``ValueError(f"{name}: {wording}")``."""
    if not isinstance(m, torch.Tensor):
        m = torch.as_tensor(np.asarray(m, dtype=np.float64), device=dev)
    if shapes is not None and not any(len(s) == m.dim() and all(w in (None, n) for w, n in zip(s, m.shape)) for s in shapes):
        raise ValueError(f"{name}: {wording or ' or '.join(str(list(s)) for s in shapes)}")
    return m.to(torch.float64).contiguous()


def k_table(K, F, dev, exact=False):
    """Intrinsics shared by ``F`` frames or one per frame -> ``(K [1 or F, 9] float64 contiguous, k_shared)``.  Anything that reshapes to
    that is taken; ``exact``: only ``[3, 3]`` and ``[F, 3, 3]``."""
    wording = f"[3, 3] shared, or [{F}, 3, 3]"
    K = mat64("K", K, ((3, 3), (F, 3, 3)) if exact else None, dev, wording).reshape(-1, 9)
    if K.shape[0] not in (1, F):
        raise ValueError(f"K: {wording}")
    return K, int(K.shape[0] == 1)


def point_tables(name_a, a, width_a, name_b, b, width_b, max_rows=None, min_rows=0):
    """The float32 pair ``a [cap, width_a]``, ``b [cap, width_b]`` of a match table, contiguous"""
    if a.dim() != 2 or a.shape[1] != width_a or b.dim() != 2 or b.shape[1] != width_b or a.shape[0] != b.shape[0] or a.shape[0] < min_rows:
        raise ValueError((f"{name_a} and {name_b}: [cap, {width_a}], the same length" if width_a == width_b else
                          f"{name_a} [cap, {width_a}] and {name_b} [cap, {width_b}] must have the same length")
                         + (f", at least {min_rows}" if min_rows else ""))
    if a.dtype != torch.float32 or b.dtype != torch.float32:
        raise ValueError(f"{name_a} and {name_b}: float32")
    if max_rows is not None and a.shape[0] > max_rows:
        raise ValueError(f"at most {max_rows} rows")
    return a.contiguous(), b.contiguous()


def at_least_one_row(a, b, count=None, b_ids=None):
    """-> ``(a, b, count, b_ids)``; of an empty table: one zero row and a zero count
    (the library wants a table of at least one row; the count says it is unused)"""
    if a.shape[0]:
        return a, b, count, b_ids
    zeros = lambda shape, dtype: torch.zeros(shape, dtype=dtype, device=a.device)
    return (zeros((1, a.shape[1]), a.dtype), zeros((1, b.shape[1]), b.dtype), zeros(1, torch.int32),
            None if b_ids is None else zeros(1, torch.int64))


# ---- the packed read-back: several device tensors in one uint8 tensor, one copy to the host, cut apart there ----------------------------
def pack(tensors) -> torch.Tensor:
    """One uint8 tensor: the bytes of every tensor in order"""
    return torch.cat([t.reshape(-1).view(torch.uint8) for t in tensors])


def packed_layout(tensors) -> list:
    """Per tensor ``(numpy dtype, shape, bytes)``: what :func:`unpack` needs of :func:`pack`'s arguments"""
    return [(torch.empty(0, dtype=t.dtype).numpy().dtype, tuple(t.shape), t.numel() * t.element_size()) for t in tensors]


def packed_bytes(tensors) -> int:
    return sum(nbytes for _, _, nbytes in packed_layout(tensors))


def unpack(host_bytes, layout, offset=0):
    """-> (the arrays of ``layout`` as views of ``host_bytes`` (a uint8 numpy array) from ``offset`` on, the offset behind them)"""
    out = []
    for dtype, shape, nbytes in layout:
        out.append(host_bytes[offset:offset + nbytes].view(dtype).reshape(shape))
        offset += nbytes
    return out, offset
