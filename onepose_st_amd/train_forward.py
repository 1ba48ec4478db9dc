"""The training-mode forward's own step on the device (opt-in): the reference's ``CoarseMatching.get_coarse_match``
in training (``coarse_matching.py:174-240``) -- the predicted coarse matches cut to ``max_num_matches_train - train_pad_num_gt_min``
random picks and padded with random ground-truth matches of confidence 0 up to ``max_num_matches_train`` rows -- from the SPARSE ground
truth of :mod:`supervision` (``GroundTruth.gt_j [B, N]``) instead of a ``torch.where`` over a dense ``conf_matrix_gt [B, N, M]``.

The specification is ``include/ext/onepose_train_forward.h`` (``tests/train_forward_oracle.py`` restates it in numpy).  The padded list
always has exactly ``T = train_rows(B, N, M, train_coarse_percent)`` rows, so every buffer behind this step has a host-known capacity and
the split between predicted and padded rows (``n_keep``) stays a device int.  The draws are a counter-based sampler of this project's own
(``seed``, ``step``): they cannot equal ``torch.randint``'s stream; two calls with one ``(seed, step)`` give identical bytes.

Not here: the backward of the transformers, the window gather and the backbone (``loss_backward.py`` stops at their outputs), ``mask0``, and
a dense ground truth with several entries in one row (``GroundTruth.from_dense`` keeps the first).

The kernels are HIP (``csrc/train_forward.hip`` in ``libonepose_train_forward.so``, the row of ``cabi.TRAINING``).  CPU tensors raise
:class:`hip.HipLibraryError` (no CPU fallback); nothing is synchronised and no count is read on the host.
"""
from __future__ import annotations

import torch

from . import cabi, devargs, hip
from .matchcall import MatchLists

_BINDING = cabi.Binding.of(__name__)                # the header is the one place a signature or a constant is written
library_path, load, check_arity, call, order = _BINDING.library_path, _BINDING.load, _BINDING.check_arity, _BINDING.call, _BINDING.order
launch = hip.launcher(_BINDING, globals())          # every stream-taking entry is called through it, by the header's parameter names
EXPORTED_SYMBOLS = _BINDING.exported_symbols
ABI_VERSION = _BINDING.abi_version
BLOCK, MAX_BATCH, MAX_ROWS, MAX_STEP, OK, NO_GT = map(_BINDING.constant, ("BLOCK", "MAX_BATCH", "MAX_ROWS", "MAX_STEP", "OK", "NO_GT"))


def train_rows(B, N, M, percent) -> int:
    """``max_num_matches_train``: the reference's ``int(num_candidates_max * train_coarse_percent)`` on a Python float"""
    return int(int(B) * min(int(N), int(M)) * percent)


class GtRows:
    """What :func:`gt_list` leaves on the device: ``rows`` int32 ``[B * N]`` (``r = b * N + i`` of the ground-truth rows, ascending; the
    entries at or past the total are not written) and ``total`` int32 ``[1]``."""

    def __init__(self, rows, total, keep=()):
        self.rows, self.total, self._keep = rows, total, keep


def gt_list(gt, *, stream=None) -> GtRows:
    """The reference's ``torch.where(conf_matrix_gt)`` in its order, from ``gt`` (a :class:`supervision.GroundTruth`)"""
    hip.need_device([("gt_j", gt.gt_j)])
    B, N, M = gt.shape
    if gt.gt_j.dtype != torch.int64 or B < 1 or N < 1:
        raise ValueError("gt_j: int64 [B, N] with at least one row")
    gt_j, dev = gt.gt_j.contiguous(), gt.gt_j.device
    nbytes = load().optrn_gt_list_bytes(B, N)
    with hip.enqueue_on(dev, stream):
        workspace = torch.empty(max(int(nbytes), 1), dtype=torch.uint8, device=dev)
        rows = torch.empty(B * N, dtype=torch.int32, device=dev)
        total = torch.empty(1, dtype=torch.int32, device=dev)
        launch("optrn_gt_list", dict(gt_j=gt_j, B=B, N=N, M=M, workspace=workspace, workspace_bytes=workspace.numel(), gt_rows=rows,
                                     n_gt_total=total), stream)
    return GtRows(rows, total, keep=(gt_j, workspace))


class PaddedLists:
    """What :func:`pad_matches` leaves on the device: ``lists`` (a :class:`matchcall.MatchLists` of ``T`` rows; ``m_bids`` is ``b_ids``,
    of which the first ``n_keep`` rows are the reference's; ``count`` is ``T``, or 0 with ``NO_GT``), ``n_keep`` and ``status`` int32 ``[1]``."""

    def __init__(self, lists, n_keep, status, keep=()):
        self.lists, self.n_keep, self.status, self._keep = lists, n_keep, status, keep


def pad_matches(lists, gt, keypoints3d, *, T, G, seed, step, w_c, scale, query_scale=None, gt_rows=None, out=None, n_keep=None,
                status=None, stream=None) -> PaddedLists:
    """``lists``: the eval forward's :class:`matchcall.MatchLists` (its ``count`` a device int, ``None``: every row); ``gt``: the
    :class:`supervision.GroundTruth`; ``keypoints3d [B or 1, N, 3]`` float32.  ``T``: :func:`train_rows`; ``G``: ``train_pad_num_gt_min``;
    ``seed``, ``step``: the sampler's (``step`` the caller's call counter); ``w_c``, ``scale``: the coarse grid's width and its pixels per
    cell; ``query_scale``: float32 ``[B, 2]`` or ``None``.  ``gt_rows``: a :func:`gt_list` of ``gt`` (``None``: made here).  ``out``, ``n_keep``,
    ``status``: where to write (a ``MatchLists`` of at least ``T`` rows, int32 ``[1]`` each; ``None``: allocated here).  Rows at or past ``T``
    of a longer ``out`` are not written."""
    named = [(k, getattr(lists, k)) for k in ("b_ids", "i_ids", "j_ids", "mconf", "mk3d", "mkc")] + [("gt_j", gt.gt_j), ("keypoints3d", keypoints3d)]
    named += [(k, v) for k, v in (("query_scale", query_scale), ("n_keep", n_keep), ("status", status)) if v is not None]
    hip.need_device(named)
    dev = gt.gt_j.device
    B, N, M = gt.shape
    T, G = int(T), int(G)
    cap = int(lists.b_ids.shape[0])
    for name, t in named[:3]:
        if t.dim() != 1 or t.shape[0] != cap or t.dtype != torch.int64:
            raise ValueError(f"{name}: int64 [{cap}]")
    if tuple(lists.mconf.shape) != (cap,) or tuple(lists.mk3d.shape) != (cap, 3) or tuple(lists.mkc.shape) != (cap, 2):
        raise ValueError(f"mconf [{cap}], mk3d [{cap}, 3], mkc [{cap}, 2]")
    if keypoints3d.dim() != 3 or keypoints3d.shape[0] not in (1, B) or tuple(keypoints3d.shape[1:]) != (N, 3) or keypoints3d.dtype != torch.float32:
        raise ValueError(f"keypoints3d: float32 [{B} or 1, {N}, 3]")
    if keypoints3d.stride(2) != 1 or keypoints3d.stride(1) != 3:
        keypoints3d = keypoints3d.contiguous()
    if query_scale is not None:
        if tuple(query_scale.shape) != (B, 2):
            raise ValueError(f"query_scale: [{B}, 2]")
        query_scale = query_scale.to(torch.float32).contiguous()
    count = lists.count
    if isinstance(count, torch.Tensor) and count.numel() > 1:          # a coarse call's count block: the count is its first int
        count = count[:1]
    count = devargs.count_arg(count, dev)
    if out is not None and (out.b_ids.shape[0] < T or any(not getattr(out, k).is_contiguous() for k in ("b_ids", "i_ids", "j_ids", "mconf", "mk3d", "mkc", "gt_mask"))):
        raise ValueError(f"out: contiguous lists of at least {T} rows")
    with hip.enqueue_on(dev, stream):
        if gt_rows is None:
            gt_rows = gt_list(gt, stream=stream)
        if out is None:
            out = MatchLists.empty(max(T, 1), dev, count_ints=1)
            out.m_bids = out.b_ids
        n_keep = torch.empty(1, dtype=torch.int32, device=dev) if n_keep is None else n_keep
        status = torch.empty(1, dtype=torch.int32, device=dev) if status is None else status
        src = [t.contiguous() for _, t in named[:6]]
        if cap == 0:                                        # nothing predicted and no room for it: one unused row (empty tensors have no address)
            src, count, cap = [torch.zeros(1, *t.shape[1:], dtype=t.dtype, device=dev) for t in src], torch.zeros(1, dtype=torch.int32, device=dev), 1
        launch("optrn_pad_matches", dict(b_ids=src[0], i_ids=src[1], j_ids=src[2], mconf=src[3], mkpts_3d=src[4], mkpts_c=src[5], count=count,
                                         cap=cap, gt_rows=gt_rows.rows, n_gt_total=gt_rows.total, gt_j=gt.gt_j.contiguous(),
                                         keypoints3d=keypoints3d, kp_bstride=hip.bstride(keypoints3d), B=B, N=N, M=M, w_c=w_c, T=T, G=G,
                                         seed=seed, step=step, scale=scale, query_scale=query_scale, out_b_ids=out.b_ids,
                                         out_i_ids=out.i_ids, out_j_ids=out.j_ids, out_mconf=out.mconf, out_mkpts_3d=out.mk3d,
                                         out_mkpts_c=out.mkc, out_gt_mask=out.gt_mask, out_count=out.count, n_keep=n_keep, status=status),
               stream)
    return PaddedLists(out, n_keep, status, keep=(src, gt_rows, gt, keypoints3d, query_scale, count))


class stages:
    """The two entries one by one (device tensors in, device tensors out): what a training-mode ``enqueue_features`` enqueues between the
    coarse and the fine stage"""
    gt_list = staticmethod(gt_list)
    pad_matches = staticmethod(pad_matches)
