"""Device detection: the object detector's vote -- one affine RANSAC per reference view, the box every view votes, the winning view and
the track state of its box -- from the LoFTR matcher's device-side matches, without a host round trip (opt-in; the host vote of
``detector.LocalFeatureObjectDetector.match_worker`` with ``pnp.estimate_affine2d`` stays the default).

The work is HIP (``csrc/detect_affine.hip`` in ``libonepose_detect.so``, include/onepose_detect.h).  CPU tensors raise
:class:`hip.HipLibraryError` (no CPU fallback).  The specification (written out in the header;
``tests/detect_device_oracle.py`` restates it in numpy float64, one function per stage) is the host estimator's model, inlier rule and
fit with a fixed number of counter-based trials in place of the sequential generator and the adaptive stop:

1. ``ranges``: a view's rows ``[begin, end)`` by binary search in the ascending ``b_ids``; ``count`` is clamped to the capacity, a row
   whose id lies outside ``[0, V)`` belongs to no view.
2. ``score``: trial ``t`` of view ``v`` draws three distinct rows (``pnp_device``'s sampler with ``v`` in place of the frame), forms
   ``affine_from3`` of them and counts the view's rows with ``ex^2 + ey^2 < thr^2``; a degenerate sample counts 0; a view of fewer than
   ``max(min_matches, 3)`` rows runs no trials.
3. ``select``: per view the trial with the highest count, the lowest trial among equals; its count and inlier mask;
   ``STATUS_NEEDS_MORE`` when the host's stop formula asks for more trials than ran (informational).
4. ``fit_box``: the host's normal equations on the winner's inliers, every sum in the header's fixed order; the view's corners through
   the affinity, truncated toward zero, their minimum and maximum.  The centre box ``[W // 2 - 500, H // 2 - 500, W // 2 + 500,
   H // 2 + 500]`` with 0 inliers and ``STATUS_NO_MODEL`` for a view of fewer than ``min_matches`` rows, a best count below 3, a singular
   system, or a corner that is not finite or outside int32.
5. ``vote``: the view with the most inliers, the first among equals; the ``track_device.TrackState`` of its box (bit-equal to
   ``track_device.set_box`` of it); a winning box with ``x1 <= x0`` or ``y1 <= y0`` gives the centre box and ``STATUS_DEGENERATE``.

Nothing is synchronised or read back: every launch is sized by the capacity.
"""
from __future__ import annotations

import numpy as np
import torch

from . import cabi, devargs, hip
from .pnp_device import check_ransac_options
from .track_device import MAX_CROP, TrackState, check_crop_size, check_K

_BINDING = cabi.Binding.of(__name__)                # the header is the one place a signature or a constant is written
library_path, load, check_arity, call = _BINDING.library_path, _BINDING.load, _BINDING.check_arity, _BINDING.call
launch = hip.launcher(_BINDING, globals())          # every stream-taking entry is called through it, by the header's parameter names
EXPORTED_SYMBOLS = _BINDING.exported_symbols
ABI_VERSION = _BINDING.abi_version
MAX_VIEWS, MAX_TRIALS, DEFAULT_TRIALS, MAX_ROWS, MAX_SIDE, SCORE_CHUNK, STATUS_NO_MODEL, STATUS_DEGENERATE, STATUS_NEEDS_MORE = map(_BINDING.constant, (
    "MAX_VIEWS", "MAX_TRIALS", "DEFAULT_TRIALS", "MAX_ROWS", "MAX_SIDE", "SCORE_CHUNK", "STATUS_NO_MODEL", "STATUS_DEGENERATE", "STATUS_NEEDS_MORE"))


def _check_options(min_matches, reproj, confidence, trials):
    if int(min_matches) != min_matches or min_matches < 0:
        raise ValueError("min_matches: an integer >= 0")
    check_ransac_options("ransac_reproj_threshold", reproj, confidence, trials, MAX_TRIALS)


class _Inputs:
    """The checked tensors of one call: types, shapes and dtypes first, then the device, all before the library is loaded"""

    def __init__(self, mkpts0, mkpts1, b_ids, view_hw, query_hw, K, crop_size, count):
        tensors = [("mkpts0", mkpts0), ("mkpts1", mkpts1), ("b_ids", b_ids)]
        tensors += [(k, v) for k, v in (("view_hw", view_hw), ("K", K), ("count", count)) if isinstance(v, torch.Tensor)]
        hip.need_tensors(tensors)
        mkpts0, mkpts1 = devargs.point_tables("mkpts0", mkpts0, 2, "mkpts1", mkpts1, 2, max_rows=MAX_ROWS)
        n, dev = mkpts0.shape[0], mkpts0.device
        if b_ids.dtype != torch.int64 or tuple(b_ids.shape) != (n,):
            raise ValueError(f"b_ids: int64 [{n}]")
        if not isinstance(view_hw, torch.Tensor):
            view_hw = torch.as_tensor(np.asarray(view_hw, dtype=np.int32).reshape(-1, 2))
            view_hw = view_hw.to(dev)
        if view_hw.dtype != torch.int32 or view_hw.dim() != 2 or view_hw.shape[1] != 2 or not 1 <= view_hw.shape[0] <= MAX_VIEWS:
            raise ValueError(f"view_hw: int32 [V, 2] (H, W of every view), V in [1, {MAX_VIEWS}]")
        H, W = (int(v) for v in query_hw)
        if not (1 <= H <= MAX_SIDE and 1 <= W <= MAX_SIDE):
            raise ValueError(f"query_hw: (H, W) in [1, {MAX_SIDE}]")
        S = check_crop_size(crop_size)
        K = check_K(K) if isinstance(K, torch.Tensor) else check_K(K).to(dev)
        count = devargs.count_arg(count, dev)
        hip.on_device(t for t in (mkpts0, mkpts1, b_ids, view_hw, K, count) if t is not None)
        self.mk0, self.mk1, self.count, b_ids = devargs.at_least_one_row(mkpts0, mkpts1, count, b_ids)
        self.b_ids = b_ids.contiguous()
        self.view_hw, self.K = view_hw.contiguous(), K
        self.cap, self.V, self.H, self.W, self.S, self.dev = self.mk0.shape[0], int(view_hw.shape[0]), H, W, S, dev


class DeviceDetection:
    """What :func:`vote` returns, on the device: ``state`` (the ``track_device.TrackState`` of the winning box), ``boxes [V, 4]``,
    ``n_inliers [V]`` and ``status [V]`` int32, ``affine [V, 6]`` float64 (row-major 2 x 3; the identity where a view has no model),
    ``winner [1]`` int32, ``inlier_mask [cap]`` uint8 over the rows (``ranges [V, 2]``: the rows of every view)."""

    def __init__(self, state, boxes, n_inliers, affine, status, winner, inlier_mask, ranges, keep=()):
        self.state, self.boxes, self.n_inliers, self.affine, self.status = state, boxes, n_inliers, affine, status
        self.winner, self.inlier_mask, self.ranges = winner, inlier_mask, ranges
        self.status_host = None
        self._keep = keep                                   # the inputs and the workspace stay referenced while the work may be queued

    def to_host(self):
        """``({view: {"inliers", "bbox"}}, winner)``: ``match_worker``'s dict (``inliers``: uint8 ``[n, 1]`` over the view's rows, or an
        empty array where the view votes the centre box) and the winning view.  The one read-back."""
        fields = (self.boxes, self.status, self.ranges, self.winner, self.inlier_mask)
        (boxes, status, ranges, winner, mask), _ = devargs.unpack(devargs.pack(fields).cpu().numpy(), devargs.packed_layout(fields))
        self.status_host, winner = status.copy(), int(winner[0])
        votes = {}
        for v in range(boxes.shape[0]):
            b, e = int(ranges[v, 0]), int(ranges[v, 1])
            inl = np.empty((0)) if int(status[v]) & STATUS_NO_MODEL else mask[b:e].reshape(-1, 1).copy()
            votes[v] = {"inliers": inl, "bbox": boxes[v].copy()}
        return votes, winner


def vote(mkpts0, mkpts1, b_ids, view_hw, query_hw, K, crop_size: int = 512, count=None, trials: int = DEFAULT_TRIALS, seed: int = 1,
         min_matches: int = 6, ransac_reproj_threshold: float = 6.0, confidence: float = 0.99, stream=None) -> DeviceDetection:
    """The module docstring's vote on device tensors: ``mkpts0 [cap, 2]`` (reference view) and ``mkpts1 [cap, 2]`` (query) float32,
    ``b_ids [cap]`` int64 ascending; ``view_hw [V, 2]`` int32 (a device tensor, or host numbers, uploaded); ``query_hw = (H, W)``; ``K``
    the full-frame intrinsics (a float64 device tensor, or host numbers, uploaded); ``count`` int32[1] on the device (default: all
    rows).  Everything is enqueued on ``stream`` (default: the current one); nothing is read back."""
    _check_options(min_matches, float(ransac_reproj_threshold), float(confidence), trials)
    a = _Inputs(mkpts0, mkpts1, b_ids, view_hw, query_hw, K, crop_size, count)
    V, cap, dev = a.V, a.cap, a.dev
    nbytes = load().opdet_workspace_bytes(cap, V, int(trials))
    with hip.enqueue_on(dev, stream):
        ws = torch.empty(nbytes, dtype=torch.uint8, device=dev)
        boxes = torch.empty(V, 4, dtype=torch.int32, device=dev)
        n_in, status = torch.empty(V, dtype=torch.int32, device=dev), torch.empty(V, dtype=torch.int32, device=dev)
        affine = torch.empty(V, 6, dtype=torch.float64, device=dev)
        mask = torch.zeros(cap, dtype=torch.uint8, device=dev)
        winner = torch.empty(1, dtype=torch.int32, device=dev)
        st = TrackState(dev)
        launch("opdet_detect", dict(mk0=a.mk0, mk1=a.mk1, b_ids=a.b_ids, count=a.count, cap=cap, V=V, view_hw=a.view_hw, H=a.H, W=a.W, K=a.K, S=a.S,
                                    min_matches=min_matches, reproj_thr=ransac_reproj_threshold, confidence=confidence, trials=trials, seed=seed,
                                    workspace=ws, workspace_bytes=nbytes, boxes=boxes, n_inliers=n_in, affine=affine, status=status,
                                    inlier_mask=mask, winner=winner, box=st.box, flag=st.flag, K_crop=st.K_crop, trans=st.trans), stream)
    ranges = ws[:8 * V].view(torch.int32).view(V, 2)       # the first table of the workspace
    return DeviceDetection(st, boxes, n_in, affine, status, winner, mask, ranges, keep=(ws, a))


class stages:
    """Thin wrappers over the per-stage entries (device tensors in, device tensors out); what ``opdet_detect`` enqueues in this order"""

    @staticmethod
    def ranges(b_ids, count, cap, views, stream=None):
        out = torch.empty(views, 2, dtype=torch.int32, device=b_ids.device)
        launch("opdet_ranges", dict(b_ids=b_ids, count=count, cap=cap, V=views, ranges=out), stream)
        return out

    @staticmethod
    def score(mkpts0, mkpts1, ranges, trials, seed, min_matches=6, reproj=6.0, stream=None):
        """-> ``samples [V, trials, 3]``, ``cnt [V, trials]``"""
        V, dev = ranges.shape[0], mkpts0.device
        samples = torch.empty(V, trials, 3, dtype=torch.int32, device=dev)
        cnt = torch.empty(V, trials, dtype=torch.int32, device=dev)
        launch("opdet_score", dict(mk0=mkpts0, mk1=mkpts1, ranges=ranges, cap=mkpts0.shape[0], V=V, trials=trials, min_matches=min_matches,
                                   reproj_thr=reproj, seed=seed, samples=samples, cnt=cnt), stream)
        return samples, cnt

    @staticmethod
    def select(mkpts0, mkpts1, ranges, count, samples, cnt, min_matches=6, reproj=6.0, confidence=0.99, stream=None):
        """-> ``best [V]``, ``n_inliers [V]``, ``status [V]``, ``inlier_mask [cap]``"""
        V, trials, dev = cnt.shape[0], cnt.shape[1], mkpts0.device
        best, n_in, status = (torch.empty(V, dtype=torch.int32, device=dev) for _ in range(3))
        mask = torch.zeros(mkpts0.shape[0], dtype=torch.uint8, device=dev)
        launch("opdet_select", dict(mk0=mkpts0, mk1=mkpts1, ranges=ranges, count=count, samples=samples, cnt=cnt, cap=mkpts0.shape[0], V=V,
                                    trials=trials, min_matches=min_matches, reproj_thr=reproj, confidence=confidence, best=best, n_inliers=n_in,
                                    status=status, inlier_mask=mask), stream)
        return best, n_in, status, mask

    @staticmethod
    def fit_box(mkpts0, mkpts1, ranges, view_hw, query_hw, n_inliers, status, mask, stream=None):
        """Updates ``n_inliers``, ``status`` and ``mask`` in place; returns ``affine [V, 6]``, ``boxes [V, 4]``"""
        V, dev = ranges.shape[0], mkpts0.device
        affine = torch.empty(V, 6, dtype=torch.float64, device=dev)
        boxes = torch.empty(V, 4, dtype=torch.int32, device=dev)
        launch("opdet_fit_box", dict(mk0=mkpts0, mk1=mkpts1, ranges=ranges, view_hw=view_hw, cap=mkpts0.shape[0], V=V, H=query_hw[0], W=query_hw[1],
                                     n_inliers=n_inliers, status=status, inlier_mask=mask, affine=affine, boxes=boxes), stream)
        return affine, boxes

    @staticmethod
    def vote(boxes, n_inliers, status, query_hw, K, crop_size=512, stream=None):
        """Updates ``status`` in place; returns ``winner [1]`` and the ``TrackState``"""
        dev = boxes.device
        winner = torch.empty(1, dtype=torch.int32, device=dev)
        st = TrackState(dev)
        K = K.contiguous().view(9)
        launch("opdet_vote", dict(boxes=boxes, n_inliers=n_inliers, status=status, V=boxes.shape[0], H=query_hw[0], W=query_hw[1], K=K, S=crop_size,
                                  winner=winner, box=st.box, flag=st.flag, K_crop=st.K_crop, trans=st.trans), stream)
        return winner, st
