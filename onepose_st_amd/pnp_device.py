"""Device PnP: the pose of a frame from the matcher's device-side matches, without a host round trip (opt-in; ``pnp.ransac_PnP`` on the
host stays the default).

The float64 work is HIP (``csrc/pnp_device.hip`` in ``libonepose_pnp_device.so``, include/onepose_pnp_device.h).  Like the host solver
this is the project's own estimator, not a restatement of pycolmap; only the ``use_pycolmap_ransac=True`` policy exists here: P3P
samples, every root scored on every match, a fixed number of trials.  ``solver="dlt6"`` and the adaptive policy raise
``NotImplementedError``; CPU tensors raise :class:`hip.HipLibraryError` (no CPU fallback).

The specification (``tests/pnp_device_oracle.py`` restates it in numpy float64, one function per stage):

1. ``ranges`` + ``prep``: a frame's rows ``[begin, end)`` by binary search in the ascending ``b_ids``; per row ``X = scale * pts3d``, the
   pixel and ``ray = K^-1 (u, v, 1)`` in float64.  ``count`` is clamped to the capacity, rows at or beyond it are never read, a row whose
   ``b_ids`` lies outside ``[0, frames)`` belongs to no frame.
2. ``sample``: trial ``t`` of frame ``f`` draws ``k = 0, 1, 2`` with ``h = mix(seed + G * (((f << 32 | t) * 4 + k) + 1))`` (``G =
   0x9E3779B97F4A7C15``, ``mix`` the splitmix64 finaliser, arithmetic mod 2^64); index ``k`` is ``h % (n - k)`` stepped past the earlier
   picks in ascending order.  A frame of fewer than 4 rows runs no trials.
3. ``p3p``: the host solver's ``p3p_poses`` (Grunert's quartic, Ferrari, three Newton steps, triangle alignment): up to four poses per
   trial, the valid roots first in the solver's order, ``4 * trials`` slots per frame, unused slots NaN.
4. ``score``: ``count_inliers``' expression on every row of the frame in row order: ``zc > 1e-12``, ``e2 < thr2``,
   ``cost += e2 if inlier else thr2``.  A hypothesis with a non-finite entry: count 0, cost inf.
5. ``select``: the winner under the total order (count descending, cost ascending, trial ascending, root ascending) among the
   hypotheses with a count above 0; its inlier mask; status bit ``STATUS_NEEDS_MORE`` when the frame has at least 4 rows and the host's
   ``needed_for(count) = ceil(log(1 - confidence) / log(1 - w^3))`` (1 when ``w^3 > 1 - 1e-12``, ``MAX_NEEDED`` when ``w^3 <= 1e-12`` or
   above it) exceeds ``trials``.
6. ``refine``: the host's ``finish``: ``refine_lm`` (lambda 1e-3, x 0.3 on an accepted step while above 1e-9, x 10 on a rejected one, at
   most 8 tries per iteration, 20 iterations, stop at a relative cost decrease below 1e-12) on the masked rows, the inlier set
   re-evaluated, a second round unless it is unchanged.  Fewer than 4 inliers: status ``STATUS_NO_POSE``, the identity pose, an empty
   mask.  ``t`` is divided by ``scale``.

Nothing is synchronised and the match count is never read on the host: every launch is sized by the capacity.
"""
from __future__ import annotations

import math

import numpy as np
import torch

from . import cabi, devargs, hip

_BINDING = cabi.Binding.of(__name__)                # the header is the one place a signature or a constant is written
library_path, load, check_arity, call = _BINDING.library_path, _BINDING.load, _BINDING.check_arity, _BINDING.call
launch = hip.launcher(_BINDING, globals())          # every stream-taking entry is called through it, by the header's parameter names
EXPORTED_SYMBOLS = _BINDING.exported_symbols
ABI_VERSION = _BINDING.abi_version
(MAX_TRIALS, DEFAULT_TRIALS, MAX_ROWS, MAX_FRAMES, ROW_DOUBLES, SELECT_BLOCK, SCORE_CHUNK, STATUS_NO_POSE, STATUS_NEEDS_MORE, MIN_INLIERS,
 MAX_NEEDED) = map(_BINDING.constant, (
    "MAX_TRIALS", "DEFAULT_TRIALS", "MAX_ROWS", "MAX_FRAMES", "ROW_DOUBLES", "SELECT_BLOCK", "SCORE_CHUNK", "STATUS_NO_POSE", "STATUS_NEEDS_MORE",
    "MIN_INLIERS", "MAX_NEEDED"))


def _check_policy(solver, use_pycolmap_ransac) -> None:
    if solver not in (None, "p3p"):
        raise NotImplementedError(f"solver={solver!r}: the device path implements P3P only (the host's pnp.ransac_PnP has the 6-point DLT)")
    if not use_pycolmap_ransac:
        raise NotImplementedError("the adaptive policy (use_pycolmap_ransac=False) exists on the host only: pnp.ransac_PnP")


class _Inputs:
    """The checked device tensors of one call"""

    def __init__(self, K, pts_2d, pts_3d, count, b_ids, frames):
        hip.need_device([("pts_2d", pts_2d), ("pts_3d", pts_3d)] + [(k, v) for k, v in (("K", K), ("count", count), ("b_ids", b_ids))
                                                                    if isinstance(v, torch.Tensor)])
        dev = pts_2d.device
        pts_2d, pts_3d = devargs.point_tables("pts_2d", pts_2d, 2, "pts_3d", pts_3d, 3)
        self.frames = int(frames)
        if not 1 <= self.frames <= MAX_FRAMES:
            raise ValueError(f"frames: an integer in [1, {MAX_FRAMES}]")
        n = pts_2d.shape[0]
        if n > MAX_ROWS:
            raise ValueError(f"at most {MAX_ROWS} rows")
        self.pts_2d, self.pts_3d, count, b_ids = devargs.at_least_one_row(pts_2d, pts_3d, count, b_ids)
        self.cap = self.pts_2d.shape[0]
        self.count = devargs.count_arg(count, dev, default=n)
        if b_ids is None:
            if self.frames != 1:
                raise ValueError("frames > 1 needs b_ids")
        elif b_ids.dtype != torch.int64 or tuple(b_ids.shape) != (self.cap,):
            raise ValueError(f"b_ids: int64 [{self.cap}]")
        self.b_ids = None if b_ids is None else b_ids.contiguous()
        (self.K, self.k_shared), self.dev = devargs.k_table(K, self.frames, dev), dev


def check_ransac_options(reproj_name, reproj, confidence, trials, max_trials):
    """The options this estimator and ``detect_device``'s share: the inlier threshold (under the caller's name for it), the confidence
    and the number of trials"""
    if not (math.isfinite(reproj) and reproj > 0):
        raise ValueError(f"{reproj_name}: a finite number > 0")
    if not 0 < confidence < 1:
        raise ValueError("confidence: in (0, 1)")
    if int(trials) != trials or not 1 <= trials <= max_trials:
        raise ValueError(f"trials: an integer in [1, {max_trials}]")


def _check_options(scale, reproj, confidence, trials):
    if not (math.isfinite(scale) and scale > 0):
        raise ValueError("scale: a finite number > 0")
    check_ransac_options("pnp_reprojection_error", reproj, confidence, trials, MAX_TRIALS)


class DevicePoses:
    """What :func:`ransac_pnp` returns, on the device: ``pose [F, 3, 4]`` float64, ``n_inliers [F]`` and ``status [F]`` int32,
    ``inlier_mask [cap]`` uint8 over the rows (``ranges [F, 2]``: the rows of every frame)."""

    def __init__(self, pose, n_inliers, status, inlier_mask, ranges, keep=()):
        self.pose, self.n_inliers, self.status, self.inlier_mask, self.ranges = pose, n_inliers, status, inlier_mask, ranges
        self.status_host = None
        self._keep = keep                                   # the inputs and the workspace stay referenced while the work may be queued

    @property
    def needs_more(self) -> torch.Tensor:
        return (self.status & STATUS_NEEDS_MORE) != 0

    def pack(self, extra=()) -> torch.Tensor:
        """One uint8 device tensor for one read-back: pose, status, ranges, the inlier mask, then every 1-D uint8 device tensor of
        ``extra`` (what a caller wants read with the pose); :meth:`unpack` reads it on the host"""
        return devargs.pack((*self._packed(), *extra))

    def _packed(self):
        return self.pose, self.status, self.ranges, self.inlier_mask

    @property
    def packed_bytes(self) -> int:
        """The length of :meth:`pack` without extras"""
        return devargs.packed_bytes(self._packed())

    def unpack(self, packed, extra_sizes=()):
        """:meth:`to_host`'s result from the host bytes of :meth:`pack` (a uint8 numpy array); with ``extra_sizes`` a pair of that and the
        byte arrays of the extras"""
        (pose, status, ranges, mask, *_), o = devargs.unpack(packed, devargs.packed_layout(self._packed()))
        self.status_host = status.copy()                    # the status of every frame, read with the rest
        out = []
        for f in range(pose.shape[0]):
            b, e = int(ranges[f, 0]), int(ranges[f, 1])
            ok = not (int(status[f]) & STATUS_NO_POSE)
            p = pose[f].copy()
            homo = np.concatenate([p, np.array([[0.0, 0.0, 0.0, 1.0]])], axis=0)
            inl = np.nonzero(mask[b:e])[0].astype(np.int64) if ok else np.array([], dtype=np.int64)
            out.append((p, homo, inl))
        if not extra_sizes:
            return out
        extras = []
        for n in extra_sizes:
            extras.append(packed[o:o + n].copy()); o += n
        return out, extras

    def to_host(self):
        """Per frame ``(pose [3, 4], pose_homo [4, 4], inliers int64)`` in ``pnp.ransac_PnP``'s shape (the inliers are row numbers
        within the frame); a frame without a pose: the identity and an empty array.  The one read-back."""
        return self.unpack(self.pack().cpu().numpy())


def ransac_pnp(K, pts_2d, pts_3d, *, count=None, b_ids=None, frames=1, scale=1, pnp_reprojection_error=5, confidence=0.99,
               trials=DEFAULT_TRIALS, seed=1, stream=None, solver=None, use_pycolmap_ransac=True) -> DevicePoses:
    """The module docstring's estimator on device tensors ``pts_2d [cap, 2]``, ``pts_3d [cap, 3]`` float32; ``count`` int32[1] on the
    device (default: all rows), ``b_ids [cap]`` int64 ascending with ``frames`` frames (default: one frame); ``K [3, 3]`` shared or
    ``[frames, 3, 3]``.  Everything is enqueued on ``stream`` (default: the current one); nothing is read back."""
    _check_policy(solver, use_pycolmap_ransac)
    _check_options(float(scale), float(pnp_reprojection_error), float(confidence), trials)
    a = _Inputs(K, pts_2d, pts_3d, count, b_ids, frames)
    F, cap, dev = a.frames, a.cap, a.dev
    nbytes = load().oppnpd_workspace_bytes(cap, F, int(trials))
    if nbytes == 0:
        raise ValueError("frames x trials: too many hypotheses for one call")
    with hip.enqueue_on(dev, stream):
        ws = torch.empty(nbytes, dtype=torch.uint8, device=dev)
        pose = torch.empty(F, 3, 4, dtype=torch.float64, device=dev)
        n_in = torch.zeros(F, dtype=torch.int32, device=dev)
        status = torch.zeros(F, dtype=torch.int32, device=dev)
        mask = torch.zeros(cap, dtype=torch.uint8, device=dev)
        launch("oppnpd_solve", dict(pts2d=a.pts_2d, pts3d=a.pts_3d, count=a.count, cap=cap, b_ids=a.b_ids, F=F, K=a.K, k_shared=a.k_shared,
                                    scale=scale, reproj_err_px=pnp_reprojection_error, confidence=confidence, trials=trials, seed=seed,
                                    workspace=ws, workspace_bytes=nbytes, pose=pose, n_inliers=n_in, status=status, inlier_mask=mask), stream)
    ranges = ws[:8 * F].view(torch.int32).view(F, 2)       # the first table of the workspace
    return DevicePoses(pose, n_in, status, mask, ranges, keep=(ws, a))


def enqueue_after(pending_frame, K, **kw) -> DevicePoses:
    """:func:`ransac_pnp` on a ``PendingFrame``'s own capacity-sized result buffers (``count``, ``b_ids``, ``mk3d``, ``mk2d``), before its
    ``finish()``: the current stream is ordered behind the frame's last kernel and the solve is enqueued there.  The match count is not
    read on the host.  ``frames`` defaults to the frame's batch size."""
    pf = pending_frame
    _check_policy(kw.get("solver"), kw.get("use_pycolmap_ransac", True))
    if getattr(pf, "_slot", None) is not None:              # the one-call frame: its fine stage may be kept back or on its side stream
        hip.call("ophip_frame_order_after_fine", hip.stream_handle())
        bufs = pf.bufs if pf.bufs is not None else pf._block_views()
    else:
        torch.cuda.current_stream(pf.dev).wait_event(pf.event)
        bufs = pf.bufs
    mk2d = bufs["mkf"] if pf.fine_on and bufs.get("mkf") is not None else bufs["mkc"]
    kw.setdefault("frames", pf.B)
    out = ransac_pnp(K, mk2d, bufs["mk3d"], count=bufs["count"], b_ids=bufs["b_ids"], **kw)
    out._keep = (*out._keep, bufs)
    return out


class stages:
    """Thin wrappers over the per-stage entries (device tensors in, device tensors out); what ``oppnpd_solve`` enqueues in this order"""

    @staticmethod
    def ranges(b_ids, count, cap, frames, stream=None):
        out = torch.empty(frames, 2, dtype=torch.int32, device=count.device)
        launch("oppnpd_ranges", dict(b_ids=b_ids, count=count, cap=cap, F=frames, ranges=out), stream)
        return out

    @staticmethod
    def prep(K, pts_2d, pts_3d, count, b_ids, frames, scale=1.0, stream=None):
        K, k_shared = devargs.k_table(K, int(frames), pts_2d.device)
        cap = pts_2d.shape[0]
        rows = torch.zeros(cap, ROW_DOUBLES, dtype=torch.float64, device=pts_2d.device)
        launch("oppnpd_prep", dict(pts2d=pts_2d, pts3d=pts_3d, count=count, cap=cap, b_ids=b_ids, F=frames, K=K, k_shared=k_shared, scale=scale,
                                   rows=rows), stream)
        return rows

    @staticmethod
    def sample(ranges, trials, seed, stream=None):
        F = ranges.shape[0]
        out = torch.empty(F, trials, 3, dtype=torch.int32, device=ranges.device)
        launch("oppnpd_sample", dict(ranges=ranges, F=F, trials=trials, seed=seed, samples=out), stream)
        return out

    @staticmethod
    def p3p(rows, ranges, samples, stream=None):
        F, trials = samples.shape[0], samples.shape[1]
        hyps = torch.empty(F, 4 * trials, 3, 4, dtype=torch.float64, device=rows.device)
        nsol = torch.empty(F, trials, dtype=torch.int32, device=rows.device)
        launch("oppnpd_p3p", dict(rows=rows, ranges=ranges, samples=samples, cap=rows.shape[0], F=F, trials=trials, hyps=hyps, nsol=nsol), stream)
        return hyps, nsol

    @staticmethod
    def score(rows, ranges, K, hyps, reproj, stream=None):
        F, H = hyps.shape[0], hyps.shape[1]
        K, k_shared = devargs.k_table(K, F, rows.device)
        cnt = torch.empty(F, H, dtype=torch.int32, device=rows.device)
        cost = torch.empty(F, H, dtype=torch.float64, device=rows.device)
        launch("oppnpd_score", dict(rows=rows, ranges=ranges, K=K, k_shared=k_shared, hyps=hyps, cap=rows.shape[0], F=F, H=H, reproj_err_px=reproj,
                                    cnt=cnt, cost=cost), stream)
        return cnt, cost

    @staticmethod
    def select(cnt, cost, rows, ranges, count, K, hyps, reproj, confidence, trials, stream=None):
        F, H, dev = hyps.shape[0], hyps.shape[1], rows.device
        K, k_shared = devargs.k_table(K, F, rows.device)
        nblk = (H + SELECT_BLOCK - 1) // SELECT_BLOCK
        partial = torch.empty(16 * F * nblk, dtype=torch.uint8, device=dev)
        best, n_in, status = (torch.empty(F, dtype=torch.int32, device=dev) for _ in range(3))
        mask = torch.zeros(rows.shape[0], dtype=torch.uint8, device=dev)
        launch("oppnpd_select", dict(cnt=cnt, cost=cost, rows=rows, ranges=ranges, count=count, K=K, k_shared=k_shared, hyps=hyps, cap=rows.shape[0],
                                     F=F, H=H, reproj_err_px=reproj, confidence=confidence, trials=trials, partial=partial, best=best,
                                     n_inliers=n_in, status=status, inlier_mask=mask), stream)
        return best, n_in, status, mask

    @staticmethod
    def refine(rows, ranges, K, hyps, best, n_inliers, status, mask, reproj, scale=1.0, stream=None):
        """Updates ``n_inliers``, ``status`` and ``mask`` in place; returns ``pose [F, 3, 4]``"""
        F, H = hyps.shape[0], hyps.shape[1]
        K, k_shared = devargs.k_table(K, F, rows.device)
        pose = torch.empty(F, 3, 4, dtype=torch.float64, device=rows.device)
        launch("oppnpd_refine", dict(rows=rows, ranges=ranges, K=K, k_shared=k_shared, hyps=hyps, best=best, cap=rows.shape[0], F=F, H=H,
                                     reproj_err_px=reproj, scale=scale, pose=pose, n_inliers=n_inliers, status=status, inlier_mask=mask), stream)
        return pose
