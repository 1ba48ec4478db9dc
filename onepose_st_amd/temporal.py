"""Temporal pose refinement on the device (opt-in): the second half of the reference's ``inference_core``
(``inference.py:237-368``, ``src/utils/optimization_utils.py``).  For every frame ``t >= temp_thresh`` the 2D inliers of the previous
``temp_thresh`` frames are carried into frame ``t`` by a point tracker, appended with their 3D points to frame ``t``'s own matches, and
the PnP runs a second time on the larger table.

The reference tracks with CoTracker2 (a submodule and a checkpoint this project does not have).  The tracker here is the project's own: a
pyramidal, translation-only Lucas-Kanade tracker with a forward-backward check, float64 per point in a fixed order, specified entry by
entry in ``include/onepose_temporal.h`` and restated in numpy by ``tests/temporal_oracle.py``.  Which rows are carried, the crop <->
original mapping (``MKPT.map_to_original`` / ``map_to_crop``), the concatenation order and the second PnP are the reference's.

The kernels are HIP (``csrc/temporal_refine.hip`` in ``libonepose_temporal.so``).  CPU tensors raise :class:`hip.HipLibraryError` (no CPU
fallback); nothing is synchronised and no count is read on the host until :meth:`RefinedSequence.to_host`.
"""
from __future__ import annotations

import ctypes
import math

import numpy as np
import torch

from . import cabi, devargs, hip

_BINDING = cabi.Binding.of(__name__)                # the header is the one place a signature or a constant is written
library_path, load, check_arity, call = _BINDING.library_path, _BINDING.load, _BINDING.check_arity, _BINDING.call
launch = hip.launcher(_BINDING, globals())          # every stream-taking entry is called through it, by the header's parameter names
EXPORTED_SYMBOLS = _BINDING.exported_symbols
ABI_VERSION = _BINDING.abi_version
(DEGENERATE, OUT_OF_IMAGE, FB_FAIL, BAD_INPUT, FLAG_MAX_ITERS, LOST,
 MAX_LEVELS, MIN_WINDOW, MAX_WINDOW, MAX_ITERS, MAX_ROWS, MAX_SOURCES) = map(_BINDING.constant, (
    "DEGENERATE", "OUT_OF_IMAGE", "FB_FAIL", "BAD_INPUT", "FLAG_MAX_ITERS", "LOST",
    "MAX_LEVELS", "MIN_WINDOW", "MAX_WINDOW", "MAX_ITERS", "MAX_ROWS", "MAX_SOURCES"))
DEFAULTS = dict(levels=4, window=21, max_iters=30, eps=0.01, min_eig=1.0, fb_threshold=1.0)


class Pyramid:
    """``levels`` float32 levels of an ``H x W`` frame in one device allocation (``data``, uint8); ``level(l)`` is a view of it"""

    def __init__(self, data, H, W, levels):
        self.data, self.H, self.W, self.levels = data, H, W, levels

    def level(self, l: int) -> torch.Tensor:
        h, w, off = self.H, self.W, 0
        for _ in range(l):
            off += (h * w + 63) // 64 * 256
            h, w = (h + 1) // 2, (w + 1) // 2
        return self.data[off:off + 4 * h * w].view(torch.float32).view(h, w)


class Tracks:
    """What :func:`track` returns, on the device: ``pts [cap, 2]`` float64 (NaN on a lost row), ``flags [cap]`` and ``iterations [cap]``
    int32, ``fb_error [cap]`` float64; ``count``: the device count of the call (``None``: every row).  Rows at or past the count are not
    written."""

    def __init__(self, pts, flags, iterations, fb_error, count=None, keep=()):
        self.pts, self.flags, self.iterations, self.fb_error, self.count = pts, flags, iterations, fb_error, count
        self._keep = keep


class Queries:
    """What :func:`collect` returns, on the device: ``pts [cap, 2]`` float64 in the original image, ``pts_3d [cap, 3]`` float32, ``count``
    int32 ``[1]``"""

    def __init__(self, pts, pts_3d, count, keep=()):
        self.pts, self.pts_3d, self.count = pts, pts_3d, count
        self._keep = keep


def build_pyramid(frame_u8: torch.Tensor, levels: int = DEFAULTS["levels"], stream=None) -> Pyramid:
    """uint8 ``[H, W]`` gray frame on the device -> its :class:`Pyramid` (``optmp_pyramid``: one launch per level)"""
    hip.need_device([("frame_u8", frame_u8)])
    if frame_u8.dtype != torch.uint8 or frame_u8.dim() != 2:
        raise ValueError("frame_u8: uint8 [H, W]")
    H, W = int(frame_u8.shape[0]), int(frame_u8.shape[1])
    nbytes = load().optmp_pyramid_bytes(H, W, int(levels))
    if nbytes == 0:
        raise ValueError(f"levels={levels} for a {H} x {W} frame: levels in [1, {MAX_LEVELS}], sides in [2, 16384], the smallest level at least 2 x 2")
    frame_u8 = frame_u8.contiguous()
    data = torch.empty(nbytes, dtype=torch.uint8, device=frame_u8.device)
    launch("optmp_pyramid", dict(frame=frame_u8, H=H, W=W, levels=levels, pyramid=data, pyramid_bytes=nbytes), stream)
    return Pyramid(data, H, W, int(levels))


def track(src: Pyramid, dst: Pyramid, pts, *, count=None, guess=None, pts_3d=None, pose=None, K=None, scale=1, window=DEFAULTS["window"],
          max_iters=DEFAULTS["max_iters"], eps=DEFAULTS["eps"], min_eig=DEFAULTS["min_eig"], fb_threshold=DEFAULTS["fb_threshold"], out=None,
          stream=None) -> Tracks:
    """Track ``pts [cap, 2]`` (float64, level-0 pixels of ``src``) into ``dst`` (``optmp_track``: one wave per point).  ``guess [cap, 2]``:
    where to start each row (default: the point itself); ``pts_3d [cap, 3]`` float32 with ``pose [3, 4]``, ``K [3, 3]`` and ``scale``:
    start a row from the projection of its 3D point where that is usable.  ``fb_threshold=None``: no forward-backward check.  ``out``: a
    :class:`Tracks` to write into (rows at or past the count keep what it holds)."""
    if not isinstance(src, Pyramid) or not isinstance(dst, Pyramid):
        raise TypeError("src, dst: Pyramid (build_pyramid)")
    if (src.H, src.W, src.levels) != (dst.H, dst.W, dst.levels):
        raise ValueError(f"mismatched pyramids: {src.H} x {src.W} x {src.levels} and {dst.H} x {dst.W} x {dst.levels}")
    named = [("pts", pts)] + [(k, v) for k, v in (("guess", guess), ("pts_3d", pts_3d), ("count", count), ("pose", pose), ("K", K))
                              if isinstance(v, torch.Tensor)]
    hip.need_device(named)
    if int(window) != window or not MIN_WINDOW <= window <= MAX_WINDOW or window % 2 == 0:
        raise ValueError(f"window: an odd integer in [{MIN_WINDOW}, {MAX_WINDOW}]")
    if int(max_iters) != max_iters or not 1 <= max_iters <= MAX_ITERS:
        raise ValueError(f"max_iters: an integer in [1, {MAX_ITERS}]")
    if not (math.isfinite(eps) and eps > 0 and math.isfinite(min_eig) and min_eig >= 0 and math.isfinite(scale) and scale > 0):
        raise ValueError("eps > 0, min_eig >= 0, scale > 0, all finite")
    if fb_threshold is not None and not fb_threshold >= 0:
        raise ValueError("fb_threshold: a number >= 0, or None for no check")
    if pts.dim() != 2 or pts.shape[1] != 2 or pts.dtype != torch.float64 or not 1 <= pts.shape[0] <= MAX_ROWS:
        raise ValueError(f"pts: float64 [cap, 2], 1 <= cap <= {MAX_ROWS}")
    cap, dev = int(pts.shape[0]), pts.device
    pts = pts.contiguous()
    if guess is not None:
        if guess.dtype != torch.float64 or tuple(guess.shape) != (cap, 2):
            raise ValueError(f"guess: float64 [{cap}, 2]")
        guess = guess.contiguous()
    if (pts_3d is None) != (pose is None) or (pts_3d is None) != (K is None):
        raise ValueError("pts_3d, pose and K: all three or none")
    if pts_3d is not None:
        if pts_3d.dtype != torch.float32 or tuple(pts_3d.shape) != (cap, 3):
            raise ValueError(f"pts_3d: float32 [{cap}, 3]")
        pts_3d, pose, K = pts_3d.contiguous(), devargs.mat64("pose", pose, [(3, 4)], dev), devargs.mat64("K", K, [(3, 3)], dev)
    count = devargs.count_arg(count, dev)
    if out is None:
        out = Tracks(torch.empty(cap, 2, dtype=torch.float64, device=dev), torch.empty(cap, dtype=torch.int32, device=dev),
                     torch.empty(cap, dtype=torch.int32, device=dev), torch.empty(cap, dtype=torch.float64, device=dev))
    elif (tuple(out.pts.shape), tuple(out.flags.shape), tuple(out.iterations.shape), tuple(out.fb_error.shape)) != ((cap, 2), (cap,), (cap,), (cap,)):
        raise ValueError(f"out: Tracks of {cap} rows")
    launch("optmp_track", dict(src=src.data, dst=dst.data, H=src.H, W=src.W, levels=src.levels, pts=pts, count=count, cap=cap, guess=guess,
                               pts_3d=pts_3d, pose=pose, K=K, scale=scale, window=window, max_iters=max_iters, eps=eps, min_eig_threshold=min_eig,
                               fb_threshold=-1.0 if fb_threshold is None else fb_threshold, out_pts=out.pts, flags=out.flags,
                               iterations=out.iterations, fb_error=out.fb_error), stream)
    out.count = count
    out._keep = (src, dst, pts, guess, pts_3d, pose, K)
    return out


def collect(pts_2d, pts_3d, trans, *, count=None, mask=None, stream=None) -> Queries:
    """The selected rows of one frame's match table (``pts_2d [cap, 2]`` crop pixels, ``pts_3d [cap, 3]``, float32; rows below ``count``
    and, with ``mask [cap]`` uint8, of a non-zero mask), compacted in row order and mapped to the original image by the inverse of
    ``trans`` (``optmp_collect``)."""
    hip.need_device([("pts_2d", pts_2d), ("pts_3d", pts_3d)] + [(k, v) for k, v in (("trans", trans), ("count", count), ("mask", mask))
                                                             if isinstance(v, torch.Tensor) or k == "mask" and v is not None])
    pts_2d, pts_3d = devargs.point_tables("pts_2d", pts_2d, 2, "pts_3d", pts_3d, 3, max_rows=MAX_ROWS, min_rows=1)
    cap, dev = int(pts_2d.shape[0]), pts_2d.device
    if mask is not None:
        if mask.dtype != torch.uint8 or tuple(mask.shape) != (cap,):
            raise ValueError(f"mask: uint8 [{cap}]")
        mask = mask.contiguous()
    trans, count = devargs.mat64("trans", trans, [(3, 3)], dev), devargs.count_arg(count, dev)
    out = Queries(torch.empty(cap, 2, dtype=torch.float64, device=dev), torch.empty(cap, 3, dtype=torch.float32, device=dev),
                  torch.empty(1, dtype=torch.int32, device=dev), keep=(pts_2d, pts_3d, mask, trans, count))
    launch("optmp_collect", dict(pts_2d=pts_2d, pts_3d=pts_3d, count=count, cap=cap, mask=mask, trans=trans, pts_orig=out.pts, out_3d=out.pts_3d,
                                 out_count=out.count), stream)
    return out


def inject(own_2d, own_3d, own_count, sources, trans, *, stream=None):
    """The injected table of a frame: its own rows unchanged, then per ``(Queries, Tracks)`` pair of ``sources`` (oldest first) the rows
    that were not lost, mapped to the crop by ``trans`` and rounded to float32 (``optmp_inject``).  -> ``(pts_2d [cap_total, 2],
    pts_3d [cap_total, 3], count)``, which go straight into ``pnp_device.ransac_pnp(K_crop, pts_2d, pts_3d, count=count)``."""
    sources = list(sources)
    named = [("own_2d", own_2d), ("own_3d", own_3d)] + [(k, v) for k, v in (("own_count", own_count), ("trans", trans)) if isinstance(v, torch.Tensor)]
    for q, tr in sources:
        if not isinstance(q, Queries) or not isinstance(tr, Tracks):
            raise TypeError("sources: (Queries, Tracks) pairs")
        named += [("source pts_3d", q.pts_3d), ("source pts", tr.pts), ("source flags", tr.flags)]
    hip.need_device(named)
    own_2d, own_3d = devargs.point_tables("own_2d", own_2d, 2, "own_3d", own_3d, 3, min_rows=1)
    cap_own, dev = int(own_2d.shape[0]), own_2d.device
    if len(sources) > MAX_SOURCES:
        raise ValueError(f"at most {MAX_SOURCES} sources")
    caps = []
    for q, tr in sources:
        cap = int(tr.pts.shape[0])
        if tuple(q.pts_3d.shape) != (cap, 3) or tuple(tr.pts.shape) != (cap, 2) or tuple(tr.flags.shape) != (cap,) or cap < 1:
            raise ValueError("a source's Queries and Tracks must have the same number of rows")
        if q.pts_3d.dtype != torch.float32 or tr.pts.dtype != torch.float64 or tr.flags.dtype != torch.int32:
            raise ValueError("a source: pts_3d float32, tracked pts float64, flags int32")
        if not (q.pts_3d.is_contiguous() and tr.pts.is_contiguous() and tr.flags.is_contiguous()):
            raise ValueError("a source's tensors must be contiguous")
        caps.append(cap)
    cap_total = cap_own + sum(caps)
    if cap_total > MAX_ROWS:
        raise ValueError(f"at most {MAX_ROWS} rows")
    trans, own_count = devargs.mat64("trans", trans, [(3, 3)], dev), devargs.count_arg(own_count, dev)
    out_2d = torch.empty(cap_total, 2, dtype=torch.float32, device=dev)
    out_3d = torch.empty(cap_total, 3, dtype=torch.float32, device=dev)
    out_count = torch.empty(1, dtype=torch.int32, device=dev)
    n = len(sources)
    table = lambda tensors: (ctypes.c_void_p * max(n, 1))(*[None if t is None else t.data_ptr() for t in tensors])
    # a source's count: the Tracks' own (the rows the tracker wrote); the capacity when it tracked every row
    a_pts, a_3d, a_flags = table([tr.pts for _, tr in sources]), table([q.pts_3d for q, _ in sources]), table([tr.flags for _, tr in sources])
    a_count = table([tr.count for _, tr in sources])
    a_cap = (ctypes.c_int * max(n, 1))(*caps)
    launch("optmp_inject", dict(own_2d=own_2d, own_3d=own_3d, own_count=own_count, cap_own=cap_own, src_pts=a_pts, src_3d=a_3d, src_flags=a_flags,
                                src_count=a_count, src_cap=ctypes.cast(a_cap, ctypes.c_void_p), n_sources=n, trans=trans, out_2d=out_2d,
                                out_3d=out_3d, out_count=out_count, cap_total=cap_total), stream)
    return out_2d, out_3d, out_count


class RefinedSequence:
    """What :func:`refine_sequence` returns: per frame ``None`` (an initialisation frame, ``t < temp_thresh``) or a dict of device
    results -- ``poses`` (``pnp_device.DevicePoses``), the injected table ``pts_2d`` / ``pts_3d`` / ``count`` and the frame's ``tracks``.
    :meth:`to_host` is the one read-back."""

    def __init__(self, frames):
        self.frames = frames

    def pack(self) -> torch.Tensor:
        parts = [f["poses"].pack(extra=(f["count"].view(torch.uint8),)) for f in self.frames if f is not None]
        return torch.cat(parts) if parts else torch.empty(0, dtype=torch.uint8)

    def to_host(self):
        """Per frame ``None`` or ``dict(pose [3, 4], inliers int64 (rows of the injected table), status, count)``"""
        packed = self.pack().cpu().numpy()
        out, o = [], 0
        for f in self.frames:
            if f is None:
                out.append(None)
                continue
            n_count = devargs.packed_bytes((f["count"],))
            n = f["poses"].packed_bytes + n_count
            ((pose, _, inliers),), (raw,) = f["poses"].unpack(packed[o:o + n], (n_count,))
            o += n
            out.append({"pose": pose, "inliers": inliers, "status": int(f["poses"].status_host[0]), "count": int(raw.view(np.int32)[0])})
        return out


def refine_sequence(frames, entries, K=None, *, temp_thresh=5, inliers_only=True, pose_guess=False, levels=DEFAULTS["levels"],
                    window=DEFAULTS["window"], max_iters=DEFAULTS["max_iters"], eps=DEFAULTS["eps"], min_eig=DEFAULTS["min_eig"],
                    fb_threshold=DEFAULTS["fb_threshold"], scale=1000, pnp_reprojection_error=7, confidence=0.99, trials=None, seed=1,
                    device=None) -> RefinedSequence:
    """The reference's second pass over a sequence, in frame order, everything enqueued on the current stream and nothing read.

    ``frames``: uint8 ``[H, W]`` gray frames (host arrays, or tensors on the device).  ``entries[t]``: what the first pass left of frame
    ``t``: ``pts_2d [cap, 2]`` (crop pixels) and ``pts_3d [cap, 3]`` float32 on the device, ``K_crop`` and ``trans`` (``[3, 3]``), and
    optionally ``count`` (device int32), ``mask`` (uint8 ``[cap]``: the first pass's inliers; the rows carried when ``inliers_only``) and
    ``pose`` (``[3, 4]``; with ``pose_guess`` and the full-frame ``K`` a carried point starts from its projection under frame ``t``'s
    first-pass pose).  A ring of ``temp_thresh + 1`` pyramids; each frame's pyramid and queries are built once; per frame
    ``t >= temp_thresh``: ``temp_thresh`` track launches (oldest source first), one inject, one ``pnp_device.ransac_pnp``."""
    from . import pnp_device
    if int(temp_thresh) != temp_thresh or not 1 <= temp_thresh <= MAX_SOURCES:
        raise ValueError(f"temp_thresh: an integer in [1, {MAX_SOURCES}]")
    frames, entries = list(frames), list(entries)
    if len(frames) != len(entries):
        raise ValueError("one entry per frame")
    if pose_guess and K is None:
        raise ValueError("pose_guess needs the full-frame K")
    kw_pnp = dict(scale=scale, pnp_reprojection_error=pnp_reprojection_error, confidence=confidence, seed=seed)
    if trials is not None:
        kw_pnp["trials"] = trials
    kw_track = dict(window=window, max_iters=max_iters, eps=eps, min_eig=min_eig, fb_threshold=fb_threshold)
    ring, out = {}, []                                  # t -> (Pyramid, Queries) of the last temp_thresh + 1 frames
    for t, (frame, e) in enumerate(zip(frames, entries)):
        dev = e["pts_2d"].device if device is None else device
        if not isinstance(frame, torch.Tensor):
            frame = torch.from_numpy(np.ascontiguousarray(frame, dtype=np.uint8)).to(dev)
        pyr = build_pyramid(frame, levels)
        mask = e.get("mask") if inliers_only else None
        if inliers_only and mask is None:
            raise ValueError("inliers_only needs every entry's inlier mask")
        ring[t] = (pyr, collect(e["pts_2d"], e["pts_3d"], e["trans"], count=e.get("count"), mask=mask))
        ring.pop(t - temp_thresh - 1, None)
        if t < temp_thresh:
            out.append(None)
            continue
        sources = []
        for s in range(t - temp_thresh, t):
            src, q = ring[s]
            guess = dict(pts_3d=q.pts_3d, pose=e["pose"], K=K, scale=1) if pose_guess else {}
            sources.append((q, track(src, pyr, q.pts, count=q.count, **guess, **kw_track)))
        pts_2d, pts_3d, count = inject(e["pts_2d"], e["pts_3d"], e.get("count"), sources, e["trans"])
        poses = pnp_device.ransac_pnp(e["K_crop"], pts_2d, pts_3d, count=count, **kw_pnp)
        out.append({"poses": poses, "pts_2d": pts_2d, "pts_3d": pts_3d, "count": count, "tracks": [tr for _, tr in sources]})
    return RefinedSequence(out)
