"""Frame-loop harness and input formats around the matcher.

What the reference does per sequence (``inference.py:100-190``) with the pieces either side of ``OnePosePlus_model``:

* the per-object 3D block comes from ``anno_3d_average.npz`` + ``anno_3d_average_coarse.npz`` (keys ``keypoints3d [N,3]``,
  ``descriptors3d [dim,N]``, ``scores3d [N,1]``; reader ``OnePosePlus_inference_dataset.py:112-169``), truncated to
  ``shape3d`` points by a random index draw when larger, and is kept on the device for the whole sequence;
* frame 0 and every frame after a failed pose (< 20 PnP inliers) get their object box from a detector, every other frame
  from the projection of the 3D box with the previous pose (``local_feature_2D_detector.py:249-266``);
* the box is cropped and resized to 512 x 512 with the intrinsics updated accordingly
  (``local_feature_2D_detector.py:164-190``, ``data_utils.py:249-290``), matched, and solved by RANSAC-PnP
  (``metric_utils.py:121-209`` with reprojection error 7, scale 1000).

Here the crop runs on the GPU from the uploaded uint8 frame (``ophip_crop_resize_gray``), the matcher is the HIP path and
PnP the C++ solver.  ``SequenceRunner`` takes the object detector as a callable ``detector(frame, t) -> box``: the LoFTR 2D-2D
detector of row f-3 is :class:`onepose_st_amd.detector.LocalFeatureObjectDetector` (its ``__call__``).  ``.npz`` files are read
with ``allow_pickle=False``.
"""
from __future__ import annotations

import os

import numpy as np
import torch

from . import devargs, hip
from .pnp import ransac_PnP

MIN_INLIERS = 20          # inference.py:152


def load_object_block(avg_anno3d_file: str, device, shape3d: int | None = None, generator: torch.Generator | None = None) -> dict:
    """``read_anno3d`` (``OnePosePlus_inference_dataset.py:112-169``): returns the batch-1 device tensors the model reads
    (``keypoints3d [1,N,3]``, ``descriptors3d_db [1,dim,N]``, ``descriptors3d_coarse_db [1,dim_c,N]``) plus ``scores3d``,
    ``scores3d_coarse`` (host) and ``num_3d_orig``.  With ``shape3d`` smaller than the stored point count the points are
    drawn like ``pad_keypoints3d_random`` / ``pad_features3d_random`` (``data_utils.py:222-246``): ``torch.randint`` with
    replacement, the same index for every array."""
    root, ext = os.path.splitext(avg_anno3d_file)
    fine, coarse = np.load(avg_anno3d_file, allow_pickle=False), np.load(root + "_coarse" + ext, allow_pickle=False)
    for name, z in (("fine", fine), ("coarse", coarse)):
        for k in ("keypoints3d", "descriptors3d", "scores3d") if name == "fine" else ("descriptors3d", "scores3d"):
            if k not in z.files:
                raise KeyError(f"{name} annotation file lacks '{k}'")
    kp = torch.tensor(fine["keypoints3d"], dtype=torch.float32)                 # [N, 3]
    d_f = torch.tensor(fine["descriptors3d"], dtype=torch.float32)              # [dim, N]
    s_f = torch.tensor(fine["scores3d"], dtype=torch.float32)                   # [N, 1]
    d_c = torch.tensor(coarse["descriptors3d"], dtype=torch.float32)
    s_c = torch.tensor(coarse["scores3d"], dtype=torch.float32)
    n = kp.shape[0]
    if kp.dim() != 2 or kp.shape[1] != 3 or d_f.shape[1] != n or d_c.shape[1] != n:
        raise ValueError("annotation arrays disagree on the number of 3D points")
    if shape3d is not None and n > shape3d:
        idx = torch.randint(n, (shape3d,), generator=generator)
        kp, d_f, s_f, d_c, s_c = kp[idx], d_f[:, idx], s_f[idx, :], d_c[:, idx], s_c[idx, :]
    return {"keypoints3d": kp[None].to(device), "descriptors3d_db": d_f[None].to(device), "descriptors3d_coarse_db": d_c[None].to(device),
            "scores3d": s_f, "scores3d_coarse": s_c, "num_3d_orig": n}


def save_object_block(avg_anno3d_file: str, keypoints3d, descriptors3d, scores3d, descriptors3d_coarse, scores3d_coarse) -> None:
    """Writer of the same format (what ``feature_process.py:316-319,646-649`` stores), for tests and synthetic objects."""
    root, ext = os.path.splitext(avg_anno3d_file)
    np.savez(avg_anno3d_file, keypoints3d=np.asarray(keypoints3d, np.float32), descriptors3d=np.asarray(descriptors3d, np.float32),
             scores3d=np.asarray(scores3d, np.float32))
    np.savez(root + "_coarse" + ext, keypoints3d=np.asarray(keypoints3d, np.float32), descriptors3d=np.asarray(descriptors3d_coarse, np.float32),
             scores3d=np.asarray(scores3d_coarse, np.float32))


def crop_geometry(bbox, K, crop_size: int = 512):
    """``crop_img_by_bbox`` without the pixels: ``(K_crop [3,3], trans [3,3])`` for box ``[x0, y0, x1, y1]``.  The reference
    composes two ``get_affine_transform`` warps (``data_utils.py:32-62``): a shift of the box to the origin, then an
    isotropic scale ``crop_size / box_width`` that keeps the crop's vertical centre in the middle of the output."""
    x0, y0, x1, y1 = [float(v) for v in bbox]
    wb, hb = x1 - x0, y1 - y0
    if wb <= 0 or hb <= 0:
        raise ValueError("empty bounding box")
    s = crop_size / wb
    trans = np.array([[s, 0.0, -s * x0], [0.0, s, 0.5 * crop_size - s * (y0 + 0.5 * hb)], [0.0, 0.0, 1.0]])
    K = np.asarray(K, dtype=np.float64)
    return trans @ K[:3, :3], trans


def project_bbox(K, pose, bbox3d) -> np.ndarray:
    """``previous_pose_detect`` (``local_feature_2D_detector.py:263-266``): int32 ``[x0, y0, x1, y1]`` of the projected 3D box."""
    K, pose, pts = np.asarray(K, np.float64)[:3, :3], np.asarray(pose, np.float64)[:3, :4], np.asarray(bbox3d, np.float64).reshape(-1, 3)
    cam = pose[:, :3] @ pts.T + pose[:, 3:4]
    uv = K @ cam
    uv = (uv[:2] / uv[2:]).T
    return np.concatenate([uv.min(axis=0), uv.max(axis=0)]).astype(np.int32)


def crop_query(frame_u8: torch.Tensor, bbox, crop_size: int = 512) -> torch.Tensor:
    """uint8 ``[H, W]`` frame on the HIP device -> ``[1, 1, S, S]`` float query image in [0, 1] (``ophip_crop_resize_gray``)."""
    if frame_u8.dtype != torch.uint8 or frame_u8.dim() != 2 or not frame_u8.is_cuda:
        raise hip.HipLibraryError("crop_query needs a uint8 [H, W] frame on the HIP device (no CPU fallback)")
    frame_u8 = frame_u8.contiguous()
    out = torch.empty(1, 1, crop_size, crop_size, dtype=torch.float32, device=frame_u8.device)
    x0, y0, x1, y1 = [int(v) for v in bbox]
    hip.launch("ophip_crop_resize_gray", dict(image=frame_u8, H=frame_u8.shape[0], W=frame_u8.shape[1], x0=x0, y0=y0, x1=x1, y1=y1, S=crop_size,
                                              out=out))
    return out


class SequenceRunner:
    """The per-sequence loop of ``inference.py:136-190``.

    ``model``: an ``OnePosePlus_model`` on the device; ``object_block``: :func:`load_object_block`; ``K``: full-frame
    intrinsics; ``bbox3d [8, 3]``; ``detector(frame_u8_host, index) -> [x0, y0, x1, y1]``: the object detector used on
    frame 0 and after a failed pose.  ``run(frames)`` takes host uint8 ``[H, W]`` arrays and returns one record per frame:
    ``pose [3,4]``, ``inliers``, ``bbox``, ``K_crop``, ``trans``, ``num_matches``, ``redetected``.

    Within a sequence frame t + 1's crop depends on frame t's pose, so frames are processed strictly in order; the next
    frame's upload is queued on a side stream while the current one is matched.

    ``pnp="host"`` (the default): the matches are copied to the host and solved by ``pnp.ransac_PnP``.  ``pnp="device"``: the pose is
    solved on the device from ``data["mkpts_3d_db"]`` / ``data["mkpts_query_f"]`` (``pnp_device.ransac_pnp``) and only pose, status and
    inlier mask are read back; a frame whose status asks for more trials than ran falls back to the host call.

    ``track="host"`` (the default): the box of frame t + 1 is projected on the host from frame t's pose, so frame t + 1 is enqueued after
    frame t's pose has been read.  ``track="device"`` (needs ``pnp="device"``): box, crop intrinsics and crop are computed on the device
    from the device pose (``track_device``), and up to ``lookahead`` frames are enqueued before the oldest one's record is read (one
    packed read-back per frame, queued with the frame).  The device marks the frames the host loop would not have projected a box for
    (``track_device``'s flags); the frames enqueued past the first marked one are abandoned and the loop goes on from there as the host
    loop would (the detector, or the host solver's pose), so the records and the detector calls do not depend on ``lookahead``.
    ``crop_fn`` is not used then.  ``data`` also carries ``frame_index`` (host int) and ``crop_trans`` / ``K_crop`` (device float64
    ``[3, 3]``); a ``model`` without ``enqueue`` is called as ``model(data)`` and may fill ``mkpts_query_f`` / ``mkpts_3d_db`` from those
    without leaving the device.

    ``detect="host"`` (the default): ``detector(frame, t)`` gives the box of frame 0 and of every frame after a lost track as host
    integers.  ``detect="device"`` (needs ``track="device"`` and a detector with ``detect_state``, such as
    ``detector.LocalFeatureObjectDetector(vote="device")``): ``detector.detect_state(frame_u8_dev, K_dev, crop_size)`` gives that box's
    ``track_device.TrackState`` on the device, enqueued behind the frame's upload, and ``detector(...)`` is never called.

    ``refine=None`` (the default): the records are the first pass's.  ``refine="device"`` (needs ``pnp="device"``; either ``track``): the
    reference's second pass (``inference.py:237-368``) runs after the loop on what the unchanged first pass left of every frame (its
    match tables, ``K_crop``, ``trans`` and final inlier rows): ``temporal.refine_sequence`` carries the inliers of the previous
    ``temp_thresh`` frames into every frame ``t >= temp_thresh`` and solves the pose again (``inliers_only`` and ``refine_options``: its
    keywords).  It feeds nothing back, so every other key of a record is what a ``refine=None`` run gives; every record gains
    ``pose_refined``, ``inliers_refined`` (rows of the injected table: the frame's own rows first) and ``refined`` (false for the
    initialisation frames, which repeat the first-pass pose).  A refined frame whose status asks for more trials is solved by the host
    solver on the injected table, as in the first pass.
    """

    MAX_LOOKAHEAD = 8         # the one-call frame keeps 16 frames in flight at most

    def __init__(self, model, object_block: dict, K, bbox3d, detector, crop_size: int = 512, pnp_reprojection_error: float = 7,
                 pnp_scale: float = 1000, min_inliers: int = MIN_INLIERS, crop_fn=crop_query, pnp: str = "host", track: str = "host",
                 lookahead: int = 2, detect: str = "host", refine: str | None = None, temp_thresh: int = 5, inliers_only: bool = True,
                 refine_options: dict | None = None):
        if pnp not in ("host", "device"):
            raise ValueError(f"pnp={pnp!r}: 'host' or 'device'")
        if track not in ("host", "device"):
            raise ValueError(f"track={track!r}: 'host' or 'device'")
        if track == "device" and pnp != "device":
            raise ValueError("track='device' needs pnp='device': the box is computed from the device pose")
        if detect not in ("host", "device"):
            raise ValueError(f"detect={detect!r}: 'host' or 'device'")
        if detect == "device" and track != "device":
            raise ValueError("detect='device' needs track='device': the detected box stays on the device")
        if detect == "device" and not hasattr(detector, "detect_state"):
            raise ValueError("detect='device' needs a detector with detect_state(frame_u8_dev, K_dev, crop_size)")
        if int(lookahead) != lookahead or not 1 <= lookahead <= self.MAX_LOOKAHEAD:
            raise ValueError(f"lookahead: an integer in [1, {self.MAX_LOOKAHEAD}]")
        if refine not in (None, "device"):
            raise ValueError(f"refine={refine!r}: None or 'device'")
        if refine == "device" and pnp != "device":
            raise ValueError("refine='device' needs pnp='device': the second pose is solved on the device")
        if int(temp_thresh) != temp_thresh or temp_thresh < 1:
            raise ValueError("temp_thresh: an integer >= 1")
        self.refine, self.temp_thresh, self.inliers_only, self.refine_options = refine, int(temp_thresh), bool(inliers_only), dict(refine_options or {})
        self._kept = None                                 # refine: the match tables of every recorded frame, in record order
        self.pnp, self.track, self.lookahead, self.detect = pnp, track, int(lookahead), detect
        self.model, self.block, self.crop_fn = model, object_block, crop_fn
        self.K, self.bbox3d, self.detector = np.asarray(K, np.float64), np.asarray(bbox3d, np.float64), detector
        self.crop_size, self.reproj, self.scale, self.min_inliers = crop_size, pnp_reprojection_error, pnp_scale, min_inliers
        self.device = object_block["keypoints3d"].device
        self._copy_stream = torch.cuda.Stream(device=self.device) if self.device.type == "cuda" else None

    def _upload(self, frame):
        host = torch.from_numpy(np.ascontiguousarray(frame, dtype=np.uint8))
        if self._copy_stream is None:
            return host.to(self.device), None
        with torch.cuda.stream(self._copy_stream):
            dev = host.pin_memory().to(self.device, non_blocking=True)
            ev = torch.cuda.Event()
            ev.record()
        return dev, ev

    def run(self, frames):
        frames = list(frames)
        self._kept = [] if self.refine else None
        records = self._run_device_tracked(frames) if self.track == "device" else self._run_host_tracked(frames)
        if self.refine:
            self._refine(frames, records)
        return records

    def _keep_tables(self, data):
        """refine: a frame's match tables as its record saw them (copies: a model may reuse its buffers for a later frame)"""
        if self._kept is not None:
            self._kept.append((data["mkpts_query_f"].float().clone(), data["mkpts_3d_db"].float().clone()))

    def _refine(self, frames, records):
        """The second pass (class docstring): reads ``self._kept`` and the records, adds the three keys"""
        from . import pnp_device, temporal
        dev, entries = self.device, []
        up = lambda a, dt: torch.from_numpy(np.ascontiguousarray(a, dtype=dt)).to(dev)
        for rec, (mk2d, mk3d) in zip(records, self._kept):
            n = int(mk2d.shape[0])
            mask = np.zeros(max(n, 1), np.uint8)
            mask[np.asarray(rec["inliers"], np.int64)] = 1
            mk2d, mk3d, count, _ = devargs.at_least_one_row(mk2d, mk3d, devargs.count_arg(n, dev))
            entries.append({"pts_2d": mk2d, "pts_3d": mk3d, "count": count, "mask": up(mask, np.uint8),
                            "K_crop": up(rec["K_crop"], np.float64), "trans": up(rec["trans"], np.float64), "pose": up(rec["pose"], np.float64)})
        self._kept = None
        kw = dict(scale=self.scale, pnp_reprojection_error=self.reproj)
        kw.update(self.refine_options)
        seq = temporal.refine_sequence(frames, entries, self.K[:3, :3], temp_thresh=self.temp_thresh, inliers_only=self.inliers_only, device=dev, **kw)
        for rec, dev_out, got in zip(records, seq.frames, seq.to_host()):
            if got is None:
                rec.update(pose_refined=rec["pose"], inliers_refined=rec["inliers"], refined=False)
                continue
            pose, inliers = got["pose"], got["inliers"]
            if got["status"] & pnp_device.STATUS_NEEDS_MORE:        # the host's open-ended policy on the injected table, as in _device_pose
                k = got["count"]
                pose, _, inliers = ransac_PnP(rec["K_crop"], dev_out["pts_2d"][:k].cpu().numpy(), dev_out["pts_3d"][:k].cpu().numpy(), scale=kw["scale"],
                                              pnp_reprojection_error=kw["pnp_reprojection_error"], img_hw=[self.crop_size, self.crop_size],
                                              use_pycolmap_ransac=True)
            rec.update(pose_refined=pose, inliers_refined=inliers, refined=True)

    def _run_host_tracked(self, frames):
        records = []
        nxt = self._upload(frames[0]) if frames else None
        prev = None                                   # (pose, inliers) of the previous frame
        for t, frame in enumerate(frames):
            dev_frame, ev = nxt
            nxt = self._upload(frames[t + 1]) if t + 1 < len(frames) else None
            redetect = prev is None or len(prev[1]) < self.min_inliers
            bbox = np.asarray(self.detector(frame, t) if redetect else project_bbox(self.K, prev[0], self.bbox3d)).astype(np.int32)
            if bbox[2] <= bbox[0] or bbox[3] <= bbox[1]:      # degenerate projection: treat as a lost track
                redetect = True
                bbox = np.asarray(self.detector(frame, t)).astype(np.int32)
            K_crop, trans = crop_geometry(bbox, self.K, self.crop_size)
            if ev is not None:
                torch.cuda.current_stream().wait_event(ev)
            data = {"query_image": self.crop_fn(dev_frame, bbox, self.crop_size), "keypoints3d": self.block["keypoints3d"],
                    "descriptors3d_db": self.block["descriptors3d_db"], "descriptors3d_coarse_db": self.block["descriptors3d_coarse_db"]}
            with torch.no_grad():
                self.model(data)
            if self.pnp == "device":
                pose, inliers, num_matches = self._device_pose(K_crop, data)
                self._keep_tables(data)
                prev = (pose, inliers)
                records.append({"pose": pose, "inliers": inliers, "bbox": bbox, "K_crop": K_crop, "trans": trans,
                                "num_matches": num_matches, "redetected": bool(redetect)})
                continue
            mk3d, mk2d = data["mkpts_3d_db"].cpu().numpy(), data["mkpts_query_f"].cpu().numpy()
            pose, _, inliers = ransac_PnP(K_crop, mk2d, mk3d, scale=self.scale, pnp_reprojection_error=self.reproj,
                                          img_hw=[self.crop_size, self.crop_size], use_pycolmap_ransac=True)
            prev = (pose, inliers)
            records.append({"pose": pose, "inliers": inliers, "bbox": bbox, "K_crop": K_crop, "trans": trans,
                            "num_matches": int(mk2d.shape[0]), "redetected": bool(redetect)})
        return records

    def _device_pose(self, K_crop, data):
        """``pnp="device"``: the matches stay on the device; the read-back is pose, status and inlier mask"""
        from . import pnp_device
        mk3d, mk2d = data["mkpts_3d_db"].float().contiguous(), data["mkpts_query_f"].float().contiguous()
        out = pnp_device.ransac_pnp(K_crop, mk2d, mk3d, scale=self.scale, pnp_reprojection_error=self.reproj)
        (pose, _, inliers), = out.to_host()
        if int(out.status_host[0]) & pnp_device.STATUS_NEEDS_MORE:          # the confidence asks for more trials than ran: the host's open-ended policy
            pose, _, inliers = ransac_PnP(K_crop, mk2d.cpu().numpy(), mk3d.cpu().numpy(), scale=self.scale, pnp_reprojection_error=self.reproj,
                                          img_hw=[self.crop_size, self.crop_size], use_pycolmap_ransac=True)
        return pose, inliers, int(mk2d.shape[0])

    # ---- track="device" ------------------------------------------------------------------------------------------------------------------
    def _enqueue_tracked(self, t, frame_dev, state):
        """Crop, matcher, pose and the next frame's state of frame ``t``, and the packed read-back into pinned memory: all enqueued on the
        current stream, nothing read.  -> the in-flight entry"""
        from . import pnp_device, track_device
        data = {"query_image": track_device.crop(frame_dev, state, self.crop_size), "keypoints3d": self.block["keypoints3d"],
                "descriptors3d_db": self.block["descriptors3d_db"], "descriptors3d_coarse_db": self.block["descriptors3d_coarse_db"],
                "frame_index": t, "crop_trans": state.trans, "K_crop": state.K_crop}
        kw = dict(scale=self.scale, pnp_reprojection_error=self.reproj)
        pend = None
        with torch.no_grad():
            if hasattr(self.model, "enqueue"):
                pend = self.model.enqueue(data)
                poses = pnp_device.enqueue_after(pend, state.K_crop, **kw)
            else:
                self.model(data)
                poses = pnp_device.ransac_pnp(state.K_crop, data["mkpts_query_f"].float().contiguous(), data["mkpts_3d_db"].float().contiguous(), **kw)
        nxt = track_device.next_box(poses, state, self._K_dev, self._bbox3d_dev, min_inliers=self.min_inliers, crop_size=self.crop_size)
        packed = poses.pack(extra=(state.blob, nxt.flag.view(torch.uint8)))
        pool = self._pins.setdefault(packed.numel(), [])
        pin = pool.pop() if pool else torch.empty(packed.numel(), dtype=torch.uint8).pin_memory()
        pin.copy_(packed, non_blocking=True)
        ev = torch.cuda.Event()
        ev.record()
        return {"t": t, "state": state, "next": nxt, "data": data, "pend": pend, "poses": poses, "pin": pin, "event": ev}

    def _release(self, entry, abandon=False):
        if abandon and entry["pend"] is not None:
            entry["pend"].close()
        pool = self._pins.setdefault(entry["pin"].numel(), [])
        if len(pool) < 2 * self.MAX_LOOKAHEAD:      # copies into a reused buffer are ordered by the stream; the host reads behind its own event
            pool.append(entry["pin"])

    def _host_pose(self, K_crop, data):
        mk3d, mk2d = data["mkpts_3d_db"].float().cpu().numpy(), data["mkpts_query_f"].float().cpu().numpy()
        pose, _, inliers = ransac_PnP(K_crop, mk2d, mk3d, scale=self.scale, pnp_reprojection_error=self.reproj,
                                      img_hw=[self.crop_size, self.crop_size], use_pycolmap_ransac=True)
        return pose, inliers

    def _run_device_tracked(self, frames):
        from collections import deque

        from . import pnp_device, track_device
        if self.device.type != "cuda":
            raise hip.HipLibraryError("track='device' needs the object block on the HIP device (no CPU fallback)")
        self._K_dev = torch.as_tensor(np.ascontiguousarray(self.K[:3, :3])).to(self.device)
        self._bbox3d_dev = torch.as_tensor(np.ascontiguousarray(self.bbox3d.reshape(8, 3))).to(self.device)
        self._pins = {}
        n, records, uploads, queue = len(frames), [], {}, deque()
        t_next, state, redetected = 0, None, {}             # state None: the host loop would call the detector for frame t_next
        while len(records) < n:
            while len(queue) < self.lookahead and t_next < n:
                t = t_next
                for k in (t, t + 1):
                    if k < n and k not in uploads:
                        uploads[k] = self._upload(frames[k])
                if state is None and self.detect == "device":      # the same place, the box never leaves the device
                    if uploads[t][1] is not None:
                        torch.cuda.current_stream().wait_event(uploads[t][1])
                    state, redetected[t] = self.detector.detect_state(uploads[t][0], self._K_dev, self.crop_size), True
                if state is None:                           # frame 0 and the frame after a lost one: the queue is empty here
                    bbox = np.asarray(self.detector(frames[t], t)).astype(np.int32)
                    state, redetected[t] = track_device.set_box(bbox, self._K_dev, self.crop_size), True
                frame_dev, ev = uploads[t]
                if ev is not None:
                    torch.cuda.current_stream().wait_event(ev)
                entry = self._enqueue_tracked(t, frame_dev, state)
                queue.append(entry)
                state, t_next = entry["next"], t + 1
            e = queue.popleft()
            t, data, rerun = e["t"], e["data"], False
            if e["pend"] is not None:
                before = getattr(self.model, "lazy_reruns", 0)
                e["pend"].finish()
                rerun = getattr(self.model, "lazy_reruns", 0) != before
            e["event"].synchronize()                        # the frame's one read-back, queued with the frame
            ((pose, _, inliers),), (raw_state, raw_flag) = e["poses"].unpack(e["pin"].numpy(), (track_device.STATE_BYTES, 4))
            status, next_flag = int(e["poses"].status_host[0]), int(raw_flag.view(np.int32)[0])
            bbox, _, K_crop, trans = track_device.TrackState.unpack(raw_state)
            self._release(e)
            host_step = rerun or bool(status & pnp_device.STATUS_NEEDS_MORE)
            if rerun:                                       # finish() ran the frame again: the early solve saw the abandoned run's buffers
                out = pnp_device.ransac_pnp(e["state"].K_crop, data["mkpts_query_f"].float().contiguous(), data["mkpts_3d_db"].float().contiguous(),
                                            scale=self.scale, pnp_reprojection_error=self.reproj)
                (pose, _, inliers), = out.to_host()
                status = int(out.status_host[0])
            if status & pnp_device.STATUS_NEEDS_MORE:       # the host's open-ended policy replaces the pose, as in the host-tracked loop
                pose, inliers = self._host_pose(K_crop, data)
            records.append({"pose": pose, "inliers": inliers, "bbox": bbox, "K_crop": K_crop, "trans": trans,
                            "num_matches": int(data["mkpts_3d_db"].shape[0]), "redetected": bool(redetected.pop(t, False))})
            self._keep_tables(data)
            uploads.pop(t, None)
            if not host_step and next_flag == 0:
                continue
            # rewind: what was enqueued past this frame used a box the host loop would not have used
            while queue:
                self._release(queue.popleft(), abandon=True)
            t_next, state = t + 1, None
            if host_step and len(inliers) >= self.min_inliers:      # the pose changed on the host: its box, as the host loop computes it
                nb = project_bbox(self.K, pose, self.bbox3d)
                if nb[2] > nb[0] and nb[3] > nb[1]:
                    state = track_device.set_box(nb, self._K_dev, self.crop_size)
        return records
