"""``LocalFeatureObjectDetector`` -- the 2D object detector in front of the matcher.

Mirrors ``src/local_feature_object_detector/local_feature_2D_detector.py:40-280``: the query frame is matched against ~15
reference views of the object with LoFTR (:class:`onepose_st_amd.loftr.LoFTR_for_OnePose_Plus` on the HIP kernels), each view votes
a box -- the view's four corners through the RANSAC affinity of its matches, or a fixed 1000 x 1000 box around the image centre
when it has fewer than 6 matches -- and the view with the most inliers wins; the box is cropped to 512 x 512 with the intrinsics
updated (``crop_img_by_bbox``: :func:`onepose_st_amd.frameloop.crop_geometry` / ``ophip_crop_resize_gray``).

What differs from the reference by design: reference views of one common size (any size: the reference's are 512 x 512 crops against a
full frame) are matched as a batch -- consecutive chunks of views, one matcher call and one read-back per chunk, as many views per chunk
as ``LoFTR_for_OnePose_Plus.coarse_batch_bytes`` fits into ``batch_budget_bytes`` (:func:`plan_chunks`), with
``conf_matrix="lazy"`` for a dual-softmax matcher since nothing here reads the matrix; the per-view RANSACs run in parallel on the host
-- instead of one call and one synchronisation per view.  Views of mixed sizes keep the view-by-view loop.  What differs by necessity:
the reference views are handed over as arrays (its constructor reads a COLMAP model and decodes images with ``cv2`` / ``natsort``, neither of which exists here); ``cv2.estimateAffine2D`` is the build's own RANSAC
(``oppnp_estimate_affine2d``, parity unpinned).  The control flow, thresholds, integer truncations and the tie rule (first view
among equals) are the reference's.  ``detect`` plugs into :class:`onepose_st_amd.frameloop.SequenceRunner` as its ``detector``.
"""
from __future__ import annotations

import numpy as np
import torch

from . import frameloop
from .pnp import estimate_affine2d


def sample_reference_views(n_images: int, n_ref_view: int = 15) -> list:
    """``load_ref_view_images`` (``local_feature_2D_detector.py:66-76``): every ``len // n_ref_view``-th image starting at index 1 of
    the naturally sorted image list."""
    gap = n_images // n_ref_view
    if gap < 1:
        raise ValueError(f"{n_images} reference images for n_ref_view = {n_ref_view}: the reference's sample gap would be 0")
    return list(range(1, n_images, gap))


def plan_chunks(n_views: int, estimate, budget) -> list:
    """The batched call's chunks: ``[(first, last + 1), ...]``, consecutive, covering ``range(n_views)`` once, each of the largest
    ``Vc >= 1`` with ``estimate(Vc) <= budget`` (the last one may be shorter).  ``estimate(Vc) -> bytes`` is non-decreasing in ``Vc``;
    ``budget=None``: no limit, one chunk.  A budget below ``estimate(1)`` still gives one view per chunk."""
    vc = n_views if budget is None else 1
    while vc < n_views and estimate(vc + 1) <= budget:
        vc += 1
    return [(a, min(a + vc, n_views)) for a in range(0, n_views, max(vc, 1))]


class LocalFeatureObjectDetector:
    def __init__(self, matcher, db_imgs, device=None, min_matches: int = 6, ransac_reproj_threshold: float = 6.0, vote: str = "host",
                 batch_budget_bytes=4 << 30):
        """``matcher``: a ``LoFTR_for_OnePose_Plus`` on the device; ``db_imgs``: the reference views, grayscale ``[H, W]`` uint8 arrays
        (or float tensors in [0, 1]) -- already sampled (:func:`sample_reference_views`).  ``vote="device"`` adds
        :meth:`match_worker_device` and :meth:`detect_state`: the per-view RANSACs, the vote and the box's track state on the device
        (``detect_device``), nothing read back; the host path stays as it is.  ``batch_budget_bytes``: what the coarse stage of one batched
        matcher call may allocate by the matcher's own estimate (``coarse_batch_bytes``; the fine stage's buffers are not part of it);
        the views are split into chunks under it.  4 GiB is a design constant, not a measurement; ``None``: no
        limit."""
        if vote not in ("host", "device"):
            raise ValueError(f"vote={vote!r}: 'host' or 'device'")
        self.vote = vote
        if batch_budget_bytes is not None and int(batch_budget_bytes) < 0:
            raise ValueError("batch_budget_bytes: a number of bytes >= 0, or None for no limit")
        self.batch_budget_bytes = None if batch_budget_bytes is None else int(batch_budget_bytes)
        if vote == "device":                          # only then: ``hasattr(detector, "detect_state")`` is how SequenceRunner asks
            self.match_worker_device, self.detect_state, self._view_hw_dev = self._match_worker_device, self._detect_state, None
        self.matcher = matcher
        self.device = torch.device(device) if device is not None else next(matcher.parameters()).device
        self.min_matches, self.thr = int(min_matches), float(ransac_reproj_threshold)
        self.db_imgs, self.db_corners_homo = [], []
        for im in db_imgs:
            t = torch.as_tensor(np.asarray(im)) if not torch.is_tensor(im) else im
            t = (t.float() / 255.0) if t.dtype == torch.uint8 else t.float()
            if t.dim() != 2:
                raise ValueError("reference views must be [H, W] grayscale images")
            self.db_imgs.append(t[None, None].contiguous().to(self.device))          # torch.from_numpy(img)[None][None] / 255.0
            H, W = t.shape
            self.db_corners_homo.append(np.array([[0, 0, 1], [W, 0, 1], [0, H, 1], [W, H, 1]], dtype=np.float64).T)      # 3 x 4

    # ------------------------------------------------------------------------------------------
    def common_view_size(self):
        """``(H, W)`` when all reference views have one size (any size, not necessarily the query's), else ``None``"""
        sizes = {tuple(v.shape[-2:]) for v in self.db_imgs}
        return next(iter(sizes)) if len(sizes) == 1 else None

    def plans_batch(self, batched: bool = True) -> bool:
        """whether :meth:`match_worker` / :meth:`match_worker_device` take the batched call: more than one view, all of one size"""
        return bool(batched) and len(self.db_imgs) > 1 and self.common_view_size() is not None

    def _batched_matches(self, query):
        """the batched form: one matcher call per chunk of views; yields each call's ``(mkpts0_f, mkpts1_f, b_ids)`` with ``b_ids``
        counted from view 0.  A generator that hands out the match lists only: a call's data dict -- its ``conf_matrix``, or the rows a
        lazy one keeps -- is dropped before the next chunk's call, or the chunks would add up to what the budget was to avoid"""
        # nothing here reads conf_matrix: a dual-softmax LoFTR matcher is asked not to store it (sinkhorn needs the matrix; a stand-in
        # without a config or without the estimate is called as it always was, all views at once)
        cfg = getattr(self.matcher, "config", None)
        lazy = cfg is not None and cfg["match_coarse"]["match_type"] == "dual_softmax"
        kw = {"conf_matrix": "lazy", "budget_bytes": self.batch_budget_bytes} if lazy else {}
        hv, wv = self.common_view_size()
        hw0_c, hw1_c = (hv // 8, wv // 8), (query.shape[-2] // 8, query.shape[-1] // 8)
        estimate = getattr(self.matcher, "coarse_batch_bytes", None)
        chunks = plan_chunks(len(self.db_imgs), lambda n: estimate(n, hw0_c, hw1_c, lazy), self.batch_budget_bytes if estimate is not None else None)
        for a, b in chunks:
            pair = {"image0": torch.cat(self.db_imgs[a:b], 0), "image1": query}
            self.matcher(pair, **kw)
            out = (pair["mkpts0_f"], pair["mkpts1_f"], pair["b_ids"] + a)
            del pair
            yield out

    def _vote(self, idx: int, mkpts0: np.ndarray, mkpts1: np.ndarray, hw) -> dict:
        """One view's vote (:104-144): the view's corners through the RANSAC affinity of its matches; a fixed 1000 x 1000 box around the
        image centre when the view has fewer than ``min_matches`` matches (or RANSAC finds no model)."""
        H, W = hw
        centre = {"inliers": np.empty((0)), "bbox": np.array([W // 2 - 500, H // 2 - 500, W // 2 + 500, H // 2 + 500])}
        if mkpts0.shape[0] < self.min_matches:
            return centre
        affine, inliers = estimate_affine2d(mkpts0, mkpts1, ransac_reproj_threshold=self.thr)
        if affine is None:                                        # (cv2 returns None when RANSAC finds no model: the reference would raise)
            return centre
        corners = (affine @ self.db_corners_homo[idx]).T.astype(np.int32)            # 4 x 2, truncated like the reference
        lo, hi = corners.min(axis=0), corners.max(axis=0)
        return {"inliers": inliers, "bbox": np.array([lo[0], lo[1], hi[0], hi[1]])}

    @torch.no_grad()
    def match_worker(self, query: torch.Tensor, batched: bool = True) -> dict:
        """``{view index: {"inliers", "bbox"}}`` for every reference view (:89-144).  The reference loops over the views -- one LoFTR call
        and one device -> host copy each; here views of one common size (the query may have another) go through the matcher as a batch
        (``image0 [V, 1, H, W]`` against the one query: every kernel launched once over V pairs), in chunks under
        ``batch_budget_bytes`` -- one call and one copy of the matches per chunk, one of each when all views fit; the per-view RANSACs
        then run side by side on host threads (``oppnp_estimate_affine2d`` releases the GIL).  ``batched=False`` keeps the view-by-view
        form (views of mixed sizes take it as well); both give the same boxes."""
        hw = tuple(query.shape[-2:])
        if not self.plans_batch(batched):
            out = {}
            for idx, view in enumerate(self.db_imgs):
                pair = {"image0": view, "image1": query}
                self.matcher(pair)
                both = torch.cat([pair["mkpts0_f"], pair["mkpts1_f"]], 1).cpu().numpy()
                out[idx] = self._vote(idx, both[:, :2], both[:, 2:], hw)
            return out
        # one read-back per chunk; b_ids counts from the chunk's first view
        packed = np.concatenate([torch.cat([b_ids.to(torch.float32)[:, None], mk0, mk1], 1).cpu().numpy()
                                 for mk0, mk1, b_ids in self._batched_matches(query)], 0)
        view_of = packed[:, 0].astype(np.int64)
        # matches arrive in ascending (view, cell) order: a view's matches are one slice
        bounds = np.searchsorted(view_of, np.arange(len(self.db_imgs) + 1))
        from concurrent.futures import ThreadPoolExecutor
        with ThreadPoolExecutor(max_workers=min(8, len(self.db_imgs))) as ex:
            votes = list(ex.map(lambda i: self._vote(i, packed[bounds[i]:bounds[i + 1], 1:3], packed[bounds[i]:bounds[i + 1], 3:5], hw),
                                range(len(self.db_imgs))))
        return dict(enumerate(votes))

    # ---- vote="device" -------------------------------------------------------------------------------
    @torch.no_grad()
    def _match_worker_device(self, query: torch.Tensor, K=None, crop_size: int = 512):
        """:meth:`match_worker` with the vote on the device -> a ``detect_device.DeviceDetection``.  The matcher calls are the batched
        ones (one per chunk of views, ``b_ids`` counted from the chunk's first view); views of mixed sizes take one call each with
        their view index as ``b_ids``; the device tensors are concatenated, then ONE vote call.  ``K`` (default: the identity) and ``crop_size`` go into the winning box's track state.  Nothing is read back after
        the matcher's own count."""
        from . import detect_device
        hw = tuple(query.shape[-2:])
        if self.plans_batch():
            parts = list(self._batched_matches(query))
        else:
            parts = []
            for idx, view in enumerate(self.db_imgs):
                pair = {"image0": view, "image1": query}
                self.matcher(pair)
                parts.append((pair["mkpts0_f"], pair["mkpts1_f"], torch.full((pair["mkpts0_f"].shape[0],), idx, dtype=torch.int64, device=self.device)))
        mk0, mk1, b_ids = parts[0] if len(parts) == 1 else (torch.cat([p[k] for p in parts], 0) for k in range(3))
        if self._view_hw_dev is None:
            self._view_hw_dev = torch.tensor([list(v.shape[-2:]) for v in self.db_imgs], dtype=torch.int32).to(self.device)
        if K is None:
            K = torch.eye(3, dtype=torch.float64, device=self.device)
        return detect_device.vote(mk0.float().contiguous(), mk1.float().contiguous(), b_ids.to(torch.int64), self._view_hw_dev, hw, K,
                                  crop_size=crop_size, min_matches=self.min_matches, ransac_reproj_threshold=self.thr)

    def _detect_state(self, frame_u8_dev: torch.Tensor, K_dev, crop_size: int = 512):
        """The ``track_device.TrackState`` of the detected box for a uint8 ``[H, W]`` frame on the device and the full-frame intrinsics
        ``K_dev`` (float64 on the device): what ``track_device.set_box(self(frame), K, crop_size)`` gives, without a host round trip."""
        if not torch.is_tensor(frame_u8_dev) or frame_u8_dev.dtype != torch.uint8 or frame_u8_dev.dim() != 2:
            raise ValueError("detect_state: a uint8 [H, W] grayscale frame on the device")
        query = (frame_u8_dev.float() / 255.0)[None, None].contiguous()
        return self._match_worker_device(query, K_dev, crop_size).state

    def detect_by_matching(self, query: torch.Tensor) -> np.ndarray:
        """(:146-162): the box of the view with the most inliers; among equals the first view (the reference's stable descending sort)"""
        votes = self.match_worker(query)
        best = max(votes, key=lambda i: (votes[i]["inliers"].sum(), -i))
        return votes[best]["bbox"]

    def detect(self, query_img, K, crop_size: int = 512):
        """(:208-247) ``query_img``: the full frame, uint8 ``[H, W]`` (host array or device tensor).  Returns ``(bbox, crop [1, 1, S, S]
        float on the device, K_crop, transformation)`` like the reference."""
        frame = torch.as_tensor(np.ascontiguousarray(query_img)) if not torch.is_tensor(query_img) else query_img
        if frame.dtype != torch.uint8 or frame.dim() != 2:
            raise ValueError("detect: a uint8 [H, W] grayscale frame")
        frame = frame.to(self.device)
        query = (frame.float() / 255.0)[None, None].contiguous()
        bbox = np.asarray(self.detect_by_matching(query)).astype(np.int32)
        K_crop, trans = frameloop.crop_geometry(bbox, K, crop_size)
        crop = frameloop.crop_query(frame, bbox, crop_size)
        return bbox, crop, K_crop, trans

    def __call__(self, frame, index=None):
        """the ``detector(frame, t) -> [x0, y0, x1, y1]`` hook of :class:`onepose_st_amd.frameloop.SequenceRunner`"""
        frame_t = torch.as_tensor(np.ascontiguousarray(frame)).to(self.device)
        query = (frame_t.float() / 255.0)[None, None].contiguous()
        return np.asarray(self.detect_by_matching(query)).astype(np.int32)

    def previous_pose_detect(self, K, pre_pose, bbox3D_corner):
        """(:249-266) the box of the projected 3D bounding box under the previous pose"""
        return frameloop.project_bbox(K, pre_pose, bbox3D_corner)
