"""The supervised signals of training and validation on the device, forward only (opt-in): what the reference's
``train_onepose_plus.py`` computes from labelled frames and the matcher's outputs -- the ground-truth assignment of a frame
(``src/datasets/OnePosePlus_dataset.py:341-445`` and ``build_assignmatrix``), ``fine_supervision`` and ``Loss``
(``src/lightning_model/losses.py``) -- without a dense ``[N, M]`` ground truth and without a torch pass over ``conf_matrix``.

The specification is ``include/ext/onepose_supervision.h`` (``tests/supervision_oracle.py`` restates it in numpy).  The ground truth is
SPARSE: a 3D point has at most one cell, so ``gt_j [B, N]`` and ``gt_xy [B, N, 2]`` hold everything the dense ``conf_matrix_gt`` /
``fine_location_matrix_gt`` hold (:meth:`GroundTruth.to_dense` / :meth:`GroundTruth.from_dense` for callers of reference code).  The focal
loss is one streaming pass over ``conf_matrix`` with float64 sums in a fixed order: two runs give identical bytes.

Not here: the backward pass (the gradient of these losses at the matcher's four feature tensors is ``loss_backward.py``; the backward of
the transformers, the window gather and the backbone behind them is not built), the homography augmentation (the training-mode forward and its random GT padding: ``train_forward.py``),
``mask0`` / ``mask1`` loss weights, an image scale other than 1 in :func:`ground_truth`, and a loss taken from the lazy ``conf_matrix``
without making the matrix.

The kernels are HIP (``csrc/supervision.hip`` in ``libonepose_supervision.so``, the row of ``cabi.ADDONS``).  CPU tensors raise
:class:`hip.HipLibraryError` (no CPU fallback); nothing is synchronised and no count is read on the host until ``Loss.forward``'s one
packed read-back of three scalars and a status.
"""
from __future__ import annotations

import numpy as np
import torch

from . import cabi, devargs, hip
from .lazy_conf import LazyConfMatrixBase

_BINDING = cabi.Binding.of(__name__)                # the header is the one place a signature or a constant is written
library_path, load, check_arity, call, order = _BINDING.library_path, _BINDING.load, _BINDING.check_arity, _BINDING.call, _BINDING.order
launch = hip.launcher(_BINDING, globals())          # every stream-taking entry is called through it, by the header's parameter names
EXPORTED_SYMBOLS = _BINDING.exported_symbols
ABI_VERSION = _BINDING.abi_version
BLOCK, MAX_BATCH, MAX_ROWS, OK, NONE, FORCED, EMPTY = map(_BINDING.constant, ("BLOCK", "MAX_BATCH", "MAX_ROWS", "OK", "NONE", "FORCED", "EMPTY"))
NO_GT_XY = -50.0                                    # the reference's fill of fine_location_matrix_gt
DENSE_BUDGET_BYTES = 1 << 30


def _f32(name, m, shapes, dev):
    """A pose or intrinsics table as float32 (the reference's ``.to(torch.float)``), contiguous, on ``dev``"""
    if not isinstance(m, torch.Tensor):
        m = torch.as_tensor(np.asarray(m, dtype=np.float64), device=dev)
    if not any(len(s) == m.dim() and all(w in (None, n) for w, n in zip(s, m.shape)) for s in shapes):
        raise ValueError(f"{name}: {' or '.join(str(list(s)).replace('None', 'B') for s in shapes)}")
    return m.to(torch.float32).contiguous()


class GroundTruth:
    """The sparse ground truth of ``B`` frames on the device: ``gt_j [B, N]`` int64 (the cell of a 3D point, -1: none), ``gt_xy [B, N, 2]``
    float32 (its projection in pixels, (-50, -50): none), ``gt_i [B, M]`` int64 (the point of a cell, -1: none), ``n_gt [B]`` int32;
    ``hw_c``: the coarse grid."""

    def __init__(self, gt_j, gt_xy, gt_i, n_gt, hw_c, keep=()):
        self.gt_j, self.gt_xy, self.gt_i, self.n_gt, self.hw_c = gt_j, gt_xy, gt_i, n_gt, (int(hw_c[0]), int(hw_c[1]))
        self._keep = keep                                   # the inputs and the workspace stay referenced while the work may be queued

    @property
    def shape(self):
        return (*self.gt_j.shape, self.gt_i.shape[1])       # (B, N, M)

    def to_dense(self, budget_bytes=DENSE_BUDGET_BYTES):
        """-> the reference's ``conf_matrix_gt [B, N, M]`` int16 and ``fine_location_matrix_gt [B, N, M, 2]`` float32: 10 bytes per
        entry, refused above ``budget_bytes``.  For tests and for callers of reference code: nothing here reads the dense form."""
        B, N, M = self.shape
        if 10 * B * N * M > budget_bytes:
            raise ValueError(f"the dense ground truth of [{B}, {N}, {M}] takes {10 * B * N * M} bytes, budget_bytes is {budget_bytes}")
        dev = self.gt_j.device
        conf = torch.zeros(B, N, M, dtype=torch.int16, device=dev)
        loc = torch.full((B, N, M, 2), NO_GT_XY, dtype=torch.float32, device=dev)
        have = self.gt_j >= 0
        b, i = have.nonzero(as_tuple=True)
        j = self.gt_j[b, i]
        conf[b, i, j] = 1
        loc[b, i, j] = self.gt_xy[b, i]
        return conf, loc

    @classmethod
    def from_dense(cls, conf_matrix_gt, fine_location_matrix_gt, hw_c=None):
        """The sparse form of a reference data loader's batch (``[B, N, M]`` and ``[B, N, M, 2]``, where they lie: on the device for the
        entries above): a torch ``max`` and a gather, no kernel.  A row with several entries keeps its first."""
        hip.need_tensors([("conf_matrix_gt", conf_matrix_gt), ("fine_location_matrix_gt", fine_location_matrix_gt)])
        if conf_matrix_gt.dim() != 3 or tuple(fine_location_matrix_gt.shape) != (*conf_matrix_gt.shape, 2):
            raise ValueError("conf_matrix_gt [B, N, M] and fine_location_matrix_gt [B, N, M, 2]")
        B, N, M = conf_matrix_gt.shape
        hit = conf_matrix_gt == 1
        val, j = hit.to(torch.uint8).max(dim=2)             # the first maximum
        have = val > 0
        gt_j = torch.where(have, j, torch.full_like(j, -1))
        xy = torch.gather(fine_location_matrix_gt.float(), 2, j.clamp(min=0)[:, :, None, None].expand(B, N, 1, 2))[:, :, 0]
        gt_xy = torch.where(have[..., None], xy, torch.full_like(xy, NO_GT_XY)).contiguous()
        gt_i = torch.full((B, M), -1, dtype=torch.int64, device=gt_j.device)
        b, i = have.nonzero(as_tuple=True)
        gt_i[b, gt_j[b, i]] = i
        return cls(gt_j.contiguous(), gt_xy, gt_i, have.sum(dim=1).to(torch.int32), hw_c if hw_c is not None else (1, M))


def _need_unit_scale(scale):
    if scale is None:
        return
    s = scale.detach().cpu().numpy() if isinstance(scale, torch.Tensor) else np.asarray(scale)
    if not np.all(s == 1):
        raise NotImplementedError("ground_truth with a query_image_scale other than 1: the reference's second rounding can then merge "
                                  "cells and its result depends on the order of a scatter")


def ground_truth(keypoints3d, point_ids, pose_gt, K, image_hw, *, counts=None, resolution=(8, 2), scale=None, stream=None) -> GroundTruth:
    """``keypoints3d [B or 1, N, 3]`` float32 (batch 1 or a stride-0 expand: one object for every frame), ``point_ids [B, A]`` int64 (the
    annotation's 3D index per annotated 2D keypoint, ``assign_matrix[1]``, in annotation order), ``pose_gt [B, 4, 4]`` and ``K [3, 3]`` or
    ``[B, 3, 3]`` (converted to float32 as the reference does), ``image_hw`` and the coarse stride ``resolution[0]``.  ``counts``: int32
    ``[B]`` on the device, the annotated rows of each frame (``None``: ``A``).  ``scale``: must be all ones (a host value; checked on the
    host).  The reference's quirks are kept and said in the header: NO depth test; first row of a cell wins.  Enqueued on ``stream``
    (default: the current one); nothing is read back."""
    _need_unit_scale(scale)
    named = [("keypoints3d", keypoints3d), ("point_ids", point_ids)] + [(k, v) for k, v in (("pose_gt", pose_gt), ("K", K), ("counts", counts))
                                                                          if isinstance(v, torch.Tensor)]
    hip.need_device(named)
    dev = keypoints3d.device
    if point_ids.dim() != 2 or point_ids.dtype != torch.int64 or point_ids.shape[0] < 1 or point_ids.shape[1] < 1:
        raise ValueError("point_ids: int64 [B, A] with at least one row")
    B, A = map(int, point_ids.shape)
    if keypoints3d.dim() != 3 or keypoints3d.shape[2] != 3 or keypoints3d.dtype != torch.float32 or keypoints3d.shape[0] not in (1, B) \
            or keypoints3d.shape[1] < 1:
        raise ValueError(f"keypoints3d: float32 [{B} or 1, N, 3]")
    if keypoints3d.stride(2) != 1 or keypoints3d.stride(1) != 3:
        keypoints3d = keypoints3d.contiguous()
    N = int(keypoints3d.shape[1])
    pose = _f32("pose_gt", pose_gt, [(B, 4, 4)], dev)
    Kf = _f32("K", K, [(3, 3), (B, 3, 3)], dev)
    if counts is not None and (counts.dtype != torch.int32 or tuple(counts.shape) != (B,)):
        raise ValueError(f"counts: int32 [{B}] on the device")
    H, W, s = int(image_hw[0]), int(image_hw[1]), int(resolution[0])
    if s < 1 or H < s or W < s:
        raise ValueError("image_hw: at least one coarse cell each way")
    hw_c = (H // s, W // s)
    M = hw_c[0] * hw_c[1]
    point_ids, counts = point_ids.contiguous(), None if counts is None else counts.contiguous()
    with hip.enqueue_on(dev, stream):
        owner = torch.empty(B, M, dtype=torch.int32, device=dev)
        gt_j = torch.empty(B, N, dtype=torch.int64, device=dev)
        gt_xy = torch.empty(B, N, 2, dtype=torch.float32, device=dev)
        gt_i = torch.empty(B, M, dtype=torch.int64, device=dev)
        n_gt = torch.empty(B, dtype=torch.int32, device=dev)
        launch("opsup_ground_truth", dict(keypoints3d=keypoints3d, kp_bstride=hip.bstride(keypoints3d), point_ids=point_ids, counts=counts,
                                          pose_gt=pose, K=Kf, k_shared=Kf.dim() == 2, B=B, N=N, A=A, H=H, W=W, stride=s, owner=owner, gt_j=gt_j,
                                          gt_xy=gt_xy, gt_i=gt_i, n_gt=n_gt), stream)
    return GroundTruth(gt_j, gt_xy, gt_i, n_gt, hw_c, keep=(keypoints3d, point_ids, counts, pose, Kf, owner))


def fine_targets(b_ids, i_ids, j_ids, gt: GroundTruth, w_c, *, count=None, resolution=(8, 2), radius=2, scale=None, out=None, stream=None):
    """``expec_f_gt [cap, 2]`` float32 of the matches ``(b_ids, i_ids, j_ids)`` (int64 ``[cap]``) against ``gt``; rows at or past the
    device ``count`` are not written.  ``scale``: float32 ``[B, 2]`` (``query_image_scale``) or ``None`` -- and then the coarse scale is
    the FINE one, the reference's ``else fine_scale`` on line 18 of ``fine_supervision.py``, kept literally."""
    named = [("b_ids", b_ids), ("i_ids", i_ids), ("j_ids", j_ids), ("gt_j", gt.gt_j), ("gt_xy", gt.gt_xy)]
    named += [(k, v) for k, v in (("scale", scale), ("out", out)) if v is not None]
    hip.need_device(named)
    dev = b_ids.device
    cap = int(b_ids.shape[0])
    for name, t in named[:3]:
        if t.dim() != 1 or t.shape[0] != cap or t.dtype != torch.int64:
            raise ValueError(f"{name}: int64 [{cap}]")
    B, N, _ = gt.shape
    if scale is not None:
        if tuple(scale.shape) != (B, 2):
            raise ValueError(f"scale: [{B}, 2]")
        scale = scale.to(torch.float32).contiguous()
    count = devargs.count_arg(count, dev)
    if out is None:
        out = torch.empty(cap, 2, dtype=torch.float32, device=dev)
    elif tuple(out.shape) != (cap, 2) or out.dtype != torch.float32 or not out.is_contiguous():
        raise ValueError(f"out: float32 [{cap}, 2], contiguous")
    if cap == 0:                                            # nothing to launch (and empty tensors have no address to hand over)
        return out
    with hip.enqueue_on(dev, stream):
        launch("opsup_fine_targets", dict(b_ids=b_ids.contiguous(), i_ids=i_ids.contiguous(), j_ids=j_ids.contiguous(), count=count, cap=cap,
                                          gt_j=gt.gt_j, gt_xy=gt.gt_xy, B=B, N=N, w_c=w_c, coarse_res=resolution[0], fine_res=resolution[1],
                                          radius=radius, scale=scale, expec_f_gt=out), stream)
    return out


class CoarseLoss:
    """What :func:`coarse_loss` leaves on the device: ``sums`` float64 ``[3]`` (``pos_sum``, ``neg_sum``, ``loss_c``) and ``counts``
    int64 ``[2]`` (``n_pos``, ``n_neg``)."""

    def __init__(self, sums, counts, keep=()):
        self.sums, self.counts, self._keep = sums, counts, keep

    @property
    def loss_c(self):
        return self.sums[2]

    def to_host(self) -> dict:
        (sums, counts), _ = devargs.unpack(devargs.pack([self.sums, self.counts]).cpu().numpy(), devargs.packed_layout([self.sums, self.counts]))
        return {"pos_sum": float(sums[0]), "neg_sum": float(sums[1]), "loss_c": float(sums[2]), "n_pos": int(counts[0]), "n_neg": int(counts[1])}


def coarse_loss(conf_matrix, gt: GroundTruth, *, alpha=0.25, gamma=2.0, pos_weight=1.0, neg_weight=1.0, stream=None) -> CoarseLoss:
    """The focal loss of ``conf_matrix [B, N, M]`` float32 (any batch and row stride, contiguous rows) against ``gt``: one pass over the
    matrix.  A lazy ``conf_matrix`` is materialised by its own first-use rule: that costs the matrix."""
    if isinstance(conf_matrix, LazyConfMatrixBase):
        conf_matrix = conf_matrix.materialize()
    hip.need_device([("conf_matrix", conf_matrix), ("gt_j", gt.gt_j)])
    if conf_matrix.dim() != 3 or conf_matrix.dtype != torch.float32 or tuple(conf_matrix.shape) != gt.shape or 0 in conf_matrix.shape:
        raise ValueError(f"conf_matrix: float32 {list(gt.shape)}, got {conf_matrix.dtype} {list(conf_matrix.shape)}")
    if conf_matrix.stride(2) != 1 or conf_matrix.stride(1) < conf_matrix.shape[2] or conf_matrix.stride(0) < 0:
        conf_matrix = conf_matrix.contiguous()
    B, N, M = gt.shape
    dev = conf_matrix.device
    with hip.enqueue_on(dev, stream):
        partials = torch.empty(B * N + 1, 2, dtype=torch.float64, device=dev)
        sums = torch.empty(3, dtype=torch.float64, device=dev)
        counts = torch.empty(2, dtype=torch.int64, device=dev)
        launch("opsup_coarse_loss", dict(conf=conf_matrix, conf_bstride=conf_matrix.stride(0), conf_rstride=conf_matrix.stride(1), gt_j=gt.gt_j,
                                         B=B, N=N, M=M, alpha=alpha, gamma=gamma, pos_weight=pos_weight, neg_weight=neg_weight,
                                         partials=partials, sums=sums, counts=counts), stream)
    return CoarseLoss(sums, counts, keep=(conf_matrix, gt, partials))


def fine_loss(expec_f, expec_f_gt, *, count=None, correct_thr=1.0, training=False, stream=None):
    """``_compute_fine_loss_l2_std`` over ``expec_f [cap, 3]`` and ``expec_f_gt [cap, 2]`` float32 with the device ``count`` ->
    ``(loss_f float64 [1], n_correct int32 [1], status int32 [1])`` on the device.  ``status``: ``OK``; ``NONE`` (eval, no correct row:
    ``loss_f`` is NaN and the caller reports 1.0); ``FORCED`` (training, no correct row: row 0 with the weight 1e-6); ``EMPTY`` (training
    and a device count of 0).  An empty table in training is a ``ValueError``, as the reference raises on it."""
    hip.need_tensors([("expec_f", expec_f), ("expec_f_gt", expec_f_gt)])
    cap = int(expec_f.shape[0])
    if expec_f.dim() != 2 or expec_f.shape[1] != 3 or tuple(expec_f_gt.shape) != (cap, 2) or expec_f.dtype != torch.float32 \
            or expec_f_gt.dtype != torch.float32:
        raise ValueError("expec_f: float32 [cap, 3], expec_f_gt: float32 [cap, 2]")
    if cap == 0 and training:
        raise ValueError("fine_loss in training needs at least one match: the reference forces row 0")
    hip.on_device([expec_f, expec_f_gt])
    dev = expec_f.device
    count = devargs.count_arg(count, dev)
    expec_f, expec_f_gt, count, _ = devargs.at_least_one_row(expec_f.contiguous(), expec_f_gt.contiguous(), count)
    cap = int(expec_f.shape[0])
    with hip.enqueue_on(dev, stream):
        loss_f = torch.empty(1, dtype=torch.float64, device=dev)
        n_correct, status = (torch.empty(1, dtype=torch.int32, device=dev) for _ in range(2))
        launch("opsup_fine_loss", dict(expec_f=expec_f, expec_f_gt=expec_f_gt, count=count, cap=cap, correct_thr=correct_thr,
                                       training=bool(training), loss_f=loss_f, n_correct=n_correct, status=status), stream)
    return loss_f, n_correct, status


def _ground_truth_of(data) -> GroundTruth:
    if "ground_truth" in data:
        return data["ground_truth"]
    return GroundTruth.from_dense(data["conf_matrix_gt"], data["fine_location_matrix_gt"], data.get("q_hw_c"))


def fine_supervision(data, config):
    """The reference's ``fine_supervision(data, config)``: reads ``b_ids`` / ``i_ids`` / ``j_ids``, ``q_hw_c``, optionally
    ``query_image_scale``, and ``data["ground_truth"]`` (a :class:`GroundTruth`) or the two dense keys; writes ``data["expec_f_gt"]``.
    ``config``: the reference's, with the model block under ``"OnePosePlus"`` (or that block itself)."""
    block = config["OnePosePlus"] if "OnePosePlus" in config else config
    resolution = list(block["loftr_backbone"]["resolution"])
    radius = block["loftr_fine"]["window_size"] // 2
    data.update({"expec_f_gt": fine_targets(data["b_ids"], data["i_ids"], data["j_ids"], _ground_truth_of(data), data["q_hw_c"][1],
                                            resolution=resolution, radius=radius, scale=data.get("query_image_scale"))})


class Loss:
    """The reference's ``Loss(config)`` (``config``: its ``loss`` block: ``coarse_type``, ``coarse_weight``, ``focal_alpha``,
    ``focal_gamma``, ``pos_weight``, ``neg_weight``, ``fine_type``, ``fine_weight``, ``fine_correct_thr``), forward only.  Not an
    ``nn.Module``: there is nothing to differentiate and no parameter."""

    def __init__(self, config):
        if config["coarse_type"] != "focal":
            raise NotImplementedError(f"coarse_type {config['coarse_type']!r}: the reference implements 'focal' only")
        if config["fine_type"] != "l2_with_std":
            raise NotImplementedError(f"fine_type {config['fine_type']!r}: the reference implements 'l2_with_std' only")
        self.config, self.training = config, True           # a fresh nn.Module is in training mode

    def train(self, mode=True):
        self.training = bool(mode)
        return self

    def eval(self):
        return self.train(False)

    def forward(self, data):
        """Writes ``data["loss"]`` (a float64 scalar on the device) and ``data["loss_scalars"]``: ``loss_c``, ``loss_f`` (when
        ``expec_f`` is in ``data``; 1.0 with the eval ``NONE`` status, the reference's upper bound) and ``loss`` as host floats from ONE
        packed read-back.  ``mask0`` in ``data`` (the padding weights of ``compute_c_weight``) is not implemented: OnePose++ data
        never carries it."""
        if "mask0" in data:
            raise NotImplementedError("mask0 / mask1 loss weights (compute_c_weight): OnePose++ data never carries them")
        cfg, gt = self.config, _ground_truth_of(data)
        coarse = coarse_loss(data["conf_matrix"], gt, alpha=cfg["focal_alpha"], gamma=cfg["focal_gamma"], pos_weight=cfg["pos_weight"],
                             neg_weight=cfg["neg_weight"])
        loss = coarse.loss_c * float(cfg["coarse_weight"])
        fields = [coarse.sums[2:3]]
        if "expec_f" in data:
            loss_f, _, status = fine_loss(data["expec_f"], data["expec_f_gt"], correct_thr=cfg["fine_correct_thr"], training=self.training)
            loss = torch.where(status[0] == NONE, loss, loss + loss_f[0] * float(cfg["fine_weight"]))
            fields += [loss_f, status]
        fields.append(loss.reshape(1))
        host, _ = devargs.unpack(devargs.pack(fields).cpu().numpy(), devargs.packed_layout(fields))
        scalars = {"loss_c": float(host[0][0]), "loss": float(host[-1][0])}
        if "expec_f" in data:
            scalars["loss_f"] = 1.0 if int(host[2][0]) == NONE else float(host[1][0])
        data.update({"loss": loss, "loss_scalars": scalars})

    __call__ = forward


class stages:
    """The four entries one by one (device tensors in, device tensors out): what ``fine_supervision`` and ``Loss.forward`` enqueue"""
    ground_truth = staticmethod(ground_truth)
    fine_targets = staticmethod(fine_targets)
    coarse_loss = staticmethod(coarse_loss)
    fine_loss = staticmethod(fine_loss)
