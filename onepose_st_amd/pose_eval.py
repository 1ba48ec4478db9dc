"""Pose evaluation on the device (opt-in): what the reference's ``src/utils/metric_utils.py`` computes between "pose
out" and the numbers of the paper -- ``query_pose_error`` (cm-degree), ``add_metric`` (ADD, and ADD-S with ``syn=True``),
``projection_2d_error`` and ``aggregate_metrics`` -- for every pose of a sequence at once, next to ``pnp_device.DevicePoses``.

The specification is ``include/onepose_pose_eval.h`` (``tests/pose_eval_oracle.py`` restates it in numpy, one function per stage): float64 in the
written order, every mean summed in one fixed order (blocks of 256 vertices, a stride-128 .. 1 tree, the partials in ascending order), so
the device outputs are bit-equal to the oracle.  ADD-S is the exact nearest-neighbour mean (the reference builds a ``cKDTree`` per frame
on one host core): every target vertex against every predicted vertex, the predicted ones staged through LDS, launches chunked over
frames by ``MAX_PAIRS_PER_LAUNCH``.  The arc cosine is taken on the host after the one read-back, on ``F`` scalars.

The kernels are HIP (``csrc/pose_eval.hip`` in ``libonepose_pose_eval.so``).  CPU tensors raise :class:`hip.HipLibraryError` (no CPU
fallback); nothing is synchronised and nothing is read on the host until :meth:`DevicePoseErrors.to_host`.
"""
from __future__ import annotations

import numpy as np
import torch

from . import cabi, devargs, hip

_BINDING = cabi.Binding.of(__name__)                # the header is the one place a signature or a constant is written
library_path, load, check_arity, call = _BINDING.library_path, _BINDING.load, _BINDING.check_arity, _BINDING.call
launch = hip.launcher(_BINDING, globals())          # every stream-taking entry is called through it, by the header's parameter names
EXPORTED_SYMBOLS = _BINDING.exported_symbols
ABI_VERSION = _BINDING.abi_version
MAX_FRAMES, MAX_VERTICES, BLOCK, MAX_PAIRS_PER_LAUNCH, NO_POSE, BAD_INPUT = map(_BINDING.constant, (
    "MAX_FRAMES", "MAX_VERTICES", "BLOCK", "MAX_PAIRS_PER_LAUNCH", "NO_POSE", "BAD_INPUT"))
UNIT_SCALE = {"m": 100.0, "cm": 1.0, "mm": 0.1}

_PLY_TYPES = {"char": "i1", "int8": "i1", "uchar": "u1", "uint8": "u1", "short": "i2", "int16": "i2", "ushort": "u2", "uint16": "u2",
              "int": "i4", "int32": "i4", "uint": "u4", "uint32": "u4", "float": "f4", "float32": "f4", "double": "f8", "float64": "f8"}


def model_corners(vertices) -> np.ndarray:
    """The eight corners of the axis-aligned box of ``vertices`` in the reference's ``get_model_corners`` order (x slowest, z fastest)
    and the box centre: ``[9, 3]`` in the vertices' dtype"""
    lo, hi = vertices.min(axis=0), vertices.max(axis=0)
    corners = np.array([[(lo, hi)[i][0], (lo, hi)[j][1], (lo, hi)[k][2]] for i in (0, 1) for j in (0, 1) for k in (0, 1)])
    return np.concatenate([corners, (corners.max(axis=0, keepdims=True) + corners.min(axis=0, keepdims=True)) / 2], axis=0)


def load_model_points(path, max_num: int = -1):
    """``model_eval.ply`` -> ``(vertices float32 [V, 3], bbox float32 [9, 3])`` like the reference's ``load_points_from_cad``: a small PLY
    reader (``ascii`` and ``binary_little_endian``; ``x y z`` as float or double, other vertex properties skipped, faces ignored).  The
    reference samples the mesh with open3d when it has more than ``max_num`` vertices; that is not restated."""
    with open(path, "rb") as fh:
        raw = fh.read()
    end = raw.find(b"end_header")
    if not raw.startswith(b"ply") or end < 0:
        raise ValueError(f"{path}: not a PLY file")
    body = raw.find(b"\n", end) + 1
    if body == 0:
        raise ValueError(f"{path}: truncated after the header")
    fmt, elements = None, []                                # elements: [name, count, [(type, name), ...]] in file order
    for words in (l.split() for l in raw[:end].decode("ascii", errors="replace").splitlines()[1:]):
        if not words or words[0] in ("comment", "obj_info"):
            continue
        if words[0] == "format":
            fmt = words[1]
        elif words[0] == "element":
            elements.append([words[1], int(words[2]), []])
        elif words[0] == "property" and elements:
            if words[1] == "list":
                elements[-1][2].append(("list", words[-1]))
            elif words[1] in _PLY_TYPES:
                elements[-1][2].append((_PLY_TYPES[words[1]], words[2]))
            else:
                raise ValueError(f"{path}: property type {words[1]!r}")
    if fmt not in ("ascii", "binary_little_endian"):
        raise ValueError(f"{path}: format {fmt!r} (ascii and binary_little_endian are read)")
    if not elements or elements[0][0] != "vertex":
        raise ValueError(f"{path}: the first element must be 'vertex'")
    _, count, props = elements[0]
    names = [n for _, n in props]
    if any(t == "list" for t, _ in props) or not all(c in names for c in "xyz"):
        raise ValueError(f"{path}: the vertex element needs scalar properties x, y, z")
    if any(props[names.index(c)][0] not in ("f4", "f8") for c in "xyz"):
        raise ValueError(f"{path}: x, y, z must be float or double")
    if fmt == "ascii":
        rows = raw[body:].decode("ascii", errors="replace").split("\n")[:count]
        table = [r.split() for r in rows if r.strip()]
        if len(table) < count or any(len(r) < len(props) for r in table):
            raise ValueError(f"{path}: truncated: {len(table)} complete vertex rows of {count}")
        xyz = np.array([[float(r[names.index(c)]) for c in "xyz"] for r in table], dtype=np.float64).reshape(count, 3)
    else:
        dtype = np.dtype([(n, "<" + t) for t, n in props])
        if len(raw) - body < count * dtype.itemsize:
            raise ValueError(f"{path}: truncated: {(len(raw) - body) // dtype.itemsize} complete vertex rows of {count}")
        rec = np.frombuffer(raw, dtype=dtype, count=count, offset=body)
        xyz = np.stack([rec[c].astype(np.float64) for c in "xyz"], axis=1).reshape(count, 3)
    if count < 1:
        raise ValueError(f"{path}: no vertices")
    if max_num != -1 and count > max_num:
        raise NotImplementedError(f"{count} vertices with max_num={max_num}: the reference samples the mesh with open3d here; that is out of scope")
    return xyz.astype(np.float32), model_corners(xyz).astype(np.float32)


def model_diameter(bbox) -> float:
    """The reference's ``model_diameter_from_bbox``: the box diagonal ``|bbox[7] - bbox[0]|``"""
    bbox = np.asarray(bbox)
    return float(np.linalg.norm(bbox[7] - bbox[0]))


class DevicePoseErrors:
    """What :func:`pose_errors` returns, on the device: ``rot_cos [F]`` and ``t_err [F]`` (cm) float64, ``add_dist [F]`` (the ADD mean, or
    the ADD-S mean with ``symmetric``; ``None`` without a model), ``proj2d [F]`` (``None`` without a model and ``K``), ``flags [F]`` int32
    (``NO_POSE`` / ``BAD_INPUT``: ``rot_cos`` NaN, everything else ``+inf``)."""

    def __init__(self, rot_cos, t_err, add_dist, proj2d, flags, symmetric=False, diameter=None, keep=()):
        self.rot_cos, self.t_err, self.add_dist, self.proj2d, self.flags = rot_cos, t_err, add_dist, proj2d, flags
        self.symmetric, self.diameter = symmetric, diameter
        self._keep = keep                                   # the inputs and the workspace stay referenced while the work may be queued

    def _doubles(self):
        return [t for t in (self.rot_cos, self.t_err, self.add_dist, self.proj2d) if t is not None]

    def pack(self) -> torch.Tensor:
        """One uint8 device tensor for one read-back: the float64 outputs that exist in the order above, then the flags"""
        return devargs.pack(self._doubles() + [self.flags])

    def unpack(self, packed) -> dict:
        """The host arrays of :meth:`pack`'s bytes (a uint8 numpy array): ``rot_cos``, ``t_err``, ``flags`` and, where they exist,
        ``add_dist`` and ``proj2d``"""
        names = [n for n in ("rot_cos", "t_err", "add_dist", "proj2d", "flags") if getattr(self, n) is not None]
        arrays, _ = devargs.unpack(packed, devargs.packed_layout(getattr(self, n) for n in names))
        return {n: a.copy() for n, a in zip(names, arrays)}

    def to_host(self, diameter=None, percentage=0.1) -> dict:
        """The one read-back, in the reference's keys: ``R_errs`` (degrees: ``rad2deg(arccos(rot_cos))``) and ``t_errs`` (cm), both
        ``inf`` on a frame without a pose; with a model ``add_dist`` and, given a ``diameter`` (here or from
        :func:`compute_query_pose_errors`), ``ADD_metric``: ``add_dist < diameter * percentage`` (strict; ``False`` without a pose); with
        ``K`` ``proj2D_metric`` (pixels).  ``flags`` as well."""
        host = self.unpack(self.pack().cpu().numpy())
        with np.errstate(invalid="ignore"):
            r_errs = np.rad2deg(np.arccos(host["rot_cos"]))
        out = {"R_errs": np.where(host["flags"] != 0, np.inf, r_errs), "t_errs": host["t_err"], "flags": host["flags"]}
        diameter = self.diameter if diameter is None else diameter
        if "add_dist" in host:
            out["add_dist"] = host["add_dist"]
            if diameter is not None:
                out["ADD_metric"] = host["add_dist"] < float(diameter) * percentage
        if "proj2d" in host:
            out["proj2D_metric"] = host["proj2d"]
        return out


def pose_errors(poses, pose_gt, *, status=None, unit="m", model_points=None, K=None, symmetric=False, stream=None,
                pair_budget=None) -> DevicePoseErrors:
    """The errors of ``poses`` (``[F, 3, 4]`` or ``[F, 4, 4]`` on the device, or a ``pnp_device.DevicePoses``: its ``pose`` and
    ``status``) against ``pose_gt`` (the same shapes; a host array is uploaded).  ``status``: int32 ``[F]`` of ``pnp_device`` status words,
    a frame with ``STATUS_NO_POSE`` counts as no pose.  ``unit``: the unit of the translations (``t_err`` is in cm).  ``model_points``:
    float32 ``[V, 3]`` (a host array is uploaded) adds ``add_dist`` -- ADD-S with ``symmetric`` -- and, with ``K`` (``[3, 3]`` shared or
    ``[F, 3, 3]``, the ORIGINAL intrinsics), ``proj2d``.  ``pair_budget``: the most vertex pairs of one ADD-S launch (default
    ``MAX_PAIRS_PER_LAUNCH``).  Everything is enqueued on ``stream`` (default: the current one); nothing is read back."""
    from . import pnp_device
    if isinstance(poses, pnp_device.DevicePoses):
        if status is not None:
            raise ValueError("status comes with the DevicePoses")
        poses, status = poses.pose, poses.status
    if unit not in UNIT_SCALE:
        raise NotImplementedError(f"unit={unit!r}: 'm', 'cm' or 'mm'")
    if K is not None and model_points is None:
        raise ValueError("K without model_points: the projection error is a mean over the model's vertices")
    named = [("poses", poses)] + [(k, v) for k, v in (("pose_gt", pose_gt), ("status", status), ("model_points", model_points), ("K", K))
                                  if isinstance(v, torch.Tensor) or k == "status" and v is not None]
    hip.need_device(named)
    dev = poses.device
    pred, gt = (devargs.mat64(n, p, [(None, 3, 4), (None, 4, 4)], dev, "[F, 3, 4] or [F, 4, 4]") for n, p in (("poses", poses), ("pose_gt", pose_gt)))
    F, pred_stride, gt_stride = int(pred.shape[0]), 4 * int(pred.shape[1]), 4 * int(gt.shape[1])        # strides in doubles
    if gt.shape[0] != F or not 1 <= F <= MAX_FRAMES:
        raise ValueError(f"poses and pose_gt: the same number of frames, in [1, {MAX_FRAMES}]")
    if status is not None:
        if status.dtype != torch.int32 or tuple(status.shape) != (F,):
            raise ValueError(f"status: int32 [{F}]")
        status = status.contiguous()
    verts = None
    if model_points is not None:
        verts = model_points if isinstance(model_points, torch.Tensor) else torch.as_tensor(
            np.ascontiguousarray(model_points, dtype=np.float32), device=dev)
        if verts.dim() != 2 or verts.shape[1] != 3 or verts.dtype != torch.float32 or not 1 <= verts.shape[0] <= MAX_VERTICES:
            raise ValueError(f"model_points: float32 [V, 3], 1 <= V <= {MAX_VERTICES}")
        verts = verts.contiguous()
    if K is not None:
        K, k_shared = devargs.k_table(K, F, dev, exact=True)
    if pair_budget is not None and (int(pair_budget) != pair_budget or not 1 <= pair_budget <= MAX_PAIRS_PER_LAUNCH):
        raise ValueError(f"pair_budget: an integer in [1, {MAX_PAIRS_PER_LAUNCH}]")
    with hip.enqueue_on(dev, stream):
        rot_cos, t_err = (torch.empty(F, dtype=torch.float64, device=dev) for _ in range(2))
        flags = torch.empty(F, dtype=torch.int32, device=dev)
        launch("opevl_errors", dict(pose_pred=pred, pred_stride=pred_stride, pose_gt=gt, gt_stride=gt_stride, status=status,
                                    status_mask=pnp_device.STATUS_NO_POSE, frames=F, unit_scale=UNIT_SCALE[unit], rot_cos=rot_cos, t_err=t_err,
                                    flags=flags), stream)
        add_dist = proj2d = partials = None
        if verts is not None:
            V = int(verts.shape[0])
            partials = torch.empty(F * ((V + BLOCK - 1) // BLOCK), dtype=torch.float64, device=dev)     # used by one launch after the other
            add_dist = torch.empty(F, dtype=torch.float64, device=dev)
            tables = dict(verts=verts, V=V, pose_pred=pred, pred_stride=pred_stride, pose_gt=gt, gt_stride=gt_stride, flags=flags, frames=F,
                          partials=partials)
            if symmetric:
                launch("opevl_adds", dict(tables, pair_budget=0 if pair_budget is None else pair_budget, adds_dist=add_dist), stream)
            else:
                launch("opevl_add", dict(tables, add_dist=add_dist), stream)
            if K is not None:
                proj2d = torch.empty(F, dtype=torch.float64, device=dev)
                launch("opevl_proj2d", dict(tables, K=K, k_shared=k_shared, proj2d=proj2d), stream)
    return DevicePoseErrors(rot_cos, t_err, add_dist, proj2d, flags, symmetric=bool(symmetric),
                            keep=(pred, gt, status, verts, K, partials))


def aggregate_metrics(metrics, pose_thres=(1, 3, 5), proj2d_thres=5) -> dict:
    """The reference's ``aggregate_metrics`` on the host, once per dataset: ``"{k}cm@{k}degree"`` (both errors strictly below ``k``; NaN
    and ``inf`` fail), and with ``ADD_metric`` in ``metrics`` ``"ADD metric"`` and ``"proj2D metric"`` (strictly below ``proj2d_thres``
    pixels).  An empty list gives NaN."""
    def mean(x):
        x = np.asarray(x, dtype=np.float64)
        return float(np.mean(x)) if x.size else float("nan")
    r, t = np.asarray(metrics["R_errs"], dtype=np.float64), np.asarray(metrics["t_errs"], dtype=np.float64)
    out = {}
    with np.errstate(invalid="ignore"):
        for k in pose_thres:
            out[f"{k}cm@{k}degree"] = mean((r < k) & (t < k))
        if "ADD_metric" in metrics:
            out["ADD metric"] = mean(np.asarray(metrics["ADD_metric"], dtype=bool))
            out["proj2D metric"] = mean(np.asarray(metrics["proj2D_metric"], dtype=np.float64) < proj2d_thres)
    return out


def compute_query_pose_errors(data, K, pose_gt, configs, *, model_points=None, diameter=None, K_origin=None, symmetric=False):
    """The device counterpart of the reference's ``compute_query_pose_errors`` on a ``data`` dict after ``forward``: one
    ``pnp_device.ransac_pnp`` over the batch (``mkpts_query_f`` / ``mkpts_3d_db`` with ``b_ids=data["m_bids"]``, ``frames=B``; the
    ``eval_metrics`` keys ``point_cloud_rescale``, ``pnp_reprojection_error``, ``model_unit`` and ``use_pycolmap_ransac`` of ``configs``),
    then :func:`pose_errors` against ``pose_gt [B, 3, 4]`` or ``[B, 4, 4]``.  ``K [B, 3, 3]``: the intrinsics the matches live in;
    ``K_origin`` (default ``K``): those of the projection error.  -> ``(DevicePoses, DevicePoseErrors)``, nothing read back."""
    from . import pnp_device
    B = int(pose_gt.shape[0])
    poses = pnp_device.ransac_pnp(K, data["mkpts_query_f"], data["mkpts_3d_db"], b_ids=data["m_bids"], frames=B,
                                  scale=configs["point_cloud_rescale"], pnp_reprojection_error=configs["pnp_reprojection_error"],
                                  use_pycolmap_ransac=configs.get("use_pycolmap_ransac", True))
    K_eval = None if model_points is None else (K if K_origin is None else K_origin)
    errors = pose_errors(poses, pose_gt, unit=configs.get("model_unit", "m"), model_points=model_points, K=K_eval, symmetric=symmetric)
    errors.diameter = diameter
    return poses, errors


def evaluate_records(records, poses_gt, *, key="pose", unit="m", model_points=None, K=None, symmetric=False, diameter=None, percentage=0.1,
                     pose_thres=(1, 3, 5), proj2d_thres=5, device="cuda") -> dict:
    """The records of ``frameloop.SequenceRunner.run`` against ``poses_gt [F, 3, 4]`` or ``[F, 4, 4]``: the poses are uploaded once, the
    errors come back in one read-back.  ``key="pose_refined"`` evaluates the second pass (its inliers are ``inliers_refined``).  A record
    with an empty inlier array counts as no pose.  -> :meth:`DevicePoseErrors.to_host`'s per-frame dict plus ``"aggregate"``
    (:func:`aggregate_metrics`; the ADD keys when a model, ``K`` and a diameter are given)."""
    from . import pnp_device
    records = list(records)
    if not records:
        raise ValueError("no records")
    if not key.startswith("pose"):
        raise ValueError("key: 'pose' or 'pose_refined'")
    inliers_key = "inliers" + key[len("pose"):]
    pred = np.stack([np.asarray(r[key], dtype=np.float64)[:3] for r in records])
    no_pose = np.array([pnp_device.STATUS_NO_POSE if len(r[inliers_key]) == 0 else 0 for r in records], dtype=np.int32)
    dev = torch.device(device)
    errors = pose_errors(torch.as_tensor(pred, device=dev), poses_gt, status=torch.as_tensor(no_pose, device=dev), unit=unit,
                         model_points=model_points, K=K, symmetric=symmetric)
    out = errors.to_host(diameter=diameter, percentage=percentage)
    agg = {k: v for k, v in out.items() if k in ("R_errs", "t_errs")}
    if "ADD_metric" in out and "proj2D_metric" in out:
        agg.update(ADD_metric=out["ADD_metric"], proj2D_metric=out["proj2D_metric"])
    out["aggregate"] = aggregate_metrics(agg, pose_thres, proj2d_thres)
    return out
