"""Generate ``pose_eval_small.npz`` FROM THE REFERENCE ITSELF.

Run in the build container only (needs the reference checkout beside the repository; the GPU box never sees it):

    python tests/golden/make_golden_pose_eval.py

The inputs are seeded (``tests/pose_eval_oracle.scene(7, F=12, V=300, max_angle=6, max_shift=0.03)``: 12 pose pairs, 300 float32
vertices, one ``K``).  The outputs are what the reference's own ``src/utils/metric_utils.py`` returns for them: ``query_pose_error`` for
each of the three units, ``projection_2d_error``, ``add_metric`` with ``syn`` False and True at the stated diameter (the diagonal of the
model's box, ``model_diameter_from_bbox`` of ``get_model_corners``) and ``aggregate_metrics``.

Import shims, behaviour-neutral, for what is not installed: ``cv2``, ``loguru``, ``open3d`` and ``plyfile`` (none of them is touched by the
five functions).  Only data is stored.

The recipe asserts what makes the stored values robust: every angular distance is at least 0.1 degree (the arc cosine is well
conditioned), and every mean distance (computed here with numpy and ``scipy.spatial.cKDTree``, stored as ``add_mean`` / ``adds_mean``) is
further than 1e-6 x threshold from its ADD threshold, so no boolean can flip on rounding.
"""
from __future__ import annotations

import logging
import os
import sys
import types

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
REPO = os.path.abspath(os.path.join(HERE, "..", ".."))
REF = os.environ.get("ONEPOSE_REFERENCE", "/root/reference")
sys.dont_write_bytecode = True
sys.path.insert(0, REPO)

SCENE_ARGS = dict(seed=7, F=12, V=300, max_angle=6.0, max_shift=0.03)
UNITS = ("m", "cm", "mm")
PERCENTAGE = 0.1


def _install_shims():
    for name in ("cv2", "open3d", "plyfile"):
        sys.modules[name] = types.ModuleType(name)
    sys.modules["plyfile"].PlyData = None
    sys.modules["loguru"] = types.ModuleType("loguru")
    sys.modules["loguru"].logger = logging.getLogger("ref")


def main():
    from scipy import spatial

    from tests import pose_eval_oracle as oracle
    _install_shims()
    sys.path.insert(0, REF)
    from src.utils import metric_utils as mu
    from src.utils.sample_points_on_cad import get_model_corners, model_diameter_from_bbox

    # the hand-made pair the import was checked with
    hand_gt = np.concatenate([np.eye(3), [[0.0], [0.0], [0.5]]], axis=1)
    hand_pred = np.concatenate([oracle.rotation([0.0, 0.0, 1.0], 1.0) @ oracle.rotation([1.0, 0.0, 0.0], 0.625), [[0.01], [0.002], [0.5]]], axis=1)
    print("hand-made pair:", mu.query_pose_error(hand_pred, hand_gt, unit="m"))

    s = oracle.scene(**SCENE_ARGS)
    verts, gt, pred, K = s["verts"], s["pose_gt"], s["pose_pred"], s["K"]
    F = len(gt)
    diameter = float(model_diameter_from_bbox(get_model_corners(verts.astype(np.float64))))
    thr = diameter * PERCENTAGE
    out = {"verts": verts, "pose_gt": gt, "pose_pred": pred, "K": K, "diameter": np.float64(diameter), "percentage": np.float64(PERCENTAGE)}
    for unit in UNITS:
        pairs = [mu.query_pose_error(pred[f], gt[f], unit=unit) for f in range(F)]
        out[f"R_errs_{unit}"] = np.array([p[0] for p in pairs], dtype=np.float64)
        out[f"t_errs_{unit}"] = np.array([p[1] for p in pairs], dtype=np.float64)
    assert (out["R_errs_m"] >= 0.1).all(), out["R_errs_m"]
    out["proj2d"] = np.array([mu.projection_2d_error(verts, pred[f], gt[f], K) for f in range(F)], dtype=np.float64)
    out["add"] = np.array([mu.add_metric(verts, diameter, pred[f], gt[f], percentage=PERCENTAGE, syn=False) for f in range(F)], dtype=bool)
    out["adds"] = np.array([mu.add_metric(verts, diameter, pred[f], gt[f], percentage=PERCENTAGE, syn=True) for f in range(F)], dtype=bool)

    # the means behind the booleans, by independent forms, and their distance from the threshold
    x = verts.astype(np.float64)
    add_mean, adds_mean = np.zeros(F), np.zeros(F)
    for f in range(F):
        a, b = x @ pred[f][:, :3].T + pred[f][:, 3], x @ gt[f][:, :3].T + gt[f][:, 3]
        add_mean[f] = np.mean(np.linalg.norm(a - b, axis=-1))
        adds_mean[f] = np.mean(spatial.cKDTree(a).query(b, k=1)[0])
    for mean, flag in ((add_mean, out["add"]), (adds_mean, out["adds"])):
        assert (np.abs(mean - thr) > 1e-6 * thr).all(), (mean, thr)
        assert np.array_equal(mean < thr, flag)
    assert 0 < out["add"].sum() < F, out["add"]              # both outcomes occur
    out["add_mean"], out["adds_mean"] = add_mean, adds_mean

    metrics = {"R_errs": list(out["R_errs_m"]), "t_errs": list(out["t_errs_m"]), "ADD_metric": list(out["add"]), "proj2D_metric": list(out["proj2d"])}
    agg = mu.aggregate_metrics(metrics)
    out["aggregate_keys"] = np.array(list(agg))
    out["aggregate_values"] = np.array([float(v) for v in agg.values()], dtype=np.float64)
    print("R_errs", out["R_errs_m"], "\nt_errs", out["t_errs_m"], "\nproj2d", out["proj2d"], "\nadd", out["add"], "\nadds", out["adds"], "\n", agg)
    path = os.path.join(HERE, "pose_eval_small.npz")
    np.savez_compressed(path, **out)
    print("wrote", path, os.path.getsize(path), "bytes")


if __name__ == "__main__":
    main()
