"""Generate ``supervision_small.npz`` FROM THE REFERENCE ITSELF.

Run in the build container only (needs the reference checkout beside the repository; the GPU box never sees it):

    python tests/golden/make_supervision_golden.py

The inputs are seeded (``tests/supervision_oracle.scene(5, B=2, N=64, A=48, out_of_range=False, exact_frame=True)``: two labelled frames
with the planted rows, the second one the exact frame; a ``conf_matrix`` with clamped, ordinary and planted-positive values; match lists on
and off the ground truth).  The outputs are the reference's:

* ``Loss`` (``src/lightning_model/losses.py``) and ``fine_supervision`` (``src/models/OnePosePlus/utils/fine_supervision.py``) are imported
  by file path and run as they are, ``loguru`` shimmed (logging only).
* The ground truth is NOT imported: ``src/datasets/OnePosePlus_dataset.py`` triggers a download at import.  Its lines 341-354 and 411-445
  and ``build_assignmatrix`` (174-236) are restated below with the same torch and numpy calls in the same order, ``np.unique`` included.
  Ids out of range are left out of the inputs: the reference's gather raises on them.

Only data is stored.  The recipe asserts ``min_margin >= 1e-3`` px for the frames that are not exact, so no rounding can flip between the
reference's ``R @ X + t`` and the written-order projection."""
from __future__ import annotations

import importlib.util
import logging
import os
import sys
import types

import numpy as np
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
REPO = os.path.abspath(os.path.join(HERE, "..", ".."))
REF = os.environ.get("ONEPOSE_REFERENCE", "/root/reference")

SCENE_ARGS = dict(seed=5, B=2, N=64, A=48, image_hw=(280, 296), out_of_range=False, exact_frame=True)
LOSS_CONFIG = {"coarse_type": "focal", "coarse_weight": 1.0, "focal_alpha": 0.25, "focal_gamma": 2.0, "pos_weight": 1.0, "neg_weight": 1.0,
               "fine_type": "l2_with_std", "fine_weight": 1.0, "fine_correct_thr": 1.0}
MODEL_CONFIG = {"OnePosePlus": {"loftr_backbone": {"resolution": [8, 2]}, "loftr_fine": {"window_size": 5}}}


def _by_path(name, path):
    spec = importlib.util.spec_from_file_location(name, os.path.join(REF, path))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


def reference_ground_truth(keypoints3d, point_ids, pose_gt, K_crop, image_hw, coarse_scale=0.125):
    """One frame, lines 341-354, 411-445 and build_assignmatrix as written there"""
    h_i, w_i = image_hw
    h_c, w_c = int(h_i * coarse_scale), int(w_i * coarse_scale)
    n_query_coarse_grid, shape3d = int(h_c * w_c), keypoints3d.shape[0]
    query_img_scale = torch.tensor([1.0, 1.0])
    A = point_ids.shape[0]
    assign_matrix = torch.stack([torch.arange(A), torch.from_numpy(point_ids)])
    keypoints2d_coarse = torch.zeros((A, 2), dtype=torch.float)
    keypoints3d, pose_gt, K_crop = torch.from_numpy(keypoints3d), torch.from_numpy(pose_gt), torch.from_numpy(K_crop)

    assign_matrix = assign_matrix.long()
    mkpts_3d = keypoints3d[assign_matrix[1, :]]
    R = pose_gt[:3, :3].to(torch.float)
    t = pose_gt[:3, [3]].to(torch.float)
    K_crop = K_crop.to(torch.float)
    keypoints2d_fine = torch.zeros((keypoints2d_coarse.shape[0], 2), dtype=torch.float)
    mkpts_3d_camera = R @ mkpts_3d.transpose(1, 0) + t
    mkpts_proj = (K_crop @ mkpts_3d_camera).transpose(1, 0)
    mkpts_proj = mkpts_proj[:, :2] / (mkpts_proj[:, [2]] + 1e-6)

    mkpts_proj_rounded = (mkpts_proj / int(1 / coarse_scale)).round() * int(1 / coarse_scale)
    invalid = ((mkpts_proj_rounded[:, 0] < 0) | (mkpts_proj_rounded[:, 0] > w_i - 1)
               | (mkpts_proj_rounded[:, 1] < 0) | (mkpts_proj_rounded[:, 1] > h_i - 1))
    mkpts_proj_rounded = mkpts_proj_rounded[~invalid]
    mkpts_proj = mkpts_proj[~invalid]
    assign_matrix = assign_matrix[:, ~invalid]
    unique, index = np.unique(mkpts_proj_rounded, return_index=True, axis=0)
    mkpts_proj_rounded = mkpts_proj_rounded[index]
    mkpts_proj = mkpts_proj[index]
    assign_matrix = assign_matrix[:, index]
    keypoints2d_coarse[assign_matrix[0, :]] = mkpts_proj_rounded
    keypoints2d_fine[assign_matrix[0, :]] = mkpts_proj

    # build_assignmatrix(keypoints2d_coarse, keypoints2d_fine, assign_matrix, pad=True)
    assign_matrix = assign_matrix.long()
    conf_matrix = torch.zeros(shape3d, n_query_coarse_grid, dtype=torch.int16)
    fine_location_matrix = torch.full((shape3d, n_query_coarse_grid, 2), -50, dtype=torch.float)
    valid = assign_matrix[1] < shape3d
    assign_matrix = assign_matrix[:, valid]
    keypoints_idx = assign_matrix[0]
    keypoints2D_coarse_selected = keypoints2d_coarse[keypoints_idx]
    keypoints2D_fine_selected = keypoints2d_fine[keypoints_idx]
    keypoints2D_coarse_selected_rescaled = keypoints2D_coarse_selected / query_img_scale[[1, 0]] * coarse_scale
    keypoints2D_coarse_selected_rescaled = keypoints2D_coarse_selected_rescaled.round()
    j_ids = keypoints2D_coarse_selected_rescaled[:, 1] * w_c + keypoints2D_coarse_selected_rescaled[:, 0]
    j_ids = j_ids.long()
    invalid_mask = j_ids > conf_matrix.shape[1]
    j_ids = j_ids[~invalid_mask]
    assign_matrix = assign_matrix[:, ~invalid_mask]
    keypoints2D_fine_selected = keypoints2D_fine_selected[~invalid_mask]
    conf_matrix[assign_matrix[1], j_ids] = 1
    fine_location_matrix[assign_matrix[1], j_ids] = keypoints2D_fine_selected
    return conf_matrix, fine_location_matrix


def make_inputs(oracle):
    """The loss inputs: everything beside the scene, seeded"""
    s = oracle.scene(**SCENE_ARGS)
    gt = oracle.ground_truth(s["keypoints3d"], s["point_ids"], s["counts"], s["pose_gt"], s["K"], s["image_hw"])
    assert oracle.ground_truth(s["keypoints3d"][:1], s["point_ids"][:1], None, s["pose_gt"][:1], s["K"][:1], s["image_hw"])["min_margin"] >= 1e-3
    rng = np.random.default_rng(SCENE_ARGS["seed"] + 100)
    B, N = gt["gt_j"].shape
    M = gt["gt_i"].shape[1]
    conf = np.exp(rng.uniform(np.log(1e-9), np.log(0.5), (B, N, M))).astype(np.float32)          # most below 1e-6, as in a real matrix
    b, i = np.nonzero(gt["gt_j"] >= 0)
    conf[b, i, gt["gt_j"][b, i]] = rng.uniform(0.05, 0.95, len(b)).astype(np.float32)
    conf[0, 0, :4] = [0.0, 1.0, 0.9999995, 3e-7]
    # matches: every second ground-truth pair, as many pairs one cell off, and some of points without ground truth
    on = np.stack([b, i, gt["gt_j"][b, i]], axis=1)[::2]
    off = on.copy()
    off[:, 2] = (off[:, 2] + 1) % M
    none_b, none_i = np.nonzero(gt["gt_j"] < 0)
    none = np.stack([none_b, none_i, rng.integers(0, M, len(none_b))], axis=1)[:10]
    matches = np.concatenate([on, off, none]).astype(np.int64)
    matches = matches[np.lexsort((matches[:, 1], matches[:, 0]))]
    expec_f = np.concatenate([rng.uniform(-0.6, 0.6, (len(matches), 2)), rng.uniform(0.05, 0.9, (len(matches), 1))], axis=1).astype(np.float32)
    scale = np.array([[1.25, 0.75], [1.0, 1.5]], np.float32)
    return s, gt, conf, matches, expec_f, scale


def main():
    from tests import supervision_oracle as oracle
    sys.modules["loguru"] = types.ModuleType("loguru")
    sys.modules["loguru"].logger = logging.getLogger("ref")
    losses = _by_path("ref_losses", "src/lightning_model/losses.py")
    fsup = _by_path("ref_fine_supervision", "src/models/OnePosePlus/utils/fine_supervision.py")

    s, gt, conf, matches, expec_f, scale = make_inputs(oracle)
    B = len(s["point_ids"])
    dense = [reference_ground_truth(s["keypoints3d"][b], s["point_ids"][b], s["pose_gt"][b], s["K"][b], s["image_hw"]) for b in range(B)]
    conf_gt, loc_gt = torch.stack([d[0] for d in dense]), torch.stack([d[1] for d in dense])
    H, W = s["image_hw"]
    out = {"keypoints3d": s["keypoints3d"], "point_ids": s["point_ids"], "pose_gt": s["pose_gt"], "K": s["K"], "image_hw": np.array([H, W]),
           "conf_matrix": conf, "matches": matches, "expec_f": expec_f, "scale": scale}
    # the dense ground truth, stored sparse: where conf_matrix_gt is 1, and fine_location_matrix_gt there; the rest is 0 / -50 (asserted)
    where = torch.nonzero(conf_gt == 1)
    out["ref_gt_where"] = where.numpy()
    out["ref_gt_xy"] = loc_gt[where[:, 0], where[:, 1], where[:, 2]].numpy()
    rest = loc_gt.clone()
    rest[where[:, 0], where[:, 1], where[:, 2]] = -50
    assert bool((rest == -50).all()) and int(conf_gt.sum()) == len(where)

    for name, sc in (("plain", None), ("scaled", scale)):
        data = {"b_ids": torch.from_numpy(matches[:, 0]), "i_ids": torch.from_numpy(matches[:, 1]), "j_ids": torch.from_numpy(matches[:, 2]),
                "q_hw_c": (H // 8, W // 8), "fine_location_matrix_gt": loc_gt, "conf_matrix_gt": conf_gt,
                "conf_matrix": torch.from_numpy(conf), "expec_f": torch.from_numpy(expec_f)}
        if sc is not None:
            data["query_image_scale"] = torch.from_numpy(sc)
        fsup.fine_supervision(data, MODEL_CONFIG)
        out[f"ref_expec_f_gt_{name}"] = data["expec_f_gt"].numpy()
        for mode in ("eval", "train"):
            loss = losses.Loss(LOSS_CONFIG)
            loss.train(mode == "train")
            loss(data)
            for k, v in data["loss_scalars"].items():
                out[f"ref_{k}_{name}_{mode}"] = np.float32(v.item())
    # the corner case: no correct match.  Every target pushed out of the window
    far = {"expec_f": torch.from_numpy(expec_f), "expec_f_gt": torch.full((len(matches), 2), 3.0)}
    for mode in ("eval", "train"):
        loss = losses.Loss(LOSS_CONFIG)
        loss.train(mode == "train")
        got = loss.compute_fine_loss(far["expec_f"], far["expec_f_gt"])
        out[f"ref_loss_f_none_{mode}"] = np.float32("nan") if got is None else np.float32(got.item())
    path = os.path.join(HERE, "supervision_small.npz")
    np.savez_compressed(path, **out)
    print(f"wrote {path}: {os.path.getsize(path)} bytes;", {k: float(v) for k, v in out.items() if k.startswith("ref_loss")})


if __name__ == "__main__":                                  # tests/test_supervision_cpu.py imports make_inputs: no side effect on import
    sys.dont_write_bytecode = True
    sys.path.insert(0, REPO)
    main()
