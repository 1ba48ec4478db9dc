"""Generate ``loss_backward_small.npz`` FROM THE REFERENCE ITSELF.

Run in the build container only (needs the reference checkout beside the repository; the GPU box never sees it):

    python tests/golden/make_loss_backward_golden.py

The inputs are seeded (:func:`make_inputs`: B = 2, N = 19, M = 23 coarse features with planted pairs -- confident positives, positives
below 1e-6, confident negatives, one frame's positive above 1 - 1e-6 -- and T = 11 fine matches of 5 x 5 windows, four of them not correct).
The outputs are the reference's, in float64 under autograd:

* the expression of ``CoarseMatching.forward`` (``src/models/OnePosePlus/utils/coarse_matching.py:102-115``, the ``sqrt_feat_dim``
  normaliser and the dual softmax) is restated with its own torch calls: the module's constructor needs the whole model configuration.
  Its ``self.temperature + 1e-4`` is taken as the float32 value the device's forward forms of it (``(float)(temperature + 1e-4)``), so
  that the fixture differentiates the function the device computes;
* ``FineMatching._s2d_heatmap`` (``src/models/OnePosePlus/utils/fine_matching.py``) and ``Loss`` (``src/lightning_model/losses.py``) are
  imported by file path and run as they are, ``loguru`` shimmed (logging only) and kornia's two helpers restated as in
  ``tests/golden/make_golden.py`` (kornia is not installed; ``create_meshgrid`` and ``spatial_expectation2d`` of 0.4.1).

Only data is stored: the inputs, the loss and its four gradients."""
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

B, N, M, T, W = 2, 19, 23, 11, 5
TEMPERATURE = 0.1
LOSS_CONFIG = {"coarse_type": "focal", "coarse_weight": 1.0, "focal_alpha": 0.25, "focal_gamma": 2.0, "pos_weight": 1.0, "neg_weight": 1.0,
               "fine_type": "l2_with_std", "fine_weight": 0.5, "fine_correct_thr": 1.0}


def make_inputs():
    """-> dict of the seeded inputs (float32 features, int64 ``gt_j``, float32 ``expec_f_gt``)"""
    rng = np.random.default_rng(31)
    feat0 = rng.standard_normal((B, N, 256)).astype(np.float32)
    feat1 = rng.standard_normal((B, M, 256)).astype(np.float32)
    gt_j = np.full((B, N), -1, np.int64)
    for b in range(B):
        rows, cells = rng.permutation(N)[:10], rng.permutation(M)[:12]
        gt_j[b, rows] = cells[:10]
        for k, (i, j) in enumerate(zip(rows, cells)):
            if k % 4 != 3:
                feat1[b, j] = feat0[b, i] + (0.15 * rng.standard_normal(256)).astype(np.float32)
            else:
                feat1[b, j] = np.float32(-0.6) * feat0[b, i] + (0.15 * rng.standard_normal(256)).astype(np.float32)
        feat1[b, cells[10]] = feat0[b, rows[1]] + (0.15 * rng.standard_normal(256)).astype(np.float32)      # a confident negative
        feat1[b, cells[11]] = np.float32(0.8) * feat0[b, rows[2]]
    i = int(np.nonzero(gt_j[0] >= 0)[0][0])                           # one positive above 1 - 1e-6
    feat0[0, i] *= np.float32(1.8)
    feat1[0, gt_j[0, i]] = feat0[0, i]
    feat_f0 = rng.standard_normal((T, 128)).astype(np.float32)
    feat_f1 = rng.standard_normal((T, W * W, 128)).astype(np.float32)
    expec_f_gt = rng.uniform(-0.9, 0.9, (T, 2)).astype(np.float32)
    expec_f_gt[[2, 5, 6, 9]] = [[1.2, 0.1], [-0.3, -1.0], [2.0, 2.0], [0.5, 1.5]]
    return {"feat0": feat0, "feat1": feat1, "gt_j": gt_j, "feat_f0": feat_f0, "feat_f1": feat_f1, "expec_f_gt": expec_f_gt}


def _by_path(name, path):
    spec = importlib.util.spec_from_file_location(name, os.path.join(REF, path))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


def _install_shims():
    sys.modules["loguru"] = types.ModuleType("loguru")
    sys.modules["loguru"].logger = logging.getLogger("ref")

    def create_meshgrid(height, width, normalized_coordinates=True, device=None):
        xs = torch.linspace(0, width - 1, width, device=device)
        ys = torch.linspace(0, height - 1, height, device=device)
        if normalized_coordinates:
            xs = (xs / (width - 1) - 0.5) * 2
            ys = (ys / (height - 1) - 0.5) * 2
        base = torch.stack(torch.meshgrid([xs, ys], indexing="ij")).transpose(1, 2)
        return base.unsqueeze(0).permute(0, 2, 3, 1)

    def spatial_expectation2d(inp, normalized_coordinates=True):
        b, c, h, w = inp.shape
        grid = create_meshgrid(h, w, normalized_coordinates, inp.device).to(inp.dtype)
        flat = inp.view(b, c, -1)
        ex = torch.sum(grid[..., 0].reshape(-1) * flat, -1, keepdim=True)
        ey = torch.sum(grid[..., 1].reshape(-1) * flat, -1, keepdim=True)
        return torch.cat([ex, ey], -1).view(b, c, 2)

    for name in ("kornia", "kornia.geometry", "kornia.geometry.subpix", "kornia.geometry.subpix.dsnt", "kornia.utils", "kornia.utils.grid"):
        sys.modules[name] = types.ModuleType(name)
    sys.modules["kornia.geometry.subpix.dsnt"].spatial_expectation2d = spatial_expectation2d
    sys.modules["kornia.geometry.subpix"].dsnt = sys.modules["kornia.geometry.subpix.dsnt"]
    sys.modules["kornia.utils.grid"].create_meshgrid = create_meshgrid


def main():
    _install_shims()
    losses = _by_path("ref_losses", "src/lightning_model/losses.py")
    fine = _by_path("ref_fine_matching", "src/models/OnePosePlus/utils/fine_matching.py")
    inp = make_inputs()
    leaves = {k: torch.tensor(inp[k], dtype=torch.float64, requires_grad=True) for k in ("feat0", "feat1", "feat_f0", "feat_f1")}

    # CoarseMatching.forward, lines 102-115 (feat_normalizer: sqrt_feat_dim)
    feat_db_3d, feat_query = map(lambda feat: feat / feat.shape[-1] ** .5, [leaves["feat0"], leaves["feat1"]])
    sim_matrix = torch.einsum("nlc,nsc->nls", feat_db_3d, feat_query) / (float(np.float32(TEMPERATURE + 1e-4)))
    conf_matrix = torch.nn.functional.softmax(sim_matrix, 1) * torch.nn.functional.softmax(sim_matrix, 2)

    matcher = fine.FineMatching({"s2d": {"type": "heatmap"}})
    matcher.W, matcher.WW, matcher.C = W, W * W, 128
    data = {}
    matcher._s2d_heatmap(leaves["feat_f0"], leaves["feat_f1"], data)

    conf_gt = torch.zeros(B, N, M, dtype=torch.int16)
    b, i = np.nonzero(inp["gt_j"] >= 0)
    conf_gt[b, i, inp["gt_j"][b, i]] = 1
    data.update({"conf_matrix": conf_matrix, "conf_matrix_gt": conf_gt, "expec_f_gt": torch.tensor(inp["expec_f_gt"], dtype=torch.float64)})
    loss = losses.Loss(LOSS_CONFIG)
    loss.train()
    loss(data)
    data["loss"].backward()
    out = dict(inp)
    out["expec_f"] = data["expec_f"].detach().numpy().astype(np.float32)        # the forward's output, as the device hands it to the loss
    out["ref_expec_f"] = data["expec_f"].detach().numpy()
    out["ref_conf_matrix"] = conf_matrix.detach().numpy()
    out["ref_loss"] = np.float64(data["loss"].item())
    for k, leaf in leaves.items():
        out[f"ref_grad_{k}"] = leaf.grad.numpy()
    path = os.path.join(HERE, "loss_backward_small.npz")
    np.savez_compressed(path, **out)
    conf = out["ref_conf_matrix"]
    pos = conf_gt.numpy() == 1
    print(f"wrote {path}: {os.path.getsize(path)} bytes; loss {out['ref_loss']:.6f}; positives below 1e-6: {(conf[pos] < 1e-6).sum()}, above "
          f"1 - 1e-6: {(conf[pos] > 1 - 1e-6).sum()}; negatives above 0.1: {(conf[~pos] > 0.1).sum()}")


if __name__ == "__main__":                                  # tests/test_loss_backward_cpu.py imports make_inputs: no side effect on import
    sys.dont_write_bytecode = True
    sys.path.insert(0, REPO)
    main()
