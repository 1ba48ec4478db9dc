"""Generate the full-attention golden fixtures in this directory FROM THE REFERENCE ITSELF.

Run in the build container only (needs the reference; the GPU box never sees it):

    python tests/golden/make_golden_full_attention.py

Same inputs, hooks and packing as ``make_golden.py`` (cases A and B) with ``attention = "full"``
(``loftr_module/transformer.py:29-38`` then builds ``FullAttention``, ``linear_attention.py:64-95``):
``*_full_attention_*`` with both encoders full, ``*_full_coarse_*`` with the coarse encoder full and the fine
one linear.  Both attention forms use the same 195 ``state_dict`` keys, so the synthetic state dict loads strictly.
"""
from __future__ import annotations

import os
import sys

import numpy as np
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
sys.dont_write_bytecode = True
sys.path.insert(0, HERE)

from make_golden import load_reference_model, pack_feature_case, run_feature_case  # noqa: E402


def full_config(fine="full"):
    from onepose_st_amd.config import default_config
    cfg = default_config()
    cfg["loftr_coarse"]["attention"] = "full"
    cfg["loftr_fine"]["attention"] = fine
    return cfg


def write_cases(sd, cfg, tag):
    from onepose_st_amd.synthetic import make_synthetic_inputs
    model = load_reference_model(cfg, sd)
    key = lambda i, j: i.astype(np.int64) * 100000 + j

    # ---- case A: c1-size planted frame (B = 1) ---------------------------------------------------------------------
    inp = make_synthetic_inputs(sd, n_points=1000, image_hw=(240, 320), n_plant=600, seed=1, config=cfg)
    data, caps = run_feature_case(model, inp)
    g = pack_feature_case(inp, data, caps)
    rm = g["conf_rowmax"]
    print(f"case c1 {tag}: K =", len(g["i_ids"]),
          "planted-correct =", int(np.isin(key(g["i_ids"], g["j_ids"]), key(g["planted_i"], g["planted_j"])).sum()),
          "min |mconf - thr| =", float(np.abs(g["mconf"] - 0.1).min()),
          "row maxima within 1e-3 of thr:", int((np.abs(rm - 0.1) < 1e-3).sum()))
    np.savez_compressed(os.path.join(HERE, f"c1_{tag}_feature_boundary.npz"), **g)

    # ---- case B: ragged B = 2 (two frames of one object) -------------------------------------------------------------
    i0 = make_synthetic_inputs(sd, n_points=333, image_hw=(96, 136), n_plant=120, seed=3, config=cfg, frame=0)
    i1 = make_synthetic_inputs(sd, n_points=333, image_hw=(96, 136), n_plant=120, seed=3, config=cfg, frame=1)
    both = {k: torch.cat([i0[k], i1[k]], 0) for k in ("keypoints3d", "descriptors3d_db", "descriptors3d_coarse_db", "feat_c", "feat_f")}
    both["image_hw"] = i0["image_hw"]
    both["planted_i"], both["planted_j"] = i0["planted_i"], i0["planted_j"]
    both["pose_gt"], both["K"] = i0["pose_gt"], i0["K"]
    data, caps = run_feature_case(model, both)
    g = pack_feature_case(both, data, caps)
    print(f"case b2 {tag}: K =", len(g["i_ids"]), "per batch:", np.bincount(g["b_ids"], minlength=2),
          "min |mconf - thr| =", float(np.abs(g["mconf"] - 0.1).min()))
    np.savez_compressed(os.path.join(HERE, f"b2_{tag}_feature_boundary.npz"), **g)


def main():
    from onepose_st_amd.config import default_config
    from onepose_st_amd.synthetic import make_synthetic_state_dict

    torch.set_num_threads(4)
    sd = make_synthetic_state_dict(seed=0, config=default_config())
    write_cases(sd, full_config("full"), "full_attention")
    write_cases(sd, full_config("linear"), "full_coarse")


if __name__ == "__main__":
    main()
