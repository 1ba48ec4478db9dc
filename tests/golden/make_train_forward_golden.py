"""Generate ``train_forward_small.npz`` FROM THE REFERENCE ITSELF.

Run in the build container only (needs the reference checkout beside the repository; the GPU box never sees it):

    python tests/golden/make_train_forward_golden.py

The inputs are seeded (:func:`make_inputs`): B = 2, N = 64, a 5 x 6 coarse grid (M = 30), ``train_coarse_percent`` 0.3 and
``train_pad_num_gt_min`` 5, so T = 18 and T - G = 13; a ``conf_matrix`` with P planted mutual maxima above ``thr`` for P = 0, 5, 13, 14 and
40 (nothing predicted; the keep-all branch; both sides of its ``<=``; P > T), a ground truth with one entry in the whole batch, one with
entries in batch 1 only, and a ``query_image_scale`` case.  The outputs are the reference's:

* ``src/models/OnePosePlus/utils/coarse_matching.py`` is imported by file path and run as it is, ``loguru`` and ``src.utils.profiler``
  shimmed (logging and profiling only).  Nothing else of the reference is imported.
* ``CoarseMatching(config).eval().get_coarse_match`` gives the predicted lists (stored as ``pred_*``: the inputs of the padding);
  ``.train().get_coarse_match`` gives every key stored as ``ref_*``.
* ``torch.randint`` is patched, inside this recipe only, to return the picks of the project's own sampler
  (``tests/train_forward_oracle.picks``) for that call: the draws are the project's specification and cannot equal torch's stream.  With
  P > T - G the first call is the predicted picks and the second the ground-truth picks; else the one call is the ground-truth picks.
* The dense ``conf_matrix_gt`` comes from ``supervision.GroundTruth.to_dense()``.

Only data is stored."""
from __future__ import annotations

import contextlib
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

B, N, HW_C, HW_I = 2, 64, (5, 6), (40, 48)
M = HW_C[0] * HW_C[1]
PERCENT, G, SEED = 0.3, 5, 20240229
CONFIG = {"type": "dual-softmax", "dual_softmax": {"temperature": 0.08}, "thr": 0.2, "border_rm": 0, "feat_norm_method": "sqrt_feat_dim",
          "train": {"train_padding": True, "train_coarse_percent": PERCENT, "train_pad_num_gt_min": G}}
# case -> (P, the ground truth's kind, with a query_image_scale); its position is the sampler's step
CASES = {"p0": (0, "plain", False), "p5": (5, "plain", False), "p13": (13, "plain", False), "p14": (14, "plain", False),
         "p40": (40, "plain", False), "one_gt": (14, "one", False), "batch1_gt": (5, "batch1", False), "scaled": (14, "plain", True)}
SCALE = np.array([[1.25, 0.75], [1.0, 1.5]], np.float32)
KEYS = ("b_ids", "i_ids", "j_ids", "gt_mask", "m_bids", "mkpts_3d_db", "mkpts_query_c", "mconf")


def make_inputs():
    """-> {case: dict(conf_matrix [B, N, M] float32, gt_j [B, N] int64, keypoints3d [B, N, 3] float32, scale [B, 2] or None, step)}"""
    out = {}
    for step, (name, (P, kind, scaled)) in enumerate(CASES.items()):
        rng = np.random.default_rng(1000 + step)
        conf = rng.uniform(0.0, 0.05, (B, N, M)).astype(np.float32)
        cells = rng.permutation(B * M)[:P]                   # distinct (b, j), and a distinct i per frame: mutual maxima
        points = [rng.permutation(N) for _ in range(B)]
        used = [0] * B
        for cell in cells:
            b, j = divmod(int(cell), M)
            conf[b, points[b][used[b]], j] = np.float32(rng.uniform(0.5, 0.9))
            used[b] += 1
        gt_j = np.full((B, N), -1, np.int64)
        for b in range(B):
            ids, js = rng.permutation(N)[:20], rng.permutation(M)[:20]
            if kind == "plain" or (kind == "batch1" and b == 1):
                gt_j[b, ids] = js
            elif kind == "one" and b == 1:
                gt_j[b, ids[0]] = js[0]
        out[name] = dict(conf_matrix=conf, gt_j=gt_j, keypoints3d=rng.uniform(-1, 1, (B, N, 3)).astype(np.float32),
                         scale=SCALE if scaled else None, step=step)
    return out


def _by_path(name, path):
    spec = importlib.util.spec_from_file_location(name, os.path.join(REF, path))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


def _shims():
    sys.modules["loguru"] = types.ModuleType("loguru")
    sys.modules["loguru"].logger = logging.getLogger("ref")
    profiler = types.ModuleType("src.utils.profiler")

    class PassThroughProfiler:
        @staticmethod
        def record_function(name):
            return contextlib.nullcontext()
    profiler.PassThroughProfiler = PassThroughProfiler
    for name in ("src", "src.utils"):
        sys.modules.setdefault(name, types.ModuleType(name))
    sys.modules["src.utils.profiler"] = profiler


def main():
    from onepose_st_amd import supervision
    from onepose_st_amd.train_forward import train_rows
    from tests import train_forward_oracle as oracle
    _shims()
    ref = _by_path("ref_coarse_matching", "src/models/OnePosePlus/utils/coarse_matching.py")
    T = train_rows(B, N, M, PERCENT)
    assert T == 18 == oracle.train_rows(B, N, M, PERCENT)
    out = {}
    for name, inp in make_inputs().items():
        gt_j = torch.from_numpy(inp["gt_j"])
        gt_i = torch.full((B, M), -1, dtype=torch.int64)
        b, i = (gt_j >= 0).nonzero(as_tuple=True)
        gt_i[b, gt_j[b, i]] = i
        sparse = supervision.GroundTruth(gt_j, torch.zeros(B, N, 2), gt_i, (gt_j >= 0).sum(1).to(torch.int32), HW_C)
        conf = torch.from_numpy(inp["conf_matrix"])
        data = {"q_hw_c": HW_C, "q_hw_i": HW_I, "keypoints3d": torch.from_numpy(inp["keypoints3d"]), "conf_matrix_gt": sparse.to_dense()[0]}
        if inp["scale"] is not None:
            data["query_image_scale"] = torch.from_numpy(inp["scale"])
        pred = ref.CoarseMatching(CONFIG).eval().get_coarse_match(conf, data)
        P = len(pred["b_ids"])
        assert P == CASES[name][0] and bool((pred["mconf"] > CONFIG["thr"]).all())
        plan = [0, 1] if P > T - G else [1]

        def randint(high, size, device=None, _plan=plan, _step=inp["step"]):
            return torch.from_numpy(oracle.picks(SEED, _step, _plan.pop(0), high, size[0]))
        real = torch.randint
        torch.randint = randint
        try:
            got = ref.CoarseMatching(CONFIG).train().get_coarse_match(conf, data)
        finally:
            torch.randint = real
        assert not plan and set(got) == set(KEYS) and len(got["b_ids"]) == T
        for k, v in inp.items():
            if v is not None:
                out[f"{name}__{k}"] = np.asarray(v)
        for k in ("b_ids", "i_ids", "j_ids", "mconf", "mkpts_3d_db", "mkpts_query_c"):
            out[f"{name}__pred_{k}"] = pred[k].numpy()
        for k in KEYS:
            out[f"{name}__ref_{k}"] = got[k].numpy()
    path = os.path.join(HERE, "train_forward_small.npz")
    np.savez_compressed(path, **out)
    print(f"wrote {path}: {os.path.getsize(path)} bytes, {len(out)} arrays")


if __name__ == "__main__":                                  # tests/test_train_forward_cpu.py imports make_inputs: no side effect on import
    sys.dont_write_bytecode = True
    sys.path.insert(0, REPO)
    main()
