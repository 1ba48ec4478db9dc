"""Time the SfM object block on the device against the numpy oracle.

    python tools/time_sfm_objectblock.py [--case realistic|large] [--iters 5] [--reference-form]

``realistic``: ~60 000 points before filtering, max_num_kp3d 15 000, 150 images, mean track length ~20 (the case of
tests/test_gpu_sfm_objectblock.py); ``large``: 200 000 points, kept count ~20 000.  One JSON line:
  * ``device_ms``: wall time of one synchronised ``sfm_objectblock.build_object_block`` call, inputs on the device, input checks and
    read-backs included (median of ``--iters`` after a warm-up); ``select_points_ms`` the same for stage B alone;
  * ``vectorised_oracle_s``: one run of ``tests/sfm_objectblock_oracle.vectorised_form`` (numpy, single-threaded);
  * ``reference_form_s`` (``--reference-form``): the dict / pdist form the reference runs; it forms the N x N matrix.
"""
from __future__ import annotations

import argparse
import json
import os
import statistics
import sys
import time

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

from onepose_st_amd import sfm_objectblock as sob  # noqa: E402
from tests import sfm_objectblock_oracle as orc  # noqa: E402

TRACK_KEYS = ("assigned_image", "assigned_kpt", "row_offsets", "ref_image", "ref_kpt", "feature_c0", "feature_c1", "feature0", "feature1")
CASES = {"realistic": dict(seed=21, Q=57000, I=150, mean_track=20, max_num_kp3d=15000, n_close=2500, n_chains=400, cluster=70, collisions=3000),
         "large": dict(seed=22, Q=195000, I=150, mean_track=8, max_num_kp3d=20000, n_close=4000, n_chains=600, cluster=70)}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--case", default="realistic", choices=sorted(CASES))
    ap.add_argument("--iters", type=int, default=5)
    ap.add_argument("--reference-form", action="store_true")
    a = ap.parse_args()
    torch.set_num_threads(1)
    case = orc.make_case(**CASES[a.case])
    t = {k: torch.from_numpy(np.ascontiguousarray(v)).cuda() for k, v in case.items() if isinstance(v, np.ndarray)}

    def whole():
        return sob.build_object_block({k: t[k] for k in TRACK_KEYS}, {k: t[k] for k in ("point_ids", "xyz", "track_len")}, t["point3D_ids"],
                                      t["kpt_offsets"], bbox_corners=t.get("bbox_corners"), max_num_kp3d=case["max_num_kp3d"])

    def stage_b():
        return sob.select_points(t["point_ids"], t["xyz"], t["track_len"], t.get("bbox_corners"), case["max_num_kp3d"])

    out = {"case": a.case, "points": len(case["xyz"]), "rows": len(case["ref_image"]), "keypoints2d": int(case["kpt_offsets"][-1])}
    for name, fn in (("device_ms", whole), ("select_points_ms", stage_b)):
        res = fn()
        torch.cuda.synchronize()
        ts = []
        for _ in range(a.iters):
            t0 = time.perf_counter()
            res = fn()
            torch.cuda.synchronize()
            ts.append((time.perf_counter() - t0) * 1e3)
        out[name] = round(statistics.median(ts), 3)
        out.setdefault("counts", res["counts"])
    t0 = time.perf_counter()
    orc.vectorised_form(case)
    out["vectorised_oracle_s"] = round(time.perf_counter() - t0, 3)
    if a.reference_form:
        t0 = time.perf_counter()
        orc.reference_form(case)
        out["reference_form_s"] = round(time.perf_counter() - t0, 3)
    print(json.dumps(out))


if __name__ == "__main__":
    main()
