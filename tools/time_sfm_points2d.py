"""Time the SfM coarse-match merge on the device against the numpy / dict oracle (the reference's form of it).

    python tools/time_sfm_points2d.py [--rows 1000000,4000000,16000000] [--iters 5] [--oracle-max-rows 4000000]

Synthetic inputs like an object's pair list: 150 images, 15 covisible neighbours each (2 250 pairs), the rows spread over the pairs,
keypoints on 8 px cells of a 480 x 640 image times per-image scales, mconf in [0.2, 1].  For each row count T, one JSON line:
  * ``device_ms``: wall time of one ``sfm_coarse.merge_pair_matches`` call, inputs already on the device, input checks and the
    read-back included (median of ``--iters`` after a warm-up);
  * ``scatter_ms``: the summed device time of the ``sfm_p2d_radix_scatter`` launches of one call (``ophip_timing_select``: each
    launch's own begin and end), the largest share of the kernel work;
  * ``oracle_s``: one run of ``tests/sfm_points2d_oracle.oracle_merge`` (dicts keyed by coordinate tuples, as the reference does it;
    single-threaded Python) when T <= ``--oracle-max-rows``, and ``vectorised_oracle_s`` of ``oracle_merge_vectorised`` (numpy).
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

from onepose_st_amd import hip, sfm_coarse  # noqa: E402
from tests import sfm_points2d_oracle as so  # noqa: E402


def make_case(T: int, n_images: int = 150, neighbours: int = 15, seed: int = 0):
    rng = np.random.default_rng(seed)
    pim = np.array([(a, (a + 1 + k) % n_images) for a in range(n_images) for k in range(neighbours)], np.int64)
    P = len(pim)
    cuts = np.sort(rng.integers(0, T, P - 1))
    off = np.concatenate([[0], cuts, [T]]).astype(np.int64)
    pr = np.repeat(np.arange(P), np.diff(off))
    scale = rng.uniform(0.55, 1.8, (n_images, 2)).astype(np.float32)
    cells = lambda: np.stack([rng.integers(0, 80, T), rng.integers(0, 60, T)], 1).astype(np.float32) * np.float32(8)
    return cells() * scale[pim[pr, 0]], cells() * scale[pim[pr, 1]], rng.uniform(0.2, 1.0, T).astype(np.float32), off, pim, n_images


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rows", default="1000000,4000000,16000000")
    ap.add_argument("--iters", type=int, default=5)
    ap.add_argument("--oracle-max-rows", type=int, default=4_000_000)
    args = ap.parse_args()
    hip.load()
    dev = torch.device("cuda:0")
    for T in (int(x) for x in args.rows.split(",")):
        case = make_case(T)
        d = [torch.from_numpy(a).to(dev) for a in case[:5]]

        def call():
            return sfm_coarse.merge_pair_matches(*d, case[5])

        out = call()
        torch.cuda.synchronize()
        walls = []
        for _ in range(args.iters):
            t0 = time.perf_counter()
            call()
            torch.cuda.synchronize()
            walls.append((time.perf_counter() - t0) * 1e3)
        hip.timing_select("sfm_p2d_radix_scatter")
        call()
        torch.cuda.synchronize()
        n, kms = hip.timing_read()
        hip.timing_select("")
        row = {"rows": T, "pairs": len(case[4]), "images": case[5], "unique_keys": int(out["keypoints"].shape[0]),
               "device_ms": round(statistics.median(walls), 2), "scatter_launches": n, "scatter_ms": round(kms, 2)}
        t0 = time.perf_counter()
        want = so.oracle_merge_vectorised(*case)
        row["vectorised_oracle_s"] = round(time.perf_counter() - t0, 2)
        if T <= args.oracle_max_rows:
            t0 = time.perf_counter()
            so.oracle_merge(*case)
            row["oracle_s"] = round(time.perf_counter() - t0, 2)
        got = {k: v.cpu().numpy() for k, v in out.items()}
        row["bit_exact"] = all(np.array_equal(got[k], want[k]) for k in ("keypoints", "scores", "kpt_offsets", "match_ids"))
        print(json.dumps(row), flush=True)


if __name__ == "__main__":
    main()
