"""Time the device vote of the detector (``onepose_st_amd/detect_device.py``) against the host vote it is an alternative to.

    python tools/time_detect_device.py [--views 15] [--rows 300] [--trials 2048] [--iters 20] [--warmup 3] [--crop 512]

The matches are planted ones, left on the device as the LoFTR matcher leaves its own: ``--views`` reference views of ``--rows`` matches
each under one affinity per view (0.5 px noise, 30 % outliers), ``b_ids`` ascending.  Hot steps only: every timed call is preceded by
``--warmup`` untimed ones, and the two paths alternate call by call inside one loop.  One JSON line:

  * ``host_vote_ms``: what ``LocalFeatureObjectDetector.match_worker`` does after the matcher and what the loop does with the result --
    the one read-back of all matches, one ``oppnp_estimate_affine2d`` per view on the thread pool, the vote, ``track_device.set_box`` of
    the winning box -- on the host clock, ending when the state is on the device (a synchronisation);
  * ``device_vote_ms``: ``detect_device.vote`` on the same tensors: host clock to the same point, and ``device_vote_gpu_ms`` from HIP
    events around the call; ``stage_ms``: HIP events around each stage entry;
  * ``agree``: whether both paths chose the same view, box and per-view inlier counts.
"""
from __future__ import annotations

import argparse
import json
import math
import os
import statistics
import sys
import time

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

from onepose_st_amd import detect_device as dd, detector, track_device  # noqa: E402


def stats(ts):
    return {"median": round(statistics.median(ts), 4), "min": round(min(ts), 4), "max": round(max(ts), 4)}


def event_ms(fn):
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    res = fn()
    b.record()
    b.synchronize()
    return res, a.elapsed_time(b)


def planted_matches(views, rows, hw, seed=1):
    g = np.random.default_rng(seed)
    H, W = hw
    mk0, mk1 = [], []
    for _ in range(views):
        a, s = g.uniform(-0.5, 0.5), g.uniform(0.6, 1.2)
        A = np.array([[s * math.cos(a), -s * math.sin(a), g.uniform(20, 120)], [s * math.sin(a), s * math.cos(a), g.uniform(20, 120)]])
        src = np.stack([g.uniform(0, W, rows), g.uniform(0, H, rows)], axis=1)
        dst = src @ A[:, :2].T + A[:, 2] + g.uniform(-0.35, 0.35, size=(rows, 2))
        bad = g.permutation(rows)[:int(round(0.3 * rows))]
        ang, mag = g.uniform(0, 2 * math.pi, len(bad)), g.uniform(22.0, 200.0, len(bad))
        dst[bad] += np.stack([mag * np.cos(ang), mag * np.sin(ang)], axis=1)
        mk0.append(src.astype(np.float32)); mk1.append(dst.astype(np.float32))
    return np.concatenate(mk0), np.concatenate(mk1), np.repeat(np.arange(views, dtype=np.int64), rows)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--views", type=int, default=15)
    ap.add_argument("--rows", type=int, default=300)
    ap.add_argument("--trials", type=int, default=dd.DEFAULT_TRIALS)
    ap.add_argument("--iters", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--crop", type=int, default=512)
    a = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("time_detect_device.py measures on the GPU: none found")
    dev = torch.device("cuda:0")
    hw = (480, 640)
    V = a.views
    m0, m1, ids = planted_matches(V, a.rows, hw)
    mk0, mk1, b_ids = torch.from_numpy(m0).to(dev), torch.from_numpy(m1).to(dev), torch.from_numpy(ids).to(dev)
    K = np.array([[600.0, 0, 320.0], [0, 600.0, 240.0], [0, 0, 1]])
    Kd = torch.as_tensor(K).to(dev)
    view_hw = torch.tensor([hw] * V, dtype=torch.int32).to(dev)
    det = detector.LocalFeatureObjectDetector(None, [np.zeros(hw, np.uint8)] * V, device=dev)
    from concurrent.futures import ThreadPoolExecutor

    def host_vote():
        packed = torch.cat([b_ids.to(torch.float32)[:, None], mk0, mk1], 1).cpu().numpy()      # the one read-back
        bounds = np.searchsorted(packed[:, 0].astype(np.int64), np.arange(V + 1))
        with ThreadPoolExecutor(max_workers=min(8, V)) as ex:
            votes = list(ex.map(lambda i: det._vote(i, packed[bounds[i]:bounds[i + 1], 1:3], packed[bounds[i]:bounds[i + 1], 3:5], hw), range(V)))
        best = max(range(V), key=lambda i: (votes[i]["inliers"].sum(), -i))
        state = track_device.set_box(np.asarray(votes[best]["bbox"]).astype(np.int32), Kd, a.crop)
        torch.cuda.synchronize()
        return votes, best, state

    def device_vote():
        return dd.vote(mk0, mk1, b_ids, view_hw, hw, Kd, crop_size=a.crop, trials=a.trials)

    S = dd.stages
    count = torch.full((1,), mk0.shape[0], dtype=torch.int32, device=dev)
    st = {k: [] for k in ("ranges", "score", "select", "fit_box", "vote")}
    host_ms, dev_ms, dev_gpu_ms = [], [], []
    for it in range(a.warmup + a.iters):
        t0 = time.perf_counter()
        h_votes, h_best, h_state = host_vote()
        t1 = time.perf_counter()
        d = device_vote()
        torch.cuda.synchronize()
        t2 = time.perf_counter()
        _, t_gpu = event_ms(device_vote)
        rng, t_r = event_ms(lambda: S.ranges(b_ids, count, mk0.shape[0], V))
        (smp, cnt), t_sc = event_ms(lambda: S.score(mk0, mk1, rng, a.trials, 1))
        (best, n_in, status, mask), t_se = event_ms(lambda: S.select(mk0, mk1, rng, count, smp, cnt))
        (affine, boxes), t_f = event_ms(lambda: S.fit_box(mk0, mk1, rng, view_hw, hw, n_in, status, mask))
        _, t_v = event_ms(lambda: S.vote(boxes, n_in, status, hw, Kd, a.crop))
        if it >= a.warmup:
            for k, v in zip(st, (t_r, t_sc, t_se, t_f, t_v)):
                st[k].append(v)
            host_ms.append(1e3 * (t1 - t0)); dev_ms.append(1e3 * (t2 - t1)); dev_gpu_ms.append(t_gpu)
    d_votes, d_best = d.to_host()
    out = {"views": V, "rows_per_view": a.rows, "trials": a.trials, "device": torch.cuda.get_device_name(0),
           "host_vote_ms": stats(host_ms), "device_vote_ms": stats(dev_ms), "device_vote_gpu_ms": stats(dev_gpu_ms),
           "stage_ms": {k: stats(v) for k, v in st.items()},
           "agree": {"winner": h_best == d_best, "box": bool(np.array_equal(h_state.to_host()[0], d.state.to_host()[0])),
                     "inlier_counts": [int(np.asarray(h_votes[v]["inliers"]).sum()) for v in range(V)] == d.n_inliers.cpu().tolist()}}
    print(json.dumps(out))


if __name__ == "__main__":
    main()
