"""Time the pose evaluation on the device against the same work on the host (HIP events, hot rounds; both sides in one process).

    python tools/time_pose_eval.py [--frames 1000] [--vertices 2048 20000] [--iters 10] [--host-frames 50] [--pair-budget N]

The scene is seeded (``tests/pose_eval_oracle.scene``): ``--frames`` pose pairs a few degrees and centimetres apart and a model of V
random vertices, for every V of ``--vertices``.  Prints one JSON line; per V:
  * ``errors_ms``: the cm-degree kernel alone (no model);
  * ``add_ms`` / ``adds_ms`` / ``proj2d_ms``: one ``pose_eval.pose_errors`` call with the model (``symmetric`` for ADD-S; with ``K`` for
    the projection error, the ADD part of that call subtracted) over all frames, nothing read back, minus ``errors_ms``;
  * ``adds_launches`` and ``adds_pairs_per_s``: how many launches the pair budget cut the ADD-S work into and the rate of vertex pairs,
    from which ``adds_launch_ms``, the time of one full launch of ``MAX_PAIRS_PER_LAUNCH`` (or ``--pair-budget``) pairs, follows;
  * ``host_*_ms_per_frame``: the reference's expressions on one host core -- numpy for ADD and the projection error,
    ``scipy.spatial.cKDTree`` for ADD-S (a numpy brute force if scipy is missing: ``host_adds`` says which) -- timed over
    ``--host-frames`` frames; ``device_*_ms_per_frame`` beside them.
Device figures are the median of ``--iters`` timed rounds after two warm-up rounds (ADD-S at V >= 10000: a third of the rounds).
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

from onepose_st_amd import pose_eval  # noqa: E402
from tests import pose_eval_oracle as po  # noqa: E402


def event_ms(fn):
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    torch.cuda.synchronize()
    a.record()
    fn()
    b.record()
    b.synchronize()
    return a.elapsed_time(b)


def median_ms(fn, iters):
    for _ in range(2):
        fn()
    return statistics.median(event_ms(fn) for _ in range(max(1, iters)))


def host_ms_per_frame(fn, frames):
    t0 = time.perf_counter()
    for f in range(frames):
        fn(f)
    return (time.perf_counter() - t0) * 1e3 / frames


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--frames", type=int, default=1000)
    ap.add_argument("--vertices", type=int, nargs="+", default=[2048, 20000])
    ap.add_argument("--iters", type=int, default=10)
    ap.add_argument("--host-frames", type=int, default=50)
    ap.add_argument("--pair-budget", type=int, default=None)
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("time_pose_eval.py needs the GPU: a time taken anywhere else says nothing")
    pose_eval.load()
    try:
        from scipy.spatial import cKDTree
    except ImportError:
        cKDTree = None
    dev = torch.device("cuda:0")
    F = args.frames
    budget = pose_eval.MAX_PAIRS_PER_LAUNCH if args.pair_budget is None else args.pair_budget
    out = {"frames": F, "iters": args.iters, "host_frames": min(args.host_frames, F), "pair_budget": budget,
           "host_adds": "cKDTree" if cKDTree is not None else "numpy brute force", "cases": []}
    for V in args.vertices:
        s = po.scene(V, F, V)
        verts, pred, gt, K = s["verts"], s["pose_pred"], s["pose_gt"], s["K"]
        d_verts, d_pred, d_gt, d_K = (torch.from_numpy(a).to(dev) for a in (verts, pred, gt, K))
        run = lambda **kw: pose_eval.pose_errors(d_pred, d_gt, **kw)
        errors_ms = median_ms(lambda: run(), args.iters)
        add_ms = median_ms(lambda: run(model_points=d_verts), args.iters) - errors_ms
        proj_ms = median_ms(lambda: run(model_points=d_verts, K=d_K), args.iters) - errors_ms - add_ms
        adds_ms = median_ms(lambda: run(model_points=d_verts, symmetric=True, pair_budget=args.pair_budget),
                            args.iters if V < 10000 else args.iters // 3) - errors_ms
        per_launch = budget // (V * V) if V * V <= budget else 0
        launches = -(-F // min(per_launch, 65535)) if per_launch else F * -(-((V + 255) // 256) // (budget // (256 * V)))
        rate = F * V * V / (adds_ms * 1e-3)
        case = {"V": V, "errors_ms": round(errors_ms, 4), "add_ms": round(add_ms, 4), "proj2d_ms": round(proj_ms, 4), "adds_ms": round(adds_ms, 3),
                "adds_launches": launches, "adds_pairs_per_s": float(f"{rate:.4g}"), "adds_launch_ms": round(budget / rate * 1e3, 3)}
        x = verts.astype(np.float64)
        n = out["host_frames"]

        def both(f):
            return x @ pred[f][:, :3].T + pred[f][:, 3], x @ gt[f][:, :3].T + gt[f][:, 3]

        def host_add(f):
            a, b = both(f)
            return np.mean(np.linalg.norm(a - b, axis=-1))

        def host_adds(f):
            a, b = both(f)
            if cKDTree is not None:
                return np.mean(cKDTree(a).query(b, k=1)[0])
            return np.mean([np.sqrt(((a - t) ** 2).sum(axis=1).min()) for t in b])

        def host_proj(f):
            a, b = both(f)
            ua, ub = a @ K.T, b @ K.T
            return np.mean(np.linalg.norm(ua[:, :2] / ua[:, 2:] - ub[:, :2] / ub[:, 2:], axis=-1))

        for name, fn, ms in (("add", host_add, add_ms), ("adds", host_adds, adds_ms), ("proj2d", host_proj, proj_ms)):
            case[f"host_{name}_ms_per_frame"] = round(host_ms_per_frame(fn, n), 4)
            case[f"device_{name}_ms_per_frame"] = float(f"{ms / F:.4g}")
        # the two sides computed the same thing: frame 0 within the summation-order bound
        errs = pose_eval.pose_errors(d_pred[:1], d_gt[:1], model_points=d_verts, symmetric=True).add_dist.item()
        ref = host_adds(0)
        assert abs(errs - ref) <= po.mean_bound(po.coordinate_scale(verts, pred[:1], gt[:1]), V, ref), (errs, ref)
        out["cases"].append(case)
    print(json.dumps(out), flush=True)


if __name__ == "__main__":
    main()
