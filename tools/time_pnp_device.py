"""Time the device PnP (``onepose_st_amd/pnp_device.py``) against the host solver it is an alternative to.

    python tools/time_pnp_device.py [--workload c2] [--trials 10240] [--iters 20] [--warmup 3] [--threads 12] [--frames 40] [--no-sequence]

The matches are the matcher's own: one synthetic frame of ``--workload`` (c2: 7 000 points, 480 x 640, about 2 975 matches) through the
model, left on the device.  Hot steps only: every timed call is preceded by ``--warmup`` untimed ones, and the paths that are compared
alternate call by call inside one loop.  One JSON line:

  * ``matches``; ``stage_ms``: HIP events around each stage entry (``ranges`` + ``prep``, ``sample``, ``p3p``, ``score``, ``select``,
    ``refine``) and ``solve_ms`` around ``oppnpd_solve``; median, minimum and maximum of ``--iters`` calls;
  * ``host_one_thread_ms``: ``pnp.ransac_PnP(use_pycolmap_ransac=True)`` on the same matches (host clock, one thread), and
    ``host_pool_ms``: submit -> wait -> result of a ``PnPPool`` of ``--threads`` threads: the pool's pose latency;
  * ``sequence``: the dependent sequence (one frame in flight: frame t + 1 is enqueued after frame t's pose is on the host), model + pose
    latency per frame with ``pnp="host"`` (``host_copy`` read-back, pool) and ``pnp="device"`` (``enqueue_after``, one read-back of pose,
    status and mask), ``--frames`` frames each in alternation;
  * ``agree``: whether the device's inlier set equals the host's and the relative pose difference.
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

from onepose_st_amd import pnp, pnp_device as pd  # noqa: E402
from onepose_st_amd.config import default_config  # noqa: E402
from onepose_st_amd.model import OnePosePlus_model  # noqa: E402
from onepose_st_amd.synthetic import CONFIG_SIZES, make_synthetic_inputs, make_synthetic_state_dict, workload_kwargs  # noqa: E402


def stats(ts):
    return {"median": round(statistics.median(ts), 4), "min": round(min(ts), 4), "max": round(max(ts), 4)}


def event_ms(fn):
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    res = fn()
    b.record()
    b.synchronize()
    return res, a.elapsed_time(b)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--workload", default="c2", choices=sorted(CONFIG_SIZES))
    ap.add_argument("--trials", type=int, default=pd.DEFAULT_TRIALS)
    ap.add_argument("--iters", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--threads", type=int, default=12)
    ap.add_argument("--frames", type=int, default=40)
    ap.add_argument("--reproj", type=float, default=7.0)
    ap.add_argument("--no-sequence", action="store_true")
    a = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("time_pnp_device.py measures on the GPU: none found")
    dev = torch.device("cuda:0")
    cfg = default_config()
    sd = make_synthetic_state_dict(0, cfg)
    model = OnePosePlus_model(cfg).eval()
    model.load_state_dict(sd, strict=True)
    model.to(dev)
    n, hw, plant = CONFIG_SIZES[a.workload]
    inp = make_synthetic_inputs(sd, n_points=n, image_hw=hw, n_plant=plant, seed=1, config=cfg, **workload_kwargs(a.workload))
    obj = {k: inp[k].to(dev) for k in ("keypoints3d", "descriptors3d_db", "descriptors3d_coarse_db")}
    fc, ff, K = inp["feat_c"].to(dev), inp["feat_f"].to(dev), inp["K"].numpy()
    data = dict(obj)
    model.forward_features(data, fc, ff, inp["image_hw"])
    mk2d, mk3d = data["mkpts_query_f"].contiguous(), data["mkpts_3d_db"].contiguous()
    h2, h3 = mk2d.cpu().numpy(), mk3d.cpu().numpy()
    M = mk2d.shape[0]
    out = {"workload": a.workload, "matches": M, "trials": a.trials, "reproj_px": a.reproj, "device": torch.cuda.get_device_name(0)}

    # ---- the stages, one entry each, and the whole solve; the host call and the pool in the same loop -------------------------------------------
    S = pd.stages
    count = torch.full((1,), M, dtype=torch.int32, device=dev)
    Kd = torch.as_tensor(K, device=dev)
    pool = pnp.PnPPool(K, threads=a.threads, pnp_reprojection_error=a.reproj, policy="reference")
    st = {k: [] for k in ("ranges_prep", "sample", "p3p", "score", "select", "refine")}
    solve_ms, host_ms, pool_ms = [], [], []
    dev_res = None
    for it in range(a.warmup + a.iters):
        (rng, rows), t_rp = event_ms(lambda: (S.ranges(None, count, M, 1), S.prep(Kd, mk2d, mk3d, count, None, 1)))
        smp, t_s = event_ms(lambda: S.sample(rng, a.trials, 1))
        (hyps, _), t_p = event_ms(lambda: S.p3p(rows, rng, smp))
        (cnt, cost), t_sc = event_ms(lambda: S.score(rows, rng, Kd, hyps, a.reproj))
        (best, n_in, status, mask), t_se = event_ms(lambda: S.select(cnt, cost, rows, rng, count, Kd, hyps, a.reproj, 0.99, a.trials))
        _, t_r = event_ms(lambda: S.refine(rows, rng, Kd, hyps, best, n_in, status, mask, a.reproj))
        dev_res, t_solve = event_ms(lambda: pd.ransac_pnp(K, mk2d, mk3d, pnp_reprojection_error=a.reproj, trials=a.trials))
        t0 = time.perf_counter()
        host_res = pnp.ransac_PnP(K, h2, h3, pnp_reprojection_error=a.reproj, use_pycolmap_ransac=True)
        t1 = time.perf_counter()
        ticket = pool.submit(h2, h3)
        pool.wait_all()
        pool.result(ticket)
        t2 = time.perf_counter()
        if it >= a.warmup:
            for k, v in zip(st, (t_rp, t_s, t_p, t_sc, t_se, t_r)):
                st[k].append(v)
            solve_ms.append(t_solve)
            host_ms.append(1e3 * (t1 - t0))
            pool_ms.append(1e3 * (t2 - t1))
    out["stage_ms"] = {k: stats(v) for k, v in st.items()}
    out["solve_ms"], out["host_one_thread_ms"], out["host_pool_ms"] = stats(solve_ms), stats(host_ms), stats(pool_ms)
    (d_pose, _, d_inl), = dev_res.to_host()
    dR = float(np.abs(d_pose[:, :3] - host_res[0][:, :3]).max())
    dt = float(np.linalg.norm(d_pose[:, 3] - host_res[0][:, 3]) / np.linalg.norm(host_res[0][:, 3]))
    out["agree"] = {"same_inlier_set": bool(np.array_equal(d_inl, host_res[2])), "inliers": int(len(d_inl)), "pose_difference": max(dR, dt),
                    "status": int(dev_res.status_host[0])}

    # ---- the dependent sequence: one frame in flight, model + pose latency --------------------------------------------------------------------
    if not a.no_sequence:
        def frame_host():
            got = {}
            pend = model.enqueue_features(dict(obj), fc, ff, inp["image_hw"], host_copy=True)
            pend.finish(on_host=lambda h: got.update(t=pool.submit(h["mkpts_2d"], h["mkpts_3d_db"])))
            pool.wait_all()
            return pool.result(got["t"])[0]

        def frame_device():
            pend = model.enqueue_features(dict(obj), fc, ff, inp["image_hw"])
            res = pd.enqueue_after(pend, K, pnp_reprojection_error=a.reproj, trials=a.trials).to_host()[0][0]
            pend.finish()
            return res
        lat = {"host": [], "device": []}
        for it in range(a.warmup + a.frames):
            for mode, fn in (("host", frame_host), ("device", frame_device)):
                torch.cuda.synchronize()
                t0 = time.perf_counter()
                fn()
                if it >= a.warmup:
                    lat[mode].append(1e3 * (time.perf_counter() - t0))
        out["sequence"] = {"latency_ms_" + m: stats(v) for m, v in lat.items()}
    pool.close()
    print(json.dumps(out))


if __name__ == "__main__":
    main()
