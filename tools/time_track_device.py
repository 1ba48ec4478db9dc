"""Time the dependent chain of a tracked sequence -- crop, matcher, pose, next box -- with the box step on the host (today's
``SequenceRunner(pnp="device")`` loop) and on the device (``track_device``) at ``lookahead`` 1, 2, 3.

    python tools/time_track_device.py [--workloads c1 c2] [--frames 40] [--reps 3] [--warmup 1] [--trials 10240]

Per workload one JSON line.  Hot steps only: ``--warmup`` untimed rounds first; the compared paths alternate inside one loop, round by
round.  Every path runs the same kernels on the same data per frame:

  * the crop of a random uint8 frame to ``S x S`` (256 at c1, 512 at c2), the HIP backbone and the matcher on that crop against an
    object block of the workload's size (``model.enqueue``);
  * the device PnP on the *planted* matches of the workload's synthetic frame (a random crop holds no object, and a solve without
    matches would do no work), with that frame's ``K``;
  * the next box from that pose.

``host_box``: the pose is read (``DevicePoses.to_host``), ``project_bbox`` and ``crop_geometry`` run in numpy, the box goes into
``ophip_crop_resize_gray`` as host integers; frame t + 1 is enqueued after that.  ``device_box_la<L>``: ``track_device.next_box`` and
``track_device.crop``; up to L frames are enqueued before the oldest one's packed record (pose, status, mask, state, next flag; copied
to pinned memory behind the frame) is read.  The flags do not change which kernels run, so the device chain is driven WITHOUT
rewinding: the solve takes the planted frame's ``K`` (its matches were made for it) instead of ``state.K_crop``, which is computed and
read back all the same.  The output says so (``"rewind": false``).

Reported per path: ``fps`` (frames over the host clock from the first enqueue to the last record), ``latency_ms`` (enqueue of a frame
to its record on the host: median, minimum, maximum) and ``gpu_ms_per_frame`` (HIP events around the round, over its frames).
"""
from __future__ import annotations

import argparse
import json
import os
import statistics
import sys
import time
from collections import deque

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

from onepose_st_amd import frameloop as fl, pnp_device as pd, track_device as td  # noqa: E402
from onepose_st_amd.config import default_config  # noqa: E402
from onepose_st_amd.model import OnePosePlus_model  # noqa: E402
from onepose_st_amd.synthetic import CONFIG_SIZES, make_synthetic_inputs, make_synthetic_state_dict, workload_kwargs  # noqa: E402

CROP = {"c1": 256, "c2": 512}


def stats(ts):
    return {"median": round(statistics.median(ts), 4), "min": round(min(ts), 4), "max": round(max(ts), 4)}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--workloads", nargs="+", default=["c1", "c2"], choices=sorted(CROP))
    ap.add_argument("--frames", type=int, default=40)
    ap.add_argument("--reps", type=int, default=3)
    ap.add_argument("--warmup", type=int, default=1)
    ap.add_argument("--trials", type=int, default=pd.DEFAULT_TRIALS)
    ap.add_argument("--reproj", type=float, default=7.0)
    a = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("time_track_device.py measures on the GPU: none found")
    dev = torch.device("cuda:0")
    cfg = default_config()
    sd = make_synthetic_state_dict(0, cfg)
    model = OnePosePlus_model(cfg).eval()
    model.load_state_dict(sd, strict=True)
    model.to(dev)
    for wl in a.workloads:
        n, hw, plant = CONFIG_SIZES[wl]
        S = CROP[wl]
        inp = make_synthetic_inputs(sd, n_points=n, image_hw=hw, n_plant=plant, seed=1, config=cfg, **workload_kwargs(wl))
        obj = {k: inp[k].to(dev) for k in ("keypoints3d", "descriptors3d_db", "descriptors3d_coarse_db")}
        K = inp["K"].numpy().astype(np.float64)
        planted = dict(obj)
        model.forward_features(planted, inp["feat_c"].to(dev), inp["feat_f"].to(dev), inp["image_hw"])
        mk2d, mk3d = planted["mkpts_query_f"].contiguous(), planted["mkpts_3d_db"].contiguous()
        pts = inp["keypoints3d"][0].numpy().astype(np.float64)
        lo, hi = pts.min(axis=0), pts.max(axis=0)
        bbox3d = np.array([[x, y, z] for x in (lo[0], hi[0]) for y in (lo[1], hi[1]) for z in (lo[2], hi[2])])
        Kd, cube = torch.as_tensor(K).to(dev), torch.as_tensor(bbox3d).to(dev)
        frame = torch.from_numpy(np.random.default_rng(5).integers(0, 256, size=(480, 640), dtype=np.uint8)).to(dev)
        box0 = [80, 60, 560, 420]
        kw = dict(pnp_reprojection_error=a.reproj, trials=a.trials)

        def match(img):
            data = dict(obj)
            data["query_image"] = img
            with torch.no_grad():
                return model.enqueue(data)

        def run_host_box():
            lat, box, last = [], np.asarray(box0, dtype=np.int32), None
            for _ in range(a.frames):
                t0 = time.perf_counter()
                K_crop, _ = fl.crop_geometry(box, K, S)
                pend = match(fl.crop_query(frame, box, S))
                pend.finish()                                                   # SequenceRunner's model(data)
                out = pd.ransac_pnp(K, mk2d, mk3d, **kw)
                (pose, _, inl), = out.to_host()
                nb = fl.project_bbox(K, pose, bbox3d)
                box = nb if len(inl) >= fl.MIN_INLIERS and nb[2] > nb[0] and nb[3] > nb[1] else np.asarray(box0, dtype=np.int32)
                lat.append(1e3 * (time.perf_counter() - t0))
                last = (pose, box, K_crop)
            return lat, last

        pins = {}

        def run_device_box(lookahead):
            lat, queue, last = [], deque(), None
            state = td.set_box(box0, Kd, S)

            def retire():
                t0, pend, poses, pin, ev = queue.popleft()
                pend.finish()
                ev.synchronize()
                ((pose, _, inl),), (raw, flag) = poses.unpack(pin.numpy(), (td.STATE_BYTES, 4))
                lat.append(1e3 * (time.perf_counter() - t0))
                pins.setdefault(pin.numel(), []).append(pin)
                return pose, td.TrackState.unpack(raw), int(flag.view(np.int32)[0])
            for _ in range(a.frames):
                if len(queue) == lookahead:
                    last = retire()
                t0 = time.perf_counter()
                pend = match(td.crop(frame, state, S))
                poses = pd.ransac_pnp(Kd, mk2d, mk3d, **kw)
                nxt = td.next_box(poses, state, Kd, cube, min_inliers=fl.MIN_INLIERS, crop_size=S)
                packed = poses.pack(extra=(state.blob, nxt.flag.view(torch.uint8)))
                pool = pins.setdefault(packed.numel(), [])
                pin = pool.pop() if pool else torch.empty(packed.numel(), dtype=torch.uint8).pin_memory()
                pin.copy_(packed, non_blocking=True)
                ev = torch.cuda.Event()
                ev.record()
                queue.append((t0, pend, poses, pin, ev))
                state = nxt
            while queue:
                last = retire()
            return lat, last

        paths = [("host_box", run_host_box)] + [(f"device_box_la{L}", (lambda L=L: run_device_box(L))) for L in (1, 2, 3)]
        res = {name: {"fps": [], "lat": [], "gpu": []} for name, _ in paths}
        final = {}
        for rep in range(a.warmup + a.reps):
            for name, fn in paths:
                torch.cuda.synchronize()
                e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                e0.record()
                t0 = time.perf_counter()
                lat, final[name] = fn()
                wall = time.perf_counter() - t0
                e1.record()
                e1.synchronize()
                if rep >= a.warmup:
                    res[name]["fps"].append(a.frames / wall)
                    res[name]["lat"] += lat
                    res[name]["gpu"].append(e0.elapsed_time(e1) / a.frames)
        out = {"workload": wl, "points": n, "crop": S, "planted_matches": int(mk2d.shape[0]), "trials": a.trials, "frames": a.frames, "reps": a.reps,
               "rewind": False, "device": torch.cuda.get_device_name(0)}
        for name, _ in paths:
            r = res[name]
            out[name] = {"fps": stats(r["fps"]), "latency_ms": stats(r["lat"]), "gpu_ms_per_frame": stats(r["gpu"])}
        # the two box steps agree: the box the last frame was cropped with on the device (every frame has the same pose here) against the host loop's
        pose, (box, _, K_crop, _), flag = final["device_box_la2"]
        out["agree"] = {"next_flag": flag, "device_box": box.tolist(), "host_box_of_that_pose": final["host_box"][1].tolist(),
                        "same_pose": bool(np.array_equal(pose, final["host_box"][0]))}
        print(json.dumps(out), flush=True)


if __name__ == "__main__":
    main()
