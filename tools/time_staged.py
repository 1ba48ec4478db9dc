"""Time the model's staged path: ``forward_features`` with ``hip_frame_call = False``, every stage its own C call from Python.

    python tools/time_staged.py [--windows 5] [--frames 200] [--warmup 30]

The host cost of the Python call sites shows here and not in ``bench.py``, whose frame call does not pass through Python per layer.  Synthetic
frames of ``onepose_st_amd/synthetic.py`` at the sizes of ``tests/test_gpu_model_scratch.py`` (128 x 160 image, 900 points, 350 planted):
``--warmup`` untimed frames, then ``--windows`` windows of ``--frames`` frames on the host clock, each ending in one synchronise.  One JSON
line: the windows' frames / s with their median, min and max, the matches of a frame and the library's build stamp.
"""
from __future__ import annotations

import argparse
import json
import os
import statistics
import sys
import time

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

from onepose_st_amd import hip  # noqa: E402
from onepose_st_amd.config import default_config  # noqa: E402
from onepose_st_amd.model import OnePosePlus_model  # noqa: E402
from onepose_st_amd.synthetic import make_synthetic_inputs, make_synthetic_state_dict  # noqa: E402


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--windows", type=int, default=5)
    ap.add_argument("--frames", type=int, default=200)
    ap.add_argument("--warmup", type=int, default=30)
    args = ap.parse_args()
    dev = torch.device("cuda:0")
    cfg = default_config()
    cfg["hip_frame_call"] = False
    sd = make_synthetic_state_dict(seed=0, config=cfg)
    model = OnePosePlus_model(cfg).eval()
    model.load_state_dict(sd, strict=True)
    model.to(dev)
    assert not model.frame_call
    f = make_synthetic_inputs(sd, n_points=900, image_hw=(128, 160), n_plant=350, seed=47, config=cfg, frame=0)
    obj = {k: f[k].to(dev) for k in ("keypoints3d", "descriptors3d_db", "descriptors3d_coarse_db")}
    fc, ff = f["feat_c"].to(dev), f["feat_f"].to(dev)

    def frame():
        d = dict(obj)
        model.forward_features(d, fc, ff, f["image_hw"])
        return d
    for _ in range(args.warmup):
        d = frame()
    torch.cuda.synchronize()
    fps = []
    for _ in range(args.windows):
        t0 = time.perf_counter()
        for _ in range(args.frames):
            frame()
        torch.cuda.synchronize()
        fps.append(args.frames / (time.perf_counter() - t0))
    print(json.dumps({"item": "staged_path", "frames_per_s": [round(v, 1) for v in fps], "median": round(statistics.median(fps), 1),
                      "min": round(min(fps), 1), "max": round(max(fps), 1), "matches": int(d["i_ids"].shape[0]), "build_stamp": hip.build_stamp()}))


if __name__ == "__main__":
    main()
