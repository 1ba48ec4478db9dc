"""Time the SfM triangulation on the device, and the numpy oracle on the CPU.

    python tools/time_sfm_triangulate.py [--iters 20] [--warmup 3] [--images 150] [--points 60000] [--track 20] [--oracle] [--no-device]

The scene (tests/sfm_triangulate_scenes.timing_scene): 150 images on a ring, 60 000 points each seen by 20 consecutive images (about
1.2 M observations), match rows between ring neighbours at distance 1 and 2.  One JSON line:
  * ``triangulate_ms``: HIP events around one ``sfm_triangulate.triangulate`` call, inputs on the device, input checks and read-backs
    included: median, minimum and maximum of ``--iters`` calls after ``--warmup``;
  * ``components_ms``: the union-find launches alone (``opstr_components``);
  * ``points``, ``elements``, ``rounds`` of the result, ``launches`` (HIP kernels of this library: 2 for the components, 2 for cameras and
    rays, 1 or 2 per round; the torch sorts and scans between them are not counted);
  * ``oracle_s`` (``--oracle``): one run of ``tests/sfm_triangulate_oracle.triangulate`` (numpy, single-threaded), the reference here, not
    the code under test.  ``--no-device`` skips everything that needs a GPU.
Per-kernel times come from a ``rocprofv3 --kernel-trace --stats`` run of this script with ``--iters 1``.
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

from tests import sfm_triangulate_oracle as orc  # noqa: E402
from tests import sfm_triangulate_scenes as scenes  # noqa: E402


def timed(fn, iters, warmup):
    for _ in range(warmup):
        res = fn()
    torch.cuda.synchronize()
    ts = []
    for _ in range(iters):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        res = fn()
        b.record()
        b.synchronize()
        ts.append(a.elapsed_time(b))
    return res, {"median": round(statistics.median(ts), 3), "min": round(min(ts), 3), "max": round(max(ts), 3)}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--iters", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--images", type=int, default=150)
    ap.add_argument("--points", type=int, default=60000)
    ap.add_argument("--track", type=int, default=20)
    ap.add_argument("--oracle", action="store_true")
    ap.add_argument("--no-device", action="store_true")
    a = ap.parse_args()
    torch.set_num_threads(1)
    s = scenes.timing_scene(a.images, a.points, a.track)
    mg = s["merged"]
    out = {"images": a.images, "planted_points": a.points, "observations": a.points * a.track, "slots": len(mg["keypoints"]),
           "match_rows": len(mg["match_ids"]), "pairs": len(mg["pair_images"])}
    if not a.no_device:
        from onepose_st_amd import sfm_triangulate as tri

        merged = {k: torch.from_numpy(np.ascontiguousarray(v)).cuda() for k, v in mg.items()}
        cams = {k: torch.from_numpy(np.ascontiguousarray(v)).cuda() for k, v in s["cameras"].items()}
        model, out["triangulate_ms"] = timed(lambda: tri.triangulate(merged, cams), a.iters, a.warmup)
        d = tri.check_inputs(merged, cams)
        _, out["components_ms"] = timed(lambda: tri.components(d["slot0"], d["slot1"], d["U"]), a.iters, a.warmup)
        out.update(points=int(model["point_ids"].numel()), elements=int(model["track_image"].numel()), rounds=model["n_rounds"],
                   launches={"components": 2, "prepare": 2, "per_round": "1 (+1 with components above %d candidates)" % tri.SHORT_TRACK})
    if a.oracle:
        t0 = time.perf_counter()
        m = orc.triangulate(mg, s["cameras"])
        out["oracle_s"] = round(time.perf_counter() - t0, 3)
        out["oracle_points"] = len(m["point_ids"])
        if not a.no_device:
            out["points_equal_oracle"] = bool(np.array_equal(m["point3D_ids"], model["point3D_ids"].cpu().numpy()))
    print(json.dumps(out))


if __name__ == "__main__":
    main()
