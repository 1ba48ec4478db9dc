"""Time the SfM track assignment on the device against the numpy oracle.

    python tools/time_sfm_tracks.py [--case realistic|large] [--iters 20] [--warmup 3] [--loop-form]

``realistic``: 60 000 points, 150 images, mean track length 20 (1.2 M track elements; the case of tests/test_gpu_sfm_tracks.py);
``large``: 200 000 points, 300 images, mean track length 20.  One JSON line:
  * ``assign_tracks_ms``, ``matching_pairs_ms``, ``optimisation_rows_ms``: HIP events around one call each, inputs on the device, input
    checks and read-backs included: median, minimum and maximum of ``--iters`` calls after ``--warmup``;
  * ``rounds_ms``: HIP events around the enqueued rounds alone (``opsft_assign``: the launches of all I rounds, the idle ones included);
  * ``keyframes`` (= rounds that did work), ``rounds_enqueued``, ``launches`` per stage (HIP kernels of this library; the torch sorts and
    scans between them are not counted);
  * ``vectorised_oracle_s``: one run of ``tests/sfm_tracks_oracle.vectorised_form`` (numpy, single-threaded);
  * ``loop_form_s`` (``--loop-form``): the reference's own loop form, ``reference_form``.  Both are references here, not the code
    under test.
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

from onepose_st_amd import sfm_tracks as st  # noqa: E402
from tests import sfm_tracks_oracle as orc  # noqa: E402

CASES = {"realistic": dict(seed=21, Q=60000, I=150, mean_track=20, n_dup=500, shuffle_ids=True),
         "large": dict(seed=22, Q=200000, I=300, mean_track=20, n_dup=2000, shuffle_ids=True)}


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
    ap.add_argument("--case", default="realistic", choices=sorted(CASES))
    ap.add_argument("--iters", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--loop-form", action="store_true")
    a = ap.parse_args()
    torch.set_num_threads(1)
    m = orc.make_model(**CASES[a.case])
    model = {k: torch.from_numpy(np.ascontiguousarray(v)).cuda() for k, v in m.items()}
    I = len(m["image_ids"])
    out = {"case": a.case, "points": len(m["point_ids"]), "images": I, "slots": len(m["point3D_ids"]), "elements": len(m["track_image"])}
    plan, out["assign_tracks_ms"] = timed(lambda: st.assign_tracks(model), a.iters, a.warmup)

    def fresh_pairs():
        plan.pop("_rows", None)                                            # the element pass is part of the first stage that needs it
        return st.matching_pairs(plan, model)

    pairs, out["matching_pairs_ms"] = timed(fresh_pairs, a.iters, a.warmup)
    rows, out["optimisation_rows_ms"] = timed(lambda: st.optimisation_rows(plan, model, pairs), a.iters, a.warmup)

    # the rounds alone: the same launch as assign_tracks makes, on tables prepared once
    d = plan["_tables"]
    Pt, i32, i64 = st.hip.ptr, torch.int32, torch.int64
    reg = d["slot_point"] >= 0
    count0 = torch.zeros(I, dtype=i64, device="cuda").index_add_(0, d["slot_image"], reg.to(i64)).to(i32)

    def rounds():
        state = torch.where(reg, -2, -1).to(i32)
        bufs = [state, count0.clone(), torch.arange(I, dtype=i32, device="cuda"), torch.full((d["Q"],), -1, dtype=i32, device="cuda"),
                torch.full((d["Q"],), -1, dtype=i32, device="cuda"), torch.full((I,), -1, dtype=i32, device="cuda"),
                torch.tensor([0, I, 0, -1], dtype=i32, device="cuda")]
        torch.cuda.synchronize()
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        st.call("opsft_assign", Pt(model["kpt_offsets"], i64), Pt(d["slot_point"], i64), Pt(model["track_offsets"], i64), Pt(model["track_image"], i64),
                Pt(d["elem_slot"], i64), I, d["U"], d["Q"], d["E"], d["max_slots"], *(Pt(b, i32) for b in bufs), st.hip.stream_handle())
        e1.record()
        e1.synchronize()
        return e0.elapsed_time(e1)

    ts = [rounds() for _ in range(a.warmup + a.iters)][a.warmup:]
    out["rounds_ms"] = {"median": round(statistics.median(ts), 3), "min": round(min(ts), 3), "max": round(max(ts), 3)}
    out.update(keyframes=int(plan["keyframes"].numel()), rounds_enqueued=I, pairs=int(pairs["pair_left"].numel()),
               pair_rows=int(pairs["mkpts0_idx"].numel()), optimiser_rows=int(rows["fine_row"].numel()),
               launches={"assign_tracks": 2 * I + 2, "matching_pairs": 3, "optimisation_rows": 1})
    t0 = time.perf_counter()
    orc.vectorised_form(m)
    out["vectorised_oracle_s"] = round(time.perf_counter() - t0, 3)
    if a.loop_form:
        t0 = time.perf_counter()
        orc.reference_form(m)
        out["loop_form_s"] = round(time.perf_counter() - t0, 3)
    print(json.dumps(out))


if __name__ == "__main__":
    main()
