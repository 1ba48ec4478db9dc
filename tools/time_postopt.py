"""Time the SfM depth refinement on the device against the reference's form of it.

    python tools/time_postopt.py [--tracks 5000,20000,100000] [--mean-len 20] [--ref-steps 20] [--iters 3] [--solver first|lm]

For each track count P (synthetic tracks of mean length ``--mean-len``, plus three single-row tracks and one of 1 200 rows), prints one
JSON line:
  * ``refine_ms``: HIP-event time of one ``postopt.refine_depths`` call (prep, every step, the read-back; median of ``--iters``) and
    ``per_step_us`` = refine_ms / steps run;
  * ``step_kernel_us``: the device time of one ``postopt_step`` launch (``ophip_timing_select``: each launch's own begin and end),
    averaged over a run of exactly the steps that do work, and ``step_GBps`` = the bytes one step must move (64 per row, 64 per
    track) over that time;
  * ``ref_step_us``: one step of the oracle's autograd + ``torch.optim.Adam`` loop moved to the same GPU (the reference's form,
    ``first_order_solver.py``), averaged over ``--ref-steps`` steps, and ``ref_total_ms`` = that times the steps run.

``--solver lm`` times the second-order solver beside the first-order one in the same run and prints, instead of the reference's form:
  * ``refine_ms`` / ``steps`` as above, ``lm_refine_ms``: one ``postopt.refine_depths_lm`` call (validation, the solve, the read-back;
    median of ``--iters``) and ``lm_iterations`` (largest) / ``lm_rejects`` (sum) / ``lm_not_converged``;
  * ``lm_launch_us``: the library call alone, i.e. the solve kernel and the one-workgroup totals kernel between two HIP events with no
    read-back (median of ``--iters``; the depths are reset outside the timed region), and ``lm_GBps`` = the bytes the solve must move
    (192 per row read, 100 per track) over that time -- a lower bound of the kernel's rate, since the time holds both launches;
  * ``cost_first`` / ``cost_lm``: the total cost at each solver's depths (both by the second-order solver's own first evaluation), and
    ``depth_err_first`` / ``depth_err_lm``: the median relative error against the synthetic scene's true depths.
"""
from __future__ import annotations

import argparse
import json
import os
import statistics
import sys

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

from onepose_st_amd import hip, postopt  # noqa: E402
from onepose_st_amd.synthetic import make_synthetic_sfm_tracks  # noqa: E402
from tests import postopt_oracle as po  # noqa: E402

ROW_KEYS = ("depth", "n_query", "intrinsic0", "intrinsic1", "mkpts0_c", "mkpts1_f", "left_pose_idx", "right_pose_idx",
            "angle_axis_to_world")


def event_ms(fn):
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    torch.cuda.synchronize()
    a.record()
    out = fn()
    b.record()
    b.synchronize()
    return a.elapsed_time(b), out


def time_lm(d, data, depth_first, iters):
    """the ``--solver lm`` columns for the problem ``d`` (device tensors); ``depth_first``: the first-order solver's depths"""
    import ctypes

    from onepose_st_amd import postopt_lm

    def call(**kw):
        return postopt.refine_depths_lm(*(d[k] for k in ROW_KEYS), **kw)

    out = call()                                                        # warm-up
    ms = statistics.median(event_ms(call)[0] for _ in range(iters))
    # the library call alone, on the tensors refine_depths_lm would build
    dd, offs, K0, K1, mk0, mk1, li, ri, aa, P, L, F = postopt._flat_problem(*(d[k] for k in ROW_KEYS))
    start = dd.clone()
    ints = torch.empty(3, P, dtype=torch.int32, device=dd.device)
    reals = torch.empty(5, P, dtype=torch.float64, device=dd.device)
    ws_bytes = postopt_lm.load().oplm_workspace_bytes(L, P)
    ws = torch.empty(ws_bytes, dtype=torch.uint8, device=dd.device)
    p, f64, c = hip.ptr, torch.float64, postopt.LM_DEFAULTS

    def launch():
        postopt_lm.call("oplm_refine", p(dd, f64), p(offs, torch.int64), P, L, p(K0, f64), p(K1, f64), p(mk0, f64), p(mk1, f64),
                        p(li, torch.int64), p(ri, torch.int64), p(aa, f64), F, c["lam0"], c["up"], c["down"], c["lam_min"], c["lam_max"],
                        c["step_tol"], 50, p(ints[0], torch.int32), p(ints[1], torch.int32), p(ints[2], torch.int32), p(reals[0], f64),
                        p(reals[1], f64), p(reals[2], f64), p(reals[3, 0:1], f64), p(reals[4, 0:1], f64), None, p(ws, None),
                        ctypes.c_size_t(ws_bytes), hip.stream_handle())

    times = []
    for _ in range(iters + 1):
        dd.copy_(start)
        times.append(event_ms(launch)[0])
    us = statistics.median(times[1:]) * 1e3
    assert torch.equal(dd, out["depth"].reshape(-1))
    nbytes = 192 * L + 100 * P
    true = data["depth_true"].to(dd.device)
    err = lambda x: float(((x.reshape(-1, 1) - true).abs() / true).median())      # noqa: E731
    return {"lm_refine_ms": round(ms, 3), "lm_iterations": out["steps"], "lm_rejects": int(out["rejects"].sum()),
            "lm_not_converged": int((out["status"] != postopt_lm.CONVERGED).sum()), "lm_launch_us": round(us, 1), "lm_bytes": nbytes,
            "lm_GBps": round(nbytes / (us * 1e-6) / 1e9, 1), "cost_first": postopt.refine_depths_lm(*(d[k] if k != "depth" else depth_first for k in ROW_KEYS), max_iters=0)["initial_residual"],
            "cost_lm": out["final_residual"], "depth_err_first": err(depth_first), "depth_err_lm": err(out["depth"])}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--tracks", default="5000,20000,100000")
    ap.add_argument("--mean-len", type=int, default=20)
    ap.add_argument("--ref-steps", type=int, default=20)
    ap.add_argument("--iters", type=int, default=3)
    ap.add_argument("--solver", choices=("first", "lm"), default="first")
    args = ap.parse_args()
    hip.load()
    dev = torch.device("cuda:0")
    for P in (int(x) for x in args.tracks.split(",")):
        data = make_synthetic_sfm_tracks(0, n_frames=40, n_tracks=P, mean_len=args.mean_len)
        d = {k: data[k].to(dev) for k in ROW_KEYS}
        L = int(data["n_query"].sum())

        def call(max_steps=postopt.MAX_STEPS):
            return postopt.refine_depths(*(d[k] for k in ROW_KEYS), max_steps=max_steps)

        call()                                                          # warm-up
        runs = [event_ms(call) for _ in range(args.iters)]
        ms = statistics.median(r[0] for r in runs)
        steps = runs[0][1]["steps"]
        if args.solver == "lm":
            print(json.dumps({"P": P, "L": L, "mean_len": round(L / P, 2), "steps": steps, "refine_ms": round(ms, 3),
                              **time_lm(d, data, runs[0][1]["depth"], args.iters)}), flush=True)
            continue
        hip.timing_select("postopt_step")
        call(steps)                                                     # every launch does work
        n, kms = hip.timing_read()
        hip.timing_select("")
        step_us = kms * 1e3 / max(n, 1)
        step_bytes = 64 * L + 64 * P
        # the reference's form on the same GPU: autograd through the residual + torch.optim.Adam, one loss read per step
        ref = {k: (v.to(dev) if torch.is_tensor(v) else v) for k, v in data.items()}
        po.solve_literal(ref, max_steps=2)
        rms, _ = event_ms(lambda: po.solve_literal(ref, max_steps=args.ref_steps))
        ref_step_us = rms * 1e3 / args.ref_steps
        print(json.dumps({"P": P, "L": L, "mean_len": round(L / P, 2), "steps": steps, "refine_ms": round(ms, 3),
                          "per_step_us": round(ms * 1e3 / steps, 2), "step_kernel_us": round(step_us, 2), "step_launches": n,
                          "step_bytes": step_bytes, "step_GBps": round(step_bytes / (step_us * 1e-6) / 1e9, 1),
                          "ref_step_us": round(ref_step_us, 1), "ref_total_ms": round(ref_step_us * steps / 1e3, 1),
                          "speedup_per_step": round(ref_step_us / (ms * 1e3 / steps), 1)}), flush=True)


if __name__ == "__main__":
    main()
