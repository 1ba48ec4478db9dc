"""Time the LoFTR coarse-matching stage on the device, dual softmax (``ophip_coarse_match_2d``) against optimal transport
(``ophip_coarse_match_2d_sinkhorn``, csrc/coarse_sinkhorn.hip) at the same shapes.

    python tools/time_sinkhorn.py [--iters 20] [--warmup 5] [--skh-iters 3]

Prints one JSON line per shape, HIP-event times of the whole stage (median of ``--iters`` after ``--warmup``):
  * 4096 x 4096: one 512 x 512 view against one 512 x 512 frame;
  * 15 x (4096 x 4096): the batched detector, 15 views against one query;
  * 4096 x 43200: a 512 x 512 view against a 1920 x 1440 frame.
Per kernel (``ophip_timing_select``: each launch's own begin and end, summed per call): ``sweep_us`` is the log-sum-exp sweeps
(``skh_rows`` + ``skh_cols`` + ``skh_colcomb``; the first row update comes from the similarity tiles, so ``2 skh_iters - 1`` passes over
the B x L0 x L1 f32 matrix) and ``final_us`` the prefilter read plus the confidence read and write (``skh_final``, 3 passes);
``*_tbps`` are those bytes over those times.
"""
from __future__ import annotations

import argparse
import ctypes
import json
import os
import sys

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

from onepose_st_amd import hip, matchcall  # noqa: E402


def timed(fn, iters, warmup):
    for _ in range(warmup):
        fn()
    torch.cuda.synchronize()
    ts = []
    for _ in range(iters):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        fn()
        b.record()
        b.synchronize()
        ts.append(a.elapsed_time(b) * 1e3)
    ts.sort()
    return ts[len(ts) // 2]


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--iters", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--skh-iters", type=int, default=3)
    args = ap.parse_args()
    dev = torch.device("cuda:0")
    lib = hip.load()
    shapes = [("4096x4096", 1, (64, 64), (64, 64), False), ("15x4096x4096_shared_query", 15, (64, 64), (64, 64), True),
              ("4096x43200", 1, (64, 64), (180, 240), False)]
    for name, B, (h0, w0), (h1, w1), shared in shapes:
        L0, L1 = h0 * w0, h1 * w1
        g = torch.Generator(device=dev).manual_seed(0)
        f0 = torch.randn(B, L0, 256, device=dev, generator=g)
        f1 = torch.randn(1, L1, 256, device=dev, generator=g).expand(B, -1, -1).contiguous() if shared else torch.randn(B, L1, 256, device=dev, generator=g)
        ii = torch.arange(L0, device=dev)
        pts0 = torch.stack([(ii % w0).float() * 8, (ii // w0).float() * 8, torch.zeros(L0, device=dev)], 1)[None].contiguous()
        lists = matchcall.MatchLists.empty(B * L0, dev, conf_shape=(B, L0, L1))
        outs = dict(w0c=w0, w1c=w1, thr=0.2, border_rm=2, scale=8.0, lists=lists, conf=lists.conf)
        ws_d = torch.empty(lib.ophip_coarse_workspace_floats(B, L0, L1), device=dev)
        ws_s = torch.empty(lib.ophip_coarse_sinkhorn_workspace_floats(B, L0, L1), device=dev)

        def dual():
            matchcall.coarse_match_2d(f0, f1, pts0, temperature=0.1, workspace=ws_d, **outs)

        def skh(iters, prefilter):
            return lambda: matchcall.coarse_match_2d(f0, f1, pts0, sinkhorn=(1.0, iters, prefilter), workspace=ws_s, **outs)
        t_dual = timed(dual, args.iters, args.warmup)
        run = skh(args.skh_iters, 1)
        t_skh = timed(run, args.iters, args.warmup)
        per = {}
        for k in ("skh_rows", "skh_cols", "skh_colcomb", "skh_final"):
            lib.ophip_timing_select(k.encode())
            run()
            torch.cuda.synchronize()
            hip.call("ophip_timing_read", ctypes.byref(ctypes.c_int()), ctypes.byref(ctypes.c_double()))      # drop the first call
            for _ in range(args.iters):
                run()
            n, ms = ctypes.c_int(), ctypes.c_double()
            hip.call("ophip_timing_read", ctypes.byref(n), ctypes.byref(ms))
            per[k] = ms.value * 1e3 / args.iters
        lib.ophip_timing_select(b"")
        mat = B * L0 * L1 * 4
        sweep_passes = max(2 * args.skh_iters - 1, 0)
        t_sweep = per["skh_rows"] + per["skh_cols"] + per["skh_colcomb"]
        print(json.dumps({"shape": name, "B": B, "L0": L0, "L1": L1, "skh_iters": args.skh_iters, "dual_softmax_us": round(t_dual, 1),
                          "sinkhorn_us": round(t_skh, 1), "ratio": round(t_skh / t_dual, 2),
                          "kernels_us_per_call": {k: round(v, 1) for k, v in per.items()},
                          "sweep_us": round(t_sweep, 1), "sweep_passes": sweep_passes, "sweep_bytes": sweep_passes * mat,
                          "sweep_tbps": round(sweep_passes * mat / (t_sweep * 1e-6) / 1e12, 2),
                          "final_us": round(per["skh_final"], 1), "final_bytes": 3 * mat,
                          "final_tbps": round(3 * mat / (per["skh_final"] * 1e-6) / 1e12, 2)}), flush=True)
        del lists, outs, ws_d, ws_s, f0, f1
        torch.cuda.empty_cache()


if __name__ == "__main__":
    main()
