"""Time the coarse context of the fine windows (``fine_concat_coarse_feat``; csrc/fine_context.hip) on the device.

    python tools/time_fine_context.py [--rounds 15] [--calls 40] [--warmup 3] [--K 3000]

Two forms of the same step on the same seeded inputs, both images, ``K`` matches, windows 5 and 9, alternated in ONE process (round by round:
fused, composed, fused, ...), HIP-event time of ``--calls`` back-to-back calls per round, the median round per form:

  * fused     ``fine_context.merge`` into outputs allocated once (the matcher runs it in place: the same kernels): one entry
              (``opfcx_merge``), two launches, one scratch allocation of ``2 K 128`` floats per call;
  * composed  the factored form from what the project had: per image the coarse rows gathered in torch, ``ophip_rows_linear_x3`` for
              ``down_proj`` (+ bias), for the context half of ``merge_feat`` (+ bias) and for the window half over all ``K W^2`` rows, then
              the per-match context repeated over the rows in torch and added: 6 ``rows_linear`` launches (two of them over the window
              rows) and the torch gather, repeat and add kernels.

Prints one JSON line per window with both medians (microseconds per call), their ratio, the spread of each form's rounds, and the largest
difference between the two results (in units of ``max(1, |row|)``: they compute the same split-bf16 products).
"""
from __future__ import annotations

import argparse
import json
import os
import sys

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

from onepose_st_amd import fine_context, hip, packing  # noqa: E402
from onepose_st_amd.rows import rows_linear  # noqa: E402
from onepose_st_amd.synthetic import make_synthetic_loftr_state_dict  # noqa: E402


def window_us(fn, calls):
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    for _ in range(calls):
        fn()
    b.record()
    b.synchronize()
    return a.elapsed_time(b) * 1e3 / calls


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rounds", type=int, default=15)
    ap.add_argument("--calls", type=int, default=40)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--K", type=int, default=3000)
    ap.add_argument("--L", type=int, default=4800, help="coarse cells per image")
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("time_fine_context.py measures on the device: no GPU found")
    dev = torch.device("cuda:0")
    hip.load()
    fine_context.load()
    sd = make_synthetic_loftr_state_dict(0, fine_concat_coarse_feat=True)
    wpack = packing.pack_fine_context(sd).to(dev)
    wd, wm = sd["fine_preprocess.down_proj.weight"], sd["fine_preprocess.merge_feat.weight"]
    pd, pw, pc = (packing.pack_linear_x3(w).to(dev) for w in (wd, wm[:, :128], wm[:, 128:]))
    bd, bm = sd["fine_preprocess.down_proj.bias"].to(dev), sd["fine_preprocess.merge_feat.bias"].to(dev)
    g = torch.Generator().manual_seed(2)
    K, L = args.K, args.L
    x = [torch.randn(1, L, 256, generator=g).to(dev) for _ in range(2)]
    b_ids = torch.zeros(K, dtype=torch.int64, device=dev)
    ids = [torch.randint(0, L, (K,), generator=g).to(dev) for _ in range(2)]
    for W in (5, 9):
        WW = W * W
        src = [torch.randn(K, WW, 128, generator=g).to(dev) for _ in range(2)]
        outs = tuple(torch.empty_like(t) for t in src)

        def fused():
            return fine_context.merge(src[0], src[1], x[0], x[1], b_ids, ids[0], ids[1], W, wpack, out=outs)

        def composed():
            out = []
            for s in (0, 1):
                c = rows_linear(x[s][0][ids[s]], K, pd, 128) + bd
                u = rows_linear(c, K, pc, 128) + bm
                y = rows_linear(src[s], K * WW, pw, 128)
                out.append(y.view(K, WW, 128) + u[:, None, :])
            return out
        # the same result first
        a, b = fused(), composed()
        diff = max(float(((p - q).abs() / torch.clamp(q.abs().amax(-1, keepdim=True), min=1.0)).max()) for p, q in zip(a, b))
        times = {"fused": [], "composed": []}
        for r in range(args.warmup + args.rounds):
            for name, fn in (("fused", fused), ("composed", composed)):
                t = window_us(fn, args.calls)
                if r >= args.warmup:
                    times[name].append(t)
        med = {n: sorted(t)[len(t) // 2] for n, t in times.items()}
        print(json.dumps({"item": "fine_context", "K": K, "W": W, "rows_per_image": K * WW, "fused_us": round(med["fused"], 1),
                          "composed_us": round(med["composed"], 1), "fused_over_composed": round(med["fused"] / med["composed"], 3),
                          "fused_min_max_us": [round(min(times["fused"]), 1), round(max(times["fused"]), 1)],
                          "composed_min_max_us": [round(min(times["composed"]), 1), round(max(times["composed"]), 1)],
                          "rounds": args.rounds, "calls_per_round": args.calls, "max_row_difference": diff}))
    print(json.dumps({"device": hip.device_info()}))


if __name__ == "__main__":
    main()
