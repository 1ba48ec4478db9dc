"""Time the SfM calls of the LoFTR matcher on the device (synthetic LoFTR weights, random 512 x 512 images).

    python tools/time_sfm_match.py [--iters 20] [--warmup 5]

Prints one JSON line per item, HIP-event times (median of ``--iters`` after ``--warmup``):
  * ``coarse``: one SfM coarse call (``enable_fine_matching=False``, scale0 / scale1 given);
  * ``fine_only_K``: one fine-only call with both extraction kwargs at K = 500 / 2000 / 5000 provided matches, plus the device time
    of the two new kernels inside it (``ophip_timing_select``: each launch's own begin and end) and their share of the call;
  * ``kernels_K``: ``ophip_loftr_coarse_ids`` (both images) and ``ophip_sample_features`` (four jobs) launched on their own.
"""
from __future__ import annotations

import argparse
import json
import os
import statistics
import sys

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

from onepose_st_amd import hip, loftr  # noqa: E402
from onepose_st_amd.synthetic import make_synthetic_loftr_state_dict  # noqa: E402


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
    return statistics.median(ts)


def kernel_us(name, fn, iters):
    """mean device time per call of the kernel ``name`` inside ``fn``"""
    torch.cuda.synchronize()
    hip.timing_select(name)
    for _ in range(iters):
        fn()
    torch.cuda.synchronize()
    n, ms = hip.timing_read()
    hip.timing_select("")
    return ms * 1e3 / iters if n else float("nan")


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--iters", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=5)
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("time_sfm_match.py needs the HIP device")
    dev = torch.device("cuda:0")
    hip.load()
    g = torch.Generator().manual_seed(0)
    H = W = 512
    img0, img1 = torch.rand(1, 1, H, W, generator=g).to(dev), torch.rand(1, 1, H, W, generator=g).to(dev)
    s0, s1 = torch.tensor([[1.25, 0.8]], device=dev), torch.tensor([[1.1, 0.9]], device=dev)
    sd = make_synthetic_loftr_state_dict(0)
    coarse = loftr.LoFTR_for_OnePose_Plus(enable_fine_matching=False).eval()
    coarse.load_state_dict(sd, strict=True)
    coarse.to(dev)
    full = loftr.LoFTR_for_OnePose_Plus().eval()
    full.load_state_dict(sd, strict=True)
    full.to(dev)

    def coarse_call():
        coarse({"image0": img0, "image1": img1, "scale0": s0, "scale1": s1})
    print(json.dumps({"item": "coarse", "hw": [H, W], "call_us": round(timed(coarse_call, args.iters, args.warmup), 1)}), flush=True)

    for K in (500, 2000, 5000):
        kx = torch.rand(K, 2, generator=g, dtype=torch.float64)
        k0 = (kx * torch.tensor([W - 1.0, H - 40.0], dtype=torch.float64)).to(dev)
        k1 = (kx.flip(0) * torch.tensor([W - 1.0, H - 40.0], dtype=torch.float64)).float().to(dev)

        def fine_only():
            full({"image0": img0, "image1": img1, "scale0": s0, "scale1": s1, "mkpts0_c": k0.clone(), "mkpts1_c": k1.clone()},
                 extract_coarse_feature=True, extract_fine_feature=True)
        t_call = timed(fine_only, args.iters, args.warmup)
        t_ids = kernel_us("sfm_coarse_ids", fine_only, args.iters)
        t_smp = kernel_us("sfm_sample", fine_only, args.iters)
        print(json.dumps({"item": f"fine_only_{K}", "K": K, "call_us": round(t_call, 1), "ids_us": round(t_ids, 2), "sample_us": round(t_smp, 2),
                          "new_kernels_share": round((t_ids + t_smp) / t_call, 4)}), flush=True)

        # the two kernels on their own (HIP events around one launch each: launch-bound numbers)
        hc, wc, hf, wf = H // 8, W // 8, H // 2, W // 2
        ii, jj = torch.empty(K, dtype=torch.int64, device=dev), torch.empty(K, dtype=torch.int64, device=dev)
        bad = torch.empty(1, dtype=torch.int32, device=dev)
        a0, a1 = k0.clone(), k1.clone()

        def ids():
            hip.call("ophip_loftr_coarse_ids", hip.ptr(a0, None), 1, hip.ptr(a1, None), 0, K, H, W, H, W, hc, wc, hc, wc, 8.0, hip.ptr(s0),
                     hip.ptr(s1), hip.ptr(ii, torch.int64), hip.ptr(jj, torch.int64), hip.ptr(bad, torch.int32), hip.stream_handle())
        mc, mf = torch.randn(hc * wc, 256, device=dev), torch.randn(hf * wf, 128, device=dev)
        outs = [torch.empty(K, c, device=dev) for c in (256, 256, 128, 128)]
        jobs = [hip.SampleJob(m.data_ptr(), kp.data_ptr(), s.data_ptr(), o.data_ptr(), h, w, c, K, H, W, int(kp.dtype == torch.float64), nn)
                for (m, h, w, c, nn), kp, s, o in zip(((mc, hc, wc, 256, 1), (mc, hc, wc, 256, 1), (mf, hf, wf, 128, 0), (mf, hf, wf, 128, 0)),
                                                      (a0, a1, a0, a1), (s0, s1, s0, s1), outs)]
        arr = (hip.SampleJob * 4)(*jobs)

        def sample():
            hip.call("ophip_sample_features", arr, 4, hip.stream_handle())
        print(json.dumps({"item": f"kernels_{K}", "K": K, "ids_event_us": round(timed(ids, args.iters, args.warmup), 2),
                          "ids_kernel_us": round(kernel_us("sfm_coarse_ids", ids, args.iters), 2),
                          "sample_event_us": round(timed(sample, args.iters, args.warmup), 2),
                          "sample_kernel_us": round(kernel_us("sfm_sample", sample, args.iters), 2),
                          "sample_bytes": K * 2 * (256 + 4 * 128 + 256 + 128) * 4}), flush=True)


if __name__ == "__main__":
    main()
