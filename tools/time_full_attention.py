"""Time full (softmax) attention on the device (``attention = "full"``: csrc/encoder_full.hip, csrc/fine_full.hip).

    python tools/time_full_attention.py [--iters 20] [--warmup 5]

Prints one JSON line per item, HIP-event times (median of ``--iters`` after ``--warmup``):
  * the flash-attention kernel alone (``ophip_full_attention_h8d32``) at the four c2 shapes -- 3D self 7000 x 7000, 2D self 4800 x 4800,
    the crosses 7000 x 4800 and 4800 x 7000 -- with its algorithmic rate 4 L S 256 flop (QK^T + PV; the split's three products per
    product are NOT counted), and beside it the reference's composition in torch f32 on the same device
    (``einsum`` -> ``softmax`` -> ``einsum``, linear_attention.py:82-93);
  * one whole layer (``ophip_encoder_layer_full_x3``, both streams, self and cross) at c2;
  * ``forward_features`` of a c2 frame with both encoders full, with the coarse one alone full, and with the default linear ones;
  * the detector's LoFTR shapes (``--items detector`` for these alone): the one-stream layer (``ophip_encoder_layer_full_x3_stream``) on a
    512 x 512 view's 4096 coarse tokens (self), 4096 against a 1920 x 1440 frame's 43 200 (cross), the frame's own self layer (the one the
    shared-query path runs once instead of once per view), and the window attention (``ophip_fine2_full_attention``) over 1000 matches at
    W = 9 and 11 beside the linear one (``ophip_fine2_attention``).
"""
from __future__ import annotations

import argparse
import copy
import json
import os
import sys

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

from onepose_st_amd import hip, layercall, packing  # noqa: E402
from onepose_st_amd.config import default_config  # noqa: E402
from onepose_st_amd.model import OnePosePlus_model  # noqa: E402
from onepose_st_amd.synthetic import make_synthetic_inputs, make_synthetic_loftr_state_dict, make_synthetic_state_dict  # noqa: E402


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


def torch_full_attention(q, k, v):
    B, L, S = q.shape[0], q.shape[1], k.shape[1]
    qh, kh, vh = q.view(B, L, 8, 32), k.view(B, S, 8, 32), v.view(B, S, 8, 32)
    QK = torch.einsum("nlhd,nshd->nlsh", qh, kh)
    A = torch.softmax(QK / 32 ** 0.5, dim=2)
    return torch.einsum("nlsh,nshd->nlhd", A, vh).reshape(B, L, 256)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--iters", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--items", choices=("all", "c2", "detector"), default="all")
    args = ap.parse_args()
    dev = torch.device("cuda:0")
    hip.load()
    if args.items in ("all", "c2"):
        c2_items(args, dev)
    if args.items in ("all", "detector"):
        detector_items(args, dev)
    print(json.dumps({"device": hip.device_info(), "build_stamp": hip.load().ophip_build_stamp().decode()}))


def detector_items(args, dev):
    S = hip.stream_handle
    g = torch.Generator().manual_seed(1)
    sd = make_synthetic_loftr_state_dict(0)
    w = packing.pack_coarse_layer(sd, "loftr_coarse.layers.1.").to(dev)
    for name, L, Sk in (("view_self", 4096, 4096), ("view_vs_frame_cross", 4096, 43200), ("frame_self", 43200, 43200)):
        x = torch.randn(1, L, 256, generator=g).to(dev)
        src = x if name.endswith("self") else torch.randn(1, Sk, 256, generator=g).to(dev)
        y = torch.empty_like(x)
        ws = layercall.workspace("full", 1, L, Sk, dev, stream_form=True)
        us = timed(lambda: layercall.layer_full_stream(x, src, y, wpack=w, workspace=ws), args.iters, args.warmup)
        print(json.dumps({"item": "loftr_layer_full_stream", "shape": name, "L": L, "S": Sk, "us": round(us, 1),
                          "attention_tflops_algorithmic_whole_layer": round(4.0 * L * Sk * 256 / us * 1e-6, 1)}))
        del x, src, y, ws
        torch.cuda.empty_cache()
    K = 1000
    for W in (9, 11):
        WW = W * W
        q, k, v = (torch.randn(K, WW, 128, generator=g).to(dev) for _ in range(3))
        msg = torch.empty_like(q)
        row = {"item": "loftr_fine_window_attention", "K": K, "W": W}
        for kname in ("ophip_fine2_full_attention", "ophip_fine2_attention"):
            row[kname.replace("ophip_fine2_", "") + "_us"] = round(timed(
                lambda: hip.call(kname, hip.ptr(q), hip.ptr(k), hip.ptr(v), K, WW, WW, hip.ptr(msg), S()), args.iters, args.warmup), 1)
        row["full_gflops_algorithmic"] = round(4.0 * K * WW * WW * 128 / row["full_attention_us"] * 1e-3, 1)
        print(json.dumps(row))


def c2_items(args, dev):
    S = hip.stream_handle
    g = torch.Generator().manual_seed(0)
    shapes = [("3d_self", 7000, 7000), ("2d_self", 4800, 4800), ("3d_cross", 7000, 4800), ("2d_cross", 4800, 7000)]
    tot_us = tot_torch = 0.0
    for name, L, Sk in shapes:
        q = torch.randn(1, L, 256, generator=g).to(dev)
        k, v = torch.randn(1, Sk, 256, generator=g).to(dev), torch.randn(1, Sk, 256, generator=g).to(dev)
        out = torch.empty(1, L, 256, device=dev)
        us = timed(lambda: hip.call("ophip_full_attention_h8d32", hip.ptr(q), hip.ptr(k), hip.ptr(v), 1, L, Sk, hip.ptr(out), S()),
                   args.iters, args.warmup)
        ref = torch_full_attention(q, k, v)
        err = (ref - out).abs().max().item()
        ut = timed(lambda: torch_full_attention(q, k, v), max(3, args.iters // 4), 2)
        flop = 4.0 * L * Sk * 256
        tot_us, tot_torch = tot_us + us, tot_torch + ut
        print(json.dumps({"item": "flash_attention", "shape": name, "L": L, "S": Sk, "us": round(us, 1),
                          "tflops_algorithmic": round(flop / us * 1e-6, 1), "torch_f32_us": round(ut, 1),
                          "torch_f32_tflops": round(flop / ut * 1e-6, 1), "speedup_vs_torch": round(ut / us, 2),
                          "max_abs_diff_vs_torch": err}))
        del q, k, v, out, ref
        torch.cuda.empty_cache()
    print(json.dumps({"item": "flash_attention_c2_layer_pair", "us": round(tot_us, 1), "torch_f32_us": round(tot_torch, 1)}))

    cfg = default_config()
    sd = make_synthetic_state_dict(0, cfg)
    x3, x2 = torch.randn(1, 7000, 256, generator=g).to(dev), torch.randn(1, 4800, 256, generator=g).to(dev)
    y3, y2 = torch.empty_like(x3), torch.empty_like(x2)
    w = packing.pack_coarse_layer(sd, "loftr_coarse.layers.0.").to(dev)
    ws = layercall.workspace("full", 1, 7000, 4800, dev)
    for cross in (0, 1):
        us = timed(lambda: layercall.layer(x3, x2, y3, y2, mode="full", wpack=w, is_cross=cross, workspace=ws), args.iters, args.warmup)
        attn = 4.0 * 256 * ((7000 * 4800 * 2) if cross else (7000 * 7000 + 4800 * 4800))
        print(json.dumps({"item": "layer_full_x3", "cross": cross, "us": round(us, 1), "attention_tflops_algorithmic_whole_layer": round(attn / us * 1e-6, 1)}))
    del x3, x2, y3, y2, ws

    inp = make_synthetic_inputs(sd, n_points=7000, image_hw=(480, 640), n_plant=3000, seed=1, config=cfg)
    d = {k: (v.to(dev) if torch.is_tensor(v) else v) for k, v in inp.items()}
    for coarse, fine in (("full", "full"), ("full", "linear"), ("linear", "linear")):
        c = copy.deepcopy(cfg)
        c["loftr_coarse"]["attention"], c["loftr_fine"]["attention"] = coarse, fine
        m = OnePosePlus_model(c).eval()
        m.load_state_dict(sd, strict=True)
        m.to(dev)

        def run():
            data = {k: d[k] for k in ("keypoints3d", "descriptors3d_db", "descriptors3d_coarse_db")}
            m.forward_features(data, d["feat_c"], d["feat_f"], inp["image_hw"])
        us = timed(run, max(3, args.iters // 2), 2)
        print(json.dumps({"item": "forward_features_c2", "coarse_attention": coarse, "fine_attention": fine, "us": round(us, 1)}))


if __name__ == "__main__":
    main()
