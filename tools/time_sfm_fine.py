"""Time the SfM fine matching over a pair list against the loop of per-pair ``forward`` calls it replaces.

    python tools/time_sfm_fine.py [--size 512] [--images 12] [--pairs 40] [--rows 500] [--chunk-rows 8192] [--iters 10] [--warmup 2]

One seeded pair list (float64 keypoints inside the images, unit-free random images, synthetic LoFTR weights, scales other than one);
``--pairs`` ordered pairs drawn from the ``--images`` images, about ``--rows`` rows each.  One JSON line:
  * ``per_pair_loop_ms``: HIP events around the loop the parent commit runs -- per pair ``matcher(data, extract_coarse_feature=True,
    extract_fine_feature=True)`` with that pair's slices, results left on the device (the reference also copies each to the host);
  * ``bank_ms``, ``fine_match_pairs_ms`` and their sum ``bank_and_pairs_ms``: ``build_feature_bank`` and ``fine_match_pairs``;
    each figure is the median, minimum and maximum of ``--iters`` calls after ``--warmup``, input checks and read-backs included;
  * ``bank_bytes``; ``calls``: the C-ABI entry calls of each path (``hip.call`` and this library's ``call``; an entry enqueues one
    kernel, ``opsff_row_ids`` two), counted in one extra run outside the timed ones;
  * ``equal``: whether ``mkpts1_f`` and ``feature0`` of the two paths are bit-equal on this list.
Per-kernel times come from a ``rocprofv3 --kernel-trace --stats`` run of this script with ``--iters 1``.
"""
from __future__ import annotations

import argparse
import json
import os
import statistics
import sys

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

from onepose_st_amd import hip, loftr, rows as rows_mod, sfm_fine as sf  # noqa: E402
from onepose_st_amd import backbone_hip  # noqa: E402
from onepose_st_amd.synthetic import make_synthetic_loftr_state_dict  # noqa: E402


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


def counted(fn):
    """-> (result, number of C-ABI entry calls ``fn`` made)"""
    n = [0]
    real_hip, real_sf = hip.call, sf.call

    def hip_call(*a):
        n[0] += 1
        return real_hip(*a)

    def sf_call(*a):
        n[0] += 1
        return real_sf(*a)
    hip.call, sf.call = hip_call, sf_call
    try:
        return fn(), n[0]
    finally:
        hip.call, sf.call = real_hip, real_sf


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--size", type=int, default=512)
    ap.add_argument("--images", type=int, default=12)
    ap.add_argument("--pairs", type=int, default=40)
    ap.add_argument("--rows", type=int, default=500)
    ap.add_argument("--chunk-rows", type=int, default=8192)
    ap.add_argument("--iters", type=int, default=10)
    ap.add_argument("--warmup", type=int, default=2)
    a = ap.parse_args()
    dev = torch.device("cuda:0")
    g = torch.Generator().manual_seed(7)
    S, I = a.size, a.images
    matcher = loftr.LoFTR_for_OnePose_Plus().eval()
    matcher.load_state_dict(make_synthetic_loftr_state_dict(0), strict=True)
    matcher.to(dev)
    images = torch.rand(I, 1, S, S, generator=g).to(dev)
    scales = (1.05 + 0.4 * torch.rand(I, 2, generator=g)).to(dev)                    # h factors above one: no id past the last row of cells
    every = [(l, r) for l in range(I) for r in range(I) if l != r]
    chosen = [every[k] for k in torch.randperm(len(every), generator=g)[:a.pairs].tolist()]
    chosen.sort()
    counts = [max(1, int(a.rows * (0.8 + 0.4 * float(torch.rand(1, generator=g))))) for _ in chosen]
    off = [0]
    for c in counts:
        off.append(off[-1] + c)
    M = off[-1]
    pairs = {"mkpts0_c": (torch.rand(M, 2, generator=g, dtype=torch.float64) * (S - 2)).to(dev),
             "mkpts1_c": (torch.rand(M, 2, generator=g, dtype=torch.float64) * (S - 2)).to(dev),
             "row_left": torch.tensor([l for (l, _), c in zip(chosen, counts) for _ in range(c)], device=dev),
             "row_right": torch.tensor([r for (_, r), c in zip(chosen, counts) for _ in range(c)], device=dev)}

    def per_pair_loop():
        out = []
        for n, (l, r) in enumerate(chosen):
            data = {"image0": images[l:l + 1], "image1": images[r:r + 1], "scale0": scales[l:l + 1], "scale1": scales[r:r + 1],
                    "mkpts0_c": pairs["mkpts0_c"][off[n]:off[n + 1]].clone(), "mkpts1_c": pairs["mkpts1_c"][off[n]:off[n + 1]].clone()}
            matcher(data, extract_coarse_feature=True, extract_fine_feature=True)
            out.append(data)
        return out

    def bank_only():
        return sf.build_feature_bank(matcher, images, scales)

    out = {"size": S, "images": I, "pairs": len(chosen), "pair_rows": M, "chunk_rows": a.chunk_rows}
    loop, out["per_pair_loop_ms"] = timed(per_pair_loop, a.iters, a.warmup)
    bank, out["bank_ms"] = timed(bank_only, a.iters, a.warmup)
    res, out["fine_match_pairs_ms"] = timed(lambda: sf.fine_match_pairs(matcher, bank, pairs, chunk_rows=a.chunk_rows), a.iters, a.warmup)
    _, out["bank_and_pairs_ms"] = timed(lambda: sf.fine_match_pairs(matcher, bank_only(), pairs, chunk_rows=a.chunk_rows), a.iters, a.warmup)
    out["bank_bytes"] = bank["bytes"]
    # rows.py and backbone_hip.py reach hip.call through the module attribute, so the counter sees them too
    assert rows_mod.hip is hip and backbone_hip.hip is hip
    _, n_loop = counted(per_pair_loop)
    _, n_bank = counted(bank_only)
    _, n_pairs = counted(lambda: sf.fine_match_pairs(matcher, bank, pairs, chunk_rows=a.chunk_rows))
    out["calls"] = {"per_pair_loop": n_loop, "bank": n_bank, "fine_match_pairs": n_pairs}
    out["equal"] = bool(torch.equal(torch.cat([d["mkpts1_f"] for d in loop]), res["mkpts1_f"])
                        and torch.equal(torch.cat([d["feat_ext0"] for d in loop]), res["feature0"]))
    print(json.dumps(out))


if __name__ == "__main__":
    main()
