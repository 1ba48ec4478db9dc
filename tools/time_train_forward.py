"""Diagnostic: the training-mode forward's own step at a working size.  HIP events around every step, hot steps, the
median of 20.  ``gt_list + pad_matches`` at c2 with the batch of ``train.yaml`` (B = 4, N = 7 000, M = 4 800, 3 000 ground-truth rows and
2 500 predicted matches per frame, ``train_coarse_percent`` 0.3, ``train_pad_num_gt_min`` 200), beside the torch expression of the
reference's ``coarse_matching.py:189-217`` on the same device tensors with the dense ``conf_matrix_gt`` it needs (int16, 269 MB; built
outside the timed region).  Not part of the product."""
import os
import statistics
import sys

import torch

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), ".."))
from onepose_st_amd import supervision, train_forward  # noqa: E402
from onepose_st_amd.matchcall import MatchLists  # noqa: E402

train_forward.load()
dev = torch.device("cuda:0")
HOT, STEPS = 5, 20


def median_ms(step):
    for _ in range(HOT):
        step()
    times = []
    for _ in range(STEPS):
        s, e = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        s.record()
        step()
        e.record()
        torch.cuda.synchronize()
        times.append(s.elapsed_time(e))
    return statistics.median(times)


def reference_padding(lists, P, conf_gt, T, G):
    """coarse_matching.py:189-217 as written (its ``len()`` of a ``torch.where`` is the host read the device form does without)"""
    b_ids, i_ids, j_ids, mconf = lists.b_ids[:P], lists.i_ids[:P], lists.j_ids[:P], lists.mconf[:P]
    pred = torch.arange(P, device=dev) if P <= T - G else torch.randint(P, (T - G,), device=dev)
    spv_b, spv_i, spv_j = torch.where(conf_gt)
    pad = torch.randint(len(spv_b), (max(T - P, G),), device=dev)
    mconf_gt = torch.zeros(len(spv_b), device=dev)
    return [torch.cat([x[pred], y[pad]], dim=0) for x, y in ((b_ids, spv_b), (i_ids, spv_i), (j_ids, spv_j), (mconf, mconf_gt))]


def main():
    g = torch.Generator(device=dev).manual_seed(0)
    B, N, M, w_c, n_gt, P_frame, percent, G = 4, 7000, 4800, 80, 3000, 2500, 0.3, 200
    T = train_forward.train_rows(B, N, M, percent)
    gt_j = torch.full((B, N), -1, dtype=torch.int64, device=dev)
    for b in range(B):
        gt_j[b, torch.randperm(N, generator=g, device=dev)[:n_gt]] = torch.randperm(M, generator=g, device=dev)[:n_gt]
    gt = supervision.GroundTruth(gt_j, torch.zeros(B, N, 2, device=dev), torch.zeros(B, M, dtype=torch.int64, device=dev),
                                 torch.zeros(B, dtype=torch.int32, device=dev), (M // w_c, w_c))
    kp = torch.rand(B, N, 3, device=dev, generator=g)
    P = B * P_frame
    lists = MatchLists.empty(B * N, dev)
    lists.b_ids[:P] = torch.arange(B, device=dev).repeat_interleave(P_frame)
    lists.i_ids[:P] = torch.cat([torch.randperm(N, generator=g, device=dev)[:P_frame].sort().values for _ in range(B)])
    lists.j_ids[:P] = torch.randint(M, (P,), generator=g, device=dev)
    lists.mconf[:P] = torch.empty(P, device=dev).uniform_(0.2, 0.99, generator=g)
    lists.count[0] = P
    step = [0]

    def ours():
        step[0] += 1
        return train_forward.pad_matches(lists, gt, kp, T=T, G=G, seed=1, step=step[0], w_c=w_c, scale=8.0)
    ms = median_ms(ours)
    done = ours()
    print(f"c2, B = {B}: gt_list + pad_matches  {ms * 1e3:8.1f} us  (four launches; T = {T}, P = {P}, n_keep = {int(done.n_keep)}, "
          f"status = {int(done.status)}, ground-truth rows = {B * n_gt})")
    ms_l = median_ms(lambda: train_forward.gt_list(gt))
    print(f"c2, B = {B}: gt_list alone          {ms_l * 1e3:8.1f} us  (three launches over {B * N} rows)")
    try:
        conf_gt = gt.to_dense(budget_bytes=1 << 32)[0]
        ms_t = median_ms(lambda: reference_padding(lists, P, conf_gt, T, G))
        print(f"c2, B = {B}: torch coarse_matching.py:189-217  {ms_t * 1e3:8.1f} us  on a dense conf_matrix_gt of {conf_gt.numel() * 2 / 1e6:.0f} MB"
              f"   ({ms_t / ms:.1f} x)")
    except torch.cuda.OutOfMemoryError as err:
        print(f"c2, B = {B}: torch coarse_matching.py:189-217  out of memory ({err})")


if __name__ == "__main__":
    main()
