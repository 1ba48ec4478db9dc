"""Diagnostic: the supervised signals at working sizes.  HIP events around every step, hot steps, the median of 20.
``opsup_coarse_loss`` at c2 (7 000 x 4 800, 134.4 MB) and c4 (B = 4, 15 000 x 4 800, 1 152 MB) as ms and GB/s, beside the torch expression of
the reference's ``losses.py:26-53`` on the same device tensors (with the dense ground truth it needs, built outside the timed region);
``ground_truth`` at N = 7 000, A = 3 000.  Not part of the product."""
import os
import statistics
import sys

import torch

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), ".."))
from onepose_st_amd import supervision  # noqa: E402

supervision.load()
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


def reference_focal(conf, conf_gt, alpha=0.25, gamma=2.0):
    """losses.py:26-53 as written (float32, boolean gathers)"""
    conf = torch.clamp(conf, 1e-6, 1 - 1e-6)
    loss_pos = -alpha * torch.pow(1 - conf[conf_gt == 1], gamma) * (conf[conf_gt == 1]).log()
    loss_neg = -(1 - alpha) * torch.pow(conf[conf_gt == 0], gamma) * (1 - conf[conf_gt == 0]).log()
    if loss_pos.shape[0] == 0:
        return loss_neg.mean()
    if loss_neg.shape[0] == 0:
        return loss_pos.mean()
    return loss_pos.mean() + loss_neg.mean()


def labelled(B, N, M, n_pos, g):
    """A matrix like a real one: almost every element far below 1e-6, ``n_pos`` confident positives per frame"""
    conf = torch.empty(B, N, M, device=dev).uniform_(-25.0, -14.0, generator=g).exp_()
    gt_j = torch.full((B, N), -1, dtype=torch.int64, device=dev)
    for b in range(B):
        rows = torch.randperm(N, generator=g, device=dev)[:n_pos]
        cells = torch.randperm(M, generator=g, device=dev)[:n_pos]
        gt_j[b, rows] = cells
        conf[b, rows, cells] = torch.empty(n_pos, device=dev).uniform_(0.2, 0.99, generator=g)
    gt = supervision.GroundTruth(gt_j, torch.zeros(B, N, 2, device=dev), torch.zeros(B, M, dtype=torch.int64, device=dev),
                                 torch.zeros(B, dtype=torch.int32, device=dev), (M // 80, 80))
    return conf, gt


def main():
    g = torch.Generator(device=dev).manual_seed(0)
    for name, (B, N, M) in (("c2", (1, 7000, 4800)), ("c4", (4, 15000, 4800))):
        conf, gt = labelled(B, N, M, 3000, g)
        mb = conf.numel() * 4 / 1e6
        ms = median_ms(lambda: supervision.coarse_loss(conf, gt))
        ours = supervision.coarse_loss(conf, gt).to_host()
        print(f"{name}: opsup_coarse_loss  {ms:8.3f} ms  {mb / ms:8.1f} GB/s  ({mb:.1f} MB; 8 000 GB/s nominal)  loss_c {ours['loss_c']:.9g}")
        try:
            conf_gt = torch.zeros(B, N, M, dtype=torch.int16, device=dev)
            b, i = (gt.gt_j >= 0).nonzero(as_tuple=True)
            conf_gt[b, i, gt.gt_j[b, i]] = 1
            ms_t = median_ms(lambda: reference_focal(conf, conf_gt))
            print(f"{name}: torch losses.py    {ms_t:8.3f} ms  {mb / ms_t:8.1f} GB/s  loss_c {float(reference_focal(conf, conf_gt)):.9g}"
                  f"   ({ms_t / ms:.1f} x)")
            del conf_gt
        except torch.cuda.OutOfMemoryError as err:
            print(f"{name}: torch losses.py    out of memory ({err})")
        del conf, gt
        torch.cuda.empty_cache()
    B, N, A, H, W = 1, 7000, 3000, 512, 512
    kp = (torch.rand(B, N, 3, device=dev, generator=g) - 0.5) * 0.3
    ids = torch.randperm(N, device=dev, generator=g)[:A][None].contiguous()
    pose = torch.eye(4, device=dev)[None].clone()
    pose[0, 2, 3] = 0.6
    K = torch.tensor([[700.0, 0, 256], [0, 700.0, 256], [0, 0, 1]], device=dev)
    ms = median_ms(lambda: supervision.ground_truth(kp, ids, pose, K, (H, W)))
    n_gt = int(supervision.ground_truth(kp, ids, pose, K, (H, W)).n_gt[0])
    print(f"ground_truth N = {N}, A = {A}, {H} x {W}: {ms * 1e3:8.1f} us (three launches and five allocations), n_gt {n_gt}")


if __name__ == "__main__":
    main()
