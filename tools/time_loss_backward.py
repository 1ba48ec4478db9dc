"""Diagnostic: the loss backward at working sizes.  HIP events around every step, hot steps, the median of 20.
``coarse_grads`` at c2 with B = 4 (4 x 7 000 x 4 800) and at c4 with B = 1 (15 000 x 4 800), ``fine_grads`` at T = 3 000, each as ms and as
achieved FLOP/s from the algorithmic count (coarse: 16 N M C per frame -- six evaluations of S and two gradient products; fine: 6 T WW C),
beside float32 torch autograd of the reference's expression on the same device tensors (or the note that it did not fit), and
``torch.cuda.max_memory_allocated`` of both.  Not part of the product."""
import os
import statistics
import sys

import torch

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), ".."))
from onepose_st_amd import loss_backward, supervision  # noqa: E402

loss_backward.load()
dev = torch.device("cuda:0")
HOT, STEPS = 5, 20
TEMPERATURE = 0.1


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


def peak_mb(step):
    torch.cuda.synchronize()
    torch.cuda.empty_cache()
    base = torch.cuda.memory_allocated()
    torch.cuda.reset_peak_memory_stats()
    keep = step()
    torch.cuda.synchronize()
    peak = (torch.cuda.max_memory_allocated() - base) / 1e6
    del keep
    return peak


def planted(B, N, M, n_pos, g):
    """Features like a trained model's: ``n_pos`` rows per frame have a cell that carries a noisy copy of them"""
    f0, f1 = torch.randn(B, N, 256, device=dev, generator=g), torch.randn(B, M, 256, device=dev, generator=g)
    gt_j = torch.full((B, N), -1, dtype=torch.int64, device=dev)
    gt_i = torch.full((B, M), -1, dtype=torch.int64, device=dev)
    for b in range(B):
        rows = torch.randperm(N, generator=g, device=dev)[:n_pos]
        cells = torch.randperm(M, generator=g, device=dev)[:n_pos]
        gt_j[b, rows], gt_i[b, cells] = cells, rows
        f1[b, cells] = f0[b, rows] + 0.15 * torch.randn(n_pos, 256, device=dev, generator=g)
    gt = supervision.GroundTruth(gt_j, torch.zeros(B, N, 2, device=dev), gt_i, torch.zeros(B, dtype=torch.int32, device=dev), (M // 80, 80))
    return f0, f1, gt


def reference_coarse(f0, f1, conf_gt, alpha=0.25, gamma=2.0):
    """coarse_matching.py:102-115 and losses.py:26-53 as written (float32), under autograd -> the two gradients"""
    f0, f1 = f0.detach().requires_grad_(), f1.detach().requires_grad_()
    a, b = f0 / 256 ** .5, f1 / 256 ** .5
    sim = torch.einsum("nlc,nsc->nls", a, b) / (TEMPERATURE + 1e-4)
    conf = torch.softmax(sim, 1) * torch.softmax(sim, 2)
    conf = torch.clamp(conf, 1e-6, 1 - 1e-6)
    loss_pos = -alpha * torch.pow(1 - conf[conf_gt == 1], gamma) * (conf[conf_gt == 1]).log()
    loss_neg = -(1 - alpha) * torch.pow(conf[conf_gt == 0], gamma) * (1 - conf[conf_gt == 0]).log()
    (loss_pos.mean() + loss_neg.mean()).backward()
    return f0.grad, f1.grad


def reference_fine(f0, f1, expec_f, gt):
    """fine_matching.py:78-94 and losses.py:66-101 (float32), under autograd"""
    f0, f1 = f0.detach().requires_grad_(), f1.detach().requires_grad_()
    W = int(round(f1.shape[1] ** .5))
    heat = torch.softmax(torch.einsum("mc,mrc->mr", f0, f1) / 128 ** .5, dim=1)
    lin = torch.linspace(-1, 1, W, device=dev)
    grid = torch.stack([lin.repeat(W), lin.repeat_interleave(W)], dim=1)
    co = heat @ grid
    correct = gt.abs().amax(dim=1) < 1.0
    inv = 1.0 / expec_f[:, 2].clamp(min=1e-10)
    w = (inv / inv.mean()).detach()
    (((gt[correct] - co[correct]) ** 2).sum(-1) * w[correct]).mean().backward()
    return f0.grad, f1.grad


def main():
    g = torch.Generator(device=dev).manual_seed(0)
    for name, (B, N, M) in (("c2 x 4", (4, 7000, 4800)), ("c4 x 1", (1, 15000, 4800))):
        f0, f1, gt = planted(B, N, M, 3000, g)
        flop = 16.0 * B * N * M * 256
        out = (torch.empty_like(f0), torch.empty_like(f1))
        step = lambda: loss_backward.coarse_grads(f0, f1, gt, temperature=TEMPERATURE, out=out)
        ms = median_ms(step)
        mb = peak_mb(step)
        print(f"{name}: opbwd_coarse_grads {ms:9.3f} ms  {flop / ms / 1e9:8.1f} TFLOP/s algorithmic ({flop / 1e12:.2f} TFLOP)  peak {mb:9.1f} MB")
        try:
            conf_gt = torch.zeros(B, N, M, dtype=torch.int16, device=dev)
            b, i = (gt.gt_j >= 0).nonzero(as_tuple=True)
            conf_gt[b, i, gt.gt_j[b, i]] = 1
            ref = lambda: reference_coarse(f0, f1, conf_gt)
            ms_t = median_ms(ref)
            mb_t = peak_mb(ref)
            r0, _ = reference_coarse(f0, f1, conf_gt)
            diff = float((out[0] - r0).abs().max() / r0.abs().max())
            print(f"{name}: torch autograd     {ms_t:9.3f} ms  {flop / ms_t / 1e9:8.1f} TFLOP/s algorithmic  peak {mb_t:9.1f} MB  ({ms_t / ms:.2f} x; "
                  f"max |grad0 - torch| / max |torch| {diff:.1e})")
            del conf_gt, r0
        except torch.cuda.OutOfMemoryError as err:
            print(f"{name}: torch autograd     did not fit ({err})")
        del f0, f1, gt, out
        torch.cuda.empty_cache()
    T, W = 3000, 5
    ff0, ff1 = torch.randn(T, 128, device=dev, generator=g), torch.randn(T, W * W, 128, device=dev, generator=g)
    expec_f = torch.cat([torch.rand(T, 2, device=dev, generator=g) - 0.5, torch.rand(T, 1, device=dev, generator=g) + 0.05], dim=1)
    gt_f = (torch.rand(T, 2, device=dev, generator=g) - 0.5) * 2.6
    flop = 6.0 * T * W * W * 128
    out = (torch.empty_like(ff0), torch.empty_like(ff1))
    step = lambda: loss_backward.fine_grads(ff0, ff1, expec_f, gt_f, out=out)
    ms = median_ms(step)
    print(f"fine T = {T}: opbwd_fine_grads {ms * 1e3:9.1f} us  {flop / ms / 1e6:8.2f} GFLOP/s algorithmic (float64)  peak {peak_mb(step):6.1f} MB")
    ref = lambda: reference_fine(ff0, ff1, expec_f, gt_f)
    ms_t = median_ms(ref)
    r0, _ = reference_fine(ff0, ff1, expec_f, gt_f)
    print(f"fine T = {T}: torch autograd   {ms_t * 1e3:9.1f} us  peak {peak_mb(ref):6.1f} MB  ({ms_t / ms:.2f} x; max |grad_f0 - torch| / max |torch| "
          f"{float((out[0] - r0).abs().max() / r0.abs().max()):.1e})")


if __name__ == "__main__":
    main()
