"""The seeded cases of the loss backward's device test (tests/test_gpu_loss_backward.py), shared with the CPU test that derives the precision
bar from them (tests/test_loss_backward_cpu.py): nothing here touches a device.

A coarse case is planted: about half of the rows of ``feat0`` have a ground-truth cell; three quarters of those cells carry a noisy copy of
their point's feature (confident positives), the rest do not -- half of them random, half OPPOSED to it (positives whose confidence stays
below 1e-6 at every size and must get NO direct gradient);
one ground-truth row in eight also has a noisy copy in a cell that is NOT its ground truth (confident negatives: the large gradients)."""
import numpy as np

from onepose_st_amd import loss_backward

R, S = loss_backward.OWNED_ROWS, loss_backward.SWEPT_ROWS              # the owned-row and swept-tile sizes, from the header
C, CF = loss_backward.CHANNELS, loss_backward.FINE_CHANNELS
TEMPERATURE = 0.1
FEATURE_SCALE = 1.0          # random similarities ~ N(0, 0.6) at t = 0.1; a planted pair sits near 10, an opposed one near -5
# twice this is the device test's bar: the worst frame_error of loss_backward_oracle.coarse_standin over COARSE_CASES, measured on the CPU by
# tests/test_loss_backward_cpu.py::test_the_precision_bar, which also checks that this line still holds what it measures
STANDIN_WORST = 3.0e-5
COARSE_BAR = 2 * STANDIN_WORST
FINE_RTOL = 2.0 ** -22       # one float32 rounding of the result plus libm differences in float64, of the row's largest value


def coarse_case(seed, B, N, M, empty_frames=(), pushed=False, plant=True):
    """-> dict ``feat0 [B, N, 256]``, ``feat1 [B, M, 256]`` float32, ``gt_j [B, N]``, ``gt_i [B, M]`` int64.  ``empty_frames``: frames
    whose planted pairs are NOT ground truth (confident negatives only).  ``plant=False``: random features (a one-row or two-column
    softmax saturates on a planted pair, and what is left of the gradient is cancellation)"""
    rng = np.random.default_rng(seed)
    feat0 = (rng.standard_normal((B, N, C)) * FEATURE_SCALE).astype(np.float32)
    feat1 = (rng.standard_normal((B, M, C)) * FEATURE_SCALE).astype(np.float32)
    gt_j, gt_i = np.full((B, N), -1, np.int64), np.full((B, M), -1, np.int64)
    n_gt = max(1, min(N, M) // 2)
    for b in range(B):
        rows, cells = rng.permutation(N)[:n_gt], rng.permutation(M)[:n_gt]
        if b not in empty_frames:
            gt_j[b, rows], gt_i[b, cells] = cells, rows
        if not plant:
            continue
        free = [j for j in range(M) if j not in set(cells.tolist())]
        copy = np.float32(0.7 if b in empty_frames else 1.0)       # a confident negative nearer 0.9 than 1: 1 / (1 - c) stays moderate
        for k, (i, j) in enumerate(zip(rows, cells)):
            if k % 4 != 3:
                feat1[b, j] = copy * feat0[b, i] + (0.15 * rng.standard_normal(C)).astype(np.float32)
            elif k % 8 == 3:
                feat1[b, j] = np.float32(-0.5) * feat0[b, i] + (0.15 * rng.standard_normal(C)).astype(np.float32)
            if k % 8 == 1 and free:
                feat1[b, free.pop()] = feat0[b, i] + (0.15 * rng.standard_normal(C)).astype(np.float32)
        if pushed and b == 0:                                # one positive above 1 - 1e-6: its pair 1.6 times as long, no noise
            i, j = rows[0], cells[0]
            feat0[b, i] *= np.float32(1.6)
            feat1[b, j] = feat0[b, i]
    return {"feat0": feat0, "feat1": feat1, "gt_j": gt_j, "gt_i": gt_i}


# name -> (arguments of coarse_case, keyword arguments of the entry beside temperature).  Seeds are chosen so that the condition of
# test_the_cases_meet_the_condition holds (no positive within 1 % of 1e-6, no element within 1e-9 of 1 - 1e-6).
COARSE_CASES = {f"n{N}_m{M}": (dict(seed=1000 + 7 * N + M, B=1, N=N, M=M, plant=N > 1 and M > 2), {})
                for N in (1, R - 1, R, R + 1, 2 * R + 1) for M in (2, S - 1, S, S + 1)}
COARSE_CASES.update({
    "c1_like": (dict(seed=3, B=2, N=300, M=35 * 37), {}),
    "one_empty_frame": (dict(seed=11, B=2, N=R + 5, M=2 * S + 3, empty_frames=(1,)), {}),
    "no_positive": (dict(seed=12, B=2, N=40, M=S + 9, empty_frames=(0, 1)), {}),
    "gamma_alpha": (dict(seed=13, B=1, N=R + 9, M=3 * S + 1), dict(gamma=1.5, alpha=0.4)),
    "scaled": (dict(seed=14, B=1, N=70, M=2 * S + 7), dict(scale=0.25)),
    "pushed": (dict(seed=15, B=2, N=90, M=4 * S + 5, pushed=True), {}),
})


def fine_case(seed, cap, W, far=False):
    """-> dict ``feat_f0 [cap, 128]``, ``feat_f1 [cap, W * W, 128]``, ``expec_f [cap, 3]``, ``expec_f_gt [cap, 2]`` float32.  About a third
    of the rows have ``|gt| >= 1`` (not correct); ``far``: all of them"""
    rng = np.random.default_rng(seed)
    f0 = rng.standard_normal((cap, CF)).astype(np.float32)
    f1 = rng.standard_normal((cap, W * W, CF)).astype(np.float32)
    expec_f = np.concatenate([rng.uniform(-0.6, 0.6, (cap, 2)), rng.uniform(0.05, 0.9, (cap, 1))], axis=1).astype(np.float32)
    gt = rng.uniform(-1.4, 1.4, (cap, 2)).astype(np.float32)
    if far:
        gt = (np.sign(gt) * (1.5 + np.abs(gt))).astype(np.float32)
    return {"feat_f0": f0, "feat_f1": f1, "expec_f": expec_f, "expec_f_gt": gt}
