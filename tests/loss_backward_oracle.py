"""The specification of the loss backward (include/ext/onepose_loss_backward.h) restated in numpy float64, one function per
entry (:func:`coarse_grads`, :func:`fine_grads`), and the literal float64 FORWARD they differentiate (:func:`confidence`,
:func:`coarse_loss`, :func:`fine_expectation`, :func:`fine_loss`, :func:`total_loss`: conf from the features, then the expressions of
``tests/supervision_oracle.py``'s coarse and fine loss without its float32 inputs), which the tests difference numerically.

``faults``: a set of names of seeded faults of the coarse entry (tests/test_loss_backward_cpu.py plants each and measures how far outside the
precision bar it lies): ``rc_exchanged`` (needs N == M), ``no_factor_2``, ``no_clamp_mask``, ``per_frame_counts``, ``pr_pc_exchanged``.

:func:`coarse_standin`: the coarse entry in float32 with the operands of its matrix products split as the kernel splits them
(``tests/bf16_faithful.split``): what float32 arithmetic around split-bf16 products leaves, measured without a device -- the precision bar
of the device test is twice its worst value over that test's cases."""
import numpy as np
import torch

from tests import bf16_faithful
from tests import supervision_oracle as sup

OK, NONE, FORCED, EMPTY = sup.OK, sup.NONE, sup.FORCED, sup.EMPTY
LO, HI = sup.LO, sup.HI
CHANNELS, FINE_CHANNELS = 256, 128
INV_SQRT_CF = 0.08838834764831843                            # 1 / sqrt(128.0)
assert INV_SQRT_CF == 1.0 / np.sqrt(128.0)


def temperature_of(temperature):
    """``t = (float)(temperature + 1e-4)``"""
    return float(np.float32(temperature + 1e-4))


def _logsumexp(S, axis):
    m = S.max(axis=axis, keepdims=True)
    return m + np.log(np.exp(S - m).sum(axis=axis, keepdims=True))


def confidence(feat0, feat1, temperature):
    """-> dict ``S``, ``Pr``, ``Pc``, ``conf`` ``[B, N, M]`` float64 and ``a``, ``b`` (the features / 16) and ``t``"""
    a, b = np.asarray(feat0, np.float64) / 16.0, np.asarray(feat1, np.float64) / 16.0
    t = temperature_of(temperature)
    S = np.einsum("bnc,bmc->bnm", a, b) / t
    Pr, Pc = np.exp(S - _logsumexp(S, 2)), np.exp(S - _logsumexp(S, 1))
    return {"S": S, "Pr": Pr, "Pc": Pc, "conf": Pc * Pr, "a": a, "b": b, "t": t}


def positives(gt_j, M):
    """``[B, N, M]`` bool: the positive of every row whose ``gt_j`` lies in ``[0, M)``"""
    gt_j = np.asarray(gt_j, np.int64)
    B, N = gt_j.shape
    is_pos = np.zeros((B, N, M), bool)
    b, i = np.nonzero((gt_j >= 0) & (gt_j < M))
    is_pos[b, i, gt_j[b, i]] = True
    return is_pos


def _powers(gamma):
    if gamma == 2.0:
        return (lambda v: v * v), (lambda v: v)
    return (lambda v: np.power(v, gamma)), (lambda v: np.power(v, gamma - 1.0))


# ---- the forward, float64 -----------------------------------------------------------------------------------------------------------------
def coarse_loss(conf, gt_j, alpha=0.25, gamma=2.0, pos_weight=1.0, neg_weight=1.0):
    """``opsup_coarse_loss``'s expression on a float64 ``conf`` (plain sums: the order is below what a difference quotient resolves)"""
    B, N, M = conf.shape
    is_pos = positives(gt_j, M)
    P, _ = _powers(gamma)
    c = np.where(conf < LO, LO, np.where(conf > HI, HI, conf))
    pos = ((-alpha) * P(1.0 - c[is_pos])) * np.log(c[is_pos])
    neg = ((-(1.0 - alpha)) * P(c[~is_pos])) * np.log(1.0 - c[~is_pos])
    if len(pos) == 0:
        return neg_weight * neg.mean()
    if len(neg) == 0:
        return pos_weight * pos.mean()
    return pos_weight * pos.mean() + neg_weight * neg.mean()


def fine_grid(W):
    r = np.arange(W * W)
    return np.stack([-1.0 + (r % W) * (2.0 / (W - 1)), -1.0 + (r // W) * (2.0 / (W - 1))], axis=1)


def fine_expectation(feat_f0, feat_f1):
    """-> ``(co [n, 2], p [n, WW])`` float64: the window softmax and its expectation"""
    f0, f1 = np.asarray(feat_f0, np.float64), np.asarray(feat_f1, np.float64)
    W = int(round(np.sqrt(f1.shape[1])))
    x = np.einsum("kc,krc->kr", f0, f1) * INV_SQRT_CF
    e = np.exp(x - x.max(axis=1, keepdims=True))
    p = e / e.sum(axis=1, keepdims=True)
    return p @ fine_grid(W), p


def fine_bookkeeping(expec_f, expec_f_gt, count, correct_thr, training):
    """``opsup_fine_loss``'s: -> ``(n, weight [n] float64 (detached), counts [n] bool, n_correct, status)``"""
    e, g = np.asarray(expec_f, np.float64), np.asarray(expec_f_gt, np.float64)        # (the device's are float32 values)
    cap = len(e)
    n = cap if count is None else int(min(max(int(count), 0), cap))
    e, g = e[:n], g[:n]
    with np.errstate(all="ignore"):
        inv = 1.0 / np.where(e[:, 2] < 1e-10, 1e-10, e[:, 2])
        w = inv / (sup.block_sum(inv) / np.float64(n))
        correct = np.maximum(np.abs(g[:, 0]), np.abs(g[:, 1])) < correct_thr
    if correct.any():
        return n, w, correct, int(correct.sum()), OK
    if not training:
        return n, w, correct, 0, NONE
    if n == 0:
        return n, w, correct, 0, EMPTY
    forced = np.zeros(n, bool)
    forced[0] = True
    w = w.copy()
    w[0] = 1e-6
    return n, w, forced, 1, FORCED


def fine_loss(feat_f0, feat_f1, expec_f, expec_f_gt, count=None, correct_thr=1.0, training=True):
    """The fine loss with the expectation RECOMPUTED from the features (float64) and the std weight of ``expec_f`` (detached) -> the loss,
    0.0 with ``NONE`` / ``EMPTY`` (no term)"""
    n, w, counts, n_correct, status = fine_bookkeeping(expec_f, expec_f_gt, count, correct_thr, training)
    if status in (NONE, EMPTY):
        return 0.0
    co, _ = fine_expectation(np.asarray(feat_f0)[:n][counts], np.asarray(feat_f1)[:n][counts])
    d = np.asarray(expec_f_gt, np.float64)[:n][counts] - co
    return float(((d * d).sum(axis=1) * w[counts]).sum() / n_correct)


def total_loss(feat0, feat1, gt_j, temperature, feat_f0, feat_f1, expec_f, expec_f_gt, cfg, count=None, training=True):
    """``Loss.forward``'s scalar from the four feature tensors (``cfg``: the reference's ``loss`` block)"""
    conf = confidence(feat0, feat1, temperature)["conf"]
    loss = coarse_loss(conf, gt_j, cfg["focal_alpha"], cfg["focal_gamma"], cfg["pos_weight"], cfg["neg_weight"]) * cfg["coarse_weight"]
    return loss + fine_loss(feat_f0, feat_f1, expec_f, expec_f_gt, count, cfg["fine_correct_thr"], training) * cfg["fine_weight"]


# ---- 1. the coarse gradient ---------------------------------------------------------------------------------------------------------------
def focal_derivative(conf, is_pos, wpos, wneg, alpha, gamma, faults=()):
    """``g [B, N, M]``: d loss / d conf (``wpos``, ``wneg``: scalars, or ``[B, 1, 1]`` with the ``per_frame_counts`` fault)"""
    P, Q = _powers(gamma)
    c = np.where(conf < LO, LO, np.where(conf > HI, HI, conf))
    inside = (conf >= LO) & (conf <= HI)
    with np.errstate(all="ignore"):
        g_pos = wpos * (alpha * gamma * Q(1.0 - c) * np.log(c) - alpha * P(1.0 - c) / c)
        g_neg = wneg * (-(1.0 - alpha) * (gamma * Q(c) * np.log(1.0 - c) - P(c) / (1.0 - c)))
    g = np.where(is_pos, g_pos, g_neg)
    return g if "no_clamp_mask" in faults else np.where(inside, g, 0.0)


def weights(is_pos, pos_weight, neg_weight, faults=()):
    B, N, M = is_pos.shape
    if "per_frame_counts" in faults:
        n_pos = is_pos.sum(axis=(1, 2), keepdims=True).astype(np.float64)
        n_neg = N * M - n_pos
    else:
        n_pos = np.float64(is_pos.sum())
        n_neg = np.float64(B * N * M) - n_pos
    with np.errstate(all="ignore"):
        return np.where(n_pos > 0, pos_weight / n_pos, 0.0), np.where(n_neg > 0, neg_weight / n_neg, 0.0)


def coarse_grads(feat0, feat1, gt_j, temperature, alpha=0.25, gamma=2.0, pos_weight=1.0, neg_weight=1.0, scale=1.0, faults=()):
    """-> dict ``grad0 [B, N, 256]``, ``grad1 [B, M, 256]`` float64, ``conf``, ``is_pos``, ``n_pos``, and the two margins of the device
    test's condition: ``pos_margin`` (the smallest ``|conf / 1e-6 - 1|`` over the positives) and ``hi_margin`` (the smallest
    ``|conf - (1 - 1e-6)|`` over every element)"""
    f = confidence(feat0, feat1, temperature)
    conf, Pr, Pc, t = f["conf"], f["Pr"], f["Pc"], f["t"]
    M = conf.shape[2]
    is_pos = positives(gt_j, M)
    wpos, wneg = weights(is_pos, pos_weight, neg_weight, faults)
    u = scale * conf * focal_derivative(conf, is_pos, wpos, wneg, alpha, gamma, faults)
    r, c = u.sum(axis=2, keepdims=True), u.sum(axis=1, keepdims=True)
    if "rc_exchanged" in faults:
        r, c = np.swapaxes(c, 1, 2), np.swapaxes(r, 1, 2)
    if "pr_pc_exchanged" in faults:
        Pr, Pc = Pc, Pr
    dS = (1.0 if "no_factor_2" in faults else 2.0) * u - Pr * r - Pc * c
    k = 1.0 / (16.0 * t)
    return {"grad0": k * np.einsum("bnm,bmc->bnc", dS, f["b"]), "grad1": k * np.einsum("bnm,bnc->bmc", dS, f["a"]), "conf": conf,
            "is_pos": is_pos, "n_pos": int(is_pos.sum()),
            "pos_margin": float(np.abs(conf[is_pos] / LO - 1.0).min()) if is_pos.any() else np.inf,
            "hi_margin": float(np.abs(conf - HI).min())}


def coarse_standin(feat0, feat1, gt_j, temperature, alpha=0.25, gamma=2.0, pos_weight=1.0, neg_weight=1.0, scale=1.0):
    """The coarse entry in float32 (torch, CPU) with split-bf16 operands at the kernel's operand points: ``feat / 16`` for ``S`` and as the
    swept operand of the gradient products, and ``dS``.  -> ``(grad0, grad1)`` float32 numpy"""
    f32 = torch.float32
    a, b = torch.as_tensor(np.asarray(feat0, np.float32)) * 0.0625, torch.as_tensor(np.asarray(feat1, np.float32)) * 0.0625
    (ah, al), (bh, bl) = bf16_faithful.split(a), bf16_faithful.split(b)

    def product(xh, xl, yh, yl, eq):                         # hi . hi + hi . lo + lo . hi, small terms first, float32
        return torch.einsum(eq, xl, yh) + torch.einsum(eq, xh, yl) + torch.einsum(eq, xh, yh)
    t = np.float32(temperature + 1e-4)
    S = product(ah, al, bh, bl, "bnc,bmc->bnm") * float(np.float32(1.0) / t)
    lr, lc = torch.logsumexp(S, 2, keepdim=True), torch.logsumexp(S, 1, keepdim=True)
    Pr, Pc = torch.exp(S - lr), torch.exp(S - lc)
    conf = Pr * Pc
    M = conf.shape[2]
    is_pos = torch.as_tensor(positives(gt_j, M))
    wpos, wneg = weights(is_pos.numpy(), pos_weight, neg_weight)
    wpos, wneg = float(np.float32(scale * float(wpos))), float(np.float32(scale * float(wneg)))
    lo, hi = float(np.float32(LO)), float(np.float32(HI))
    inside = (conf >= lo) & (conf <= hi)
    c = conf.clamp(lo, hi)
    if gamma == 2.0:
        P, Q = (lambda v: v * v), (lambda v: v)
    else:
        P, Q = (lambda v: torch.pow(v, np.float32(gamma))), (lambda v: torch.pow(v, np.float32(gamma - 1.0)))
    al_, ga = float(np.float32(alpha)), float(np.float32(gamma))
    g_pos = wpos * (al_ * ga * Q(1 - c) * torch.log(c) - al_ * P(1 - c) / c)
    g_neg = wneg * (-(1 - al_) * (ga * Q(c) * torch.log1p(-c) - P(c) / (1 - c)))
    u = torch.where(inside, conf * torch.where(is_pos, g_pos, g_neg), torch.zeros((), dtype=f32))
    dS = (2 * u - Pr * u.sum(2, keepdim=True)) - Pc * u.sum(1, keepdim=True)
    dh, dl = bf16_faithful.split(dS)
    k = float(np.float32(0.0625) / t)
    g0 = product(dh, dl, bh, bl, "bnm,bmc->bnc") * k
    g1 = product(dh, dl, ah, al, "bnm,bnc->bmc") * k
    assert g0.dtype == f32 and g1.dtype == f32
    return g0.numpy(), g1.numpy()


def frame_error(got, want):
    """The statistic of the precision bar: ``|y - y_ref| / max |y_ref| over the frame's tensor``, worst element over the frames; a frame
    whose reference is all zero must be zero (-> 0.0, else inf)"""
    got, want = np.asarray(got, np.float64), np.asarray(want, np.float64)
    worst = 0.0
    for b in range(want.shape[0]):
        top, err = np.abs(want[b]).max(), np.abs(got[b] - want[b]).max()
        worst = max(worst, (0.0 if err == 0 else np.inf) if top == 0 else err / top)
    return float(worst)


# ---- 2. the fine gradient -----------------------------------------------------------------------------------------------------------------
def fine_grads(feat_f0, feat_f1, expec_f, expec_f_gt, count=None, correct_thr=1.0, training=True, scale=1.0):
    """-> dict ``grad_f0 [n, 128]``, ``grad_f1 [n, WW, 128]`` float64 of the first ``n = clamp(count)`` rows, ``n_correct``, ``status``"""
    f0, f1 = np.asarray(feat_f0, np.float64), np.asarray(feat_f1, np.float64)
    n, w, counts, n_correct, status = fine_bookkeeping(expec_f, expec_f_gt, count, correct_thr, training)
    f0, f1 = f0[:n], f1[:n]
    W = int(round(np.sqrt(f1.shape[1])))
    g0, g1 = np.zeros_like(f0), np.zeros_like(f1)
    if status in (OK, FORCED) and counts.any():
        grid = fine_grid(W)
        co, p = fine_expectation(f0[counts], f1[counts])
        gt = np.asarray(expec_f_gt, np.float64)[:n][counts]
        dco = ((scale * -2.0) * (gt - co)) * w[counts][:, None] / np.float64(n_correct)
        ds = p * (dco @ grid.T - (co * dco).sum(axis=1, keepdims=True))
        g0[counts] = INV_SQRT_CF * np.einsum("kr,krc->kc", ds, f1[counts])
        g1[counts] = (INV_SQRT_CF * ds)[:, :, None] * f0[counts][:, None, :]
    return {"grad_f0": g0, "grad_f1": g1, "n_correct": n_correct, "status": status}
