"""The backward of the training loss on the device, down to the matcher's feature boundaries (opt-in): the gradient
of ``supervision.Loss`` with respect to the coarse transformer's outputs ``feat_c0 [B, N, 256]`` / ``feat_c1 [B, M, 256]`` -- the focal
loss (``src/lightning_model/losses.py:25-55``) through the dual softmax of ``coarse_matching.py:102-115`` -- and to the fine transformer's
outputs ``feat_f0 [T, 128]`` / ``feat_f1 [T, WW, 128]`` -- the std-weighted L2 loss (``losses.py:66-101``) through the window softmax and
expectation of ``fine_matching.py:78-94``.

The specification is ``include/ext/onepose_loss_backward.h`` (``tests/loss_backward_oracle.py`` restates it in numpy float64).  The coarse
entry allocates nothing ``N x M`` and does not take ``conf_matrix``: the similarity is recomputed tile by tile in three sweeps (the two
log-sum-exps, the two sums of ``u``, the two gradient products), every product a split-bf16 MFMA, every sum in a fixed order: two runs give
identical bytes.

Not here: the backward of the two transformers, of the window gather and of the backbone (they start from the four tensors
:func:`backward` writes), an optimiser or an ``autograd.Function``, and ``mask0`` / ``mask1`` loss weights.

The kernels are HIP (``csrc/loss_backward.hip`` in ``libonepose_loss_backward.so``, the row of ``cabi.BACKWARD``).  CPU tensors raise
:class:`hip.HipLibraryError` (no CPU fallback); nothing is synchronised and nothing is read on the host.
"""
from __future__ import annotations

import torch

from . import cabi, devargs, hip, supervision

_BINDING = cabi.Binding.of(__name__)                # the header is the one place a signature or a constant is written
library_path, load, check_arity, call, order = _BINDING.library_path, _BINDING.load, _BINDING.check_arity, _BINDING.call, _BINDING.order
launch = hip.launcher(_BINDING, globals())          # every stream-taking entry is called through it, by the header's parameter names
EXPORTED_SYMBOLS = _BINDING.exported_symbols
ABI_VERSION = _BINDING.abi_version
BLOCK, OWNED_ROWS, SWEPT_ROWS, CHANNELS, FINE_CHANNELS, MAX_BATCH, MAX_ROWS, OK, NONE, FORCED, EMPTY = map(_BINDING.constant, (
    "BLOCK", "OWNED_ROWS", "SWEPT_ROWS", "CHANNELS", "FINE_CHANNELS", "MAX_BATCH", "MAX_ROWS", "OK", "NONE", "FORCED", "EMPTY"))
KEEP_FEATURES_HINT = "set hip_keep_features in the model's config: the training-mode forward then leaves the four feature tensors in data"


def _features(name, t, shape):
    """float32, the given shape (``None``: any extent), contiguous rows: made contiguous where it is not"""
    if t.dtype != torch.float32 or t.dim() != len(shape) or any(w is not None and w != n for w, n in zip(shape, t.shape)):
        raise ValueError(f"{name}: float32 {str(list(shape)).replace('None', '*')}, got {t.dtype} {list(t.shape)}")
    return t.contiguous()


def _pair(out, shapes, dev):
    if out is None:
        return tuple(torch.empty(s, dtype=torch.float32, device=dev) for s in shapes)
    hip.need_device([("out[0]", out[0]), ("out[1]", out[1])])
    for o, s in zip(out, shapes):
        if tuple(o.shape) != tuple(s) or o.dtype != torch.float32 or not o.is_contiguous():
            raise ValueError(f"out: float32 {list(shapes[0])} and {list(shapes[1])}, contiguous")
    return tuple(out)


def coarse_grads(feat_c0, feat_c1, gt, *, temperature, alpha=0.25, gamma=2.0, pos_weight=1.0, neg_weight=1.0, scale=1.0, out=None, stream=None):
    """``feat_c0 [B, N, 256]``, ``feat_c1 [B, M, 256]`` float32 and ``gt`` (a :class:`supervision.GroundTruth` of ``[B, N, M]``) ->
    ``(grad_c0, grad_c1)``: ``scale`` times the gradient of the focal loss.  ``temperature``: the model's
    ``coarse_matching.dual_softmax.temperature`` (the forward adds its 1e-4).  ``out``: a pair to write into."""
    hip.need_device([("feat_c0", feat_c0), ("feat_c1", feat_c1), ("gt_j", gt.gt_j), ("gt_i", gt.gt_i)])
    B, N, M = gt.shape
    feat_c0, feat_c1 = _features("feat_c0", feat_c0, (B, N, CHANNELS)), _features("feat_c1", feat_c1, (B, M, CHANNELS))
    if gt.gt_j.dtype != torch.int64 or gt.gt_i.dtype != torch.int64 or 0 in (B, N, M):
        raise ValueError("gt: int64 gt_j [B, N] and gt_i [B, M], no empty extent")
    dev = feat_c0.device
    nbytes = int(load().opbwd_coarse_workspace_bytes(B, N, M))
    if nbytes == 0:
        raise ValueError(f"[B, N, M] = {[B, N, M]}: B at most {MAX_BATCH}, N and M at most {MAX_ROWS}")
    grad0, grad1 = _pair(out, ((B, N, CHANNELS), (B, M, CHANNELS)), dev)
    gt_j, gt_i = gt.gt_j.contiguous(), gt.gt_i.contiguous()
    with hip.enqueue_on(dev, stream):
        workspace = torch.empty(nbytes, dtype=torch.uint8, device=dev)
        launch("opbwd_coarse_grads", dict(feat0=feat_c0, feat1=feat_c1, gt_j=gt_j, gt_i=gt_i, B=B, N=N, M=M, temperature=temperature, alpha=alpha,
                                          gamma=gamma, pos_weight=pos_weight, neg_weight=neg_weight, scale=scale, workspace=workspace,
                                          workspace_bytes=nbytes, grad0=grad0, grad1=grad1), stream)
    return grad0, grad1                                     # (the workspace was allocated on the stream that uses it)


def fine_grads(feat_f0, feat_f1, expec_f, expec_f_gt, *, count=None, correct_thr=1.0, training=True, scale=1.0, out=None, stream=None):
    """``feat_f0 [cap, 128]``, ``feat_f1 [cap, W * W, 128]``, ``expec_f [cap, 3]``, ``expec_f_gt [cap, 2]`` float32 with the device
    ``count`` -> ``(grad_f0, grad_f1, n_correct int32 [1], status int32 [1])``: ``scale`` times the gradient of ``supervision.fine_loss``.
    Rows at or past the count are not written.  ``status`` as :func:`supervision.fine_loss`'s; with ``NONE`` and ``EMPTY`` every written row
    is zero.  An empty table in training is a ``ValueError``, as there."""
    hip.need_tensors([("feat_f0", feat_f0), ("feat_f1", feat_f1), ("expec_f", expec_f), ("expec_f_gt", expec_f_gt)])
    cap = int(feat_f0.shape[0])
    feat_f0 = _features("feat_f0", feat_f0, (cap, FINE_CHANNELS))
    feat_f1 = _features("feat_f1", feat_f1, (cap, None, FINE_CHANNELS))
    WW = int(feat_f1.shape[1])
    W = next((w for w in range(3, 12, 2) if w * w == WW), None)
    if W is None:
        raise ValueError(f"feat_f1: [cap, W * W, {FINE_CHANNELS}] with W odd, from 3 to 11; got {WW} rows")
    expec_f, expec_f_gt = _features("expec_f", expec_f, (cap, 3)), _features("expec_f_gt", expec_f_gt, (cap, 2))
    if cap == 0 and training:
        raise ValueError("fine_grads in training needs at least one match: the reference forces row 0")
    hip.on_device([feat_f0, feat_f1, expec_f, expec_f_gt])
    dev = feat_f0.device
    grad_f0, grad_f1 = _pair(out, ((cap, FINE_CHANNELS), (cap, WW, FINE_CHANNELS)), dev)
    count = devargs.count_arg(count, dev)
    with hip.enqueue_on(dev, stream):
        n_correct, status = (torch.empty(1, dtype=torch.int32, device=dev) for _ in range(2))
        if cap == 0:                                        # eval and nothing to differentiate: no row to write, the status of an empty table
            n_correct.zero_()
            status.fill_(NONE)
            return grad_f0, grad_f1, n_correct, status
        launch("opbwd_fine_grads", dict(feat_f0=feat_f0, feat_f1=feat_f1, expec_f=expec_f, expec_f_gt=expec_f_gt, count=count, cap=cap, W=W,
                                        correct_thr=correct_thr, training=bool(training), scale=scale, grad_f0=grad_f0, grad_f1=grad_f1,
                                        n_correct=n_correct, status=status), stream)
    return grad_f0, grad_f1, n_correct, status


def backward(data, loss_config, model_config, grad=1.0, training=True):
    """The gradient of ``supervision.Loss(loss_config)(data)``'s ``data["loss"]`` times ``grad`` at the four feature tensors the
    training-mode forward leaves with ``hip_keep_features``: reads ``feat_c0`` / ``feat_c1`` / ``feat_f0`` / ``feat_f1``, the ground truth
    (as ``Loss`` finds it), ``expec_f`` and ``expec_f_gt``; writes ``data["grad_feat_c0" | "grad_feat_c1" | "grad_feat_f0" | "grad_feat_f1"]``
    (the fine pair only when ``expec_f`` is in ``data``, as ``Loss`` adds the fine term only then).  ``model_config``: the reference's, with
    the model block under ``"OnePosePlus"`` (or that block itself).  ``training``: ``Loss``'s mode; in eval a batch without a correct row
    (the ``NONE`` status) adds no fine term, and the fine gradients are zero."""
    if "mask0" in data:
        raise NotImplementedError("mask0 / mask1 loss weights (compute_c_weight): OnePose++ data never carries them")
    for key in ("feat_c0", "feat_c1") + (("feat_f0", "feat_f1") if "expec_f" in data else ()):
        if key not in data:
            raise KeyError(f"{key}: {KEEP_FEATURES_HINT}")
    if loss_config["coarse_type"] != "focal" or loss_config["fine_type"] != "l2_with_std":
        raise NotImplementedError("the reference implements coarse_type 'focal' and fine_type 'l2_with_std' only")
    block = model_config["OnePosePlus"] if "OnePosePlus" in model_config else model_config
    cfg, gt = loss_config, supervision._ground_truth_of(data)
    g0, g1 = coarse_grads(data["feat_c0"], data["feat_c1"], gt, temperature=block["coarse_matching"]["dual_softmax"]["temperature"],
                          alpha=cfg["focal_alpha"], gamma=cfg["focal_gamma"], pos_weight=cfg["pos_weight"], neg_weight=cfg["neg_weight"],
                          scale=float(cfg["coarse_weight"]) * float(grad))
    data.update({"grad_feat_c0": g0, "grad_feat_c1": g1})
    if "expec_f" in data:
        rows = int(data["expec_f"].shape[0])                # the forward's K rows of the kept capacity
        f0, f1, _, _ = fine_grads(data["feat_f0"][:rows], data["feat_f1"][:rows], data["expec_f"], data["expec_f_gt"],
                                  correct_thr=cfg["fine_correct_thr"], training=training, scale=float(cfg["fine_weight"]) * float(grad))
        data.update({"grad_feat_f0": f0, "grad_feat_f1": f1})


class stages:
    """The two entries one by one (device tensors in, device tensors out): what :func:`backward` enqueues"""
    coarse_grads = staticmethod(coarse_grads)
    fine_grads = staticmethod(fine_grads)
