"""The coarse context of the LoFTR matcher's fine windows (``fine_concat_coarse_feat``; csrc/fine_context.hip, ``opfcx_merge``): reference,
stand-in, seeded faults, cases, bar and the whole-matcher oracle shared by tests/test_loftr_fine_context_cpu.py and
tests/test_gpu_loftr_fine_context.py.

Specification (the published ``FinePreprocess`` of zju3dv/LoFTR, ``loftr_module/fine_preprocess.py``, restated; parity unpinned as for the
rest of this matcher).  With ``down_proj = Linear(256, 128)`` (Wd, bd) and ``merge_feat = Linear(256, 128)`` (Wm, bm), for match ``k`` with
cell ``id_k`` of image ``b_k`` and window row ``r``:

    c_k        = Wd . x[b_k, id_k] + bd
    win'[k, r] = Wm . cat[win[k, r], c_k] + bm                     (the fine half first)
               = Wm[:, :128] . win[k, r] + u_k,    u_k = Wm[:, 128:] . c_k + bm

Reference = :func:`reference` (the factored form) in float64, nothing rounded; :func:`reference_published` is the unfactored form beside it
(the two agree to float64 rounding).  No rounding-faithful reference: the split keeps 16 mantissa bits, so the un-rounded value is the truth
(tests/x3_faithful.py).

Stand-in = :func:`standin`: the factored form in float32 with ``bf16_faithful``'s split (hi + lo, lo . lo dropped: ``x3_faithful.mm3``) at
the kernel's three operand points -- the coarse rows and Wd; c (with bd added in f32) and Wm[:, 128:]; the window rows and Wm[:, :128] -- and
the biases and u added in f32.  It is never compared with a device: it sizes the bar.  What the device has and the stand-in lacks is
another association of the f32 sums; the factor of two is for that.

Statistic: ``|y - y_ref| / max(1, max |y_ref row|)``, worst element (:func:`row_error`).  ``ROWS_BAR`` = twice the stand-in's worst value
over ``CASES``, measured on the CPU (tests/test_loftr_fine_context_cpu.py re-derives the figure).  Nothing here comes from a device.
"""
from __future__ import annotations

import torch
import torch.nn.functional as F

from oracle import loftr_oracle as lo
from tests import x3_faithful as x3

f32, f64 = torch.float32, torch.float64
CF, CC, TILE = 128, 256, 64                   # fine and coarse features; rows of one workgroup (OPFCX_TILE_ROWS)
PREFIX = "fine_preprocess."

ROWS_STANDIN = 1.11e-5                        # measured 1.105e-05 (case w5_k300, image 0); the other cases 7.3e-06 .. 9.8e-06
ROWS_BAR = 2 * ROWS_STANDIN

# every seeded fault (a kernel that ...): each lies outside the bar on FAULT_CASE
FAULTS = ["halves", "ij", "no_bd", "no_bm", "per_tile"]
FAULT_CASE = "w5_k3"


def _w(sd, dtype):
    g = lambda n: sd[PREFIX + n].detach().to(dtype)
    return g("down_proj.weight"), g("down_proj.bias"), g("merge_feat.weight"), g("merge_feat.bias")


def reference(sd, win, x, b_ids, ids, dtype=f64):
    """``win [K, WW, 128]``, coarse rows ``x [B, L, 256]`` (batch 1: one image for every match), the matches' ``b_ids`` and cells ``ids``
    -> ``win' [K, WW, 128]``, the factored form in ``dtype``"""
    wd, bd, wm, bm = _w(sd, dtype)
    rows = x.to(dtype)[b_ids if x.shape[0] > 1 else torch.zeros_like(b_ids), ids]
    u = (rows @ wd.T + bd) @ wm[:, CF:].T + bm
    return win.to(dtype) @ wm[:, :CF].T + u[:, None, :]


def reference_published(sd, win, x, b_ids, ids, dtype=f64):
    """the published statement: ``merge_feat(cat[win, repeat(down_proj(x[b_ids, ids]), WW)])``"""
    wd, bd, wm, bm = _w(sd, dtype)
    rows = x.to(dtype)[b_ids if x.shape[0] > 1 else torch.zeros_like(b_ids), ids]
    c = F.linear(rows, wd, bd)
    return F.linear(torch.cat([win.to(dtype), c[:, None, :].expand(-1, win.shape[1], -1)], -1), wm, bm)


def standin(sd, win, x, b_ids, ids, dtype=f32, wrong=None):
    """The kernel's arithmetic in ``dtype`` (see the module text).  ``wrong``: one of FAULTS ("ij" is made by the caller, who hands over the
    other image's cells)"""
    wd, bd, wm, bm = _w(sd, f32)
    ww, wc = (wm[:, CF:], wm[:, :CF]) if wrong == "halves" else (wm[:, :CF], wm[:, CF:])
    rows = x.to(f32)[b_ids if x.shape[0] > 1 else torch.zeros_like(b_ids), ids]
    c = x3.mm3(rows, wd, dtype)
    if wrong != "no_bd":
        c = c + bd.to(dtype)
    u = x3.mm3(c, wc, dtype)
    if wrong != "no_bm":
        u = u + bm.to(dtype)
    K, WW = win.shape[:2]
    y = x3.mm3(win.reshape(K * WW, CF), ww, dtype)
    match = torch.arange(K * WW) // WW
    if wrong == "per_tile":                   # the context of the tile's first row for all 64 rows
        match = match[(torch.arange(K * WW) // TILE) * TILE]
    return (y + u[match]).view(K, WW, CF)


def row_error(y, ref) -> float:
    """``|y - y_ref| / max(1, max |y_ref row|)``, worst element"""
    y, ref = torch.as_tensor(y).detach().cpu().to(f64), torch.as_tensor(ref).detach().cpu().to(f64)
    if ref.numel() == 0:
        return 0.0
    scale = torch.clamp(ref.abs().amax(dim=-1, keepdim=True), min=1.0)
    return float(((y - ref).abs() / scale).max())


# ---- cases: name -> (W, K, B, L0, L1, image 1 shared, what the first matches are set to) ----------------------------------------------
# Tile edges of the 64-row workgroup: W 3 with 63 and 72 rows (one tile; one tile and 8 rows), W 5 with 75 rows (match 2 lies across the
# edge) and 7500 rows (118 tiles, every phase of a match against a tile), W 9 and W 11 with one match (81 and 121 rows: two tiles).
CASES = {
    "w3_k7": (3, 7, 1, 30, 40, False), "w3_k8": (3, 8, 1, 30, 40, False), "w5_k3": (5, 3, 1, 30, 40, False),
    "w5_k300": (5, 300, 1, 192, 192, False), "w9_k1": (9, 1, 1, 30, 40, False), "w11_k1": (11, 1, 1, 30, 40, False),
    "batch3": (5, 9, 3, 30, 40, False),       # three images, matches on images 0 and 2 only
    "stride0": (5, 9, 3, 30, 40, True),       # image 1 is one image for every match (batch stride 0)
    "edge_cells": (5, 4, 2, 30, 40, False),   # cells 0 and L - 1 of the first and the last image
}


def make_case(name):
    """-> dict(W, K, B, win0, win1 [K, WW, 128], x0 [B, L0, 256], x1 [B or 1, L1, 256], b_ids, i_ids, j_ids); seeded by the name"""
    W, K, B, L0, L1, shared = CASES[name]
    g = torch.Generator().manual_seed(sum(map(ord, name)))
    win0, win1 = torch.randn(K, W * W, CF, generator=g), torch.randn(K, W * W, CF, generator=g)
    x0, x1 = torch.randn(B, L0, CC, generator=g), torch.randn(1 if shared else B, L1, CC, generator=g)
    b_ids = torch.sort(torch.randint(0, B, (K,), generator=g))[0]
    i_ids, j_ids = torch.randint(0, L0, (K,), generator=g), torch.randint(0, L1, (K,), generator=g)
    if name in ("batch3", "stride0"):
        b_ids = torch.tensor([0] * 4 + [2] * (K - 4))
    if name == "edge_cells":
        b_ids = torch.tensor([0, 0, B - 1, B - 1])
        i_ids, j_ids = torch.tensor([0, L0 - 1, 0, L0 - 1]), torch.tensor([L1 - 1, 0, L1 - 1, 0])
    same = i_ids == j_ids                     # the "ij" fault needs two different cells
    j_ids[same] = (j_ids[same] + 1) % L1
    return dict(W=W, K=K, B=B, win0=win0, win1=win1, x0=x0, x1=x1, b_ids=b_ids, i_ids=i_ids, j_ids=j_ids)


def both_images(fn, sd, case, **kw):
    """``fn`` (reference / standin) on image 0 and image 1 of a case -> (win0', win1')"""
    return (fn(sd, case["win0"], case["x0"], case["b_ids"], case["i_ids"], **kw),
            fn(sd, case["win1"], case["x1"], case["b_ids"], case["j_ids"], **kw))


def standin_worst(sd) -> float:
    """the stand-in's worst :func:`row_error` over CASES: what ROWS_STANDIN records"""
    worst = 0.0
    for name in CASES:
        case = make_case(name)
        for y, ref in zip(both_images(standin, sd, case), both_images(reference, sd, case)):
            worst = max(worst, row_error(y, ref))
    return worst


# ---- the whole matcher with the switch, from the backbone-output boundary ---------------------------------------------------------------
def forward_from_features(sd, cfg, f0, ff0, f1, ff1, hw0_i) -> dict:
    """``LoFTR_for_OnePose_Plus.forward`` with ``fine_concat_coarse_feat`` from the backbone-output boundary, composed from the pieces of
    ``oracle/loftr_oracle.py`` (float32, as that oracle): coarse rows ``f0 [V, L0, 256]`` (positional encoding added), fine maps
    ``ff0 [V, 128, hf, wf]``; ``f1`` / ``ff1`` may have batch 1 (one query for every pair).  Also returns the merged windows
    ``fine_in0`` / ``fine_in1`` the fine transformer reads."""
    V = f0.shape[0]
    rep = lambda t: t.expand(V, *t.shape[1:]) if t.shape[0] == 1 and V > 1 else t
    f1, ff1 = rep(f1), rep(ff1)
    hw0_c, hw1_c = (ff0.shape[2] // 4, ff0.shape[3] // 4), (ff1.shape[2] // 4, ff1.shape[3] // 4)
    f0, f1 = lo.transformer_two_images(sd, "loftr_coarse", cfg["coarse"]["layer_names"], cfg["coarse"]["nhead"], f0, f1)
    out = {"feat_c0": f0, "feat_c1": f1, "hw0_c": hw0_c, "hw1_c": hw1_c}
    out.update(lo.coarse_matching(f0, f1, hw0_c, hw1_c, hw0_i, cfg["match_coarse"]))
    W = cfg["fine_window_size"]
    w0 = lo.fine_windows(ff0, out["b_ids"], out["i_ids"], hw0_c, W)
    w1 = lo.fine_windows(ff1, out["b_ids"], out["j_ids"], hw1_c, W)
    out["windows0"], out["windows1"] = w0, w1
    if w0.size(0) != 0:
        w0 = reference_published(sd, w0, f0, out["b_ids"], out["i_ids"], f32)
        w1 = reference_published(sd, w1, f1, out["b_ids"], out["j_ids"], f32)
        out["fine_in0"], out["fine_in1"] = w0, w1
        w0, w1 = lo.transformer_two_images(sd, "loftr_fine", cfg["fine"]["layer_names"], cfg["fine"]["nhead"], w0, w1)
    out["fine_f0"], out["fine_f1"] = w0, w1
    out.update(lo.fine_matching(w0, w1, out["mkpts0_c"], out["mkpts1_c"], hw0_i, tuple(ff0.shape[2:])))
    return out
