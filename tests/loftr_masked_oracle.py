"""CPU oracle of the LoFTR matcher's coarse path with padding masks (``mask0`` / ``mask1``, inference), restated from the published
zju3dv/LoFTR definition (``loftr/loftr_module/transformer.py`` with masks, ``linear_attention.py`` q_mask / kv_mask,
``utils/coarse_matching.py`` masked_fill and ``mask_border_with_padding``).  Parity with the reference stays unpinned, as for the rest of
the matcher (``oracle/loftr_oracle.py``).

Builds on ``oracle/loftr_oracle.py`` and ``tests/loftr_sinkhorn_oracle.py`` by importing them; neither is edited.  With no masks every
function here reduces to those oracles.  Masks are ``[B, h, w]`` booleans at coarse resolution, ``True`` = a real cell.
"""
from __future__ import annotations

import torch
import torch.nn.functional as F

from oracle import loftr_oracle as lo
from oracle import onepose_oracle as orc
from tests import loftr_sinkhorn_oracle as lso


def masked_layer(sd, p, x, source, x_mask=None, source_mask=None, nhead=8):
    """one ``LoFTREncoderLayer`` (linear attention): Q = phi(q) * q_mask, K = phi(k) * kv_mask, V = v * kv_mask, v_length = padded S;
    masks ``[B, L]`` / ``[B, S]`` (bool or None)"""
    cast = lambda m: None if m is None else m.to(x.dtype)
    return orc.encoder_layer(sd, p, x, source, nhead, x_mask=cast(x_mask), source_mask=cast(source_mask))


def transformer_two_images(sd, prefix, layer_names, nhead, feat0, feat1, mask0=None, mask1=None):
    """``LocalFeatureTransformer.forward(feat0, feat1, mask0, mask1)``: self -> ``layer(f, f, m, m)`` per image; cross ->
    ``f0 = layer(f0, f1, m0, m1)``, then ``f1 = layer(f1, f0_new, m1, m0)``.  Masks flattened ``[B, L]`` or None."""
    if mask0 is None and mask1 is None:
        return lo.transformer_two_images(sd, prefix, layer_names, nhead, feat0, feat1)
    for i, name in enumerate(layer_names):
        p = f"{prefix}.layers.{i}."
        if name == "self":
            feat0 = masked_layer(sd, p, feat0, feat0, mask0, mask0, nhead)
            feat1 = masked_layer(sd, p, feat1, feat1, mask1, mask1, nhead)
        elif name == "cross":
            feat0 = masked_layer(sd, p, feat0, feat1, mask0, mask1, nhead)
            feat1 = masked_layer(sd, p, feat1, feat0, mask1, mask0, nhead)
        else:
            raise KeyError(name)
    return feat0, feat1


def fill(sim, mask0, mask1):
    """``sim.masked_fill_(~(mask0[..., None] * mask1[:, None]), -1e9)`` on a copy; masks ``[B, h, w]`` or None"""
    if mask0 is None:
        return sim
    valid = mask0.flatten(-2)[:, :, None] & mask1.flatten(-2)[:, None, :]
    return sim.masked_fill(~valid, -1e9)


def mask_border_with_padding(m, bd, v, p_m0, p_m1):
    """``utils/coarse_matching.py`` ``mask_border_with_padding``, literally: ``m [B, h0, w0, h1, w1]`` in place"""
    if bd <= 0:
        return
    m[:, :bd] = v
    m[:, :, :bd] = v
    m[:, :, :, :bd] = v
    m[:, :, :, :, :bd] = v
    h0s, w0s = p_m0.sum(1).max(-1)[0].int(), p_m0.sum(-1).max(-1)[0].int()
    h1s, w1s = p_m1.sum(1).max(-1)[0].int(), p_m1.sum(-1).max(-1)[0].int()
    for b_idx, (h0, w0, h1, w1) in enumerate(zip(h0s, w0s, h1s, w1s)):
        m[b_idx, h0 - bd:] = v
        m[b_idx, :, w0 - bd:] = v
        m[b_idx, :, :, h1 - bd:] = v
        m[b_idx, :, :, :, w1 - bd:] = v


def get_coarse_match(conf, hw0_c, hw1_c, hw0_i, thr, border_rm, mask0=None, mask1=None) -> dict:
    """``get_coarse_match`` (inference): threshold, ``mask_border_with_padding`` when masks are given (else the all-sides border),
    mutual nearest, first true j"""
    if mask0 is None:
        return lso.get_coarse_match(conf, hw0_c, hw1_c, hw0_i, thr, border_rm)
    B = conf.shape[0]
    h0, w0 = hw0_c
    h1, w1 = hw1_c
    mask = (conf > thr).view(B, h0, w0, h1, w1).clone()
    mask_border_with_padding(mask, border_rm, False, mask0, mask1)
    mask = mask.view(B, h0 * w0, h1 * w1)
    mask = mask * (conf == conf.max(dim=2, keepdim=True)[0]) * (conf == conf.max(dim=1, keepdim=True)[0])
    mask_v, all_j = mask.max(dim=2)
    b_ids, i_ids = torch.where(mask_v)
    j_ids = all_j[b_ids, i_ids]
    mconf = conf[b_ids, i_ids, j_ids]
    scale = hw0_i[0] / h0
    mk0 = torch.stack([i_ids % w0, i_ids // w0], dim=1).float() * scale
    mk1 = torch.stack([j_ids % w1, j_ids // w1], dim=1).float() * scale
    return {"conf_matrix": conf, "b_ids": b_ids, "i_ids": i_ids, "j_ids": j_ids, "mconf": mconf, "mkpts0_c": mk0, "mkpts1_c": mk1}


def dual_softmax_conf(feat_c0, feat_c1, temperature, mask0=None, mask1=None):
    C = feat_c0.shape[-1]
    f0, f1 = feat_c0 / C ** 0.5, feat_c1 / C ** 0.5
    sim = fill(torch.einsum("nlc,nsc->nls", f0, f1) / temperature, mask0, mask1)
    return F.softmax(sim, 1) * F.softmax(sim, 2)


def sinkhorn_conf(feat_c0, feat_c1, bin_score, iters, prefilter, mask0=None, mask1=None, dtype=torch.float64):
    """``tests/loftr_sinkhorn_oracle.sinkhorn_conf`` with the fill before the unchanged transport (padded m and n in its marginals)"""
    C = feat_c0.shape[-1]
    f0, f1 = feat_c0.to(dtype) / C ** 0.5, feat_c1.to(dtype) / C ** 0.5
    sim = fill(torch.einsum("nlc,nsc->nls", f0, f1), mask0, mask1)
    assign = lso.log_optimal_transport(sim, bin_score, iters).exp()
    conf = assign[:, :-1, :-1].clone()
    L, S = sim.shape[1:]
    filter0 = (assign.argmax(dim=2) == S)[:, :-1]
    filter1 = (assign.argmax(dim=1) == L)[:, :-1]
    if prefilter:
        conf[filter0[..., None].repeat(1, 1, S)] = 0
        conf[filter1[:, None].repeat(1, L, 1)] = 0
    return conf, assign


def coarse_matching(feat_c0, feat_c1, hw0_c, hw1_c, hw0_i, cfg, mask0=None, mask1=None, bin_score=None) -> dict:
    """``CoarseMatching.forward`` + ``get_coarse_match`` with masks, either match type (``bin_score`` for sinkhorn)"""
    if cfg["match_type"] == "sinkhorn":
        conf, _ = sinkhorn_conf(feat_c0, feat_c1, bin_score, cfg["skh_iters"], cfg["skh_prefilter"], mask0, mask1)
        conf = conf.to(feat_c0.dtype)
    else:
        conf = dual_softmax_conf(feat_c0, feat_c1, cfg["dsmax_temperature"], mask0, mask1)
    return get_coarse_match(conf, hw0_c, hw1_c, hw0_i, cfg["thr"], cfg["border_rm"], mask0, mask1)


def forward_from_features(sd, cfg, f0, ff0, f1, ff1, hw0_i, mask0=None, mask1=None, fine=True) -> dict:
    """the matcher from the backbone-output boundary: coarse rows ``f0 [V, L0, 256]`` (positional encoding added), fine maps
    ``ff0 [V, 128, hf, wf]``; ``f1`` / ``ff1`` / ``mask1`` may have batch 1 (one query for every pair).  Masks ``[V or 1, h, w]``."""
    V = f0.shape[0]
    hw0_c, hw1_c = (ff0.shape[2] // 4, ff0.shape[3] // 4), (ff1.shape[2] // 4, ff1.shape[3] // 4)
    hw0_f = tuple(ff0.shape[2:])
    rep = lambda t: None if t is None else (t.expand(V, *t.shape[1:]) if t.shape[0] == 1 and V > 1 else t)
    f1, ff1, mask1 = rep(f1), rep(ff1), rep(mask1)
    flat = lambda m: None if m is None else m.flatten(-2)
    f0, f1 = transformer_two_images(sd, "loftr_coarse", cfg["coarse"]["layer_names"], cfg["coarse"]["nhead"], f0, f1, flat(mask0), flat(mask1))
    out = {"feat_c0": f0, "feat_c1": f1, "hw0_c": hw0_c, "hw1_c": hw1_c}
    bin_score = float(sd["coarse_matching.bin_score"]) if cfg["match_coarse"]["match_type"] == "sinkhorn" else None
    out.update(coarse_matching(f0, f1, hw0_c, hw1_c, hw0_i, cfg["match_coarse"], mask0, mask1, bin_score))
    if not fine:
        return out
    W = cfg["fine_window_size"]
    w0 = lo.fine_windows(ff0, out["b_ids"], out["i_ids"], hw0_c, W)
    w1 = lo.fine_windows(ff1, out["b_ids"], out["j_ids"], hw1_c, W)
    if w0.size(0) != 0:
        w0, w1 = lo.transformer_two_images(sd, "loftr_fine", cfg["fine"]["layer_names"], cfg["fine"]["nhead"], w0, w1)
    out["fine_f0"], out["fine_f1"] = w0, w1
    out.update(lo.fine_matching(w0, w1, out["mkpts0_c"], out["mkpts1_c"], hw0_i, hw0_f))
    return out


def loftr_forward(sd, cfg, image0, image1, mask0=None, mask1=None) -> dict:
    """the matcher from the images (backbone, positional encoding, then ``forward_from_features``)"""
    fc0, ff0 = orc.backbone_8_2(sd, image0)
    fc1, ff1 = orc.backbone_8_2(sd, image1)
    pe = orc.position_table(cfg["coarse"]["d_model"])
    f0, f1 = orc.pe_add_flatten(fc0, pe), orc.pe_add_flatten(fc1, pe)
    return forward_from_features(sd, cfg, f0, ff0, f1, ff1, tuple(image0.shape[2:]), mask0, mask1)
