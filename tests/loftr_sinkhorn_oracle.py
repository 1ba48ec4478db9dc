"""CPU oracle of LoFTR's optimal-transport coarse matching (``CoarseMatching`` with ``match_type: "sinkhorn"``, inference), restated from
the published zju3dv/LoFTR sinkhorn branch and SuperGlue's ``log_optimal_transport``, in float64 unless given another dtype.

``loftr_forward`` runs ``tests/loftr_full_oracle.loftr_forward`` (attention form per encoder) with ``oracle.loftr_oracle.coarse_matching``
swapped for the sinkhorn form inside a scoped, restored override; ``bin_score`` is the state_dict's ``coarse_matching.bin_score``.  The
oracle modules themselves are not edited.
"""
from __future__ import annotations

import torch

from oracle import loftr_oracle as lo
from tests import loftr_full_oracle as lfo


def log_optimal_transport(scores, alpha, iters):
    """SuperGlue's form: scores [b, m, n], alpha 0-d -> log assignment [b, m + 1, n + 1] (multiplied by m + n)"""
    b, m, n = scores.shape
    one = scores.new_tensor(1)
    ms, ns = (m * one).to(scores), (n * one).to(scores)
    alpha = torch.as_tensor(alpha).to(scores)
    bins0, bins1, a = alpha.expand(b, m, 1), alpha.expand(b, 1, n), alpha.expand(b, 1, 1)
    Z = torch.cat([torch.cat([scores, bins0], -1), torch.cat([bins1, a], -1)], 1)
    norm = -(ms + ns).log()
    log_mu = torch.cat([norm.expand(m), ns.log()[None] + norm])[None].expand(b, -1)
    log_nu = torch.cat([norm.expand(n), ms.log()[None] + norm])[None].expand(b, -1)
    u, v = torch.zeros_like(log_mu), torch.zeros_like(log_nu)
    for _ in range(iters):
        u = log_mu - torch.logsumexp(Z + v.unsqueeze(1), dim=2)
        v = log_nu - torch.logsumexp(Z + u.unsqueeze(2), dim=1)
    return Z + u.unsqueeze(2) + v.unsqueeze(1) - norm


def sinkhorn_conf(feat_c0, feat_c1, bin_score, iters, prefilter, dtype=torch.float64):
    """-> (conf_matrix [b, L, S], assign [b, L + 1, S + 1], filter0 [b, L], filter1 [b, S])"""
    C = feat_c0.shape[-1]
    f0, f1 = feat_c0.to(dtype) / C ** 0.5, feat_c1.to(dtype) / C ** 0.5
    sim = torch.einsum("nlc,nsc->nls", f0, f1)
    assign = log_optimal_transport(sim, bin_score, iters).exp()
    conf = assign[:, :-1, :-1].clone()
    L, S = sim.shape[1:]
    filter0 = (assign.argmax(dim=2) == S)[:, :-1]
    filter1 = (assign.argmax(dim=1) == L)[:, :-1]
    if prefilter:
        conf[filter0[..., None].repeat(1, 1, S)] = 0
        conf[filter1[:, None].repeat(1, L, 1)] = 0
    return conf, assign, filter0, filter1


def get_coarse_match(conf, hw0_c, hw1_c, hw0_i, thr, border_rm) -> dict:
    """LoFTR ``get_coarse_match`` (inference) on a given conf_matrix: threshold, border on all sides, mutual nearest, first true j"""
    B = conf.shape[0]
    h0, w0 = hw0_c
    h1, w1 = hw1_c
    mask = (conf > thr).view(B, h0, w0, h1, w1).clone()
    b = border_rm
    if b > 0:
        mask[:, :b] = False
        mask[:, :, :b] = False
        mask[:, :, :, :b] = False
        mask[:, :, :, :, :b] = False
        mask[:, -b:] = False
        mask[:, :, -b:] = False
        mask[:, :, :, -b:] = False
        mask[:, :, :, :, -b:] = False
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


def coarse_matching(feat_c0, feat_c1, hw0_c, hw1_c, hw0_i, cfg, bin_score, dtype=torch.float64) -> dict:
    conf, _, _, _ = sinkhorn_conf(feat_c0, feat_c1, bin_score, cfg["skh_iters"], cfg["skh_prefilter"], dtype)
    return get_coarse_match(conf.to(feat_c0.dtype), hw0_c, hw1_c, hw0_i, cfg["thr"], cfg["border_rm"])


def loftr_forward(sd: dict, cfg: dict, image0, image1, feature_hook=None) -> dict:
    """the matcher with ``cfg["match_coarse"]["match_type"] == "sinkhorn"`` (and the attention form of each encoder from ``cfg``)"""
    assert cfg["match_coarse"]["match_type"] == "sinkhorn"
    bin_score = float(sd["coarse_matching.bin_score"])
    inner = lo.coarse_matching
    lo.coarse_matching = lambda f0, f1, hw0_c, hw1_c, hw0_i, mc: coarse_matching(f0, f1, hw0_c, hw1_c, hw0_i, mc, bin_score)
    try:
        return lfo.loftr_forward(sd, cfg, image0, image1, feature_hook=feature_hook)
    finally:
        lo.coarse_matching = inner
