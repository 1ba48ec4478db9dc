"""CPU oracle of the encoders' FULL (softmax) attention: ``loftr_module/linear_attention.py:64-95`` (``FullAttention``), and
``forward_from_features`` of ``oracle/onepose_oracle.py`` with the attention form chosen per encoder (``transformer.py:29-38``).

``onepose_oracle.encoder_layer`` reads ``linear_attention`` as a module global, so each encoder's call runs under a scoped swap of that
global; the oracle module itself is not edited.
"""
from __future__ import annotations

import contextlib

import torch

from oracle import onepose_oracle as orc


def full_attention(q: torch.Tensor, k: torch.Tensor, v: torch.Tensor, q_mask: torch.Tensor | None = None,
                   kv_mask: torch.Tensor | None = None, **_unused) -> torch.Tensor:
    """``FullAttention.forward``: q ``[N,L,H,D]``, k, v ``[N,S,H,D]``; softmax(Q K^T / sqrt(D)) V, no eps, no v_length scaling.
    With a ``kv_mask`` the reference evaluates ``q_mask[:, :, None, None]`` whatever ``q_mask`` is (``:85``): a None ``q_mask``
    raises ``TypeError`` there, as it does here."""
    QK = torch.einsum("nlhd,nshd->nlsh", q, k)
    if kv_mask is not None:
        QK.masked_fill_(~(q_mask[:, :, None, None] * kv_mask[:, None, :, None]), float("-inf"))
    softmax_temp = 1.0 / q.size(3) ** 0.5
    A = torch.softmax(softmax_temp * QK, dim=2)
    return torch.einsum("nlsh,nshd->nlhd", A, v).contiguous()


@contextlib.contextmanager
def attention_form(form: str):
    """Within the block, ``onepose_oracle.encoder_layer`` uses ``form`` ("linear" or "full")."""
    if form not in ("linear", "full"):
        raise ValueError(form)
    saved = orc.linear_attention
    if form == "full":
        orc.linear_attention = full_attention
    try:
        yield
    finally:
        orc.linear_attention = saved


def encoder_layer(sd, p, x, source, nhead, form="full", x_mask=None, source_mask=None):
    """One ``LoFTREncoderLayer`` with the given attention form."""
    with attention_form(form):
        return orc.encoder_layer(sd, p, x, source, nhead, x_mask=x_mask, source_mask=source_mask)


def forward_from_features(sd: dict, cfg: dict, data: dict, feat_c, feat_f, image_hw, trace: dict | None = None) -> dict:
    """``onepose_oracle.forward_from_features`` with ``cfg["loftr_coarse"]["attention"]`` and ``cfg["loftr_fine"]["attention"]``
    honoured per encoder."""
    forms = {"loftr_coarse": cfg["loftr_coarse"]["attention"], "loftr_fine": cfg["loftr_fine"]["attention"]}
    inner = orc.feature_transformer

    def per_encoder(sd_, prefix, *args, **kwargs):
        with attention_form(forms[prefix]):
            return inner(sd_, prefix, *args, **kwargs)

    orc.feature_transformer = per_encoder
    try:
        return orc.forward_from_features(sd, cfg, data, feat_c, feat_f, image_hw, trace)
    finally:
        orc.feature_transformer = inner
