"""Parameter holders and the checkpoint loader that ``OnePosePlus_model`` and ``LoFTR_for_OnePose_Plus`` share.  The ``nn`` modules only
*hold parameters* under the reference's ``state_dict`` names (``packing.py`` reads those names); the arithmetic runs in the HIP kernels."""
from __future__ import annotations

import torch.nn as nn


class EncoderLayerParams(nn.Module):
    """Parameter holder with the key layout of ``LoFTREncoderLayer`` (transformer.py:29-52)."""

    def __init__(self, d):
        super().__init__()
        self.q_proj = nn.Linear(d, d, bias=False)
        self.k_proj = nn.Linear(d, d, bias=False)
        self.v_proj = nn.Linear(d, d, bias=False)
        self.merge = nn.Linear(d, d, bias=False)
        self.mlp = nn.Sequential(nn.Linear(2 * d, 2 * d, bias=False), nn.Identity(), nn.Linear(2 * d, d, bias=False))
        self.norm1 = nn.LayerNorm(d)
        self.norm2 = nn.LayerNorm(d)


class EncoderParams(nn.Module):
    """``LocalFeatureTransformer`` parameter holder (transformer.py:100-131)."""

    def __init__(self, layer_names, d_model, nhead):
        super().__init__()
        self.layer_names = list(layer_names)
        self.d_model, self.nhead = d_model, nhead
        self.layers = nn.ModuleList([EncoderLayerParams(d_model) for _ in self.layer_names])
        for p in self.parameters():
            if p.dim() > 1:
                nn.init.xavier_uniform_(p)


def load_matcher_checkpoint(model, state_dict):
    """What every ``build_*model`` of the reference does with a checkpoint's ``state_dict``: strip the ``matcher.`` prefix, load
    strictly, ``eval()``.  Returns ``model``."""
    model.load_state_dict({k.replace("matcher.", ""): v for k, v in state_dict.items()}, strict=True)
    return model.eval()
