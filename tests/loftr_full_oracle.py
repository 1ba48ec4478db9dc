"""CPU oracle of the LoFTR matcher with the attention form chosen per encoder: ``oracle/loftr_oracle.loftr_forward`` with
``cfg["coarse"]["attention"]`` and ``cfg["fine"]["attention"]`` honoured (``"linear"`` or ``"full"``, the reference config's options).

``loftr_oracle.transformer_two_images`` runs ``onepose_oracle.encoder_layer``, which reads ``linear_attention`` as a module global: each
encoder's call runs under the scoped swap of ``tests/full_attention_oracle.attention_form``.  The oracle modules themselves are not edited.
"""
from __future__ import annotations

from oracle import loftr_oracle as lo
from tests.full_attention_oracle import attention_form, full_attention  # noqa: F401  (re-exported for the tests)


def loftr_forward(sd: dict, cfg: dict, image0, image1, feature_hook=None) -> dict:
    """``lo.loftr_forward`` with the attention form of each encoder taken from ``cfg``."""
    forms = {"loftr_coarse": cfg["coarse"]["attention"], "loftr_fine": cfg["fine"]["attention"]}
    inner = lo.transformer_two_images

    def per_encoder(sd_, prefix, *args, **kwargs):
        with attention_form(forms[prefix]):
            return inner(sd_, prefix, *args, **kwargs)

    lo.transformer_two_images = per_encoder
    try:
        return lo.loftr_forward(sd, cfg, image0, image1, feature_hook=feature_hook)
    finally:
        lo.transformer_two_images = inner


def encoder_layer(sd, p, x, source, form="full"):
    """One coarse ``LoFTREncoderLayer`` (8 heads) with the given attention form."""
    with attention_form(form):
        return lo.orc.encoder_layer(sd, p, x, source, 8)
