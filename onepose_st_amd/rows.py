"""One transformer encoder layer composed from the row kernels (``ophip_rows_linear_x3``, ``ophip_rows_layernorm128``): what the
full-attention fine stage of ``OnePosePlus_model`` and the fine stage of ``LoFTR_for_OnePose_Plus`` run, on the current stream.  The two
differ in the attention launch only, which the caller passes in; ``w`` is one layer's dictionary of ``packing.pack_fine_layer_full_x3``."""
from __future__ import annotations

import torch

from . import hip


def rows_linear(x, rows, w, nout, xb=None, relu=False):
    """``y [rows, nout] = [x | xb] W^T`` (split-bf16, optional ReLU) over the first ``rows`` rows of ``x`` (and ``xb``)"""
    y = torch.empty(rows, nout, device=x.device, dtype=torch.float32)
    hip.launch("ophip_rows_linear_x3", dict(xa=x, ka=x.shape[-1], xb=xb, kb=xb.shape[-1] if xb is not None else 0, T=rows, wpack=w, nout=nout,
                                            relu=1 if relu else 0, y=y))
    return y


def rows_encoder_layer(x, rows_x, src, rows_src, w, attention):
    """``LoFTREncoderLayer`` (transformer.py:65-94) on ``rows_x`` query rows ``x`` and ``rows_src`` source rows ``src`` of 128 channels;
    ``attention(q, k, v, msg)`` is the caller's one launch that fills ``msg [rows_x, 128]``.  Returns new rows shaped like ``x``."""
    q, k, v = rows_linear(x, rows_x, w["q"], 128), rows_linear(src, rows_src, w["k"], 128), rows_linear(src, rows_src, w["v"], 128)
    msg = torch.empty(rows_x, 128, device=x.device, dtype=torch.float32)
    attention(q, k, v, msg)
    m = rows_linear(msg, rows_x, w["m"], 128)
    hip.launch("ophip_rows_layernorm128", dict(x=m, gamma=w["norm1_weight"], beta=w["norm1_bias"], residual=None, T=rows_x, y=m))
    h = rows_linear(x, rows_x, w["w0"], 256, xb=m, relu=True)
    o = rows_linear(h, rows_x, w["w2"], 128)
    y = torch.empty_like(x)
    hip.launch("ophip_rows_layernorm128", dict(x=o, gamma=w["norm2_weight"], beta=w["norm2_bias"], residual=x, T=rows_x, y=y))
    return y
