"""The backward of the coarse transformer on the device (opt-in): from ``grad_feat_c0`` / ``grad_feat_c1`` -- what
``loss_backward.backward`` writes -- through the six ``LoFTREncoderLayer``s with linear attention (``loftr_module/transformer.py:65-94``,
``linear_attention.py:29-61``) to the gradients at the transformer's two inputs (the keypoint-encoded 3D rows and the position-encoded 2D rows)
and at all of its parameters.

The specification is ``include/ext/onepose_encoder_backward.h`` (``tests/encoder_backward_oracle.py`` restates it in numpy float64).  One C
entry differentiates one layer call: it takes the layer's inputs, recomputes the forward, and writes ``dx``, ``dsource`` and the flat
parameter gradient; every matrix product is a split-bf16 MFMA and every sum over rows has a fixed order, so two runs give identical bytes.
:func:`coarse_backward` chains it over the layers in Python from the layer inputs the training-mode forward keeps with
``hip_keep_layer_inputs``.

Not here: ``x_mask`` / ``source_mask``, full attention, the fine transformer, the window gather, the keypoint encoder, the position encoding
and the backbone, an optimiser or an ``autograd.Function``.  Nothing sets a ``.grad``.

The kernels are HIP (``csrc/encoder_backward.hip`` in ``libonepose_encoder_backward.so``, the row of ``cabi.ENCODER_BACKWARD``).  CPU tensors
raise :class:`hip.HipLibraryError` (no CPU fallback); nothing is synchronised and nothing is read on the host.
"""
from __future__ import annotations

import torch

from . import cabi, hip

_BINDING = cabi.Binding.of(__name__)                # the header is the one place a signature or a constant is written
library_path, load, check_arity, call, order = _BINDING.library_path, _BINDING.load, _BINDING.check_arity, _BINDING.call, _BINDING.order
launch = hip.launcher(_BINDING, globals())          # every stream-taking entry is called through it, by the header's parameter names
EXPORTED_SYMBOLS = _BINDING.exported_symbols
ABI_VERSION = _BINDING.abi_version
(CHANNELS, HEADS, HEAD_DIM, HIDDEN, MAX_BATCH, MAX_ROWS, MAX_TOTAL_ROWS, ROW_TILE, ROW_BLOCK, SPLIT_ROWS, MAX_SPLITS,
 PARAM_FLOATS) = map(_BINDING.constant, ("CHANNELS", "HEADS", "HEAD_DIM", "HIDDEN", "MAX_BATCH", "MAX_ROWS", "MAX_TOTAL_ROWS", "ROW_TILE", "ROW_BLOCK",
                                         "SPLIT_ROWS", "MAX_SPLITS", "PARAM_FLOATS"))
# state-dict name -> (the header's offset constant, shape), in the buffer's order
PARAM_NAMES = ("q_proj.weight", "k_proj.weight", "v_proj.weight", "merge.weight", "mlp.0.weight", "mlp.2.weight", "norm1.weight", "norm1.bias",
               "norm2.weight", "norm2.bias")
_OFFSET_NAMES = ("Q_PROJ", "K_PROJ", "V_PROJ", "MERGE", "MLP0", "MLP2", "NORM1_WEIGHT", "NORM1_BIAS", "NORM2_WEIGHT", "NORM2_BIAS")
_SHAPES = ((256, 256),) * 4 + ((512, 512), (256, 512)) + ((256,),) * 4
PARAM_LAYOUT = {name: (_BINDING.constant("OFF_" + off), shape) for name, off, shape in zip(PARAM_NAMES, _OFFSET_NAMES, _SHAPES)}
KEEP_LAYER_INPUTS_HINT = ("set hip_keep_layer_inputs (with hip_train_forward) in the model's config: the training-mode forward then leaves every "
                          "coarse layer's inputs in data['layer_inputs_c']")


def rows_per_split(rows: int) -> int:
    """The header's split rule: the rows one partial sum takes of ``rows``"""
    return max(SPLIT_ROWS, -(-(-(-rows // MAX_SPLITS)) // 32) * 32)


def pack_params(layer, prefix: str = "") -> torch.Tensor:
    """An ``EncoderLayerParams`` (or any module with its parameter names), or a state dict with ``prefix`` (``"loftr_coarse.layers.0."``)
    -> float32 ``[PARAM_FLOATS]`` in the header's order, on the parameters' device"""
    sd = layer if isinstance(layer, dict) else dict(layer.named_parameters())
    parts = []
    for name, (_, shape) in PARAM_LAYOUT.items():
        if prefix + name not in sd:
            raise KeyError(f"{prefix + name}: not among the layer's parameters")
        t = sd[prefix + name].detach()
        if tuple(t.shape) != shape:
            raise ValueError(f"{prefix + name}: {list(shape)} expected, got {list(t.shape)}")
        parts.append(t.to(torch.float32).reshape(-1))
    flat = torch.cat(parts)
    assert flat.numel() == PARAM_FLOATS
    return flat


def unpack_grads(flat: torch.Tensor, prefix: str = "") -> dict:
    """float32 ``[PARAM_FLOATS]`` -> ``{prefix + state-dict name: view of its shape}``"""
    if flat.dim() != 1 or flat.numel() != PARAM_FLOATS:
        raise ValueError(f"flat: [{PARAM_FLOATS}], got {list(flat.shape)}")
    return {prefix + name: flat[off:off + _numel(shape)].view(*shape) for name, (off, shape) in PARAM_LAYOUT.items()}


def _numel(shape):
    n = 1
    for s in shape:
        n *= s
    return n


def _rows(name, t, B=None, rows=None):
    if t.dtype != torch.float32 or t.dim() != 3 or t.shape[2] != CHANNELS or (B is not None and (t.shape[0], t.shape[1]) != (B, rows)):
        want = f"[{'B' if B is None else B}, {'*' if rows is None else rows}, {CHANNELS}]"
        raise ValueError(f"{name}: float32 {want}, got {t.dtype} {list(t.shape)}")
    return t.contiguous()


def workspace_bytes(B: int, L: int, S: int) -> int:
    nbytes = int(load().openb_layer_workspace_bytes(B, L, S))
    if nbytes == 0:
        raise ValueError(f"[B, L, S] = {[B, L, S]}: no empty extent, B at most {MAX_BATCH}, L and S at most {MAX_ROWS}, B * L and B * S at most "
                         f"{MAX_TOTAL_ROWS}")
    return nbytes


def layer_backward(x, source, dy, params, *, dparams=None, accumulate=False, workspace=None, out=None, stream=None):
    """One layer call ``y = layer(x, source)``: ``x [B, L, 256]``, ``source [B, S, 256]`` (may be ``x`` itself), ``dy [B, L, 256]`` and the
    flat ``params`` (:func:`pack_params`) -> ``(dx, dsource, dparams)``.  ``dparams``: the flat buffer to write, or with ``accumulate`` to
    add to once per element; ``workspace``: a uint8 buffer of at least :func:`workspace_bytes`; ``out``: a pair ``(dx, dsource)`` to write
    into."""
    hip.need_device([("x", x), ("source", source), ("dy", dy), ("params", params)])
    x = _rows("x", x)
    B, L = int(x.shape[0]), int(x.shape[1])
    source = x if source is x else _rows("source", source)
    if source.shape[0] != B:
        raise ValueError(f"source: {B} frames like x, got {source.shape[0]}")
    S = int(source.shape[1])
    dy = _rows("dy", dy, B, L)
    if params.dtype != torch.float32 or tuple(params.shape) != (PARAM_FLOATS,) or not params.is_contiguous():
        raise ValueError(f"params: float32 [{PARAM_FLOATS}], contiguous (pack_params)")
    if 0 in (B, L, S):
        raise ValueError("x, source: no empty extent")
    if accumulate and dparams is None:
        raise ValueError("accumulate: needs the dparams to add to")
    dev = x.device
    nbytes = workspace_bytes(B, L, S)
    with hip.enqueue_on(dev, stream):
        if dparams is None:
            dparams = torch.empty(PARAM_FLOATS, dtype=torch.float32, device=dev)
        elif not dparams.is_cuda or dparams.dtype != torch.float32 or tuple(dparams.shape) != (PARAM_FLOATS,) or not dparams.is_contiguous():
            raise ValueError(f"dparams: float32 [{PARAM_FLOATS}] on the device, contiguous")
        if out is None:
            dx, dsource = torch.empty_like(x), torch.empty_like(source)
        else:
            dx, dsource = out
            hip.need_device([("out[0]", dx), ("out[1]", dsource)])
            for o, like in ((dx, x), (dsource, source)):
                if o.shape != like.shape or o.dtype != torch.float32 or not o.is_contiguous():
                    raise ValueError(f"out: float32 {list(x.shape)} and {list(source.shape)}, contiguous")
        if workspace is None:
            workspace = torch.empty(nbytes, dtype=torch.uint8, device=dev)
        elif not workspace.is_cuda or workspace.dtype != torch.uint8 or workspace.numel() < nbytes:
            raise ValueError(f"workspace: uint8 on the device, at least {nbytes} bytes")
        launch("openb_layer_grads", dict(x=x, source=source, dy=dy, B=B, L=L, S=S, params=params, workspace=workspace,
                                         workspace_bytes=int(workspace.numel()), dx=dx, dsource=dsource, dparams=dparams,
                                         accumulate=bool(accumulate)), stream)
    return dx, dsource, dparams


def coarse_backward(data, model, stream=None):
    """The coarse transformer's backward behind ``loss_backward.backward``: walks ``model.loftr_coarse.layer_names`` in reverse from
    ``data["grad_feat_c0"]`` (the 3D stream) and ``data["grad_feat_c1"]`` (the 2D stream) over the kept ``data["layer_inputs_c"]`` (a list
    of ``(x3d, x2d)`` per layer).  A ``self`` layer updates each stream from itself: its input gradient is ``dx + dsource`` of its one
    call.  A ``cross`` layer updates 2D from 3D and 3D from 2D, both from the pre-update tensors: the 3D input gradient is ``dx`` of the 3D
    call plus ``dsource`` of the 2D call, and the other way round.  The two calls of a layer share its weights: the second accumulates.
    Writes ``data["grad_x3d_c"]``, ``data["grad_x2d_c"]`` and ``data["grad_params_c"]`` (``{"loftr_coarse.layers.<i>.<name>": tensor}``)."""
    if "query_image_mask" in data:
        raise NotImplementedError("data['query_image_mask']: masks (x_mask / source_mask of the encoder layers) are not implemented; the layer "
                                  "backward has no mask parameter")
    for key, hint in (("grad_feat_c0", "run loss_backward.backward first"), ("grad_feat_c1", "run loss_backward.backward first"),
                      ("layer_inputs_c", KEEP_LAYER_INPUTS_HINT)):
        if key not in data:
            raise KeyError(f"{key}: {hint}")
    names = list(model.loftr_coarse.layer_names)
    kept = data["layer_inputs_c"]
    if len(kept) != len(names):
        raise ValueError(f"layer_inputs_c: {len(names)} pairs expected, got {len(kept)}")
    g3, g2 = data["grad_feat_c0"], data["grad_feat_c1"]
    grads = {}
    for i in reversed(range(len(names))):
        x3, x2 = kept[i]
        with torch.cuda.stream(stream):                         # (None changes nothing) the packing's copy runs where its readers run
            params = pack_params(model.loftr_coarse.layers[i])
        if names[i] == "self":
            d2, s2, dp = layer_backward(x2, x2, g2, params, stream=stream)
            d3, s3, dp = layer_backward(x3, x3, g3, params, dparams=dp, accumulate=True, stream=stream)
        elif names[i] == "cross":
            d2, s3, dp = layer_backward(x2, x3, g2, params, stream=stream)                               # 2D updated from 3D
            d3, s2, dp = layer_backward(x3, x2, g3, params, dparams=dp, accumulate=True, stream=stream)  # 3D updated from 2D
        else:
            raise NotImplementedError(f"layer name {names[i]!r}")
        with torch.cuda.stream(stream):                         # (None changes nothing)
            g3, g2 = d3 + s3, d2 + s2
        grads.update(unpack_grads(dp, f"loftr_coarse.layers.{i}."))
    data.update({"grad_x3d_c": g3, "grad_x2d_c": g2, "grad_params_c": grads})


class stages:
    """The entry one by one (device tensors in, device tensors out): what :func:`coarse_backward` enqueues"""
    layer_backward = staticmethod(layer_backward)
