"""The one Python home of the encoder-layer C calls (include/onepose_hip.h): ``ophip_encoder_layer`` / ``_bf16`` / ``_x3w8`` / ``_full_x3``
with their ``_masked``, ``_masks``, ``_streams``, ``_streams_masks`` and ``_frag`` forms, ``ophip_encoder_layer_full_x3_stream``,
``ophip_encoder_kv_first_x3w8`` and ``ophip_encoder_object_x3w8``, and of the size queries that go with them; every argument is bound by
its name in the header.

The two steps of ``matchcall``: ``plan_*`` is pure, it chooses the entry and returns ``(entry, {parameter name: tensor or scalar})``
without ``stream`` and checks nothing the C side checks (in-place rows, ``streams = 0``, ``nsplit = 3``, an under-aligned workspace are
refused by C); ``hip.launch`` converts by the header's C types and calls.  ``mode`` is the arithmetic of the layer: ``"f32"`` (exact),
``"bf16"`` (plain), ``"bf16x3"`` (split, the default) or ``"full"`` (softmax attention)."""
from __future__ import annotations

import torch

from . import hip

# mode -> (entry stem, workspace helper, its unit in bytes, weight-block helper)
_MODES = {"f32": ("ophip_encoder_layer", "ophip_encoder_workspace_floats", 4, None),
          "bf16": ("ophip_encoder_layer_bf16", "ophip_encoder_bf16_workspace_bytes", 1, "ophip_encoder_bf16_wpack_bytes"),
          "bf16x3": ("ophip_encoder_layer_x3w8", "ophip_encoder_x3w8_workspace_bytes", 1, "ophip_encoder_x3w8_wpack_bytes"),
          "full": ("ophip_encoder_layer_full_x3", "ophip_encoder_full_workspace_bytes", 1, None)}
_FORMS = {(): "", ("query_mask",): "_masked", ("masks",): "_masks", ("streams",): "_streams", ("masks", "streams"): "_streams_masks",
          ("frag",): "_frag"}


def plan_layer(x3d, x2d, y3d, y2d, *, mode, wpack, is_cross, workspace, wpack_next=None, kv_from_prev=0, slot=0, nsplit=None,
               query_mask=None, masks=None, streams=None, frag=None):
    forms = tuple(k for k, v in (("query_mask", query_mask), ("masks", masks), ("streams", streams), ("frag", frag)) if v is not None)
    entry = _MODES[mode][0] + _FORMS[forms] if mode in _MODES and forms in _FORMS else None
    chained = mode in ("bf16", "bf16x3") and streams is None           # the entries with wpack_next / kv_from_prev / slot
    if entry not in hip.PROTOTYPES or (not chained and (wpack_next is not None or kv_from_prev or slot)) or (nsplit is not None and mode != "bf16"):
        given = forms + tuple(k for k, v in (("wpack_next", wpack_next is not None), ("kv_from_prev", kv_from_prev), ("slot", slot), ("nsplit", nsplit is not None)) if v)
        raise ValueError(f"no encoder-layer entry for mode {mode!r} with {', '.join(given) or 'no option'}")
    named = dict(x3d=x3d, x2d=x2d, y3d=y3d, y2d=y2d, B=x3d.shape[0], L3d=x3d.shape[1], L2d=x2d.shape[1], wpack=wpack, is_cross=is_cross,
                 workspace=workspace)
    if chained:
        named.update(wpack_next=wpack_next, kv_from_prev=kv_from_prev, slot=slot)
    if mode == "bf16":
        named["nsplit"] = 1 if nsplit is None else nsplit
    if query_mask is not None:
        named["query_mask"] = query_mask
    if masks is not None:
        named.update(mask0=masks[0], mask1=masks[1])
    if streams is not None:
        named["streams"] = streams
    if frag is not None:
        named.update(frag3d=frag[0], frag2d=frag[1])
    return entry, named


def layer(x3d, x2d, y3d, y2d, *, stream=None, **kw):
    """One encoder layer on both streams, ``x`` rows into ``y`` rows.  The entry follows the options: ``query_mask`` -> ``_masked``;
    ``masks=(mask0, mask1)`` (either may be ``None``) -> ``_masks``; ``streams`` (bit 0: the first stream runs, bit 1: the second; the
    other ``y`` may be ``None``) -> ``_streams``, with masks ``_streams_masks``; ``frag=(frag3d, frag2d)`` of
    ``ophip_coarse_frag_planes`` -> ``_frag``.  ``wpack_next`` / ``kv_from_prev`` / ``slot`` chain the two-stream ``"bf16"`` and
    ``"bf16x3"`` layers; ``nsplit`` (1) is the ``"bf16"`` entries' alone.  A combination the header has no entry for raises ``ValueError``."""
    hip.launch(*plan_layer(x3d, x2d, y3d, y2d, **kw), stream)


def plan_layer_full_stream(x, src, y, *, wpack, workspace):
    bs = lambda t: t.stride(0) if t.shape[0] > 1 else 0
    return "ophip_encoder_layer_full_x3_stream", dict(x=x, x_bstride=bs(x), src=src, src_bstride=bs(src), y=y, B=max(x.shape[0], src.shape[0]),
                                                      L=x.shape[1], S=src.shape[1], wpack=wpack, workspace=workspace)


def layer_full_stream(x, src, y, *, stream=None, **kw):
    """``y`` = the full-attention layer of the rows ``x`` against ``src``; an input of batch extent 1 is shared by the batch (stride 0)"""
    hip.launch(*plan_layer_full_stream(x, src, y, **kw), stream)


def plan_kv_first(x3d, x2d, *, wpack, slot, workspace, mask2d=None):
    return "ophip_encoder_kv_first_x3w8", dict(x3d=x3d, x2d=x2d, B=x3d.shape[0], L3d=x3d.shape[1], L2d=x2d.shape[1], wpack=wpack, slot=slot,
                                               workspace=workspace, mask2d=mask2d)


def kv_first(x3d, x2d, *, stream=None, **kw):
    """the K / V half of a frame's first ``"bf16x3"`` layer; the layer call that follows passes ``kv_from_prev=2``"""
    hip.launch(*plan_kv_first(x3d, x2d, **kw), stream)


def plan_object(x3d, *, wpack0, wpack1, workspace, y3d0, kv1, masked_frames):
    return "ophip_encoder_object_x3w8", dict(x3d=x3d, Bo=x3d.shape[0], N=x3d.shape[1], wpack0=wpack0, wpack1=wpack1, workspace=workspace,
                                             y3d0=y3d0, kv1=kv1, masked_frames=masked_frames)


def object_rows(x3d, *, stream=None, **kw):
    """the object cache's build: the first layer's 3D rows ``y3d0`` and layer 1's source block ``kv1``; workspace of ``(Bo, N, 1)``"""
    hip.launch(*plan_object(x3d, **kw), stream)


def workspace_bytes(mode, B, L3d, L2d, stream_form=False) -> int:
    """Bytes of the layer's workspace from the mode's own size query (``"f32"`` counts floats: times 4); ``stream_form``: the
    ``_full_x3_stream`` entry's ``(B, L, S)``"""
    _, helper, unit, _ = _MODES[mode]
    if stream_form:
        if mode != "full":
            raise ValueError(f"no stream-form workspace query for mode {mode!r}")
        helper = "ophip_encoder_full_stream_workspace_bytes"
    return getattr(hip.load(), helper)(B, L3d, L2d) * unit


def workspace(mode, B, L3d, L2d, device, stream_form=False):
    """The workspace tensor of one layer call: float32 elements for ``"f32"`` (its entries take ``float*``), bytes otherwise"""
    nbytes = workspace_bytes(mode, B, L3d, L2d, stream_form)
    return torch.empty(nbytes // 4, device=device, dtype=torch.float32) if mode == "f32" else torch.empty(nbytes, device=device, dtype=torch.uint8)


def wpack_bytes(mode) -> int:
    """Bytes of one packed layer block of ``"bf16"`` / ``"bf16x3"`` (the f32 block of ``"f32"`` / ``"full"`` has no query)"""
    helper = _MODES[mode][3]
    if helper is None:
        raise ValueError(f"no weight-block size query for mode {mode!r}")
    return getattr(hip.load(), helper)()


def kv_block_bytes() -> int:
    """Bytes of one ``kv1`` block of the object cache"""
    return hip.load().ophip_encoder_x3w8_kv_block_bytes()
