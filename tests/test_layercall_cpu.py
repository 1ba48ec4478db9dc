"""onepose_st_amd/layercall.py without a GPU: the pure ``plan_*`` step of the encoder-layer calls, with CPU tensors.  Each plan names an
entry of include/onepose_hip.h and binds exactly that entry's header parameters (minus ``stream``); per entry the order that reaches C is
held against the positional list the call sites spelled out before the calls were bound by name."""
import ctypes

import pytest
import torch

from onepose_st_amd import hip, layercall as lc

B, L3, L2 = 2, 5, 7
X3, X2, Y3, Y2 = torch.empty(B, L3, 256), torch.empty(B, L2, 256), torch.empty(B, L3, 256), torch.empty(B, L2, 256)
W, WN, WS = torch.empty(8), torch.empty(8), torch.empty(16)
QM, M0, M1 = torch.ones(B, L2, dtype=torch.uint8), torch.ones(B, L3, dtype=torch.bool), torch.ones(B, L2, dtype=torch.bool)
FRAG = (ctypes.c_void_p(64), ctypes.c_void_p(128))
S = object()                                                              # stands for the stream handle
E = "ophip_encoder_"


def names(entry):
    return {n for _, n in hip.PROTOTYPES[entry].params} - {"stream"}


def layer(**kw):
    """the plan of one layer over X3, X2 (``y3d`` / ``y2d``: other output rows than Y3 / Y2) and the keywords it was made with"""
    kw = {**dict(wpack=W, is_cross=1, workspace=WS, y3d=Y3, y2d=Y2), **kw}
    return lc.plan_layer(X3, X2, kw["y3d"], kw["y2d"], **{k: v for k, v in kw.items() if k not in ("y3d", "y2d")}), kw


CHAIN = dict(wpack_next=WN, kv_from_prev=1, slot=1)
X3W8 = dict(mode="bf16x3")
LAYER_ROWS = [
    (dict(mode="f32"), E + "layer"), (dict(mode="f32", is_cross=0), E + "layer"), (dict(mode="f32", query_mask=QM), E + "layer_masked"),
    (dict(mode="bf16"), E + "layer_bf16"), (dict(mode="bf16", nsplit=1, **CHAIN), E + "layer_bf16"),
    (dict(mode="bf16", query_mask=QM), E + "layer_bf16_masked"), (dict(mode="bf16", query_mask=QM, **CHAIN), E + "layer_bf16_masked"),
    (X3W8, E + "layer_x3w8"), (dict(X3W8, **CHAIN), E + "layer_x3w8"), (dict(X3W8, kv_from_prev=2), E + "layer_x3w8"),
    (dict(X3W8, query_mask=QM), E + "layer_x3w8_masked"), (dict(X3W8, query_mask=QM, kv_from_prev=2), E + "layer_x3w8_masked"),
    *[(dict(X3W8, masks=m), E + "layer_x3w8_masks") for m in ((M0, M1), (None, M1), (M0, None), (None, None))],
    (dict(X3W8, masks=(M0, M1), **CHAIN), E + "layer_x3w8_masks"),
    (dict(X3W8, frag=FRAG), E + "layer_x3w8_frag"), (dict(X3W8, frag=FRAG, kv_from_prev=2), E + "layer_x3w8_frag"),
    *[(dict(X3W8, streams=s, y3d=Y3 if s & 1 else None, y2d=Y2 if s & 2 else None), E + "layer_x3w8_streams") for s in (1, 2, 3)],
    *[(dict(X3W8, streams=s, masks=m), E + "layer_x3w8_streams_masks") for s in (1, 2, 3) for m in ((M0, M1), (None, M1), (M0, None))],
    (dict(mode="full"), E + "layer_full_x3"), (dict(mode="full", is_cross=0), E + "layer_full_x3"),
]


@pytest.mark.parametrize("kw,entry", LAYER_ROWS, ids=[f"{e[14:]}-{'-'.join(k for k in kw if k != 'mode') or 'plain'}-{i}" for i, (kw, e) in enumerate(LAYER_ROWS)])
def test_layer_entry_and_names(kw, entry):
    (got, named), kw = layer(**kw)
    assert got == entry and set(named) == names(entry)
    assert named["x3d"] is X3 and named["x2d"] is X2 and named["y3d"] is kw["y3d"] and named["y2d"] is kw["y2d"]
    assert named["wpack"] is W and named["workspace"] is WS                       # supplied tensors by identity
    assert (named["B"], named["L3d"], named["L2d"], named["is_cross"]) == (B, L3, L2, kw["is_cross"])
    chained = kw["mode"] in ("bf16", "bf16x3") and "streams" not in kw
    assert ("wpack_next" in named) == ("kv_from_prev" in named) == ("slot" in named) == chained
    if chained:
        assert named["wpack_next"] is kw.get("wpack_next") and (named["kv_from_prev"], named["slot"]) == (kw.get("kv_from_prev", 0), kw.get("slot", 0))
    assert ("nsplit" in named) == (kw["mode"] == "bf16") and named.get("nsplit", 1) == 1
    assert named.get("query_mask") is kw.get("query_mask") and named.get("streams") == kw.get("streams")
    assert (named.get("mask0"), named.get("mask1")) == tuple(kw.get("masks", (None, None))) and ("mask0" in named) == ("masks" in kw)
    assert (named.get("frag3d"), named.get("frag2d")) == tuple(kw.get("frag", (None, None)))


def test_full_stream_kv_first_and_object_plans():
    x, shared, y = torch.empty(3, L3, 256), torch.empty(1, L2, 256), torch.empty(3, L3, 256)
    entry, named = lc.plan_layer_full_stream(x, shared, y, wpack=W, workspace=WS)
    assert entry == E + "layer_full_x3_stream" and set(named) == names(entry)
    assert named["x"] is x and named["src"] is shared and named["y"] is y and named["wpack"] is W and named["workspace"] is WS
    assert (named["x_bstride"], named["src_bstride"], named["B"], named["L"], named["S"]) == (L3 * 256, 0, 3, L3, L2)      # batch 1: stride 0
    named = lc.plan_layer_full_stream(shared, x, y, wpack=W, workspace=WS)[1]
    assert (named["x_bstride"], named["src_bstride"], named["B"], named["L"], named["S"]) == (0, L3 * 256, 3, L2, L3)
    named = lc.plan_layer_full_stream(x, x, y, wpack=W, workspace=WS)[1]                                                  # the self layer
    assert named["src"] is x and (named["x_bstride"], named["src_bstride"], named["B"], named["S"]) == (L3 * 256, L3 * 256, 3, L3)
    for mask in (None, QM):
        entry, named = lc.plan_kv_first(X3, X2, wpack=W, slot=1, workspace=WS, **({} if mask is None else dict(mask2d=mask)))
        assert entry == E + "kv_first_x3w8" and set(named) == names(entry) and named["mask2d"] is mask
        assert named["x3d"] is X3 and named["x2d"] is X2 and named["wpack"] is W and named["workspace"] is WS
        assert (named["B"], named["L3d"], named["L2d"], named["slot"]) == (B, L3, L2, 1)
    kv1 = torch.empty(B, 32, dtype=torch.uint8)
    entry, named = lc.plan_object(X3, wpack0=W, wpack1=WN, workspace=WS, y3d0=Y3, kv1=kv1, masked_frames=1)
    assert entry == E + "object_x3w8" and set(named) == names(entry)
    assert named["x3d"] is X3 and named["wpack0"] is W and named["wpack1"] is WN and named["workspace"] is WS and named["y3d0"] is Y3
    assert named["kv1"] is kv1 and (named["Bo"], named["N"], named["masked_frames"]) == (B, L3, 1)


HEAD = (X3, X2, Y3, Y2, B, L3, L2)
KV1 = torch.empty(B, 32, dtype=torch.uint8)
# entry -> (its plan, the positional list of the call sites before this module: wpack, wpack_next, [nsplit,] is_cross, kv_from_prev, slot, ...)
POSITIONAL = {
    E + "layer": (layer(mode="f32")[0], (*HEAD, W, 1, WS, S)),
    E + "layer_masked": (layer(mode="f32", query_mask=QM)[0], (*HEAD, W, 1, WS, QM, S)),
    E + "layer_bf16": (layer(mode="bf16", wpack_next=WN, is_cross=0, kv_from_prev=2, slot=3)[0], (*HEAD, W, WN, 1, 0, 2, 3, WS, S)),
    E + "layer_bf16_masked": (layer(mode="bf16", wpack_next=WN, is_cross=0, kv_from_prev=2, slot=3, query_mask=QM)[0],
                              (*HEAD, W, WN, 1, 0, 2, 3, WS, QM, S)),
    E + "layer_x3w8": (layer(**X3W8, wpack_next=WN, kv_from_prev=2, slot=3)[0], (*HEAD, W, WN, 1, 2, 3, WS, S)),
    E + "layer_x3w8_frag": (layer(**X3W8, wpack_next=WN, kv_from_prev=2, slot=3, frag=FRAG)[0], (*HEAD, W, WN, 1, 2, 3, WS, *FRAG, S)),
    E + "layer_x3w8_masked": (layer(**X3W8, wpack_next=WN, kv_from_prev=2, slot=3, query_mask=QM)[0], (*HEAD, W, WN, 1, 2, 3, WS, QM, S)),
    E + "layer_x3w8_masks": (layer(**X3W8, wpack_next=WN, kv_from_prev=2, slot=3, masks=(M0, M1))[0], (*HEAD, W, WN, 1, 2, 3, WS, M0, M1, S)),
    E + "layer_x3w8_streams": (layer(**X3W8, streams=2, y3d=None)[0], (X3, X2, None, Y2, B, L3, L2, W, 1, 2, WS, S)),
    E + "layer_x3w8_streams_masks": (layer(**X3W8, streams=2, y3d=None, masks=(M0, M1))[0], (X3, X2, None, Y2, B, L3, L2, W, 1, 2, WS, M0, M1, S)),
    E + "kv_first_x3w8": (lc.plan_kv_first(X3, X2, wpack=W, slot=3, workspace=WS, mask2d=QM), (X3, X2, B, L3, L2, W, 3, WS, QM, S)),
    E + "object_x3w8": (lc.plan_object(X3, wpack0=W, wpack1=WN, workspace=WS, y3d0=Y3, kv1=KV1, masked_frames=1), (X3, B, L3, W, WN, WS, Y3, KV1, 1, S)),
    E + "layer_full_x3": (layer(mode="full")[0], (*HEAD, W, 1, WS, S)),
    E + "layer_full_x3_stream": (lc.plan_layer_full_stream(X3, X2, Y3, wpack=W, workspace=WS), (X3, L3 * 256, X2, L2 * 256, Y3, B, L3, L2, W, WS, S)),
}


@pytest.mark.parametrize("entry", list(POSITIONAL))
def test_order_equals_the_positional_list_it_replaces(entry):
    (got, named), want = POSITIONAL[entry]
    assert got == entry
    ordered = hip.order(entry, **named, stream=S)
    assert len(ordered) == len(want) and all(a is b or (not torch.is_tensor(a) and not torch.is_tensor(b) and a == b) for a, b in zip(ordered, want))


def test_every_encoder_entry_has_a_plan():
    planned = {e for _, e in LAYER_ROWS} | set(POSITIONAL)
    assert planned == set(POSITIONAL) == {n for n in hip.PROTOTYPES if n.startswith((E + "layer", E + "kv_first", E + "object"))}
    assert len(planned) == 14 and all(set(hip.converters(e)) == names(e) for e in planned)


NO_ENTRY = [dict(X3W8, frag=FRAG, query_mask=QM), dict(X3W8, frag=FRAG, masks=(M0, M1)), dict(X3W8, frag=FRAG, streams=1),
            dict(X3W8, query_mask=QM, masks=(M0, M1)), dict(X3W8, query_mask=QM, streams=1), dict(X3W8, streams=1, wpack_next=WN),
            dict(X3W8, streams=1, kv_from_prev=1), dict(X3W8, streams=2, masks=(M0, M1), slot=1), dict(X3W8, nsplit=3),
            *[dict(mode=m, **opt) for m in ("f32", "bf16", "full") for opt in (dict(streams=1), dict(masks=(M0, M1)), dict(frag=FRAG))],
            *[dict(mode=m, **opt) for m in ("f32", "full") for opt in (dict(wpack_next=WN), dict(kv_from_prev=1), dict(slot=1), dict(nsplit=1))],
            dict(mode="full", query_mask=QM), dict(mode="fp8"), dict(mode="x3w8")]


@pytest.mark.parametrize("kw", NO_ENTRY, ids=["-".join(f"{k}" if k != "mode" else v for k, v in kw.items()) for kw in NO_ENTRY])
def test_a_combination_without_an_entry_raises(kw):
    with pytest.raises(ValueError, match="no encoder-layer entry"):
        layer(**kw)


def test_what_c_refuses_is_left_alone():
    (entry, named), _ = layer(mode="f32", y3d=X3)                                  # in place
    assert entry == E + "layer" and named["y3d"] is named["x3d"]
    (entry, named), _ = layer(**X3W8, streams=0)
    assert entry == E + "layer_x3w8_streams" and named["streams"] == 0
    (entry, named), _ = layer(mode="bf16", nsplit=3)                               # the split layer is the x3w8 entry
    assert entry == E + "layer_bf16" and named["nsplit"] == 3
    (entry, named), _ = layer(**X3W8, slot=2, workspace=WS[1:])                    # a slot C does not know, an under-aligned workspace
    assert entry == E + "layer_x3w8" and named["slot"] == 2 and named["workspace"].data_ptr() == WS.data_ptr() + 4


class _Sizes:
    """in place of the library handle: every size query answers 10 and is recorded"""

    def __init__(self):
        self.asked = []

    def __getattr__(self, name):
        return lambda *args: self.asked.append((name, args)) or 10


def test_size_queries_choose_the_helper_and_the_unit(monkeypatch):
    lib = _Sizes()
    monkeypatch.setattr(hip._BINDING, "handle", lib)
    got = [lc.workspace_bytes(m, B, L3, L2) for m in ("f32", "bf16", "bf16x3", "full")] + [lc.workspace_bytes("full", B, L3, L2, stream_form=True)]
    assert got == [40, 10, 10, 10, 10]                                             # the f32 helper counts floats
    assert lib.asked == [(E + h, (B, L3, L2)) for h in ("workspace_floats", "bf16_workspace_bytes", "x3w8_workspace_bytes", "full_workspace_bytes",
                                                        "full_stream_workspace_bytes")]
    ws = {m: lc.workspace(m, B, L3, L2, "cpu") for m in ("f32", "bf16", "bf16x3", "full")}
    assert (ws["f32"].dtype, ws["f32"].numel()) == (torch.float32, 10)
    assert all((ws[m].dtype, ws[m].numel()) == (torch.uint8, 10) for m in ("bf16", "bf16x3", "full"))
    assert lc.workspace("full", B, L3, L2, "cpu", stream_form=True).dtype == torch.uint8 and lib.asked[-1][0] == E + "full_stream_workspace_bytes"
    del lib.asked[:]
    assert (lc.wpack_bytes("bf16"), lc.wpack_bytes("bf16x3"), lc.kv_block_bytes()) == (10, 10, 10)
    assert lib.asked == [(E + "bf16_wpack_bytes", ()), (E + "x3w8_wpack_bytes", ()), (E + "x3w8_kv_block_bytes", ())]
    for bad in (lambda: lc.workspace_bytes("bf16x3", B, L3, L2, stream_form=True), lambda: lc.wpack_bytes("f32"), lambda: lc.wpack_bytes("full")):
        with pytest.raises(ValueError):
            bad()


def test_launch_converts_by_the_header_type():
    conv = hip.converters(E + "layer_x3w8_frag")
    assert conv["frag3d"](FRAG[0]) is FRAG[0] and conv["frag2d"](None) is None and conv["wpack_next"](None) is None      # void*: an address or NULL as it is
    assert (conv["B"]("3"), conv["is_cross"](True)) == (3, 1)
    with pytest.raises(hip.HipLibraryError):                                       # a CPU tensor reaches no kernel
        lc.layer(X3, X2, Y3, Y2, mode="f32", wpack=W, is_cross=0, workspace=WS)
    with pytest.raises(hip.HipLibraryError):
        lc.object_rows(X3, wpack0=W, wpack1=WN, workspace=WS, y3d0=Y3, kv1=KV1, masked_frames=0)
