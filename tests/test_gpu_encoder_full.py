"""Full (softmax) attention on the device -- ``ophip_full_attention_h8d32`` (``full_flash_kernel``), ``ophip_encoder_layer_full_x3`` and
``ophip_encoder_layer_full_x3_stream`` (csrc/encoder_full.hip) -- against the UN-ROUNDED float64 reference of tests/full_faithful.py, at the tile,
tail, range and stride edges its case lists name.  Every buffer of a call is a region of one ``tests/guarded.Arena``; outputs and workspaces start
as 0xFF bytes (NaN), outputs carry spare rows that must stay NaN, and every check first asserts that nothing it reads is NaN.

The bars are ``ff.ATTENTION_BAR`` (per input family) and ``ff.LAYER_BAR``: three times the float32 stand-in's worst, pinned by
tests/test_full_faithful_cpu.py, where seeded faults of the kernel land ten bars out and more.  DESIGN.md section 6b holds the device's figures."""
import pytest
import torch

from onepose_st_amd import hip, layercall, packing
from tests import full_faithful as ff
from tests.guarded import arena_for, is_fill as is_nan_fill

pytestmark = pytest.mark.gpu

P = ff.LAYER
C = ff.C
SPARE = 3                                               # rows behind every output that no call may write


@pytest.fixture(scope="module")
def dev():
    assert torch.cuda.is_available(), "these tests need the MI355X"
    hip.load()
    return torch.device("cuda:0")


@pytest.fixture(scope="module")
def wpack(sd, dev):
    return packing.pack_coarse_layer(sd, P).to(dev)


def rows_out(a, B, L, name):
    """``[B L + SPARE][256]`` f32, NaN-filled: the call's output and the spare rows behind it"""
    return a.typed((B * L + SPARE, C), torch.float32, name=name)


def written(out, B, L, label):
    """the ``[B][L][256]`` a call wrote, on the CPU; the spare rows behind it untouched, no NaN inside"""
    assert is_nan_fill(out[B * L:]), f"{label}: rows past the output were written"
    y = out[:B * L].view(B, L, C).cpu()
    assert not bool(torch.isnan(y).any()), f"{label}: NaN in the output (rows not written, or a key tail let in)"
    return y


# ------------------------------------------------------------------------------------------------
# the attention step
# ------------------------------------------------------------------------------------------------
def run_attention(dev, c):
    B, L, S = c["q"].shape[0], c["q"].shape[1], c["k"].shape[1]
    a = arena_for(dev, B * L * C * 4, B * S * C * 4, B * S * C * 4, (B * L + SPARE) * C * 4)
    q, k, v = a.put(c["q"], name="q"), a.put(c["k"], name="k"), a.put(c["v"], name="v")
    out = rows_out(a, B, L, "msg")
    hip.launch("ophip_full_attention_h8d32", dict(q=q, k=k, v=v, B=B, L=L, S=S, msg=out))
    torch.cuda.synchronize()
    o = written(out, B, L, f"attention B={B} L={L} S={S}")
    a.check()
    return o


@pytest.mark.parametrize("family", ff.FAMILIES)
def test_attention_step(dev, family):
    """all 68 shapes of one family; the worst figure and where it fell are printed"""
    bar, worst, failed = ff.ATTENTION_BAR[family], (0.0, None), []
    for B, L, S in ff.SHAPES:
        c = ff.attention_case(family, B, L, S)
        o = run_attention(dev, c)
        e = ff.attention_error(o, ff.attention_reference(family, B, L, S), c["v"])
        worst = max(worst, (e, (B, L, S)), key=lambda t: t[0])
        if not e <= bar:
            failed.append((B, L, S, e))
        if c["sel"] is not None:                        # "planted", "peaked_last": the output IS the selected value row
            es = ff.attention_error(o, ff.selected_rows(c), c["v"])
            if not es <= bar + 2 * (1 - ff.SELECTED_WEIGHT):
                failed.append((B, L, S, "selected row", es))
        if family == "uniform":                         # equal keys: the mean of V in float64
            mean = c["v"].double().mean(1, keepdim=True).expand(B, L, C)
            em = ff.attention_error(o, mean, c["v"])
            if not em <= bar:
                failed.append((B, L, S, "mean", em))
    print(f"attention {family}: device worst {worst[0]:.3e} at B, L, S = {worst[1]} (bar {bar:.2e})")
    assert not failed, (family, failed)


@pytest.mark.parametrize("family", ff.FAMILIES)
def test_attention_step_twice_the_same_bytes(dev, family):
    c = ff.attention_case(family, 3, 160, 97)
    assert torch.equal(run_attention(dev, c).view(torch.int32), run_attention(dev, c).view(torch.int32))


def test_attention_step_rejects_a_null_pointer_without_a_launch(dev):
    c = ff.attention_case("soft", 1, 33, 31)
    a = arena_for(dev, *(4 * c[n].numel() for n in ("q", "k", "v")), (33 + SPARE) * C * 4)
    q, k, v = (a.put(c[n], name=n) for n in ("q", "k", "v"))
    out = rows_out(a, 1, 33, "msg")
    try:
        hip.timing_select("full_flash")
        for missing in ("q", "k", "v", "msg"):
            with pytest.raises(ValueError):
                hip.launch("ophip_full_attention_h8d32", dict(dict(q=q, k=k, v=v, B=1, L=33, S=31, msg=out), **{missing: None}))
        assert hip.timing_read()[0] == 0                 # no rejected call launched the kernel
        torch.cuda.synchronize()
        assert is_nan_fill(out)
        hip.launch("ophip_full_attention_h8d32", dict(q=q, k=k, v=v, B=1, L=33, S=31, msg=out))      # the counter counts: a sound call is one launch
        assert hip.timing_read()[0] == 1
    finally:
        hip.timing_select("")
    torch.cuda.synchronize()
    written(out, 1, 33, "the sound call")
    a.check()


# ------------------------------------------------------------------------------------------------
# the two-stream layer
# ------------------------------------------------------------------------------------------------
def run_layer(dev, w, x3, x2, cross):
    B, L3, L2 = x3.shape[0], x3.shape[1], x2.shape[1]
    wsb = layercall.workspace_bytes("full", B, L3, L2)
    a = arena_for(dev, x3.numel() * 4, x2.numel() * 4, (B * L3 + SPARE) * C * 4, (B * L2 + SPARE) * C * 4, wsb)
    d3, d2 = a.put(x3, name="x3d"), a.put(x2, name="x2d")
    o3, o2 = rows_out(a, B, L3, "y3d"), rows_out(a, B, L2, "y2d")
    ws = a.region(wsb, name="workspace")
    layercall.layer(d3, d2, o3[:B * L3].view(B, L3, C), o2[:B * L2].view(B, L2, C), mode="full", wpack=w, is_cross=cross, workspace=ws)
    torch.cuda.synchronize()
    label = f"layer B={B} L=({L3},{L2}) cross={cross}"
    y3, y2 = written(o3, B, L3, label + " 3D"), written(o2, B, L2, label + " 2D")
    a.check()
    return y3, y2


@pytest.mark.parametrize("cross", [0, 1])
@pytest.mark.parametrize("L3,L2", ff.LAYER_SHAPES)
def test_two_stream_layer(sd, dev, wpack, cross, L3, L2):
    alone = None
    for B in (1, 2):
        x3, x2 = ff.layer_inputs(B, L3, L2)
        y3, y2 = run_layer(dev, wpack, x3, x2, cross)
        e3 = ff.row_error(y3, ff.reference_layer(sd, P, x3, x2 if cross else x3))
        e2 = ff.row_error(y2, ff.reference_layer(sd, P, x2, x3 if cross else x2))
        print(f"two-stream layer B={B} L=({L3},{L2}) cross={cross}: rows 3D {e3:.3e} 2D {e2:.3e} (bar {ff.LAYER_BAR:.2e})")
        assert e3 <= ff.LAYER_BAR and e2 <= ff.LAYER_BAR, (B, e3, e2)
        if B == 1:
            alone = (y3, y2)
        else:                                           # a batch element's bytes are those of its B = 1 call
            assert torch.equal(y3[:1], alone[0]) and torch.equal(y2[:1], alone[1])
            b3, b2 = run_layer(dev, wpack, x3[1:].contiguous(), x2[1:].contiguous(), cross)
            assert torch.equal(y3[1:], b3) and torch.equal(y2[1:], b2)


# ------------------------------------------------------------------------------------------------
# the one-stream layer
# ------------------------------------------------------------------------------------------------
def run_stream(dev, w, x, src, B, pad=(0, 0), src_is_x=False, **override):
    """``ophip_encoder_layer_full_x3_stream`` on ``x [nx][L][256]`` against ``src [ns][S][256]`` (batch extent 1: shared, stride 0) at the
    output's batch extent ``B``.  ``pad = (px, ps)``: gap rows of NaN behind every batch element of x / src, the strides ``(L + px) 256`` and
    ``(S + ps) 256``; ``src_is_x``: the source pointer is x's; ``override``: header arguments in place of the planned ones."""
    (nx, L, _), (ns, S, _) = x.shape, src.shape
    wsb = layercall.workspace_bytes("full", B, L, S, stream_form=True)
    a = arena_for(dev, nx * (L + pad[0]) * C * 4, ns * (S + pad[1]) * C * 4, (B * L + SPARE) * C * 4, wsb)
    dx = a.typed((nx, L + pad[0], C), torch.float32, name="x")           # gap rows: the arena's NaN
    dx[:, :L].copy_(x)
    if src_is_x:
        ds = dx
    else:
        ds = a.typed((ns, S + pad[1], C), torch.float32, name="src")
        ds[:, :S].copy_(src)
    out = rows_out(a, B, L, "y")
    ws = a.region(wsb, name="workspace")
    named = dict(x=dx, x_bstride=(L + pad[0]) * C if nx > 1 else 0, src=ds, src_bstride=(S + pad[1]) * C if ns > 1 else 0, y=out, B=B, L=L, S=S,
                 wpack=w, workspace=ws)
    named.update(override)
    hip.launch("ophip_encoder_layer_full_x3_stream", named)
    torch.cuda.synchronize()
    y = written(out, B, L, f"stream layer B={B} L={L} S={S} {sorted(override)}")
    a.check()
    return y


@pytest.mark.parametrize("mode", ff.STREAM_MODES)
@pytest.mark.parametrize("L,S", ff.STREAM_SHAPES)
def test_one_stream_layer(sd, dev, wpack, mode, L, S):
    x, src = ff.stream_inputs(mode, L, S)
    B = ff.STREAM_B
    y = run_stream(dev, wpack, x, src, B, src_is_x=mode == "self")
    e = ff.row_error(y, ff.reference_layer(sd, P, x, src))
    print(f"one-stream layer {mode} L={L} S={src.shape[1]}: rows {e:.3e} (bar {ff.LAYER_BAR:.2e})")
    assert e <= ff.LAYER_BAR, e
    for b in range(B):                                  # a batch element's bytes are those of its B = 1 call
        xb, sb = x[min(b, x.shape[0] - 1)][None], src[min(b, src.shape[0] - 1)][None]
        assert torch.equal(run_stream(dev, wpack, xb, sb, 1, src_is_x=mode == "self")[0], y[b]), (mode, b)


@pytest.mark.parametrize("L,S", ff.STREAM_SHAPES)
def test_one_stream_layer_padded_strides(sd, dev, wpack, L, S):
    """batch strides of (L + 3) and (S + 5) rows with NaN in the gaps: the gap rows stay unread (no NaN in y), the bytes are the packed call's"""
    x, src = ff.stream_inputs("pair", L, S)
    y = run_stream(dev, wpack, x, src, ff.STREAM_B, pad=(3, 5))
    assert ff.row_error(y, ff.reference_layer(sd, P, x, src)) <= ff.LAYER_BAR
    assert torch.equal(y, run_stream(dev, wpack, x, src, ff.STREAM_B))


@pytest.mark.parametrize("L,S", ff.STREAM_SHAPES)
def test_one_stream_layer_both_inputs_shared(sd, dev, wpack, L, S):
    """x and src both one image (stride 0) at B = 2: the two outputs are byte-equal"""
    x, src = ff.stream_inputs("pair", L, S)
    y = run_stream(dev, wpack, x[:1], src[:1], 2)
    assert torch.equal(y[0].view(torch.int32), y[1].view(torch.int32))
    assert ff.row_error(y, ff.reference_layer(sd, P, x[:1].expand(2, -1, -1), src[:1])) <= ff.LAYER_BAR


@pytest.mark.parametrize("L", [1, 33, 129])
def test_one_stream_layer_source_is_x_at_another_stride(sd, dev, wpack, L):
    """src is x's pointer with ``src_bstride = 0`` while ``x_bstride = L 256``, B = 2: not the self layer (every element attends to element 0).
    Byte for byte the pair call on the expanded tensors."""
    x, _ = ff.stream_inputs("self", L, L)
    y = run_stream(dev, wpack, x, x[:1], 2, src_is_x=True, src_bstride=0)
    assert ff.row_error(y, ff.reference_layer(sd, P, x, x[:1])) <= ff.LAYER_BAR
    pair = run_stream(dev, wpack, x, x[:1].expand(2, -1, -1).contiguous(), 2)
    assert torch.equal(y.view(torch.int32), pair.view(torch.int32))


# ------------------------------------------------------------------------------------------------
# rejected calls: a ValueError, nothing written, no kernel launched
# ------------------------------------------------------------------------------------------------
def test_rejected_calls_write_nothing_and_launch_nothing(dev, wpack):
    B, L, S = 2, 33, 31
    x3, x2 = ff.layer_inputs(B, L, S)
    wsb = max(layercall.workspace_bytes("full", B, L, S), layercall.workspace_bytes("full", B, L, S, stream_form=True))
    a = arena_for(dev, x3.numel() * 4, x2.numel() * 4, (B * L + SPARE) * C * 4, (B * S + SPARE) * C * 4, wsb)
    d3, d2 = a.put(x3, name="x3d"), a.put(x2, name="x2d")
    o3, o2 = rows_out(a, B, L, "y3d"), rows_out(a, B, S, "y2d")
    y3, y2 = o3[:B * L].view(B, L, C), o2[:B * S].view(B, S, C)
    ws = a.region(wsb, name="workspace")
    two = dict(x3d=d3, x2d=d2, y3d=y3, y2d=y2, B=B, L3d=L, L2d=S, wpack=wpack, is_cross=1, workspace=ws)
    one = dict(x=d3, x_bstride=L * C, src=d2, src_bstride=S * C, y=y3, B=B, L=L, S=S, wpack=wpack, workspace=ws)
    refused = [("ophip_encoder_layer_full_x3", dict(two, y3d=d3)),                       # in place
               ("ophip_encoder_layer_full_x3", dict(two, y2d=d2)),
               ("ophip_encoder_layer_full_x3_stream", dict(one, y=d3)),
               ("ophip_encoder_layer_full_x3_stream", dict(one, src=d3, S=L, src_bstride=L * C, y=d3)),
               ("ophip_encoder_layer_full_x3_stream", dict(one, x_bstride=L * C - 4)),  # batch elements overlap
               ("ophip_encoder_layer_full_x3_stream", dict(one, src_bstride=128)),
               ("ophip_encoder_layer_full_x3_stream", dict(one, x_bstride=L * C + 2)),  # not a multiple of 4
               ("ophip_encoder_layer_full_x3_stream", dict(one, src_bstride=S * C + 1))]
    refused += [("ophip_encoder_layer_full_x3", dict(two, **{n: None})) for n in ("x3d", "x2d", "y3d", "y2d", "wpack", "workspace")]
    refused += [("ophip_encoder_layer_full_x3_stream", dict(one, **{n: None})) for n in ("x", "src", "y", "wpack", "workspace")]
    before = (d3.clone(), d2.clone())
    try:
        for kernel in ("full_qkv", "full_flash", "full_tail"):
            hip.timing_select(kernel)
            for entry, named in refused:
                with pytest.raises(ValueError):
                    hip.launch(entry, named)
            assert hip.timing_read()[0] == 0, kernel
        torch.cuda.synchronize()
        assert is_nan_fill(o3) and is_nan_fill(o2) and is_nan_fill(ws), "a rejected call wrote to an output or to the workspace"
        assert torch.equal(d3, before[0]) and torch.equal(d2, before[1])
        hip.launch("ophip_encoder_layer_full_x3_stream", dict(one, B=1))                 # the counter counts: a sound call is one full_tail launch
        assert hip.timing_read()[0] == 1
    finally:
        hip.timing_select("")
    torch.cuda.synchronize()
    assert not bool(torch.isnan(y3[0]).any()) and is_nan_fill(o3[L:])
    a.check()
