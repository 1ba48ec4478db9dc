"""The coarse encoder layer of the plain-bf16 mode on the device -- ``ophip_encoder_layer_bf16`` / ``_masked`` (csrc/encoder_bf16.hip:
``kv_reduce_bf16_kernel``, ``kv_sum_bf16_kernel``, ``attn_apply_bf16_kernel`` and its fused K|V tail) -- against the float64 restatement of
tests/bf16_faithful.py that rounds where the kernels round.  Outputs and the workspace start as NaN.

Per call two checks (tests/test_bf16_faithful_cpu.py shows that the reference ALONE, as an f32 stand-in of itself, stays inside every bar):

  (a) the K^T V | Ksum block, read back from the workspace and decoded (``bf.decode_kv_block``), against ``coarse_kv_faithful``.  A block
      element differs from ``bf16_round(KV_ref)`` in at most 1 % of the elements (stand-in: 0 - 0.15 %), and then by one bf16 step -- or, where the
      sum over the tokens cancels to a value whose own step is smaller than what f32 arithmetic leaves (the stand-in itself is up to 14 steps
      away there, and 28172 next to zero), within the slack of ``bf.coarse_kv_slack``, which is reasoning (accumulation + two operand flips), not
      a measurement.  Ksum (f32) within its slack of the same function.  The lo plane is the split's remainder of some f32 value.
  (b) both streams against ``coarse_layer_faithful`` FED THE DEVICE'S BLOCK (one KV element one step away reaches every token of a stream:
      the stand-in fed its own KV drops to a token share of 0.54): every element within ``bf.COARSE_WORST_BAR`` = 1.6e-2, twice the worst
      element of the stand-in over these very inputs (7.6e-3; one flip moves an output by a fixed 2^-8-scaled amount and two may coincide), and
      at least HALF of the tokens of each stream with all 256 outputs at the f32 bar (1e-4 / 2e-5; stand-in >= 0.91).  The un-rounded
      computation is 1.8e-2 - 2.4e-2 away and keeps NO token at the f32 bar, so the share sees one missing rounding point, a wrong ``1 / L`` or
      ``S``, a stale slab or a padded token in Ksum; the worst-element bar lies under the un-rounded distance, not far under it.

Measured on the MI355X (the tests print them) next to the CPU stand-in of the reference:

    case family                    KV elements that differ          most steps apart      token share (lowest)   worst element
                                   device          stand-in         device   stand-in     device   stand-in      device   stand-in
    six shapes x self, cross       0 - 0.146 %     0 - 0.146 %      14       28172        0.909    0.909         7.0e-3   6.9e-3
    three shapes x three masks     0.012 - 0.244 % 0.012 - 0.146 %  246      28172        0.967    0.966         7.7e-3   7.6e-3
    fused chain, each layer        0 - 0.024 %     --               2        --           0.933    --            7.1e-3   --

No KV element lies outside the slack (device and stand-in); Ksum: device within 0.12 of its slack (``__expf``: a few flips of ``phi(K)``), stand-in
identical to the reference.  The device's shares lie at the stand-in's, case by case (the lowest, 0.909, is the same case: 3 of 33 tokens), so the
reference misses no rounding point; every bar above comes from the stand-in or from reasoning, none from these device figures.  The chain's
layers 1 and 2 read the device's previous output, for which no stand-in is computed.
"""
import pytest
import torch

from onepose_st_amd import hip, layercall, packing
from tests import bf16_faithful as bf

pytestmark = pytest.mark.gpu

P = bf.COARSE_LAYER


@pytest.fixture(scope="module")
def dev():
    assert torch.cuda.is_available(), "these tests need the MI355X"
    hip.load()
    return torch.device("cuda:0")


@pytest.fixture(scope="module")
def wpack(sd, dev):
    cache = {}

    def get(p):
        if p not in cache:
            cache[p] = packing.pack_coarse_layer_bf16(sd, p).to(dev)
            assert cache[p].numel() == layercall.wpack_bytes("bf16")
        return cache[p]
    return get


def workspace(dev, B, L3, L2):
    """every byte 0xFF: NaN as f32 and as bf16"""
    return torch.full((layercall.workspace_bytes("bf16", B, L3, L2),), 255, dtype=torch.uint8, device=dev)


def layer(d3, d2, w, ws, cross, mask=None, w_next=None, kv_from_prev=0, slot=0, nsplit=1, y3=None, y2=None):
    """one call on the device streams ``d3, d2``; returns (y3, y2) on the device and the decoded block on the CPU"""
    B, L3, L2 = d3.shape[0], d3.shape[1], d2.shape[1]
    y3 = torch.full_like(d3, float("nan")) if y3 is None else y3
    y2 = torch.full_like(d2, float("nan")) if y2 is None else y2
    layercall.layer(d3, d2, y3, y2, mode="bf16", wpack=w, wpack_next=w_next, nsplit=nsplit, is_cross=int(cross), kv_from_prev=kv_from_prev, slot=slot,
                    workspace=ws, query_mask=None if mask is None else mask.to(d3.device).view(torch.uint8).contiguous())
    torch.cuda.synchronize()
    off = bf.kv_block_offset(ws.data_ptr(), B, L3, L2)
    blk = ws[off:off + B * 2 * bf.KV_BLOCK_BYTES].cpu().view(B, 2, bf.KV_BLOCK_BYTES)
    return y3, y2, bf.decode_kv_block(blk)


def check(sd, p, x3, x2, cross, mask, y3, y2, block, label):
    """(a) and (b) of the module docstring; ``x3, x2`` CPU f32 (what the device read), ``y3, y2`` the device's output.  Returns the figures."""
    hi, lo, ksum = block
    fig = dict(kv_off=0.0, kv_bad=0, kv_max=0, ksum=0.0)
    assert bool(torch.isfinite(hi).all()) and bool(torch.isfinite(lo).all()) and bool(torch.isfinite(ksum).all()), f"{label}: the block has unwritten elements"
    for s, (x, m) in enumerate(((x3, None), (x2, mask))):                                     # (a)
        KV, Ks = bf.coarse_kv_faithful(sd, p, x, m)
        kv_slack, ks_slack = bf.coarse_kv_slack(sd, p, x, m)
        off, bad, mx = bf.coarse_kv_check(hi[:, s].double(), KV, kv_slack)
        kerr = ((ksum[:, s].double() - Ks).abs() / ks_slack).max().item()
        fig = dict(kv_off=max(fig["kv_off"], off), kv_bad=fig["kv_bad"] + bad, kv_max=max(fig["kv_max"], mx), ksum=max(fig["ksum"], kerr))
        # lo = bf16(total - hi) of an f32 total that rounds to hi: at most half a bf16 step of hi, and hi + lo within the slack of the reference too
        half_step = 2.0 ** -8 * hi[:, s].abs().double() + 2.0 ** -134
        assert bool((lo[:, s].abs().double() <= half_step).all()), f"{label}: stream {s}: lo plane is no remainder of the hi plane"
        tot = hi[:, s].double() + lo[:, s].double()
        assert bool(((tot - KV).abs() <= kv_slack + 2.0 ** -16 * KV.abs() + 2.0 ** -134).all()), f"{label}: stream {s}: hi + lo"
    print(f"{label}: KV {100 * fig['kv_off']:.3f} % of the elements differ (max {fig['kv_max']} steps, {fig['kv_bad']} outside the slack); "
          f"Ksum error / slack {fig['ksum']:.3f}")
    assert fig["kv_bad"] == 0, (label, fig)
    assert fig["kv_off"] <= bf.COARSE_KV_ULP_SHARE, (label, fig)
    assert fig["ksum"] <= 1.0, (label, fig)
    dev_kv = ((hi[:, 0], ksum[:, 0]), (hi[:, 1], ksum[:, 1]))                                 # (b)
    r3, r2, _ = bf.coarse_streams_faithful(sd, p, x3, x2, bool(cross), mask, kv=dev_kv)
    y3, y2 = y3.cpu(), y2.cpu()
    assert bool(torch.isfinite(y3).all()) and bool(torch.isfinite(y2).all()), f"{label}: output rows were not written"
    fig["share"] = (bf.token_share_at_f32_bar(y3, r3), bf.token_share_at_f32_bar(y2, r2))
    fig["worst"] = ((y3.double() - r3).abs().max().item(), (y2.double() - r2).abs().max().item())
    print(f"{label}: token share at the f32 bar 3D {fig['share'][0]:.3f} 2D {fig['share'][1]:.3f} (required 0.5); worst element "
          f"3D {fig['worst'][0]:.2e} 2D {fig['worst'][1]:.2e} (bar {bf.COARSE_WORST_BAR:.1e})")
    assert max(fig["worst"]) <= bf.COARSE_WORST_BAR, (label, fig)
    assert min(fig["share"]) >= 0.5, (label, fig)
    return fig


@pytest.mark.parametrize("cross", [0, 1])
@pytest.mark.parametrize("B,L3,L2", bf.COARSE_SHAPES)
def test_layer_and_kv_block(sd, dev, wpack, cross, B, L3, L2):
    x3, x2 = bf.coarse_inputs(B, L3, L2)
    y3, y2, block = layer(x3.to(dev), x2.to(dev), wpack(P), workspace(dev, B, L3, L2), cross)
    check(sd, P, x3, x2, cross, None, y3, y2, block, f"B={B} L=({L3},{L2}) cross={cross}")


@pytest.mark.parametrize("cross", [0, 1])
@pytest.mark.parametrize("kind", bf.COARSE_MASKS)
@pytest.mark.parametrize("B,L3,L2", bf.COARSE_MASK_SHAPES)
def test_masked_layer_and_kv_block(sd, dev, wpack, cross, kind, B, L3, L2):
    x3, x2 = bf.coarse_inputs(B, L3, L2)
    mask = bf.coarse_mask(kind, B, L2)
    u3, u2, _ = bf.coarse_streams_faithful(sd, P, x3, x2, bool(cross), None)
    m3, m2, _ = bf.coarse_streams_faithful(sd, P, x3, x2, bool(cross), mask)
    assert (u2 - m2).abs().max().item() > 1e-2 and (not cross or (u3 - m3).abs().max().item() > 1e-4)        # the mask matters
    y3, y2, block = layer(x3.to(dev), x2.to(dev), wpack(P), workspace(dev, B, L3, L2), cross, mask)
    check(sd, P, x3, x2, cross, mask, y3, y2, block, f"B={B} L=({L3},{L2}) cross={cross} mask={kind}")


@pytest.mark.parametrize("B,L3,L2", bf.COARSE_CHAIN_SHAPES)
def test_fused_chain(sd, dev, wpack, B, L3, L2):
    """(self, cross, self) with the next layer's K|V slabs from the fused tail (``wpack_next``, ``kv_from_prev = 1``, alternating ``slot``):
    bit for bit the stand-alone chain, block included; and (a), (b) per layer with the reference fed the device's previous output, so errors
    do not compound and a wrong slab slot or a stale ping-pong set shows in the block of the layer it hits."""
    names = ["self", "cross", "self"]
    ps = [f"loftr_coarse.layers.{li}." for li in range(3)]
    x3, x2 = bf.coarse_inputs(B, L3, L2, seed=5)

    def chain(fused):
        ws = workspace(dev, B, L3, L2)
        a3, a2, out = x3.to(dev), x2.to(dev), []
        for li, nm in enumerate(names):
            nxt = wpack(ps[li + 1]) if (fused and li + 1 < 3) else None
            y3, y2, block = layer(a3, a2, wpack(ps[li]), ws, nm == "cross", None, nxt, 1 if (fused and li > 0) else 0, (li & 1) if fused else 0)
            out.append((a3.cpu(), a2.cpu(), y3, y2, block))
            a3, a2 = y3, y2
        return out
    fused, alone = chain(True), chain(False)
    for li, (f, a) in enumerate(zip(fused, alone)):
        assert torch.equal(f[2], a[2]) and torch.equal(f[3], a[3]), f"layer {li}: the fused chain's output differs from the stand-alone chain's"
        assert all(torch.equal(u, v) for u, v in zip(f[4], a[4])), f"layer {li}: the fused tail's block differs from kv_reduce's"
    for li, (i3, i2, y3, y2, block) in enumerate(fused):
        check(sd, ps[li], i3, i2, names[li] == "cross", None, y3, y2, block, f"chain B={B} L=({L3},{L2}) layer {li} ({names[li]})")


def test_arguments(dev, wpack):
    B, L3, L2 = 1, 33, 40
    x3, x2 = (t.to(dev) for t in bf.coarse_inputs(B, L3, L2))
    w, ws = wpack(P), workspace(dev, B, L3, L2)
    mask = torch.ones(B, L2, dtype=torch.bool)
    layer(x3, x2, w, ws, 0, mask)                                                    # the arguments below differ from a call that works in one thing each
    with pytest.raises(ValueError):
        layer(x3, x2, w, ws, 0, nsplit=3)
    with pytest.raises(ValueError):
        layer(x3, x2, w, ws, 0, slot=2)
    with pytest.raises(ValueError):
        layer(x3, x2, w, ws, 0, y3=x3)
    with pytest.raises(ValueError):
        layer(x3, x2, w, ws, 0, y2=x2)
    with pytest.raises(ValueError):
        layer(x3, x2, w, ws, 0, mask, slot=2)
    y3, y2 = torch.full_like(x3, float("nan")), torch.full_like(x2, float("nan"))
    entry, named = layercall.plan_layer(x3, x2, y3, y2, mode="bf16", wpack=w, is_cross=0, workspace=ws, query_mask=mask)
    assert entry == "ophip_encoder_layer_bf16_masked"
    with pytest.raises(ValueError):
        hip.launch(entry, dict(named, query_mask=None))                             # the masked entry refuses a NULL mask
    torch.cuda.synchronize()
    assert bool(torch.isnan(y3).all()) and bool(torch.isnan(y2).all())              # a refused call launches nothing
