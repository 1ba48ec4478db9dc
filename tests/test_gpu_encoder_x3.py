"""The split-bf16 coarse encoder layer on the device -- ``ophip_encoder_layer_x3w8`` with its ``_masked``, ``_masks``, ``_streams``, ``_streams_masks``
and ``_frag`` forms and ``ophip_encoder_kv_first_x3w8`` (csrc/encoder_x3w8.hip: ``enc_x3w8_kernel``, ``kv_tail``, ``kv_sum_w8_kernel``) -- and the
exact-f32 layer (csrc/encoder.hip) against the UN-ROUNDED float64 layer of tests/x3_faithful.py, at the stream lengths where each loop and guard can go
wrong.  Outputs start as NaN and the whole workspace as 0xFF bytes; every check first asserts that nothing it reads is NaN.

Per call (tests/test_x3_faithful_cpu.py shows that the stand-in ALONE stays inside every bar, and that each bar rejects wrong kernels):

  (a) the K^T V | Ksum block, read back from the workspace and decoded (``xf.decode_kv_block``): ``hi + lo`` and Ksum against the reference's, each
      element in units of the sum of the magnitudes of its terms, within ``xf.BLOCK_BAR`` of the block's family (twice the stand-in's worst) and, one
      level down (``xf.kv_terms_deep``), within ``xf.BLOCK_DEEP_BAR``; ``lo`` is a remainder of ``hi``;
  (b) every output element against the reference FED THE DEVICE'S BLOCK, in units of ``max(1, max |ref row|)``, within ``xf.ROWS_FORCED_BAR``; and
      against the reference fed its own block within ``xf.ROWS_FREE_BAR``; on unit-variance inputs today's 3e-4 / 1e-4 as well.

Measured on the MI355X (the tests print them; worst per case family) next to the CPU stand-in of the kernel.  Block: by family of the block
("many" | "one_term" | "outliers", ``xf.block_family``) and one level down; rows: forced | free:

    case family                             block many         block one_term     block outliers     one level down     rows forced        rows free
                                            device  stand-in   device  stand-in   device  stand-in   device  stand-in   device  stand-in   device  stand-in
    seven new + four old shapes             1.44e-5 1.44e-5    5.26e-4 5.38e-4    --      --         2.30e-6 2.30e-6    1.03e-5 1.03e-5    1.21e-5 1.09e-5
    K / V half, 65 to 194 slabs             1.60e-6 1.60e-6    1.23e-3 1.24e-3    --      --         1.99e-6 1.99e-6    --      --         --      --
    three shapes x eight mask cases         1.24e-5 1.23e-5    1.21e-2 1.22e-2    --      --         2.25e-6 2.25e-6    1.05e-5 1.05e-5    1.19e-5 1.14e-5
    three shapes x up, down, outliers       1.32e-5 1.32e-5    --      --         1.25e-4 1.23e-4    1.84e-6 1.84e-6    1.44e-5 1.90e-5    1.86e-5 1.90e-5
    bars (twice the stand-in's worst)       3.2e-5             2.8e-2             2.8e-4             5.2e-6             2.4e-5 | 4.2e-5    2.6e-5 | 4.2e-5

On unit-variance inputs the device needs at most 0.42 of today's 3e-4 / 1e-4 (stand-in: 0.36).  The exact-f32 layer: block error at most 0.30 of
``xf.f32_kv_slack`` (f32 restatement on the CPU: 0.07), rows at most 0.13 of ``LAYER_TOL["f32"]`` (restatement: 0.11).  The device's figures lie at the
stand-in's, family by family, so neither kernel is wrong at any edge run here and the stand-in misses no operand point; every bar above comes from the
stand-in or from reasoning, none from these device figures.  The forms (``_streams``, ``_streams_masks``, ``_frag``, ``kv_first`` + ``kv_from_prev = 2``)
are bit for bit the two-stream call at (1, 15, 17), (2, 48, 49) and (1, 96, 97).
"""
import ctypes

import pytest
import torch

from onepose_st_amd import hip, layercall, packing
from tests import x3_faithful as xf

pytestmark = pytest.mark.gpu

P = xf.LAYER


@pytest.fixture(scope="module")
def dev():
    assert torch.cuda.is_available(), "these tests need the MI355X"
    hip.load()
    return torch.device("cuda:0")


@pytest.fixture(scope="module")
def wpack(sd, dev):
    w = packing.pack_coarse_layer_x3w8(sd, P).to(dev)
    assert w.numel() == layercall.wpack_bytes("bf16x3")
    return w


@pytest.fixture(scope="module")
def wpack_f32(sd, dev):
    return packing.pack_coarse_layer(sd, P).to(dev)


def workspace(dev, B, L3, L2):
    """every byte 0xFF: NaN as f32 and as bf16"""
    return torch.full((layercall.workspace_bytes("bf16x3", B, L3, L2),), 255, dtype=torch.uint8, device=dev)


def read_block(ws, B, L3, L2):
    torch.cuda.synchronize()
    off = xf.kv_block_offset(ws.data_ptr(), B, L3, L2)
    assert off + B * 2 * xf.KV_BLOCK_BYTES <= ws.numel() and xf.KV_BLOCK_BYTES == layercall.kv_block_bytes()
    return xf.decode_kv_block(ws[off:off + B * 2 * xf.KV_BLOCK_BYTES].cpu().view(B, 2, xf.KV_BLOCK_BYTES))


def dmask(m, dev):
    return None if m is None else m.to(dev).view(torch.uint8).contiguous()


def layer(d3, d2, w, ws, cross, **kw):
    """one call on the device streams ``d3, d2``; returns (y3, y2) on the device (NaN where the call wrote nothing)"""
    y3, y2 = torch.full_like(d3, float("nan")), torch.full_like(d2, float("nan"))
    streams = kw.get("streams", 3)
    layercall.layer(d3, d2, y3 if streams & 1 else None, y2 if streams & 2 else None, mode="bf16x3", wpack=w, is_cross=int(cross), workspace=ws, **kw)
    torch.cuda.synchronize()
    return y3, y2


def check_block(sd, x, m, regime, blk, label):
    """(a) for one stream's block ``blk = (hi, lo, Ksum)``"""
    assert all(bool(torch.isfinite(t).all()) for t in blk), f"{label}: the block has unwritten elements"
    assert xf.lo_is_remainder(blk[0], blk[1]), f"{label}: the lo plane is no remainder of the hi plane"
    ref, fam = xf.reference_kv(sd, P, x, m), xf.block_family(regime, x.shape[1], m)
    e, d = max(xf.block_error(blk, ref, xf.kv_terms(sd, P, x, m))), max(xf.block_error(blk, ref, xf.kv_terms_deep(sd, P, x, m)))
    print(f"{label}: block {e:.2e} ({fam}, bar {xf.BLOCK_BAR[fam]:.1e}), one level down {d:.2e} (bar {xf.BLOCK_DEEP_BAR:.1e})")
    assert e <= xf.BLOCK_BAR[fam] and d <= xf.BLOCK_DEEP_BAR, (label, e, d)


def check(sd, x3, x2, cross, masks, regime, y3, y2, block, label):
    """(a) and (b) of the module docstring; ``x3, x2`` CPU f32 (what the device read), ``y3, y2`` the device's output, ``block`` decoded"""
    hi, lo, ksum = block
    blocks = tuple((hi[:, s], lo[:, s], ksum[:, s]) for s in (0, 1))
    y3, y2 = y3.cpu(), y2.cpu()
    assert bool(torch.isfinite(y3).all()) and bool(torch.isfinite(y2).all()), f"{label}: output rows were not written"
    for s, x in enumerate((x3, x2)):
        check_block(sd, x, masks[s], regime, blocks[s], f"{label} stream {s}")
    f = xf.figures(sd, P, x3, x2, bool(cross), masks, y3, y2, blocks)
    rf = xf.rows_family(regime)
    print(f"{label}: rows forced {f['forced']:.2e} (bar {xf.ROWS_FORCED_BAR[rf]:.1e}) free {f['free']:.2e} (bar {xf.ROWS_FREE_BAR[rf]:.1e}), "
          f"error / today's 3e-4 | 1e-4: {f['old']:.3f}")
    assert f["forced"] <= xf.ROWS_FORCED_BAR[rf] and f["free"] <= xf.ROWS_FREE_BAR[rf], (label, f)
    if regime == "randn":
        assert f["old"] <= 1.0, (label, f)


@pytest.mark.parametrize("cross", [0, 1])
@pytest.mark.parametrize("B,L3,L2", xf.SHAPES + xf.OLD_SHAPES)
def test_layer_and_kv_block(sd, dev, wpack, cross, B, L3, L2):
    x3, x2 = xf.inputs(B, L3, L2)
    ws = workspace(dev, B, L3, L2)
    y3, y2 = layer(x3.to(dev), x2.to(dev), wpack, ws, cross)
    check(sd, x3, x2, cross, (None, None), "randn", y3, y2, read_block(ws, B, L3, L2), f"B={B} L=({L3},{L2}) cross={cross}")


@pytest.mark.parametrize("B,L3,L2", xf.KV_SHAPES)
def test_kv_first_block_of_long_streams(sd, dev, wpack, B, L3, L2):
    """``kv_sum_w8_kernel`` past 64 and past 128 slabs per stream (its remainder loop and its three-way unrolled loop), K / V half only"""
    x3, x2 = xf.inputs(B, L3, L2)
    ws = workspace(dev, B, L3, L2)
    layercall.kv_first(x3.to(dev), x2.to(dev), wpack=wpack, slot=0, workspace=ws, mask2d=None)
    hi, lo, ksum = read_block(ws, B, L3, L2)
    for s, x in enumerate((x3, x2)):
        check_block(sd, x, None, "randn", (hi[:, s], lo[:, s], ksum[:, s]), f"K / V half B={B} L=({L3},{L2}) stream {s}")


@pytest.mark.parametrize("cross", [0, 1])
@pytest.mark.parametrize("regime", xf.REGIMES)
@pytest.mark.parametrize("B,L3,L2", xf.REGIME_SHAPES)
def test_input_regimes(sd, dev, wpack, cross, regime, B, L3, L2):
    x3, x2 = xf.inputs(B, L3, L2, regime=regime)
    ws = workspace(dev, B, L3, L2)
    y3, y2 = layer(x3.to(dev), x2.to(dev), wpack, ws, cross)
    check(sd, x3, x2, cross, (None, None), regime, y3, y2, read_block(ws, B, L3, L2), f"B={B} L=({L3},{L2}) {regime} cross={cross}")


@pytest.mark.parametrize("cross", [0, 1])
@pytest.mark.parametrize("mcase", xf.MASK_CASES, ids=lambda c: "-".join(map(str, c)))
@pytest.mark.parametrize("B,L3,L2", xf.MASK_SHAPES)
def test_masked_layer_and_kv_block(sd, dev, wpack, cross, mcase, B, L3, L2):
    x3, x2 = xf.inputs(B, L3, L2)
    m3, m2 = xf.masks_of(mcase, B, L3, L2)
    u3, u2, _ = xf.reference_streams(sd, P, x3, x2, bool(cross))
    r3, r2, _ = xf.reference_streams(sd, P, x3, x2, bool(cross), (m3, m2))
    assert m3 is None or (u3 - r3).abs().max().item() > 1e-2                                   # each mask matters
    assert m2 is None or (u2 - r2).abs().max().item() > 1e-2
    ws = workspace(dev, B, L3, L2)
    kw = dict(query_mask=dmask(m2, dev)) if mcase[0] == "masked" else dict(masks=(dmask(m3, dev), dmask(m2, dev)))
    y3, y2 = layer(x3.to(dev), x2.to(dev), wpack, ws, cross, **kw)
    check(sd, x3, x2, cross, (m3, m2), "randn", y3, y2, read_block(ws, B, L3, L2), f"B={B} L=({L3},{L2}) cross={cross} {'/'.join(map(str, mcase))}")


def frag_rows_of(cws, ptr, B, L):
    """the fragment planes of one stream inside the coarse workspace ``cws`` -> ``[B][rows padded to 128][plane hi, lo][256]`` f32 (CPU): row ``r``
    of k-step ``ks`` sits in 1 KiB-per-plane fragment ``(r / 32) 16 + ks`` as ``[plane][half][r % 32][8 bf16]``, feature ``16 ks + 8 half + e``
    (encoder_x3w8.hip:369-381)"""
    rows = (L + 127) // 128 * 128
    off, n = ptr.value - cws.data_ptr(), B * (rows // 32) * 32768
    assert 0 <= off and off + n <= cws.numel() * cws.element_size()
    raw = cws.view(torch.uint8)[off:off + n].cpu().view(torch.bfloat16).float().view(B, rows // 32, 16, 2, 2, 32, 8)
    return raw.permute(0, 1, 5, 3, 2, 4, 6).reshape(B, rows, 2, 256)


@pytest.mark.parametrize("cross", [0, 1])
@pytest.mark.parametrize("B,L3,L2", xf.FORM_SHAPES)
def test_forms_are_the_two_stream_call_bit_for_bit(sd, dev, wpack, cross, B, L3, L2):
    """``_streams``, ``_streams_masks``, ``_frag`` and ``kv_first`` + ``kv_from_prev = 2`` at a 16-token edge, a workgroup edge and two workgroups;
    ``_frag``: the planes hold the split of ``y / 16`` and rows from L up to the 128-row padding are zero, the planes having started as NaN."""
    x3, x2 = xf.inputs(B, L3, L2)
    d3, d2 = x3.to(dev), x2.to(dev)
    y3, y2 = layer(d3, d2, wpack, workspace(dev, B, L3, L2), cross)
    assert bool(torch.isfinite(y3).all()) and bool(torch.isfinite(y2).all())
    masks = (dmask(xf.mask("random", B, L3, 5), dev), dmask(xf.mask("random", B, L2, 11), dev))
    m3, m2 = layer(d3, d2, wpack, workspace(dev, B, L3, L2), cross, masks=masks)
    assert bool(torch.isfinite(m3).all()) and bool(torch.isfinite(m2).all()) and not torch.equal(m2, y2)
    for streams in (1, 2):
        for want, kw in (((y3, y2), {}), ((m3, m2), dict(masks=masks))):
            o3, o2 = layer(d3, d2, wpack, workspace(dev, B, L3, L2), cross, streams=streams, **kw)
            ran, idle = ((o3, want[0]), o2) if streams == 1 else ((o2, want[1]), o3)
            assert torch.equal(*ran) and bool(torch.isnan(idle).all()), (streams, sorted(kw))
    # the K / V half ahead of the layer
    ws = workspace(dev, B, L3, L2)
    layercall.kv_first(d3, d2, wpack=wpack, slot=0, workspace=ws, mask2d=None)
    k3, k2 = layer(d3, d2, wpack, ws, cross, kv_from_prev=2)
    assert torch.equal(k3, y3) and torch.equal(k2, y2)
    # the similarity kernel's operand fragments
    cws = torch.full((hip.load().ophip_coarse_workspace_floats(B, L3, L2),), float("nan"), device=dev)
    pa, pb = ctypes.c_void_p(), ctypes.c_void_p()
    hip.call("ophip_coarse_frag_planes", hip.ptr(cws), B, L3, L2, ctypes.byref(pa), ctypes.byref(pb))
    f3, f2 = layer(d3, d2, wpack, workspace(dev, B, L3, L2), cross, frag=(pa, pb))
    assert torch.equal(f3, y3) and torch.equal(f2, y2)
    for ptr, y, L in ((pa, y3, L3), (pb, y2, L2)):
        planes = frag_rows_of(cws, ptr, B, L)
        assert not bool(torch.isnan(planes).any()), "fragment rows up to the 128-row padding were not all written"
        hi, lo = xf.bf.split(y.cpu() * 0.0625)
        assert torch.equal(planes[:, :L, 0], hi) and torch.equal(planes[:, :L, 1], lo)
        assert bool((planes[:, L:] == 0).all())


# ---- the exact-f32 layer ---------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("cross", [0, 1])
@pytest.mark.parametrize("B,L3,L2", xf.F32_SHAPES)
def test_f32_layer_and_kv_block(sd, dev, wpack_f32, cross, B, L3, L2):
    """``ophip_encoder_layer`` at its own edges (32-token workgroups, a 16-way ``kv_sum``): rows at ``LAYER_TOL["f32"]`` against the float64
    reference, the ``[B][2][KV_FLOATS]`` block within ``xf.f32_kv_slack``."""
    x3, x2 = xf.inputs(B, L3, L2)
    d3, d2 = x3.to(dev), x2.to(dev)
    ws = torch.full((layercall.workspace_bytes("f32", B, L3, L2) // 4,), float("nan"), device=dev)
    y3, y2 = torch.full_like(d3, float("nan")), torch.full_like(d2, float("nan"))
    layercall.layer(d3, d2, y3, y2, mode="f32", wpack=wpack_f32, is_cross=cross, workspace=ws)
    torch.cuda.synchronize()
    off = xf.f32_kv_block_offset(B, L3, L2)
    assert off + B * 2 * xf.F32_KV_FLOATS == ws.numel()
    KV, Ksum = xf.decode_f32_kv_block(ws[off:].cpu().view(B, 2, xf.F32_KV_FLOATS))
    assert bool(torch.isfinite(KV).all()) and bool(torch.isfinite(Ksum).all()), "the block has unwritten elements"
    r3, r2, kv = xf.reference_streams(sd, P, x3, x2, bool(cross))
    use = 0.0
    for s, x in enumerate((x3, x2)):
        slack = xf.f32_kv_slack(sd, P, x)
        use = max(use, ((KV[:, s].double() - kv[s][0]).abs() / slack[0]).max().item(), ((Ksum[:, s].double() - kv[s][1]).abs() / slack[1]).max().item())
    y3, y2 = y3.cpu(), y2.cpu()
    assert bool(torch.isfinite(y3).all()) and bool(torch.isfinite(y2).all()), "output rows were not written"
    rows = max(((y.double() - r).abs() / (xf.F32_ATOL + xf.F32_RTOL * r.abs())).max().item() for y, r in ((y3, r3), (y2, r2)))
    print(f"f32 B={B} L=({L3},{L2}) cross={cross}: block error / slack {use:.3f}, row error / bar {rows:.3f}")
    assert use <= 1.0 and rows <= 1.0
