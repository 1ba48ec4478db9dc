"""The split-bf16 coarse encoder layer (csrc/encoder_x3w8.hip, the default precision) and the exact-f32 layer (csrc/encoder.hip) against the
UN-ROUNDED float64 layer: reference, stand-in, block decoders, cases and bars shared by tests/test_x3_faithful_cpu.py and
tests/test_gpu_encoder_x3.py.

Reference = ``bf.coarse_kv_faithful`` / ``bf.coarse_layer_faithful`` with ``rounded=False`` (float64, f32 weights; pinned against the oracle
in tests/test_bf16_faithful_cpu.py), here with a padding mask on EACH stream (:func:`reference_streams`).  No rounding-faithful reference:
the split keeps 16 mantissa bits, so operand rounding (2^-17) is of the order of f32 accumulation and the un-rounded layer is the truth.

Stand-in = the same restatement in float32 with the ``split`` of ``bf16_faithful`` (hi + lo, lo.lo dropped) at every operand point of the
kernel (:func:`standin_kv`, :func:`standin_layer`).  It is never compared with the device: it sizes the bars.  What the device has and the
stand-in lacks -- ``__expf``, the hardware reciprocal, another association of the f32 sums -- is what the factor of two in every bar is for.

Statistics (section "bars" below):
  block   ``|hi + lo - KV_ref| / sum_tok |phiK| |V| / L`` and ``|Ksum - Ksum_ref| / sum_tok phiK``, worst element: a sum that cancels is judged
          by the size of its terms (``bf.coarse_kv_slack``);
  rows    ``|y - y_ref| / max(1, max |y_ref row|)``, worst element; "forced": the reference fed the block under test (a block error and a row
          error cannot hide each other), "free": the reference fed its own block.
"""
from __future__ import annotations

import torch
import torch.nn.functional as F

from tests import bf16_faithful as bf

f32, f64 = torch.float32, torch.float64
C, NH, HD, TOK = 256, 8, 32, 48                       # features, heads, head dim, tokens of one workgroup (encoder_x3w8.hip:22-23)
LAYER = bf.COARSE_LAYER
_phi = bf._phi


# ---- reference ------------------------------------------------------------------------------------------------------------------------

def reference_kv(sd, p, x, mask=None):
    """``(KV [B][8][32][32], Ksum [B][8][32])`` of the stream ``x`` as a source, float64, nothing rounded"""
    return bf.coarse_kv_faithful(sd, p, x, mask, f64, False)


def reference_streams(sd, p, x3, x2, cross, masks=(None, None), kv=None):
    """Both streams of one layer, float64, nothing rounded; ``masks = (mask of the first stream, of the second)`` (bool ``[B][L]``, 1 = real
    cell, or None): a stream's mask acts where it is a source (``phi(K) = 0``) and where it is a query (``phi(Q) = 0``).  ``kv`` =
    ((KV3, Ksum3), (KV2, Ksum2)) replaces the blocks (teacher forcing).  Returns ``(y3, y2, kv)``."""
    if kv is None:
        kv = (reference_kv(sd, p, x3, masks[0]), reference_kv(sd, p, x2, masks[1]))
    s3, s2 = (kv[1], kv[0]) if cross else (kv[0], kv[1])
    L = (x3.shape[1], x2.shape[1])
    y3 = bf.coarse_layer_faithful(sd, p, x3, s3[0], s3[1], L[1] if cross else L[0], masks[0], f64, False)
    y2 = bf.coarse_layer_faithful(sd, p, x2, s2[0], s2[1], L[0] if cross else L[1], masks[1], f64, False)
    return y3, y2, kv


def kv_terms(sd, p, x, mask=None):
    """``sum_tok |phiK| |V| / L`` ``[B][8][32][32]`` and ``sum_tok phiK`` ``[B][8][32]`` (float64): what a block element's error is measured in"""
    phiK, V = bf._coarse_kv_operands(sd, p, x, mask, f64, False)
    return torch.einsum("bsthd,bsthv->bhdv", phiK.abs(), V.abs()), phiK.sum((1, 2))


def kv_terms_deep(sd, p, x, mask=None):
    """The same one level down, for blocks that a FEW tokens carry (a one-token stream, a mask with one real cell, outlier tokens): there
    ``|phiK| |V|`` is no measure of a term's error, because V (and K) are themselves sums of 256 products that may cancel to nothing.  With
    ``aK = sum_c |x_c| |Wk_c|``, ``aV`` likewise, and ``phi``'s slope ``min(1, phiK)``: ``sum_tok (min(1, phiK) aK |V| + phiK aV) / L`` for KV and
    ``sum_tok min(1, phiK) aK`` + ``sum_tok phiK`` for Ksum."""
    B, L, _ = x.shape
    xa = x.to(f64)
    wk, wv = sd[p + "k_proj.weight"].detach().to(f64), sd[p + "v_proj.weight"].detach().to(f64)
    K, V = (xa @ wk.T).view(B, L, NH, HD), (xa @ wv.T).view(B, L, NH, HD)
    aK, aV = (xa.abs() @ wk.abs().T).view(B, L, NH, HD), (xa.abs() @ wv.abs().T).view(B, L, NH, HD)
    phiK = _phi(K)
    slope = torch.clamp(phiK, max=1.0) * aK
    if mask is not None:
        phiK, slope = phiK * mask.to(f64)[:, :, None, None], slope * mask.to(f64)[:, :, None, None]
    kv = (torch.einsum("bthd,bthv->bhdv", slope, V.abs()) + torch.einsum("bthd,bthv->bhdv", phiK, aV)) / L
    return kv, slope.sum(1) + phiK.sum(1)


# ---- stand-in -------------------------------------------------------------------------------------------------------------------------

def _w(sd, name):
    return sd[name].detach().to(f32)


def mm3(x, w, dtype, drop_lohi=False):
    """``x @ w.T`` as ``mma16x3`` forms it (tile_x3.h:24-28): lo.hi + hi.lo + hi.hi of the operands' f32 values, lo.lo dropped; sums in
    ``dtype``.  ``drop_lohi``: without the (activation lo) x (weight hi) term -- a kernel that forgot it."""
    xh, xl = (t.to(dtype) for t in bf.split(x.to(f32)))
    wh, wl = (t.to(dtype) for t in bf.split(w.to(f32)))
    out = xh @ wl.T
    if not drop_lohi:
        out = xl @ wh.T + out
    return out + xh @ wh.T


def _pair3(eq, a, b, dtype):
    """the three-term product of two ACTIVATION operands under ``eq``: a.lo b.hi + a.hi b.lo + a.hi b.hi"""
    ah, al = (t.to(dtype) for t in bf.split(a.to(f32)))
    bh, bl = (t.to(dtype) for t in bf.split(b.to(f32)))
    return torch.einsum(eq, al, bh) + torch.einsum(eq, ah, bl) + torch.einsum(eq, ah, bh)


# wrong kernels, each a variant of the stand-in (tests/test_x3_faithful_cpu.py::test_the_reference_separates_wrong_kernels)
WRONG_BLOCK = ["lohi_kv", "len48", "pad_in_ksum", "slab_out", "mask_leak"]
WRONG_ROWS = ["lohi_q", "lohi_merge", "lohi_w0", "lohi_w2", "no_block_lo", "srclen"]


def standin_kv(sd, p, x, mask=None, dtype=f32, wrong=None):
    """The block of stream ``x [B][L][256]`` as a source, as the kernels form it: ``(hi, lo, Ksum)`` in ``dtype``.  Operand points
    (csrc/encoder_x3w8.hip):
      1. X planes: the input rows split into (hi, lo) (``split8``, :216-219; in the fused tail the output rows, ``store_quad``, :368); Wk, Wv are
         the packer's (hi, lo) planes; K, V f32 accumulators of ``gemm_stage`` (:97, three terms per k-step, tile_x3.h:131-132);
      2. ``phi(K)`` (``elu_plus_one_fast``, :106; 0 for tokens >= L and masked cells) and ``V * inv_len`` with ``inv_len = 1.0f / (float)L``
         (:98, :107), each split (:113-118); ``KV = sum_tok phiK (x) V`` per 48-token slab, three terms (:123-126); ``Ksum = sum_tok phiK`` of the
         UN-split f32 values (:128-132);
      3. the slabs summed in f32 (``kv_sum_w8_kernel``, :416-437), the total split into the block's (hi, lo) planes (:441-450); Ksum stays f32 (:452).
    ``wrong``: one of WRONG_BLOCK ("mask_leak" is made by the caller, through ``mask``)."""
    B, L, _ = x.shape
    xs = x.to(f32)
    K = mm3(xs, _w(sd, p + "k_proj.weight"), dtype, wrong == "lohi_kv").view(B, L, NH, HD)                  # (1)
    V = mm3(xs, _w(sd, p + "v_proj.weight"), dtype, wrong == "lohi_kv").view(B, L, NH, HD)
    phiK = _phi(K)
    if mask is not None:
        phiK = phiK * mask.to(dtype)[:, :, None, None]
    Ldiv = TOK * ((L + TOK - 1) // TOK) if wrong == "len48" else L
    inv_len = (torch.tensor(1.0, dtype=f32) / torch.tensor(float(Ldiv), dtype=f32)).to(dtype)
    V = V * inv_len                                                                                        # (2)
    pad = (-L) % TOK
    phiK, V = F.pad(phiK, (0, 0, 0, 0, 0, pad)), F.pad(V, (0, 0, 0, 0, 0, pad))
    if wrong == "pad_in_ksum" and pad:
        phiK = phiK.clone()
        phiK[:, L] = 1.0                                                                                   # phi(0) = 1: V is 0 there, only Ksum moves
    phiK, V = phiK.view(B, -1, TOK, NH, HD), V.view(B, -1, TOK, NH, HD)
    slabs = _pair3("bsthd,bsthv->bshdv", phiK, V, dtype)
    ks = phiK.sum(2)
    if wrong == "slab_out":
        slabs, ks = slabs[:, :-1], ks[:, :-1]
    hi, lo = bf.split(slabs.sum(1).to(f32))                                                                # (3)
    return hi.to(dtype), lo.to(dtype), ks.sum(1)


def standin_layer(sd, p, x, block, S, q_mask=None, dtype=f32, wrong=None):
    """``y [B][L][256]`` of ``attn_apply`` (``enc_x3w8_kernel<false>``) for the query stream ``x`` given the source's ``block = (hi, lo, Ksum)``
    and its length ``S``.  Operand points (csrc/encoder_x3w8.hip):
      4. X planes (:216-219): operand of the Q GEMM (:244) and first half of the W0 operand (:318); the residual is the f32 x (:221-222, :365);
      5. ``phi(Q)`` (:255-256; 0 for masked query cells, :252) split (:261); the denominator ``phi(Q) . Ksum`` takes the UN-split f32 values (:257);
         the numerator is block (hi, lo) x phi(Q) (hi, lo), three terms (:265);
      6. the message ``num * rcp(den + 1e-6f) * S`` (:262, :267) split into the Y planes (:268): operand of the merge GEMM (:282);
      7. LayerNorm1 (f32, biased variance, eps 1e-5: ``wave_moments`` / ``merged_stats``, :285-296) split into the Y planes (:297): second half of
         the W0 operand (:319);
      8. ``relu(hidden)`` in two 256-wide chunks split into the hidden planes (:327-328): operand of the W2 GEMM (:333-334), both chunks into one
         accumulator.
    NOT split: the accumulators, LayerNorm2 and ``y = x + LN2`` (:365).  ``wrong``: one of WRONG_ROWS ("srclen" is made by the caller)."""
    B, L, _ = x.shape
    hi, lo, ksum = (t.to(dtype) for t in block)
    g = lambda name: sd[p + name].detach().to(dtype)
    xs = x.to(f32)
    phiQ = _phi(mm3(xs, _w(sd, p + "q_proj.weight"), dtype, wrong == "lohi_q").view(B, L, NH, HD))          # (4)
    if q_mask is not None:
        phiQ = phiQ * q_mask.to(dtype)[:, :, None, None]
    den = torch.einsum("blhd,bhd->blh", phiQ, ksum)
    qh, ql = (t.to(dtype) for t in bf.split(phiQ.to(f32)))
    eq = "blhd,bhdv->blhv"
    num = torch.einsum(eq, ql, hi) + torch.einsum(eq, qh, hi)                                               # (5)
    if wrong != "no_block_lo":
        num = num + torch.einsum(eq, qh, lo)
    eps = torch.tensor(1e-6, dtype=f32).to(dtype)
    msg = (num * ((1 / (den + eps)) * float(S))[..., None]).reshape(B, L, C)
    m = mm3(msg, _w(sd, p + "merge.weight"), dtype, wrong == "lohi_merge")                                  # (6)
    m = F.layer_norm(m, (C,), g("norm1.weight"), g("norm1.bias"), 1e-5)
    hid = torch.relu(mm3(torch.cat([xs.to(dtype), m], 2), _w(sd, p + "mlp.0.weight"), dtype, wrong == "lohi_w0"))   # (4), (7)
    w2 = _w(sd, p + "mlp.2.weight")
    o = mm3(hid[..., :C], w2[:, :C], dtype, wrong == "lohi_w2") + mm3(hid[..., C:], w2[:, C:], dtype, wrong == "lohi_w2")   # (8)
    return x.to(dtype) + F.layer_norm(o, (C,), g("norm2.weight"), g("norm2.bias"), 1e-5)


def standin_streams(sd, p, x3, x2, cross, masks=(None, None), dtype=f32, wrong=None, blocks=None):
    """Both streams as ``layer_x3w8`` runs them (encoder_x3w8.hip:543-544, :580-581): stream s attends to block s ("self") or 1 - s ("cross") with
    ``srclen`` = that source's length.  Returns ``(y3, y2, blocks)``, ``blocks[s] = (hi, lo, Ksum)``."""
    if blocks is None:
        kw = wrong if wrong in WRONG_BLOCK else None
        blocks = (standin_kv(sd, p, x3, masks[0], dtype, kw), standin_kv(sd, p, x2, masks[1], dtype, kw))
    s3, s2 = (blocks[1], blocks[0]) if cross else (blocks[0], blocks[1])
    L3, L2 = x3.shape[1], x2.shape[1]
    S3, S2 = (L2, L3) if cross else (L3, L2)
    if wrong == "srclen":
        S3, S2 = S2, S3
    lw = wrong if wrong in WRONG_ROWS else None
    return standin_layer(sd, p, x3, s3, S3, masks[0], dtype, lw), standin_layer(sd, p, x2, s2, S2, masks[1], dtype, lw), blocks


# ---- statistics -----------------------------------------------------------------------------------------------------------------------

def block_error(block, ref_kv, terms):
    """worst normalised error of ``block = (hi, lo, Ksum)`` against ``ref_kv = (KV, Ksum)``: (KV, Ksum)"""
    hi, lo, ksum = block
    kv = ((hi.to(f64) + lo.to(f64) - ref_kv[0]).abs() / terms[0]).max().item()
    ks = ((ksum.to(f64) - ref_kv[1]).abs() / terms[1]).max().item()
    return kv, ks


def row_error(y, ref):
    """worst ``|y - ref| / max(1, max |ref row|)``"""
    scale = ref.abs().amax(-1, keepdim=True).clamp(min=1.0)
    return ((y.to(f64) - ref).abs() / scale).max().item()


def lo_is_remainder(hi, lo):
    """``lo = bf16(total - hi)`` of an f32 total that rounds to ``hi``: at most half a bf16 step of ``hi`` (+ the subnormal term)"""
    return bool((lo.abs().to(f64) <= 2.0 ** -8 * hi.abs().to(f64) + 2.0 ** -134).all())


def figures(sd, p, x3, x2, cross, masks, y3, y2, blocks):
    """The three statistics of one call whose outputs are ``y3, y2`` and whose blocks are ``blocks[s] = (hi, lo, Ksum)`` (the device's, or the
    stand-in's): dict(block = (first stream's, second stream's), deep = the same by ``kv_terms_deep``, forced, free, old = worst
    ``|y - ref| / (OLD_ATOL + OLD_RTOL |ref|)``, un-forced)."""
    xs = (x3, x2)
    r3, r2, kv = reference_streams(sd, p, x3, x2, cross, masks)
    blk = tuple(max(block_error(blocks[s], kv[s], kv_terms(sd, p, xs[s], masks[s]))) for s in (0, 1))
    deep = tuple(max(block_error(blocks[s], kv[s], kv_terms_deep(sd, p, xs[s], masks[s]))) for s in (0, 1))
    own = tuple(((b[0].to(f64) + b[1].to(f64)), b[2].to(f64)) for b in blocks)
    f3, f2, _ = reference_streams(sd, p, x3, x2, cross, masks, kv=own)
    old = max(((y.to(f64) - r).abs() / (OLD_ATOL + OLD_RTOL * r.abs())).max().item() for y, r in ((y3, r3), (y2, r2)))
    return dict(block=blk, deep=deep, forced=max(row_error(y3, f3), row_error(y2, f2)), free=max(row_error(y3, r3), row_error(y2, r2)), old=old)


# ---- the x3w8 block: layout and place -------------------------------------------------------------------------------------------------

KV_PART_FLOATS = NH * 1024 + NH * 32                 # one 48-token slab: KV quads (f32) + Ksum (encoder_x3w8.hip:27)
KV_FRAG_BYTES = NH * 2 * 2 * 64 * 16                 # [head][vt][plane hi, lo][lane][8 bf16] (:28)
KV_BLOCK_BYTES = KV_FRAG_BYTES + NH * 32 * 4         # + Ksum f32 [head][32] (:29) = ophip_encoder_x3w8_kv_block_bytes()


def kv_block_offset(base_addr: int, B: int, L3: int, L2: int) -> int:
    """byte offset of the ``[B][2][KV_BLOCK_BYTES]`` block inside the workspace at address ``base_addr``: behind the two slab sets, at the
    next ADDRESS that is a multiple of 256 (``layer_x3w8``, encoder_x3w8.hip:513-519)"""
    tiles = (L3 + TOK - 1) // TOK + (L2 + TOK - 1) // TOK
    off = 2 * B * tiles * KV_PART_FLOATS * 4
    return off + (-(base_addr + off)) % 256


def decode_kv_block(blk: torch.Tensor):
    """``blk [..][KV_BLOCK_BYTES]`` uint8 (CPU) -> ``KV_hi, KV_lo [..][8][32 (d)][32 (v)]`` and ``Ksum [..][8][32]`` (f32).  ``kv_tail`` stores
    the quad ``D[d = 16 dt + 4 q + r][v = 16 vt + c16]`` of lane ``16 q + c16`` at slab float ``(((head 2 + dt) 2 + vt) 64 + lane) 4 + r``
    (encoder_x3w8.hip:119-127); ``kv_sum_w8_kernel`` puts it into elements ``4 dt + r`` of the 16-byte lane slot of fragment
    ``[head][vt][plane]`` (:438-450) -- the A operand ``A[row = v][k = 8 q + j]`` that ``attn_apply`` multiplies with ``phi(Q)`` (:196-197, :265).
    Ksum: ``[head][d]`` in feature order (:132, :452)."""
    lead = blk.shape[:-1]
    frag = blk[..., :KV_FRAG_BYTES].contiguous().view(torch.bfloat16).float().view(*lead, NH, 2, 2, 64, 8)
    ksum = blk[..., KV_FRAG_BYTES:].contiguous().view(torch.float32).view(*lead, NH, HD).clone()
    vt, lane, j = torch.meshgrid(torch.arange(2), torch.arange(64), torch.arange(8), indexing="ij")
    d, v = 16 * (j >> 2) + 4 * (lane >> 4) + (j & 3), 16 * vt + (lane & 15)
    assert len(set((d * 32 + v).flatten().tolist())) == 32 * 32
    out = []
    for plane in (0, 1):
        KV = torch.full((*lead, NH, HD, HD), float("nan"))
        KV[..., d, v] = frag[..., plane, :, :]
        out.append(KV)
    return out[0], out[1], ksum


# ---- the exact-f32 layer's block (csrc/encoder.hip) ------------------------------------------------------------------------------------

F32_TOK = 32                                          # tokens of one workgroup (OPHIP_TOK)
F32_KV_FLOATS = NH * (1024 + 32)                      # per (batch element, stream): per head 1024 KV + 32 Ksum (encoder.hip:21-22)


def f32_kv_block_offset(B: int, L3: int, L2: int) -> int:
    """FLOAT offset of the ``[B][2][F32_KV_FLOATS]`` block in the f32 layer's workspace: behind one slab set (encoder.hip:256-257)"""
    return B * ((L3 + F32_TOK - 1) // F32_TOK + (L2 + F32_TOK - 1) // F32_TOK) * F32_KV_FLOATS


def decode_f32_kv_block(blk: torch.Tensor):
    """``blk [..][F32_KV_FLOATS]`` f32 -> ``KV [..][8][32 (d)][32 (v)]``, ``Ksum [..][8][32]``: per head the 32 x 32 accumulator of
    ``kv_reduce_kernel`` as lanes hold it, register ``4 kb + j`` of lane ``32 h + r`` at float ``(kb 64 + lane) 4 + j`` = ``D[d = j + 8 kb + 4 h][v = r]``
    (encoder.hip:78-86; ``acc_row``), then Ksum in feature order (:89)."""
    lead = blk.shape[:-1]
    per = blk.reshape(*lead, NH, 1024 + 32)
    kb, lane, j = torch.meshgrid(torch.arange(4), torch.arange(64), torch.arange(4), indexing="ij")
    d, v = j + 8 * kb + 4 * (lane >> 5), lane & 31
    assert len(set((d * 32 + v).flatten().tolist())) == 32 * 32
    KV = torch.full((*lead, NH, HD, HD), float("nan"))
    KV[..., d, v] = per[..., :1024].reshape(*lead, NH, 4, 64, 4)
    return KV, per[..., 1024:].clone()


def f32_kv_slack(sd, p, x, mask=None):
    """What f32 arithmetic may leave between the exact-f32 layer's block and the reference's, from reasoning alone (float64, no measurement;
    ``bf.coarse_kv_slack`` without its flip term -- nothing is rounded to bf16 here -- and with the operands' own f32 error in its place):
      accumulation: the rounding errors of an f32 sum of n terms add up to about ``sqrt(n) 2^-24`` of the sum of their magnitudes; eight times
          that, for the sum over the L tokens: ``8 sqrt(L) 2^-24 sum_tok |phiK| |V| / L`` (Ksum: ``sum_tok phiK``);
      operands: K and V are themselves f32 sums of 256 products of either sign.  The partial sums of such a sum grow like ``sqrt(k)`` times the
          size of a term, and the rounding errors of the n additions, each 2^-24 of a partial sum, add up in quadrature to about 2^-24 of the SUM OF
          THE MAGNITUDES (no ``sqrt(n)``: that factor belongs to terms of one sign); eight times that: ``eK = 8 x 2^-24 sum_c |x_c| |Wk_c|``, ``eV``
          likewise.  ``phi`` has slope ``min(1, phi)``, so ``phiK`` moves by ``min(1, phiK) eK`` and a term ``phiK V / L`` by
          ``(min(1, phiK) eK |V| + phiK eV) / L``, plus ``4 x 2^-24`` of itself for ``expf``, the division by L and the product.
    Returns (``kv [B][8][32][32]``, ``ksum [B][8][32]``)."""
    B, L, _ = x.shape
    xa = x.to(f64)
    u = 2.0 ** -24
    wk, wv = sd[p + "k_proj.weight"].detach().to(f64), sd[p + "v_proj.weight"].detach().to(f64)
    K, V = (xa @ wk.T).view(B, L, NH, HD), (xa @ wv.T).view(B, L, NH, HD)
    eK = 8 * u * (xa.abs() @ wk.abs().T).view(B, L, NH, HD)
    eV = 8 * u * (xa.abs() @ wv.abs().T).view(B, L, NH, HD)
    phiK = _phi(K)
    if mask is not None:
        phiK = phiK * mask.to(f64)[:, :, None, None]
    dphi = torch.clamp(phiK, max=1.0) * eK
    acc = 8 * L ** 0.5 * u
    terms = torch.einsum("bthd,bthv->bhdv", phiK, V.abs()) / L
    oper = (torch.einsum("bthd,bthv->bhdv", dphi, V.abs()) + torch.einsum("bthd,bthv->bhdv", phiK, eV)) / L
    return (acc + 4 * u) * terms + oper, (acc + 4 * u) * phiK.sum(1) + dphi.sum(1)


# ---- cases ----------------------------------------------------------------------------------------------------------------------------

# (B, L3, L2).  New: a one-token stream beside one whole workgroup | either side of a 16-token tile | a tile edge beside one token short of a
# workgroup | one workgroup, one token more (B = 2) | two workgroups, one token more | B = 3, unequal streams (slab index b (tiles0 + tiles1) +
# tile) | 65 slabs beside two (kv_sum's remainder loop; attn_apply with more than 64 workgroups).  Then the four of test_encoder_layer_x3.
SHAPES = [(1, 1, 48), (1, 15, 17), (1, 16, 47), (2, 48, 49), (1, 96, 97), (3, 49, 130), (1, 3073, 49)]
OLD_SHAPES = [(1, 64, 32), (2, 70, 45), (1, 1000, 1200), (3, 49, 97)]
# K / V half only (``layercall.kv_first``): 129 slabs beside one (the three-way unrolled loop runs once) | 194 and 65 slabs (once + remainder, and
# the remainder alone, in one launch)
KV_SHAPES = [(1, 6145, 1), (1, 9300, 3100)]
REGIME_SHAPES = [(2, 48, 49), (1, 96, 97), (3, 49, 130)]
MASK_SHAPES = [(2, 48, 49), (3, 49, 130), (1, 96, 97)]
FORM_SHAPES = [(1, 15, 17), (2, 48, 49), (1, 96, 97)]
MASK_KINDS = ["mid_tile", "last_wg", "random", "single"]
# (entry, kind of the first stream's mask, of the second's): ``_masked`` takes the second stream's mask; ``_masks`` both, or one NULL
MASK_CASES = [("masked", None, k) for k in MASK_KINDS] + [("masks", "random", "mid_tile"), ("masks", "single", None), ("masks", None, "last_wg"),
                                                         ("masks", "mid_tile", "single")]
REGIMES = ["up", "down", "outliers"]
# the exact-f32 layer (32-token workgroups, a 16-way kv_sum): its own edges 31, 32, 33, 64, 65 where the list above has 47, 48, 49, 96, 97;
# 545 = 18 slabs (the 16-way loop wraps) as in bf.COARSE_SHAPES
F32_SHAPES = [(1, 1, 32), (1, 15, 17), (1, 16, 31), (2, 32, 33), (1, 64, 65), (3, 33, 130), (1, 545, 33)] + OLD_SHAPES[:3]


def layer_cases():
    """every ``((B, L3, L2), regime, mask case or None)`` that runs the whole layer (each x self, cross)"""
    return ([(s, "randn", None) for s in SHAPES + OLD_SHAPES] + [(s, "randn", mc) for s in MASK_SHAPES for mc in MASK_CASES]
            + [(s, r, None) for s in REGIME_SHAPES for r in REGIMES])


def block_family(regime, L, m):
    """which constant of STANDIN_BLOCK judges a stream's block: "one_term" (one real token: an element IS one product), "outliers" or "many" (every other block)"""
    if L == 1 or (m is not None and int(m.sum(1).max()) <= 1):
        return "one_term"
    return "outliers" if regime == "outliers" else "many"


def inputs(B, L3, L2, regime="randn"):
    """``bf.coarse_inputs`` (seeded randn); "up" / "down": the same tokens times SCALE_UP / SCALE_DOWN; "outliers": four tokens of each stream times
    SCALE_UP, on both sides of the first 16-token tile edge and of the first workgroup edge that the stream has (else its last tokens)"""
    x3, x2 = bf.coarse_inputs(B, L3, L2)
    if regime == "up":
        return x3 * SCALE_UP, x2 * SCALE_UP
    if regime == "down":
        return x3 * SCALE_DOWN, x2 * SCALE_DOWN
    if regime == "outliers":
        for x in (x3, x2):
            L = x.shape[1]
            for t in sorted({min(t, L - 1) for t in (15, 16, 47, 48)}):
                x[:, t] *= SCALE_UP
    else:
        assert regime == "randn"
    return x3, x2


def mask(kind, B, L, seed=11):
    """``[B][L]`` bool, 1 = real cell; None for kind None.  The kinds of ``bf.coarse_mask`` for 48-token workgroups: "mid_tile": the real cells end
    inside the last workgroup that holds any (13 cells short of a workgroup edge, 5 fewer per batch element); "last_wg": the whole last workgroup is
    padding (and, from batch element 1 on, one more cell per element); "random": 70 % real, cell 0 real, cells 17..39 of element 0 padded (whole
    16-token tiles); "single": ONE real cell per batch element."""
    if kind is None:
        return None
    m = torch.zeros(B, L, dtype=torch.bool)
    edge = TOK * ((L - 1) // TOK) or L                # first token of the last workgroup (a stream of one workgroup: its end)
    for b in range(B):
        if kind == "random":
            m[b] = torch.rand(L, generator=torch.Generator().manual_seed(seed + 7 * b)) > 0.3
            m[b, 0] = True
            if b == 0 and L > 40:
                m[b, 17:40] = False
        elif kind == "single":
            m[b, (17 + 31 * b) % L] = True
        else:
            n = edge - 13 - 5 * b if kind == "mid_tile" else edge - b
            assert 0 < n < L and (kind == "last_wg" or n % TOK)
            m[b, :n] = True
    return m


def masks_of(case, B, L3, L2):
    entry, k3, k2 = case
    return mask(k3, B, L3, 5), mask(k2, B, L2, 11)


# ---- bars: every figure below is the f32 stand-in against the float64 reference, measured by tests/test_x3_faithful_cpu.py -------------------
# (test_standin_figures_pin_the_bars recomputes each over exactly the cases named and asserts that it lies under the constant and above a quarter
# of it).  A bar is TWICE the stand-in's worst; none comes from a device figure.

# Input regimes.  The issue expected the stand-in to leave the bars at some scale (``phi(Q) . Ksum`` near the 1e-6 of the denominator); it does not:
# measured at REGIME_SHAPES x self, cross, at every power of two from 2^-70 to 2^20 the stand-in's figures stay within 1.9e-5 (block) and 1.9e-5
# (rows), because Ksum sums 32 positive terms per head and LayerNorm removes the scale.  So no bar limits the factors and they come from what they are
# to exercise: SCALE_UP = 16 puts K at +-70, ``__expf`` results from 1 down to 1e-30 (smaller ones flush to zero and say nothing) and the splits of
# ``phi(K) = K + 1`` at 70; SCALE_DOWN = 2^-6 puts the variance of the merged message (0.026 at unit scale, 6e-6 here) at LayerNorm1's eps (1e-5),
# where ``rstd`` depends on both and leans most on the eight-wave moment merge -- it is also where the stand-in's row figures are largest.
SCALE_UP = 16.0
SCALE_DOWN = 2.0 ** -6
# Every constant below is the measured figure plus about a tenth: the worst of 10^5 elements moves by a few per cent with the summation order of the
# CPU's f32 matrix product (thread count, vector width), and the pin in tests/test_x3_faithful_cpu.py must hold on any machine.
#
# Worst normalised block error of a stream's block, by :func:`block_family`, over SHAPES + OLD_SHAPES, KV_SHAPES, MASK_SHAPES x MASK_CASES and
# REGIME_SHAPES x REGIMES.  Three constants and not one, because the normaliser ``sum_tok |phiK| |V| / L`` is the size of the ELEMENT when one token
# carries the sum, and V is a sum of 256 products that may cancel: the stand-in's worst is then the element with the smallest ``|V|``, a thousand times
# the figure of a stream of 15 tokens or more.  One constant would be 1.22e-2 for every block.
STANDIN_BLOCK = {"many": 1.6e-5,           # measured: 1.44e-5 at (1, 15, 17); 1.32e-5 at "up" (2, 48, 49); 1.23e-5 under a random mask
                 "outliers": 1.4e-4,       # measured: 1.23e-4 at (2, 48, 49) and (3, 49, 130)
                 "one_term": 1.4e-2}       # measured: 1.22e-2 (single-cell mask at (3, 49, 130)); one-token streams 5.4e-4 and 1.2e-3
# the same by ``kv_terms_deep``, ONE constant for every block: the check that still bites where a few tokens carry the sum
STANDIN_BLOCK_DEEP = 2.6e-6                # measured: 2.30e-6 at the one-token stream of (1, 1, 48); 6.6e-7 at 15 tokens; 7e-8 at 6145
# Worst row error (forced: the reference fed the stand-in's own block, free: the reference's block) over the layer cases x self, cross, by regime:
# "unit" = SHAPES + OLD_SHAPES and MASK_SHAPES x MASK_CASES on randn inputs, "scaled" = REGIME_SHAPES x REGIMES.
STANDIN_ROWS_FORCED = {"unit": 1.2e-5,     # measured: 1.05e-5 at (3, 49, 130) masks random / mid_tile, cross
                       "scaled": 2.1e-5}   # measured: 1.90e-5 at "down" (3, 49, 130) cross
STANDIN_ROWS_FREE = {"unit": 1.3e-5,       # measured: 1.15e-5
                     "scaled": 2.1e-5}     # measured: 1.90e-5 at "down" (3, 49, 130) cross
BLOCK_BAR = {k: 2 * v for k, v in STANDIN_BLOCK.items()}
BLOCK_DEEP_BAR = 2 * STANDIN_BLOCK_DEEP
ROWS_FORCED_BAR = {k: 2 * v for k, v in STANDIN_ROWS_FORCED.items()}
ROWS_FREE_BAR = {k: 2 * v for k, v in STANDIN_ROWS_FREE.items()}


def rows_family(regime):
    return "unit" if regime == "randn" else "scaled"


# Today's stage-level bar of this kernel (tests/test_gpu_parity.py LAYER_TOL["bf16x3"]).  On unit-variance inputs a row's largest element is 4 to 7.4,
# so ROWS_FREE_BAR["unit"] allows up to 1.9e-4 where ``|ref|`` is near zero, against 1e-4 there: the normalised bar ALONE would be looser at those
# elements (tests/test_x3_faithful_cpu.py prints the ratio; the stand-in itself needs 0.36 of today's bar at its worst element).  So on unit-variance
# inputs the GPU tests assert today's bar as well, against the float64 reference: what is asserted is nowhere looser than before.
OLD_RTOL, OLD_ATOL = 3e-4, 1e-4
F32_RTOL, F32_ATOL = 1e-4, 2e-5                       # LAYER_TOL["f32"]: the exact-f32 layer's rows against the float64 reference, as it stands
