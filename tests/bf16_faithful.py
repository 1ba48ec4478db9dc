"""A float64 reference that rounds WHERE THE bf16 KERNELS ROUND (CPU or device tensors).

The plain-bf16 mode (``nsplit = 1``) rounds its matrix operands to bf16 and accumulates in f32.  Compared with an un-rounded
reference the bound has to cover the rounding itself (2^-9 per operand, percents after two encoder layers) and a wrong kernel hides
under it.  A reference that applies the same roundings to the same values leaves f32 accumulation order (~1e-6) between the two --
except where a value lies so close to a bf16 rounding boundary that the kernel's f32 value and the reference's float64 value fall on
different sides of it ("flip": one operand moves by 2^-8 relative, LayerNorm and attention spread it over the match).  Hence the
statistic of the fine-stage tests: the SHARE of matches that meet the f32 bar, not a maximum.

Operand forms (csrc/tile_bf16.h):
  * ``bf16_round``  f32 -> bf16 (round to nearest even: ``(__bf16)v``, ``Tensor.to(torch.bfloat16)`` in packing.split_planes) -> back;
  * ``split``       ``split_bf16`` (tile_bf16.h:39-42): ``hi = bf16(v)``, ``lo = bf16(v - float(hi))``;
  * ``matmul_faithful(x, w, nsplit)``  ``x @ w.T`` with both operands rounded from their F32 values, products and sums in float64:
    nsplit 1 = hi.hi, 3 = hi.hi + hi.lo + lo.hi (``mma_bf16`` drops lo.lo), 0 = no rounding.

``fine_stage_faithful`` restates ``fine_pair_kernel`` (csrc/fine_bf16.hip; the one-match kernel and csrc/fine.hip compute the same).
Per match a tile of 26 tokens x 128 features: rows 0..24 the 5 x 5 window, row 25 the 3D token.
  gather (fine_bf16.hip:608, 624 / 645, 667): window row ``5 ky + kx`` = ``feat_f[b, :, stride * (j // wc) + ky - 2, stride * (j % wc) + kx - 2]``,
      zero outside the map; row 25 = ``desc3d[b, :, i]``.  Un-rounded f32: this is the residual stream.
  per layer (weights: the packer's hi / lo planes of the f32 weights, packing.pack_fine_layers_bf16) -- the activations are rounded exactly
  where the kernel writes planes with ``store_featrow_acc`` (tile_bf16.h:231-248):
    1. residual x -> X planes (fine_bf16.hip:692 before the first layer, :786 after every layer but the last): operand of the Q and K|V GEMMs
       (:712, :720) and first half of the W0 operand (:752).  The residual itself stays f32 in registers.
    2. attention message -> Y planes (:724): operand of the merge GEMM (:737).
    3. LayerNorm1(merge) -> Y planes (:743): second half of the W0 operand (:752).
    4. relu(hidden) -> H planes (:763): operand of the W2 GEMM (:772).
  NOT rounded: Q, K, V (accumulators) and the whole attention (``attend_match``, :89-183, exact-f32 matrix instructions and f32 vector
  arithmetic), both LayerNorms (eps 1e-5, biased variance), the residual add, and the last stage (``corr_partial`` / ``expect_store``, :192-227).
  attention by layer kind (``attend_match``): "self": window -> window, 3D -> itself; "cross": window -> the 3D token, 3D -> the window;
      phi = elu + 1, message = phi(Q) KV / (phi(Q) . Ksum + 1e-6) per head (8 heads of 16), no ``v_length`` factor (it cancels).
  last stage: sim[r] = <f3, win[r]> / sqrt(128) -> softmax over the 25 rows -> expectation on the grid ((r % 5 - 2) / 2, (r // 5 - 2) / 2),
      std = sqrt(max(var_x, 1e-10)) + sqrt(max(var_y, 1e-10)).
  keypoint (``store_fine_keypoint``, tile.h:89-103): ``mkpts_c + expec * fine_scale``, or with ``query_scale [B][2]`` (h, w factors)
      ``mkpts_c + (2 expec) * ((fine_scale / 2) * query_scale[b][[1, 0]])``.

``coarse_kv_faithful`` and ``coarse_layer_faithful`` restate the coarse encoder layer of csrc/encoder_bf16.hip (256 features, 8 heads of 32,
streams of any length): the first the K^T V | Ksum block of a stream as a source (``kv_reduce_bf16_kernel`` or the previous layer's fused
tail, then ``kv_sum_bf16_kernel``), the second ``attn_apply_bf16_kernel`` GIVEN a block; their docstrings list the ten rounding points with
the kernel's lines.  The two are separate because the block is a sum over the whole stream: one of its 8192 elements that the f32 sum puts on
the other side of a bf16 boundary (12 do at L = 545 in an f32 stand-in of the reference) moves every token that reads it, and the share of
tokens at the f32 bar falls from 0.97 to 0.55 although nothing is wrong.  So tests/test_gpu_encoder_bf16.py checks the device's block on its
own, element by element, and feeds THAT block to the layer reference ("teacher forcing"); what is left between the layer and its reference
is again accumulation order and flips of single tokens.  Statistic: the share of TOKENS whose 256 outputs all meet the f32 bar.
"""
from __future__ import annotations

import torch
import torch.nn.functional as F

CF, WIN, NHEAD = 128, 25, 8
F32_RTOL, F32_ATOL = 1e-4, 2e-5          # the f32 bar of tests/test_gpu_parity.py


def bf16_round(t: torch.Tensor) -> torch.Tensor:
    """The bf16 value nearest (ties to even) to the F32 value of ``t``, in ``t``'s dtype."""
    return t.to(torch.float32).to(torch.bfloat16).to(t.dtype)


def split(t: torch.Tensor):
    """``split_bf16``: (hi, lo) planes of the f32 value of ``t``, in ``t``'s dtype."""
    v = t.to(torch.float32)
    hi = v.to(torch.bfloat16)
    lo = (v - hi.to(torch.float32)).to(torch.bfloat16)
    return hi.to(t.dtype), lo.to(t.dtype)


def matmul_faithful(x: torch.Tensor, w: torch.Tensor, nsplit: int, dtype=torch.float64) -> torch.Tensor:
    """``x [.., in] @ w [out, in].T`` with the operands of mode ``nsplit`` and the arithmetic of ``dtype``."""
    x, w = x.to(torch.float32), w.to(torch.float32)
    if nsplit == 0:
        return x.to(dtype) @ w.to(dtype).T
    xh, xl = (t.to(dtype) for t in split(x))
    wh, wl = (t.to(dtype) for t in split(w))
    if nsplit == 1:
        return xh @ wh.T
    if nsplit == 3:
        return xh @ wh.T + xh @ wl.T + xl @ wh.T
    raise ValueError(f"nsplit {nsplit}")


def gather_tokens(feat_f, desc3d, b_ids, i_ids, j_ids, wc: int, stride: int, dtype=torch.float64) -> torch.Tensor:
    """``[K][26][128]``: the zero-padded 5 x 5 window around ``stride * cell`` (rows 0..24) and ``desc3d[b, :, i]`` (row 25)."""
    K = b_ids.shape[0]
    fp = F.pad(feat_f, (2, 2, 2, 2))
    cy, cx = stride * (j_ids // wc), stride * (j_ids % wc)
    d = torch.arange(5, device=feat_f.device)
    win = fp[b_ids[:, None, None], :, (cy[:, None] + d)[:, :, None], (cx[:, None] + d)[:, None, :]]      # [K, 5 (y), 5 (x), C]
    tok = torch.cat([win.reshape(K, WIN, CF), desc3d[b_ids, :, i_ids][:, None, :]], 1)
    return tok.to(dtype)


def _phi(x):
    return torch.where(x > 0, x + 1, torch.exp(torch.clamp(x, max=0)))


def _attend(q, k, v):
    """linear attention of the query tokens ``q [K][L][128]`` over the source set ``k, v [K][S][128]``, 8 heads of 16"""
    K_, L, S = q.shape[0], q.shape[1], k.shape[1]
    Q, Kk, V = _phi(q).view(K_, L, NHEAD, -1), _phi(k).view(K_, S, NHEAD, -1), v.view(K_, S, NHEAD, -1)
    KV = torch.einsum("kshd,kshv->khdv", Kk, V)
    Z = 1 / (torch.einsum("klhd,khd->klh", Q, Kk.sum(1)) + 1e-6)
    return torch.einsum("klhd,khdv,klh->klhv", Q, KV, Z).reshape(K_, L, CF)


def _layernorm(x, g, b):
    return F.layer_norm(x, (CF,), g.to(x.dtype), b.to(x.dtype), 1e-5)


def encoder_layer_faithful(sd: dict, p: str, x: torch.Tensor, cross: bool, nsplit: int, dtype=torch.float64) -> torch.Tensor:
    """One fine-encoder layer on the token tiles ``x [K][26][128]`` with rounding points 1-4 of the module docstring."""
    mm = lambda a, name: matmul_faithful(a, sd[p + name].to(a.device), nsplit, dtype)
    q, k, v = mm(x, "q_proj.weight"), mm(x, "k_proj.weight"), mm(x, "v_proj.weight")                    # (1) x is rounded inside mm
    w, t = slice(0, WIN), slice(WIN, WIN + 1)
    if cross:
        msg = torch.cat([_attend(q[:, w], k[:, t], v[:, t]), _attend(q[:, t], k[:, w], v[:, w])], 1)
    else:
        msg = torch.cat([_attend(q[:, w], k[:, w], v[:, w]), _attend(q[:, t], k[:, t], v[:, t])], 1)
    m = mm(msg, "merge.weight")                                                                        # (2)
    m = _layernorm(m, sd[p + "norm1.weight"].to(x.device), sd[p + "norm1.bias"].to(x.device))
    hid = torch.relu(mm(torch.cat([x, m], 2), "mlp.0.weight"))                                          # (1) and (3)
    o = mm(hid, "mlp.2.weight")                                                                        # (4)
    o = _layernorm(o, sd[p + "norm2.weight"].to(x.device), sd[p + "norm2.bias"].to(x.device))
    return x + o


def expectation(tok: torch.Tensor) -> torch.Tensor:
    """``expec_f [K][3]`` = (x, y, std) of the heat map of the 3D token against the window rows."""
    sim = torch.einsum("kc,krc->kr", tok[:, WIN], tok[:, :WIN]) * 0.08838834764831845
    pr = torch.softmax(sim, 1)
    r = torch.arange(WIN, device=tok.device)
    gx, gy = ((r % 5 - 2) * 0.5).to(tok.dtype), ((r // 5 - 2) * 0.5).to(tok.dtype)
    ex, ey = (pr * gx).sum(1), (pr * gy).sum(1)
    vx, vy = (pr * gx * gx).sum(1) - ex * ex, (pr * gy * gy).sum(1) - ey * ey
    sd_ = torch.sqrt(torch.clamp(vx, min=1e-10)) + torch.sqrt(torch.clamp(vy, min=1e-10))
    return torch.stack([ex, ey, sd_], 1)


def keypoints(mkpts_c, expec, fine_scale: float, b_ids=None, query_scale=None) -> torch.Tensor:
    mkc = mkpts_c.to(expec.dtype)
    if query_scale is None:
        return mkc + expec[:, :2] * fine_scale
    qs = query_scale.to(expec.dtype)[b_ids][:, [1, 0]]
    return mkc + (expec[:, :2] * 2.0) * ((fine_scale * 0.5) * qs)


def fine_stage_faithful(sd: dict, feat_f, desc3d, b_ids, i_ids, j_ids, mkpts_c, wc: int, stride: int, fine_scale: float,
                        cross_layers, nsplit: int, encoder_enable: bool = True, query_scale=None,
                        prefix: str = "loftr_fine.layers.", dtype=torch.float64) -> dict:
    """The fine stage of ``cross_layers`` (one bool per layer: True = "cross") in mode ``nsplit`` (0: no rounding, 1, 3).
    ``dtype`` is the arithmetic between the rounding points: float64 = the reference; float32 = a stand-in for the kernel
    (same roundings, f32 accumulation) that the CPU tests use to show what accumulation order alone does to the statistic.
    Returns ``windows [K][25][128]``, ``f3 [K][128]``, ``expec_f [K][3]``, ``mkpts_f [K][2]``."""
    tok = gather_tokens(feat_f, desc3d, b_ids, i_ids, j_ids, wc, stride, dtype)
    if encoder_enable:
        for l, cross in enumerate(cross_layers):
            tok = encoder_layer_faithful(sd, f"{prefix}{l}.", tok, bool(cross), nsplit, dtype)
    expec = expectation(tok)
    return {"windows": tok[:, :WIN], "f3": tok[:, WIN], "expec_f": expec,
            "mkpts_f": keypoints(mkpts_c, expec, fine_scale, b_ids, query_scale)}


# ---- the coarse encoder layer of the plain-bf16 mode (csrc/encoder_bf16.hip, nsplit = 1) ----------------------------------------------

CC, CHEADS, CDIM, SLAB = 256, 8, 32, 32


def _w(sd: dict, name: str, rounded, dtype) -> torch.Tensor:
    w = sd[name].detach().to(torch.float32)
    return (bf16_round(w) if rounded is not False else w).to(dtype)


def _rounder(rounded):
    """``rounded``: True = every rounding point, False = none (weights included), a collection of point numbers = all points BUT those
    (weights rounded): what a kernel that misses a rounding point would compute"""
    def at(point):
        on = rounded is True or (rounded is not False and point not in rounded)
        return bf16_round if on else (lambda t: t)
    return at


def _coarse_kv_operands(sd, p, source, kv_mask, dtype, rounded):
    """``phi(K)`` and ``V / L`` as the KV product takes them, ``[B][slab][32 tokens][8][32]`` (points 1-3 of :func:`coarse_kv_faithful`)"""
    B, L, _ = source.shape
    r = _rounder(rounded)
    x = r(1)(source.to(torch.float32)).to(dtype)
    K = (x @ _w(sd, p + "k_proj.weight", rounded, dtype).T).view(B, L, CHEADS, CDIM)
    V = (x @ _w(sd, p + "v_proj.weight", rounded, dtype).T).view(B, L, CHEADS, CDIM)
    phiK = _phi(K)
    if kv_mask is not None:
        phiK = phiK * kv_mask.to(dtype)[:, :, None, None]
    phiK = r(2)(phiK)
    inv_len = (torch.tensor(1.0, dtype=torch.float32) / torch.tensor(float(L), dtype=torch.float32)).to(dtype) if rounded is not False else 1.0 / L
    V = r(3)(V * inv_len)                                                                               # bf16_round goes through f32
    pad = (-L) % SLAB
    phiK, V = F.pad(phiK, (0, 0, 0, 0, 0, pad)), F.pad(V, (0, 0, 0, 0, 0, pad))
    return phiK.view(B, -1, SLAB, CHEADS, CDIM), V.view(B, -1, SLAB, CHEADS, CDIM)


def coarse_kv_faithful(sd: dict, p: str, source: torch.Tensor, kv_mask=None, dtype=torch.float64, rounded=True):
    """``KV [B][8][32 (d)][32 (v)]`` and ``Ksum [B][8][32]`` of the stream ``source [B][L][256]`` as the attention's source:
    ``kv_reduce_bf16_kernel`` / the fused tail of ``attn_apply_bf16_kernel`` (both ``kv_slab_from_planes``, encoder_bf16.hip:47-101) and
    ``kv_sum_bf16_kernel`` (:139-166), BEFORE the block's (hi, lo) split.  ``kv_mask [B][L]`` (bool, 1 = real cell): the 2D stream's padding.
    Rounding points (``rounded``: see :func:`_rounder`; False = none, which is oracle.onepose_oracle.linear_attention's KV):
      1. source rows -> bf16 planes (``load_rows_to_planes``, tile_bf16.h:252-273, called at encoder_bf16.hip:121; in the fused tail the rows
         of ``y`` at :418-427, rows >= L zero); Wk, Wv = the packer's hi plane (packing.split_planes); K, V f32 accumulators (:58);
      2. ``phi(K) = elu + 1`` -> bf16 (``acc_frag_map`` with ``f_k``, :68-71, :80); 0 for tokens >= L and for masked cells;
      3. ``V * inv_len``, ``inv_len = 1.0f / (float)L`` in f32 (:59), the product an f32 (``f_v``, :72) -> bf16 (:81);
      4. ``KV = sum phiK (x) V`` and ``Ksum = sum phiK`` over those operands (:82-83): f32 partials per 32-token slab (:86-98), summed over the
         slabs by ``kv_sum_bf16_kernel`` (:148, :154); here: per slab in ``dtype``, then over the slabs."""
    phiK, V = _coarse_kv_operands(sd, p, source, kv_mask, dtype, rounded)
    KV = torch.einsum("bsthd,bsthv->bshdv", phiK, V).sum(1)                                             # (4)
    return KV, phiK.sum(2).sum(1)


def coarse_layer_faithful(sd: dict, p: str, x: torch.Tensor, KV: torch.Tensor, Ksum: torch.Tensor, S: int, q_mask=None,
                          dtype=torch.float64, rounded=True) -> torch.Tensor:
    """``y [B][L][256]`` of ``attn_apply_bf16_kernel`` (encoder_bf16.hip:240-438) for the query stream ``x`` given the source's ``KV`` and
    ``Ksum`` (:func:`coarse_kv_faithful`, or the device's block) and its length ``S``.  ``q_mask [B][L]``: the 2D stream's padding as queries.
    Rounding points (``rounded``: see :func:`_rounder`; False = none, which is oracle.onepose_oracle.encoder_layer):
      5. KV -> bf16: the block holds (hi, lo) (``kv_sum_bf16_kernel``, :157-161), nsplit = 1 reads hi only (:305-306);
         Ksum is stored f32 (:163) and split when read, hi only (:310-315);
      6. x rows -> bf16 X planes (:273): operand of the Q GEMM (:285) and first half of the W0 operand (:364); the residual (:413-414) is f32 x;
      7. ``phi(Q)`` -> bf16 (``acc_frag``, :319), 0 for masked query cells (:298-301);
      8. ``msg = num * rcp(den + 1e-6f) * S`` in f32 (:327) -> bf16 Y planes (:328): operand of the merge GEMM (:342);
      9. LayerNorm1 (f32, biased variance, eps 1e-5: ``layernorm_featrow``, :190-238) -> bf16 Y planes (:349): second half of the W0 operand;
     10. ``relu(hidden)`` -> bf16 H planes in four 128-feature chunks (:371-372): operand of the W2 GEMM (:376).
    NOT rounded: the accumulators, LayerNorm2 (:382) and ``y = x + LN2`` (:414).  ``1 / L`` (point 3) and ``S`` do not cancel once
    ``V / L`` is rounded: both are kept."""
    B, L, _ = x.shape
    r = _rounder(rounded)
    g = lambda name: sd[p + name].detach().to(dtype)
    KVr, Ksr = r(5)(KV.to(torch.float32)).to(dtype), r(5)(Ksum.to(torch.float32)).to(dtype)
    xr = r(6)(x.to(torch.float32)).to(dtype)
    phiQ = _phi((xr @ _w(sd, p + "q_proj.weight", rounded, dtype).T).view(B, L, CHEADS, CDIM))
    if q_mask is not None:
        phiQ = phiQ * q_mask.to(dtype)[:, :, None, None]
    phiQ = r(7)(phiQ)
    num = torch.einsum("blhd,bhdv->blhv", phiQ, KVr)
    den = torch.einsum("blhd,bhd->blh", phiQ, Ksr)
    eps = torch.tensor(1e-6, dtype=torch.float32).to(dtype)
    msg = r(8)((num * (1 / (den + eps))[..., None] * float(S)).reshape(B, L, CC))
    m = msg @ _w(sd, p + "merge.weight", rounded, dtype).T
    m = r(9)(F.layer_norm(m, (CC,), g("norm1.weight"), g("norm1.bias"), 1e-5))
    hid = r(10)(torch.relu(torch.cat([xr, m], 2) @ _w(sd, p + "mlp.0.weight", rounded, dtype).T))
    o = hid @ _w(sd, p + "mlp.2.weight", rounded, dtype).T
    return x.to(dtype) + F.layer_norm(o, (CC,), g("norm2.weight"), g("norm2.bias"), 1e-5)


def coarse_streams_faithful(sd: dict, p: str, x3, x2, cross: bool, mask2=None, kv=None, dtype=torch.float64, rounded=True):
    """Both streams of one layer as ``ophip_encoder_layer_bf16[_masked]`` runs them (``layer_bf16``, encoder_bf16.hip:455-545): the block
    [b][s] is stream s as a source (s = 1, the 2D stream, under ``mask2`` as kv_mask, :126); stream s attends to block s ("self") or 1 - s
    ("cross", :513-517) and the 2D stream's queries are masked (:262, :299).  ``kv`` = ((KV3, Ksum3), (KV2, Ksum2)) replaces the blocks
    (teacher forcing: the float64 reference's, or the device's).  Returns ``(y3, y2, kv)``."""
    if kv is None:
        kv = (coarse_kv_faithful(sd, p, x3, None, dtype, rounded), coarse_kv_faithful(sd, p, x2, mask2, dtype, rounded))
    s3, s2 = (kv[1], kv[0]) if cross else (kv[0], kv[1])
    L = (x3.shape[1], x2.shape[1])
    y3 = coarse_layer_faithful(sd, p, x3, s3[0], s3[1], L[1] if cross else L[0], None, dtype, rounded)
    y2 = coarse_layer_faithful(sd, p, x2, s2[0], s2[1], L[0] if cross else L[1], mask2, dtype, rounded)
    return y3, y2, kv


def token_share_at_f32_bar(got: torch.Tensor, want: torch.Tensor) -> float:
    """share of tokens (rows of the last dim) whose 256 outputs all meet the f32 bar"""
    return meets(got.reshape(-1, got.shape[-1]), want.reshape(-1, want.shape[-1]), F32_RTOL, F32_ATOL).double().mean().item()


def bf16_ulps_apart(a: torch.Tensor, b: torch.Tensor) -> torch.Tensor:
    """distance of two tensors of bf16 VALUES in steps of the bf16 grid (int64; 0 = equal, 1 = neighbours; -0 and +0 are 0 apart)"""
    def key(t):
        i = t.to(torch.float32).to(torch.bfloat16).view(torch.int16).to(torch.int64) & 0xFFFF
        return torch.where(i >= 0x8000, 0x8000 - i, i)                                                  # sign-magnitude -> a line
    return (key(a) - key(b)).abs()


def meets(got: torch.Tensor, want: torch.Tensor, rtol: float, atol: float) -> torch.Tensor:
    """per match (dim 0): every element within ``atol + rtol |want|``"""
    g, w = got.to(torch.float64).reshape(got.shape[0], -1), want.to(torch.float64).reshape(want.shape[0], -1)
    return ((g - w).abs() <= atol + rtol * w.abs()).all(1)


def share_at_f32_bar(windows, f3, ref: dict) -> float:
    """share of matches whose windows AND 3D token all meet the f32 bar against ``ref``"""
    ok = meets(windows, ref["windows"].to(windows.device), F32_RTOL, F32_ATOL) & meets(f3, ref["f3"].to(f3.device), F32_RTOL, F32_ATOL)
    return ok.double().mean().item() if ok.numel() else 1.0


# ---- the cases of tests/test_gpu_encoder_bf16.py, shared with the CPU file that checks what they rely on ------------------------------

COARSE_LAYER = "loftr_coarse.layers.2."
# (B, L3, L2): one-token stream | one token either side of a 32-token tile | one past one and two tiles | batch strides | exactly two tiles |
# 18 slabs (kv_sum's 16-way loop wraps, ragged last slab) beside fewer than 16
COARSE_SHAPES = [(1, 1, 32), (1, 31, 33), (1, 33, 65), (3, 49, 97), (2, 64, 45), (1, 545, 300)]
COARSE_MASK_SHAPES = [(2, 64, 45), (3, 49, 97), (1, 545, 300)]
COARSE_MASKS = ["random", "mid_tile", "last_tile"]
COARSE_CHAIN_SHAPES = [(1, 100, 75), (2, 333, 260)]
# Worst element of a token against the float64 reference fed the same KV: twice the worst that the f32 stand-in of the reference shows over
# COARSE_SHAPES, COARSE_MASK_SHAPES x COARSE_MASKS and (2, 70, 45), both layer kinds (tests/test_bf16_faithful_cpu.py measures and pins it).
COARSE_STANDIN_WORST = 8.0e-3        # measured: 7.6e-3
COARSE_WORST_BAR = 2 * COARSE_STANDIN_WORST
COARSE_KV_ULP_SHARE = 0.01          # at most 1 % of the KV elements one bf16 step from the reference's, none further


def coarse_inputs(B: int, L3: int, L2: int, seed: int = 2):
    """the streams of tests/test_gpu_parity.py::test_encoder_layer_bf16"""
    g = torch.Generator().manual_seed(seed)
    return torch.randn(B, L3, CC, generator=g), torch.randn(B, L2, CC, generator=g)


def coarse_mask(kind: str, B: int, L2: int) -> torch.Tensor:
    """``[B][L2]`` bool, 1 = real cell.  "random": the mask of tests/test_gpu_masked.py; "mid_tile": the real cells end inside the last
    32-token tile that holds any (13 cells short of a tile edge, 5 fewer per batch element); "last_tile": the whole last tile is padding
    (and, from batch element 1 on, one more cell per element)."""
    if kind == "random":
        from tests.test_gpu_masked import _mask
        return _mask(B, L2, 11)
    m = torch.zeros(B, L2, dtype=torch.bool)
    edge = SLAB * ((L2 - 1) // SLAB)                    # first token of the last tile
    for b in range(B):
        n = edge - 13 - 5 * b if kind == "mid_tile" else edge - b
        assert 0 < n < L2 and (kind == "last_tile" or n % SLAB)
        m[b, :n] = True
    return m


KV_PART_FLOATS = CHEADS * 2 * 64 * 8 + CHEADS * CDIM            # one 32-token slab: KV fragments (f32) + Ksum (encoder_bf16.hip:27)
KV_FRAG_BYTES = CHEADS * 2 * 2 * 64 * 16                        # [head][k-step][plane hi, lo][lane][8 bf16] (:28)
KV_BLOCK_BYTES = KV_FRAG_BYTES + CHEADS * CDIM * 4              # + Ksum f32 [head][lane half][16] (:29)


def kv_block_offset(base_addr: int, B: int, L3: int, L2: int) -> int:
    """byte offset of the ``[B][2][KV_BLOCK_BYTES]`` block inside the workspace at address ``base_addr``: behind the two slab sets, at the
    next ADDRESS that is a multiple of 256 (``layer_bf16``, encoder_bf16.hip:468-473)"""
    part_floats = B * ((L3 + SLAB - 1) // SLAB + (L2 + SLAB - 1) // SLAB) * KV_PART_FLOATS
    off = 2 * part_floats * 4
    return off + (-(base_addr + off)) % 256


def decode_kv_block(blk: torch.Tensor):
    """``blk [..][KV_BLOCK_BYTES]`` uint8 (CPU) -> ``KV_hi, KV_lo [..][8][32 (d)][32 (v)]`` and ``Ksum [..][8][32]`` (f32).  The fragments are
    the KV accumulator ``D[d][v]`` of ``kv_slab_from_planes`` as lane and register hold it: element j of lane ``32 h + r`` in k-step ``st`` is
    register ``8 st + j``, so ``v = r`` and ``d = (reg & 3) + 8 (reg >> 2) + 4 h`` (encoder_bf16.hip:86-98, :157-163; tile_bf16.h:9-18);
    Ksum register ``reg`` of lane half ``h`` is the same ``d``."""
    lead = blk.shape[:-1]
    frag = blk[..., :KV_FRAG_BYTES].contiguous().view(torch.bfloat16).float().view(*lead, CHEADS, 2, 2, 64, 8)
    ks = blk[..., KV_FRAG_BYTES:].contiguous().view(torch.float32).view(*lead, CHEADS, 2, 16)
    st, lane, j = torch.meshgrid(torch.arange(2), torch.arange(64), torch.arange(8), indexing="ij")
    reg = 8 * st + j
    d, v = (reg & 3) + 8 * (reg >> 2) + 4 * (lane >> 5), lane & 31
    assert len(set((d * 32 + v).flatten().tolist())) == 32 * 32
    out = []
    for plane in (0, 1):
        KV = torch.full((*lead, CHEADS, CDIM, CDIM), float("nan"))
        KV[..., d, v] = frag[..., plane, :, :]
        out.append(KV)
    h, reg = torch.meshgrid(torch.arange(2), torch.arange(16), indexing="ij")
    Ksum = torch.full((*lead, CHEADS, CDIM), float("nan"))
    Ksum[..., (reg & 3) + 8 * (reg >> 2) + 4 * h] = ks
    return out[0], out[1], Ksum


def coarse_kv_slack(sd: dict, p: str, source: torch.Tensor, kv_mask=None):
    """What f32 arithmetic may leave between the device's block and the reference's BEFORE the block is rounded, from reasoning alone
    (float64, no measurement).  Two terms each:
      accumulation: the rounding errors of an f32 sum of L terms add up to about ``sqrt(L) 2^-24`` of the sum of their magnitudes (the operands
          are bf16, their products exact in f32); eight times that;
      flips: an operand ``phi(K)[tok][d]`` or ``V[tok][v] / L`` that the f32 K or V puts on the other side of a bf16 rounding boundary moves its
          term by one bf16 step of the operand, <= 2^-7 of the term; two may coincide in one sum.
    ``kv [B][8][32][32]`` for ``KV = sum_tok phiK V`` and ``ksum [B][8][32]`` for ``Ksum = sum_tok phiK``.  For KV the slack matters where the
    sum cancels to a value whose own bf16 step is smaller (and in streams of a few tokens); elsewhere it lies below the one bf16 step that
    rounding the block allows anyway."""
    L = source.shape[1]
    phiK, V = _coarse_kv_operands(sd, p, source, kv_mask, torch.float64, True)
    acc, flip = 8 * L ** 0.5 * 2.0 ** -24, 2 * 2.0 ** -7
    terms = torch.einsum("bsthd,bsthv->bsthdv", phiK.abs(), V.abs())
    return acc * terms.sum((1, 2)) + flip * terms.amax((1, 2)), acc * phiK.sum((1, 2)) + flip * phiK.amax((1, 2))


def coarse_kv_check(kv_got: torch.Tensor, kv_ref: torch.Tensor, kv_acc: torch.Tensor):
    """The block's hi plane ``kv_got`` (bf16 values) against ``bf16_round(kv_ref)``: returns (share of elements that differ, elements that
    are neither within one bf16 step nor within the slack ``kv_acc`` of :func:`coarse_kv_slack` -- there must be none, max steps apart)."""
    want = bf16_round(kv_ref)
    steps = bf16_ulps_apart(kv_got, want)
    bad = (steps > 1) & ((kv_got.double() - want.double()).abs() > kv_acc)
    return (steps > 0).double().mean().item(), int(bad.sum()), int(steps.max())


# ---- the cases of tests/test_gpu_fine_stage.py, shared with the CPU file that checks what they rely on -------------------------------

def layer_state_dict(sd: dict, nlayers: int, prefix: str = "loftr_fine.layers.", seed: int = 123) -> dict:
    """A copy of the fine layers of ``sd`` with layers beyond its own filled by seeded weights of layer 0's shapes
    (projections ~ N(0, 1 / in), LayerNorm weight 1 + 0.1 N, bias 0.1 N)."""
    out = {k: v.detach().clone().float() for k, v in sd.items() if k.startswith(prefix)}
    have = 1 + max(int(k[len(prefix):].split(".")[0]) for k in out)
    g = torch.Generator().manual_seed(seed)
    names = [k[len(prefix) + 2:] for k in out if k.startswith(prefix + "0.")]
    for l in range(have, nlayers):
        for n in names:
            ref = out[f"{prefix}0.{n}"]
            r = torch.randn(ref.shape, generator=g)
            if ref.dim() == 2:
                out[f"{prefix}{l}.{n}"] = r / ref.shape[1] ** 0.5
            else:
                out[f"{prefix}{l}.{n}"] = (1.0 + 0.1 * r) if n.endswith("weight") else 0.1 * r
    return out


def random_case(K: int, B: int = 2, N: int = 90, hc: int = 6, wc: int = 7, stride: int = 4, seed: int = 7) -> dict:
    """seeded ``randn`` maps and ids; the first four matches sit in the map's corners"""
    g = torch.Generator().manual_seed(seed)
    hf, wf = hc * stride, wc * stride
    feat = torch.randn(B, CF, hf, wf, generator=g)
    desc = torch.randn(B, CF, N, generator=g)
    b_ids = torch.sort(torch.randint(0, B, (K,), generator=g))[0]
    i_ids = torch.randint(0, N, (K,), generator=g)
    j_ids = torch.randint(0, hc * wc, (K,), generator=g)
    j_ids[:4] = torch.tensor([0, wc - 1, (hc - 1) * wc, hc * wc - 1])[:K]
    mkc = torch.stack([j_ids % wc, j_ids // wc], 1).float() * (2.0 * stride)
    return dict(feat=feat, desc=desc, b_ids=b_ids, i_ids=i_ids, j_ids=j_ids, mkc=mkc, hc=hc, wc=wc, hf=hf, wf=wf, stride=stride)


def planted_case(hc: int = 5, wc: int = 6, stride: int = 4, seed: int = 21) -> dict:
    """One match per window position r* = 0..24, twice (interior cells of batch element 0 and of batch element 2): the match's 3D descriptor IS
    row r* of its own window, scaled so that the heat map is a delta (``|f|^2 / sqrt(128)`` ~ 45 against ~N(0, 4) elsewhere).  B = 3 and
    ``b_ids`` skip element 1; hf != wf.  Matches share cells; every match has its own descriptor column."""
    g = torch.Generator().manual_seed(seed)
    B, hf, wf = 3, hc * stride, wc * stride
    feat = torch.randn(B, CF, hf, wf, generator=g)
    cells = [(y, x) for y in range(1, hc - 1) for x in range(1, wc - 1)]          # interior: the whole window is inside the map
    b_ids, j_ids, rstar = [], [], []
    for rep, b in enumerate((0, 2)):
        for r in range(WIN):
            y, x = cells[(r + 5 * rep) % len(cells)]
            b_ids.append(b); j_ids.append(y * wc + x); rstar.append(r)
    K = len(b_ids)
    b_ids, j_ids, rstar = torch.tensor(b_ids), torch.tensor(j_ids), torch.tensor(rstar)
    i_ids = torch.arange(K)
    desc = torch.zeros(B, CF, K)
    py, px = stride * (j_ids // wc) + rstar // 5 - 2, stride * (j_ids % wc) + rstar % 5 - 2
    desc[b_ids, :, i_ids] = 2.0 * feat[b_ids, :, py, px]
    mkc = torch.stack([j_ids % wc, j_ids // wc], 1).float() * (2.0 * stride)
    want_xy = torch.stack([(rstar % 5 - 2) * 0.5, (rstar // 5 - 2) * 0.5], 1).double()
    return dict(feat=feat, desc=desc, b_ids=b_ids, i_ids=i_ids, j_ids=j_ids, mkc=mkc, hc=hc, wc=wc, hf=hf, wf=wf, stride=stride,
                rstar=rstar, want_xy=want_xy)
