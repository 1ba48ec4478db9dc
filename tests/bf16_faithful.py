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


def meets(got: torch.Tensor, want: torch.Tensor, rtol: float, atol: float) -> torch.Tensor:
    """per match (dim 0): every element within ``atol + rtol |want|``"""
    g, w = got.to(torch.float64).reshape(got.shape[0], -1), want.to(torch.float64).reshape(want.shape[0], -1)
    return ((g - w).abs() <= atol + rtol * w.abs()).all(1)


def share_at_f32_bar(windows, f3, ref: dict) -> float:
    """share of matches whose windows AND 3D token all meet the f32 bar against ``ref``"""
    ok = meets(windows, ref["windows"].to(windows.device), F32_RTOL, F32_ATOL) & meets(f3, ref["f3"].to(f3.device), F32_RTOL, F32_ATOL)
    return ok.double().mean().item() if ok.numel() else 1.0


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
