"""Full (softmax) attention -- ``full_flash_kernel`` and the two layer entries of csrc/encoder_full.hip, the attention and matching kernels of
csrc/fine_full.hip -- against the UN-ROUNDED float64 oracle: reference, stand-in, cases, statistics and bars shared by
tests/test_full_faithful_cpu.py, tests/test_gpu_encoder_full.py and tests/test_gpu_fine_full.py.

Reference = ``full_attention_oracle.full_attention`` / ``encoder_layer`` in float64 on the f32 values of inputs and weights, nothing rounded.

Stand-in = float32, never compared with the device: it sizes the bars.  :func:`standin_attention` restates ``full_flash_kernel``: Q, K, V and
P each split ``hi + lo`` (``bf16_faithful.split``), every product ``lo.hi + hi.lo + hi.hi``, keys in tiles of 32 with the kernel's running
``m``, ``l``, ``alpha`` and ``o *= alpha`` in the log2 domain, tail keys at ``-inf``, ``1 / l`` at the end.  What the device has and the stand-in
lacks -- the hardware ``exp2``, the MFMA's order of sums -- is what the factor of three in every bar is for.

Statistics, worst element, every element compared:
  attention   ``|o - o_ref| / max_{s, d} |v[b, s, head, d]|``: the output is a convex combination of that head's value rows, so the largest value
              is the scale of any error of the weights;
  layer rows  ``|y - y_ref| / max(1, max |y_ref row|)`` as in tests/x3_faithful.py.

Non-finite inputs (NaN, +-inf in q, k, v or x) are OUT OF SCOPE: the kernel's ``-inf`` arithmetic is its own (masked tail keys), nothing here
feeds it one.
"""
from __future__ import annotations

import functools
import math

import torch
import torch.nn.functional as F

from tests import bf16_faithful as bf
from tests import full_attention_oracle as foracle

f32, f64 = torch.float32, torch.float64
C, NH, HD = 256, 8, 32                                 # onepose_st_amd/csrc/encoder_full.hip: C, NH, HD
KT, QT, TOK = 32, 128, 32                              # keys per tile, queries per flash workgroup, rows per qkv / tail workgroup (OPHIP_TOK)
LAYER = bf.COARSE_LAYER


# ---- reference ------------------------------------------------------------------------------------------------------------------------

def reference_attention(q, k, v, H=NH):
    """``softmax(q k^T / sqrt(D)) v`` per head in float64: q ``[B][L][H D]``, k, v ``[B][S][H D]`` -> ``[B][L][H D]``"""
    B, L, S = q.shape[0], q.shape[1], k.shape[1]
    q, k, v = (t.to(f64).view(B, -1, H, t.shape[2] // H) for t in (q, k, v))
    return foracle.full_attention(q, k, v).reshape(B, L, -1)


def weights64(sd, p=LAYER):
    """the layer's f32 weights as float64 values (what "float64, fed float32 weights" means to ``F.linear``)"""
    return {n: t.detach().to(f32).to(f64) for n, t in sd.items() if n.startswith(p)}


def reference_layer(sd, p, x, src):
    """one ``LoFTREncoderLayer`` with full attention, float64; an input of batch extent 1 is shared by the batch"""
    B = max(x.shape[0], src.shape[0])
    with torch.no_grad():
        return foracle.encoder_layer(weights64(sd, p), p, x.to(f64).expand(B, -1, -1), src.to(f64).expand(B, -1, -1), NH)


# ---- stand-in -------------------------------------------------------------------------------------------------------------------------

FAULTS = ("tail_unmasked", "last_key_dropped", "o_not_rescaled", "l_not_rescaled", "score_lohi_dropped", "p_lo_dropped", "scale_16",
          "groups_swapped", "head_xor_1", "batch_0_keys")


def _three(eq, ahi, alo, bhi, blo, drop_lohi=False):
    """``mma32x3`` of encoder_full.hip: a.lo b.hi + a.hi b.lo + a.hi b.hi, small terms first, f32"""
    out = torch.einsum(eq, ahi, blo)
    if not drop_lohi:
        out = torch.einsum(eq, alo, bhi) + out
    return out + torch.einsum(eq, ahi, bhi)


def standin_attention(q, k, v, wrong=None):
    """``full_flash_kernel`` in float32, statement by statement (each comment quotes the kernel's); ``wrong``: one of FAULTS, a kernel with that mistake"""
    assert wrong is None or wrong in FAULTS
    B, L, S = q.shape[0], q.shape[1], k.shape[1]
    Q, K, V = (t.to(f32).view(B, -1, NH, HD) for t in (q, k, v))
    if wrong == "batch_0_keys":
        K = K[:1].expand(B, -1, -1, -1)
    if wrong == "head_xor_1":
        V = V[:, :, [1, 0, 3, 2, 5, 4, 7, 6]]
    qhi, qlo = bf.split(Q)
    sc = torch.tensor(1.4426950408889634, dtype=f32) / torch.sqrt(torch.tensor(16.0 if wrong == "scale_16" else float(HD), dtype=f32))   # fa.scale_log2 = 1.4426950408889634f / sqrtf((float)HD)
    m = torch.full((B, L, NH), float("-inf"), dtype=f32)
    l = torch.zeros(B, L, NH, dtype=f32)
    o = torch.zeros(B, L, NH, HD, dtype=f32)
    for k0 in range(0, S, KT):
        n = min(KT, S - k0)
        Kt, Vt = (F.pad(t[:, k0:k0 + n], (0, 0, 0, 0, 0, KT - n)) for t in (K, V))                    # keys >= S: zero rows (split_row8's ``live``; ``key < S ? V[..] : 0.f``)
        if wrong == "groups_swapped":
            Vt = Vt[:, torch.arange(KT) ^ 8]
        khi, klo = bf.split(Kt)
        t = _three("bshd,blhd->blhs", khi, klo, qhi, qlo, wrong == "score_lohi_dropped") * sc           # x = mma32x3(khi, klo, qhi, qlo, x); t = x[reg] * sc, or -INFINITY
        live = n - 1 if (wrong == "last_key_dropped" and n < KT) else n
        if wrong != "tail_unmasked":
            t[..., live:] = float("-inf")
        mn = torch.maximum(m, t.amax(-1))                                                              # mn = fmaxf(m, swap32_max(tmax))
        alpha = torch.exp2(m - mn)                                                                     # alpha = exp2f(m - mn) (0 on the first tile)
        pr = torch.exp2(t - mn[..., None])                                                             # p = exp2f(x[reg] - mn)
        l = (l if wrong == "l_not_rescaled" else l * alpha) + pr.sum(-1)                               # l = l * alpha + swap32_sum(rs)
        m = mn
        if wrong != "o_not_rescaled":
            o = o * alpha[..., None]                                                                   # o[reg] *= alpha
        phi, plo = bf.split(pr)
        if wrong == "p_lo_dropped":
            plo = torch.zeros_like(plo)
        vhi, vlo = bf.split(Vt)
        o = o + _three("bshd,blhs->blhd", vhi, vlo, phi, plo)                                           # o = mma32x3(vhi, vlo, phi, plo, o)
    return (o * (1.0 / l)[..., None]).reshape(B, L, C)                                                 # inv = 1.0f / l; o[..] * inv


def standin_layer(sd, p, x, src, wrong=None):
    """the layer as its three kernels run it: float32 Q | K | V projections (``full_qkv``, exact-f32 tiles), :func:`standin_attention`, a
    float32 tail (merge, LayerNorm, MLP, LayerNorm, residual: ``full_tail``)"""
    B = max(x.shape[0], src.shape[0])
    w = lambda n: sd[p + n].detach().to(f32)
    xs, ss = x.to(f32).expand(B, -1, -1), src.to(f32).expand(B, -1, -1)
    msg = standin_attention(xs @ w("q_proj.weight").T, ss @ w("k_proj.weight").T, ss @ w("v_proj.weight").T, wrong)
    msg = F.layer_norm(msg @ w("merge.weight").T, (C,), w("norm1.weight"), w("norm1.bias"), 1e-5)
    msg = torch.relu(torch.cat([xs, msg], 2) @ w("mlp.0.weight").T) @ w("mlp.2.weight").T
    return xs + F.layer_norm(msg, (C,), w("norm2.weight"), w("norm2.bias"), 1e-5)


# ---- statistics -----------------------------------------------------------------------------------------------------------------------

def attention_error(o, ref, v, H=NH):
    """worst ``|o - ref| / max_{s, d} |v[b, s, head, d]|`` over every element; NaN in ``o`` gives NaN (never passes a bar)"""
    B, L = ref.shape[0], ref.shape[1]
    D = ref.shape[2] // H
    scale = v.to(f64).view(B, -1, H, D).abs().amax((1, 3))                                             # [B][H]
    err = (o.to(f64) - ref).abs().view(B, L, H, D) / scale[:, None, :, None]
    return float("nan") if bool(torch.isnan(err).any()) else err.max().item()


def row_error(y, ref):
    """worst ``|y - ref| / max(1, max |ref row|)``"""
    scale = ref.abs().amax(-1, keepdim=True).clamp(min=1.0)
    err = (y.to(f64) - ref).abs() / scale
    return float("nan") if bool(torch.isnan(err).any()) else err.max().item()


# ---- cases: the attention step ----------------------------------------------------------------------------------------------------------

LS = (1, 31, 32, 33, 127, 128, 129, 160)               # either side of the 32-query wave and of the 128-query workgroup; 160: a second workgroup with three idle waves
SS = (1, 31, 32, 33, 63, 64, 65, 97)                   # either side of one and of two 32-key tiles; 97: a fourth tile with one live key
SHAPES = [(1, L, S) for L in LS for S in SS] + [(3, L, S) for L in (LS[0], LS[-1]) for S in (SS[0], SS[-1])]
FAMILIES = ("soft", "growing", "falling", "peaked_last", "tail_bait", "uniform", "planted", "wide4", "wide16")
SELECTED_WEIGHT = 1.0 - 1e-6                           # "planted", "peaked_last": the selected key's softmax weight in float64 is above this
TAIL_GAP = 8.0                                         # "tail_bait": every real logit q.k / sqrt(D) lies below -TAIL_GAP


def _unit(g, H, D):
    e = torch.randn(H, D, generator=g, dtype=f64)
    return e / e.norm(dim=-1, keepdim=True)


def _perp(t, e):
    """``t [..][H][D]`` without its component along the heads' unit vectors ``e [H][D]``"""
    return t - (t * e).sum(-1, keepdim=True) * e


@functools.lru_cache(maxsize=None)
def _code_book(n=97, D=HD, bound=12):
    """``[n][H][D]``: per head ``n`` vectors of +-1 whose pairwise dot products lie within +-``bound`` (greedy, from a seeded generator); a case
    of S keys takes the first S"""
    g = torch.Generator().manual_seed(20240607)
    book = []
    for _ in range(NH):
        cand = (torch.randint(0, 2, (64 * n, D), generator=g) * 2 - 1).to(f64)
        keep = cand[:1]
        for c in cand[1:]:
            if len(keep) == n:
                break
            if (keep @ c).abs().max() <= bound:
                keep = torch.cat([keep, c[None]])
        assert len(keep) == n
        book.append(keep)
    return torch.stack(book, 1)


def planted_key(B, L, S):
    """``pi``: the key that query ``l`` of head ``h`` in batch element ``b`` selects, ``[B][L][H]``.  A step of 37 keys between neighbouring
    queries: the 32 queries of a wave select keys of every tile, of both 16-key k-steps and of both 8-key groups of each"""
    b, l, h = torch.meshgrid(torch.arange(B), torch.arange(L), torch.arange(NH), indexing="ij")
    return (37 * l + 11 + 5 * b + h) % S


@functools.lru_cache(maxsize=None)
def attention_case(family, B, L, S, H=NH, D=HD):
    """``dict(q [B][L][H D], k, v [B][S][H D]`` float32, ``sel [B][L][H]`` or None: the key whose value row the output is``)``; seeded by its
    arguments alone.  The tensors are shared between tests: never write to them."""
    assert family in FAMILIES
    g = torch.Generator().manual_seed(1000003 * FAMILIES.index(family) + 10007 * B + 101 * L + S + 7 * D)
    rn = lambda *s: torch.randn(*s, generator=g, dtype=f64)
    q, k, v, sel = rn(B, L, H, D), rn(B, S, H, D), rn(B, S, H, D), None
    if family in ("growing", "falling"):
        ramp = torch.linspace(0.2, 3.0, S, dtype=f64)
        k = k * (ramp if family == "growing" else ramp.flip(0)).view(1, S, 1, 1)
    elif family in ("wide4", "wide16"):
        s = 4.0 if family == "wide4" else 16.0           # logits of standard deviation s^2 (sqrt(D) products of variance s^4, over sqrt(D))
        q, k = q * s, k * s
    elif family == "uniform":
        k = k[:, :1].expand(B, S, H, D).clone()
    elif family == "peaked_last":
        e, a = _unit(g, H, D), math.sqrt(26.0 * math.sqrt(D))          # the selected logit is a^2 / sqrt(D) = 26 (+- 2), every other within +- 1
        q = a * e + 0.3 * q
        k = 0.5 * _perp(k, e)
        k[:, S - 1] = a * e
        v[:, S - 1] += 4.0
        sel = torch.full((B, L, H), S - 1)
    elif family == "tail_bait":
        e, a = _unit(g, H, D), math.sqrt(12.0 * math.sqrt(D))          # every logit -12 .. -15 (+- 1.6)
        q = a * e + 0.3 * q
        k = 0.5 * _perp(k, e) - a * (1.0 + 0.25 * torch.rand(B, S, H, 1, generator=g, dtype=f64)) * e
        v = v + 2.0
    elif family == "planted":
        assert D == HD
        assert S <= 97
        codes = _code_book()[:S]                                                                       # [S][H][D]
        flip = (torch.randint(0, 2, (B, 1, H, D), generator=g) * 2 - 1).to(f64)                         # per batch element: the dot products stay
        k = codes[None] * flip
        sel = planted_key(B, L, S)
        q = 6.0 * torch.gather(k, 1, sel[..., None].expand(B, L, H, D))                                # own logit 6 x 32 / sqrt(32) = 33.9, others <= 12.7
        s, h, d = torch.meshgrid(torch.arange(S), torch.arange(H), torch.arange(D), indexing="ij")
        v = ((s + 1) + 0.25 * h + d / 128.0).to(f64)[None] + 0.01 * v                                  # v[s] encodes s (+ bits for the lo plane)
    out = {n: t.to(f32).reshape(B, -1, H * D).contiguous() for n, t in (("q", q), ("k", k), ("v", v))}
    out["sel"] = sel
    return out


@functools.lru_cache(maxsize=None)
def attention_reference(family, B, L, S, H=NH, D=HD):
    c = attention_case(family, B, L, S, H, D)
    return reference_attention(c["q"], c["k"], c["v"], H)


def logits64(c, H=NH):
    """``q.k / sqrt(D)`` of a case in float64, ``[B][L][S][H]``"""
    B = c["q"].shape[0]
    q, k = (c[n].to(f64).view(B, -1, H, c[n].shape[2] // H) for n in ("q", "k"))
    return torch.einsum("nlhd,nshd->nlsh", q, k) / math.sqrt(q.shape[-1])


def selected_rows(c, H=NH):
    """``v[b, sel[b, l, h], h, :]`` as ``[B][L][H D]`` float64: what the output of a "planted" / "peaked_last" case is, to within
    ``2 (1 - SELECTED_WEIGHT)`` of the statistic (the other keys' weight times the largest distance between two value rows)"""
    B, L = c["q"].shape[0], c["q"].shape[1]
    v = c["v"].to(f64).view(B, -1, H, c["v"].shape[2] // H)
    return torch.gather(v, 1, c["sel"][..., None].expand(B, L, H, v.shape[-1])).reshape(B, L, -1)


# ---- cases: the layer entries -------------------------------------------------------------------------------------------------------------

LAYER_SHAPES = [(L3, L2) for L3 in (1, 31, 32, 33) for L2 in (1, 33)] + [(129, 65), (65, 129)]        # 32 = OPHIP_TOK, the row tile
STREAM_SHAPES = [(1, 1), (33, 31), (129, 65)]
STREAM_MODES = ("pair", "shared_src", "shared_x", "self")
STREAM_B = 2


def layer_inputs(B, L3, L2):
    """seeded randn streams; batch element 0 of a B = 2 case is the B = 1 case"""
    g = torch.Generator().manual_seed(31 * L3 + L2)
    return torch.randn(2, L3, C, generator=g)[:B].contiguous(), torch.randn(2, L2, C, generator=g)[:B].contiguous()


def stream_inputs(mode, L, S):
    """``(x, src)`` of a one-stream case at batch extent STREAM_B; a shared input has extent 1; "self": ``src is x`` (and S = L)"""
    x, s = layer_inputs(STREAM_B, L, L if mode == "self" else S)
    if mode == "self":
        return x, x
    return (x[:1] if mode == "shared_x" else x), (s[:1] if mode == "shared_src" else s)


# ---- the fine kernels (csrc/fine_full.hip) --------------------------------------------------------------------------------------------------

CF, FNH, FDH = 128, 8, 16
FINE_FAMILIES = ("soft", "peaked_last", "uniform", "wide4", "wide16")
FINE_SHAPES = [(32, 32), (1, 32), (32, 1), (25, 25)]                  # ophip_fine_full_attention (L, S <= 32)
FINE2_SHAPES = [(121, 121), (1, 121), (121, 1)]                       # ophip_fine2_full_attention (an 11 x 11 window)
FINE_K = 6                                                            # matches per call


def standin_fine_attention(q, k, v):
    """the two passes of ``fine_full_attention_kernel`` / ``fine2_full_attention_kernel`` in float32: scores, their exact row maximum, exp,
    sum, weighted values, ``1 / sum``"""
    K, L, S = q.shape[0], q.shape[1], k.shape[1]
    Q, Kk, V = (t.to(f32).view(K, -1, FNH, FDH) for t in (q, k, v))
    t = torch.zeros(K, L, S, FNH, dtype=f32)
    for d in range(FDH):                                                   # the kernels' chain of 16 products, in their order
        t = t + Q[:, :, None, :, d] * Kk[:, None, :, :, d]
    t = t * 0.25
    mx = t.amax(2)
    acc, tot = torch.zeros(K, L, FNH, FDH, dtype=f32), torch.zeros(K, L, FNH, dtype=f32)
    for s in range(S):                                                     # and their chain over the keys
        e = torch.exp(t[:, :, s] - mx)
        tot = tot + e
        acc = acc + e[..., None] * V[:, None, s]
    return (acc * (1.0 / tot)[..., None]).reshape(K, L, CF)


MATCH_WS = (3, 5, 7, 9, 11)
MATCH_FAMILIES = ("peak", "uniform", "sharp")
MATCH_SCALE = 2.0                                                     # image height / fine height
MATCH_B = 2


@functools.lru_cache(maxsize=None)
def match_case(family, W):
    """``dict(f3 [K][128], win [K][W W][128], mkc [K][2], b_ids [K], qscale [B][2])``.  "peak": K = 5 matches whose window token at the four
    corners and at the centre carries a logit 6 above the others'; "sharp": the same with a logit 40 above (every other weight below 1e-17:
    ``ex2 - ex^2`` cancels and the 1e-10 clamp acts); "uniform": every window token equal (the largest std)."""
    g = torch.Generator().manual_seed(97 * MATCH_FAMILIES.index(family) + W)
    WW = W * W
    spots = [0, W - 1, WW - W, WW - 1, WW // 2]
    K = len(spots)
    e = torch.randn(K, CF, generator=g, dtype=f64)
    e = e / e.norm(dim=-1, keepdim=True)
    f3 = math.sqrt(CF) * e                                            # |f3|^2 / sqrt(128) = sqrt(128): a token a e has the logit a
    noise = torch.randn(K, WW, CF, generator=g, dtype=f64)
    win = 0.3 * (noise - (noise * e[:, None]).sum(-1, keepdim=True) * e[:, None])              # logits 0.3 N(0, 1) about zero
    if family == "uniform":
        win = win[:, :1].expand(K, WW, CF).clone()
    else:
        for m, s in enumerate(spots):
            win[m, s] += (6.0 if family == "peak" else 40.0) * e[m]
    mkc = 100.0 * torch.rand(K, 2, generator=g, dtype=f64) + 20.0
    return dict(f3=f3.to(f32), win=win.to(f32), mkc=mkc.to(f32), b_ids=torch.tensor([0, 1, 1, 0, 1]),
                qscale=torch.tensor([[1.5, 0.75], [0.5, 1.25]], dtype=f32), spots=spots)


def reference_match(c, W, scaled):
    """``onepose_oracle.fine_match`` in float64: ``(expec_f [K][3], mkpts_f [K][2])``"""
    from oracle import onepose_oracle as orc
    qs = c["qscale"].to(f64) if scaled else None
    out = orc.fine_match(c["f3"].to(f64)[:, None], c["win"].to(f64), c["mkc"].to(f64), (MATCH_SCALE * 8, 0), (8, 0), qs, c["b_ids"] if scaled else None)
    return out["expec_f"], out["mkpts_query_f"]


def _wave_sum(x):
    """``wave_sum`` (tile.h): the xor butterfly over 64 lanes, ``x [K][64]`` -> ``[K]``"""
    lanes = torch.arange(64)
    for o in (32, 16, 8, 4, 2, 1):
        x = x + x[:, lanes ^ o]
    return x[:, 0]


def standin_match(c, W, scaled):
    """``fine_full_match_kernel`` in float32, in its order: the chain of 128 products per logit, softmax over lanes ``tid`` and ``tid + 64``
    with the butterfly sums, the grid ``-1 + step i``, first and second moments, the clamped std, keypoints"""
    f3, win = c["f3"], c["win"]
    K, WW = win.shape[0], W * W
    dot = torch.zeros(K, WW, dtype=f32)
    for ch in range(CF):
        dot = dot + f3[:, None, ch] * win[:, :, ch]
    t = F.pad(dot * torch.tensor(0.08838834764831845, dtype=f32), (0, 128 - WW), value=float("-inf"))
    e = torch.exp(t - t.amax(1, keepdim=True))
    ea, eb = e[:, :64], e[:, 64:]
    tot = _wave_sum(ea + eb)
    pa, pb = ea / tot[:, None], eb / tot[:, None]
    step = torch.tensor(2.0, dtype=f32) / float(W - 1)
    i = torch.arange(128)
    gx, gy = -1.0 + step * (i % W).to(f32), -1.0 + step * (i // W).to(f32)
    mom = lambda ga, gb: _wave_sum(pa * ga[:64] + pb * gb[64:])
    ex, ey = mom(gx, gx), mom(gy, gy)
    ex2, ey2 = _wave_sum(pa * gx[:64] * gx[:64] + pb * gx[64:] * gx[64:]), _wave_sum(pa * gy[:64] * gy[:64] + pb * gy[64:] * gy[64:])
    std = torch.sqrt(torch.clamp(ex2 - ex * ex, min=1e-10)) + torch.sqrt(torch.clamp(ey2 - ey * ey, min=1e-10))
    s = torch.full((K, 2), MATCH_SCALE, dtype=f32)
    if scaled:
        s = s * c["qscale"][c["b_ids"]][:, [1, 0]]
    coords = torch.stack([ex, ey], 1)
    return torch.cat([coords, std[:, None]], 1), c["mkc"] + coords * float(W // 2) * s


def match_errors(expec, mkf, ref_expec, ref_mkf, c, W):
    """worst ``|coords - ref|`` (the grid spans -1 .. 1), worst ``|std - ref|`` and worst ``|mkpts - ref| / (|mkpts_c| + (W // 2) scale)``: a
    keypoint's error in units of its terms"""
    co = (expec[:, :2].to(f64) - ref_expec[:, :2]).abs().max().item()
    sd_ = (expec[:, 2].to(f64) - ref_expec[:, 2]).abs().max().item()
    mk = ((mkf.to(f64) - ref_mkf).abs() / (c["mkc"].to(f64).abs() + (W // 2) * MATCH_SCALE * 1.5)).max().item()
    return co, sd_, mk


# ---- bars: every figure below is the f32 stand-in against the float64 reference, measured by tests/test_full_faithful_cpu.py -----------------
# (its test_the_precision_bars_* recompute each over exactly the cases named and assert ``2 worst <= bar <= 4 worst``).  A bar is THREE times the
# stand-in's worst, written with two digits; none comes from a device figure.

# Every figure moves by a few per cent with the summation order of the CPU's f32 matrix product; the factor of three leaves a third either way.

# the attention step, worst :func:`attention_error` over SHAPES, per family.  "soft" to "planted" sit at 2^-17 = 7.6e-6: the split of V keeps 16
# mantissa bits, and an output that IS a value row (S = 1, a one-hot softmax) carries that row's remainder whole; "growing" / "falling": three
# times that, the keys of norm 3 put the split's error of the score (2^-17 |q| |k|) into the weights; "wide": the same error at 16 and 256 times
# the logit, where the f32 ``t = x * scale`` itself is only good to 2^-24 |t|.
ATTENTION_BAR = {"soft": 2.1e-5,            # measured: 7.14e-6 at (3, 160, 1)
                 "growing": 6.6e-5,         # measured: 2.19e-5 at (1, 160, 32)
                 "falling": 6.1e-5,         # measured: 2.04e-5 at (1, 128, 33)
                 "peaked_last": 1.8e-5,     # measured: 6.02e-6 at (1, 33, 32)
                 "tail_bait": 2.1e-5,       # measured: 6.90e-6 at (3, 160, 1)
                 "uniform": 2.1e-5,         # measured: 7.01e-6 at (1, 33, 1)
                 "planted": 2.3e-5,         # measured: 7.60e-6 at (1, 127, 63)
                 "wide4": 3.3e-4,           # measured: 1.11e-4 at (1, 127, 33)
                 "wide16": 3.3e-3}          # measured: 1.11e-3 at (1, 33, 64)
# the layer rows, worst :func:`row_error` over LAYER_SHAPES x cross x B in (1, 2) and STREAM_SHAPES x STREAM_MODES (randn inputs)
LAYER_BAR = 1.9e-5                          # measured: 6.36e-6 at the two-stream call (65, 129), cross, 2D rows
# the fine attention kernels, worst :func:`attention_error` over FINE_SHAPES + FINE2_SHAPES at FINE_K matches, per family (plain f32: no split)
FINE_ATTENTION_BAR = {"soft": 7.2e-7,       # measured: 2.41e-7 at (32, 32)
                      "peaked_last": 9.7e-8,    # measured: 3.22e-8 at (121, 121)
                      "uniform": 9.8e-8,    # measured: 3.26e-8 at (25, 25)
                      "wide4": 7.4e-6,      # measured: 2.46e-6 at (121, 121)
                      "wide16": 1.1e-4}     # measured: 3.70e-5 at (121, 121)
# fine matching over MATCH_WS x (query_scale NULL, given), per family: (coords, std, keypoints) of :func:`match_errors`.
# "sharp", coords and std, come from REASONING, because there the stand-in only measures the float64 reference's own rounding (4e-16, 5e-13): the
# peak sits at a corner or at the centre, where the grid is +-1 or 0 exactly in f32 and in the oracle alike; every other weight is below 1e-17 and
# vanishes against the peak's 1.0f, so a correct f32 kernel returns the peak's grid point to within one ulp of 1 (2^-23) and a variance that is 0
# or below 1e-17: the clamp acts and the std is ``2 sqrtf(1e-10f)``, which f32 holds to a few ulp of 2e-5 (8 ulp of 2^-39 = 1.5e-11 > 1e-11).
# That is what float32 can hold HERE; a peak between grid points that are inexact in f32 would leave ``ex2 - ex^2`` at up to 2^-24, a std of 2.4e-4
# where the truth is 2e-5, which is why the family plants its peaks where it does.
MATCH_BAR = {"peak": (1.5e-6, 2.1e-6, 3.3e-7),          # measured: 4.85e-7, 7.04e-7, 1.11e-7
             "uniform": (7.0e-8, 4.3e-7, 4.1e-9),       # measured: 2.32e-8, 1.43e-7, 1.36e-9
             "sharp": (2.0 ** -23, 1.0e-11, 1.6e-7)}    # reasoned, reasoned, measured: 5.27e-8
