"""Float64 restatements of the six kernels of csrc/loftr_fine.hip, each written from its formula (not from the kernel, not from
oracle/loftr_oracle.py), the inputs of the edge cases that tests/test_gpu_loftr_fine.py runs on the device, and the bounds.

Every restatement takes ``dtype``: float64 is the reference, float32 is the stand-in whose distance from the reference says what f32
arithmetic alone costs (tests/test_loftr_fine_reference_cpu.py measures it and compares every restatement with the oracle).

Bounds.  ``BARS`` are the bars the suite already holds these kernels to at window 9 (tests/test_gpu_loftr.py), here against float64.
Three case families need not meet them for reasons of f32 arithmetic alone; their bound is the largest absolute error, over the family's
cases, of the float32 stand-in against float64 on the same inputs (``*_STANDIN``, measured on the CPU) times ``MARGIN``: the kernel sums
in another order than the stand-in, with ``expf`` and wave reductions.  The CPU test re-derives the ``*_STANDIN`` figures and shows that
every seeded fault lies outside the bounds.  Nothing here is taken from a device's output.
"""
import numpy as np
import torch

CF, NH, DH = 128, 8, 16
WINDOWS = (3, 5, 7, 9, 11)

# (rtol, atol) of numpy.testing.assert_allclose
BARS = {"attention": (1e-4, 1e-5), "layernorm": (1e-5, 1e-5), "linear": (2e-4, 2e-5), "expec": (1e-4, 1e-5), "std": (1e-3, 1e-3),
        "mkpts1_f": (1e-5, 1e-4)}
MARGIN = 8.0
# largest |float32 stand-in - float64| over each family's cases (the CPU test re-derives them: at most these, at least half of them)
LN_MEAN100_STANDIN = 2.4e-5        # measured 2.324e-05 (T = 1863)
ATTN_SHIFTED_STANDIN = 2.6e-6      # measured 2.534e-06
ONEHOT_STD_STANDIN = 5.1e-13       # measured 5.052e-13: the float32 rounding of sqrt(1e-10), twice
LN_MEAN100_BOUND = MARGIN * LN_MEAN100_STANDIN
ATTN_SHIFTED_BOUND = MARGIN * ATTN_SHIFTED_STANDIN
ONEHOT_STD_BOUND = MARGIN * ONEHOT_STD_STANDIN


def excess(got, ref, bar):
    """largest |got - ref| / (atol + rtol |ref|): at most 1 exactly where ``assert_allclose(got, ref, *bar)`` passes"""
    got, ref = torch.as_tensor(got).double().cpu(), torch.as_tensor(ref).double().cpu()
    if ref.numel() == 0:
        return 0.0
    return float(((got - ref).abs() / (bar[1] + bar[0] * ref.abs())).max())


def max_abs(got, ref):
    got, ref = torch.as_tensor(got).double().cpu(), torch.as_tensor(ref).double().cpu()
    return float((got - ref).abs().max()) if ref.numel() else 0.0


# ---- the restatements ----------------------------------------------------------------------------------------------------------------
def windows(feat_cl, b_ids, cells, hf, wf, wc, stride, W):
    """W x W window of the channels-last fine map ``feat_cl [B, hf * wf, C]`` around the fine pixel ``stride * (cell // wc, cell % wc)``
    of image ``b_ids[k]``, row-major, zeros outside the map -> ``[K, W * W, C]``"""
    K, C = len(cells), feat_cl.shape[-1]
    out = torch.zeros(K, W * W, C, dtype=feat_cl.dtype)
    for k in range(K):
        cy, cx = stride * (int(cells[k]) // wc), stride * (int(cells[k]) % wc)
        for r in range(W * W):
            y, x = cy + r // W - W // 2, cx + r % W - W // 2
            if 0 <= y < hf and 0 <= x < wf:
                out[k, r] = feat_cl[int(b_ids[k]), y * wf + x]
    return out


def phi(x):
    """elu(x) + 1"""
    return torch.where(x > 0, x + 1, torch.exp(x))


def linear_attention(q, k, v, dtype=torch.float64):
    """``q [K, L, 128]`` against ``k, v [K, S, 128]``, 8 heads of 16: out_l = S phi(q_l) (sum_s phi(k_s)^T v_s / S) / (phi(q_l) . sum_s phi(k_s) + 1e-6)"""
    Kn, L, S = q.shape[0], q.shape[1], k.shape[1]
    heads = lambda t, n: t.to(dtype).reshape(Kn, n, NH, DH).transpose(1, 2)               # [K, 8, n, 16]
    Q, Kf, V = phi(heads(q, L)), phi(heads(k, S)), heads(v, S) / S
    KV = Kf.transpose(2, 3) @ V                                                           # [K, 8, 16, 16]
    den = Q @ Kf.sum(dim=2)[..., None] + 1e-6                                             # [K, 8, L, 1]
    return ((Q @ KV) / den * S).transpose(1, 2).reshape(Kn, L, CF)


def layernorm(x, gamma, beta, res=None, dtype=torch.float64):
    """rows of 128: (x - mean) / sqrt(var + 1e-5) gamma + beta (+ res), the variance two-pass and biased"""
    x = x.to(dtype)
    d = x - x.mean(dim=1, keepdim=True)
    y = d / torch.sqrt((d * d).mean(dim=1, keepdim=True) + 1e-5) * gamma.to(dtype) + beta.to(dtype)
    return y if res is None else y + res.to(dtype)


def rows_linear(xa, xb, w, relu, dtype=torch.float64):
    """``[xa | xb] w^T``, optionally through ReLU"""
    x = xa.to(dtype) if xb is None else torch.cat([xa.to(dtype), xb.to(dtype)], 1)
    y = x @ w.to(dtype).T
    return y.clamp(min=0) if relu else y


def fine_grid(W, dtype=torch.float64):
    """normalised window coordinates -1 + 2 i / (W - 1), x fastest -> ``gx, gy [W * W]``"""
    i = torch.arange(W * W)
    step = torch.tensor(2.0, dtype=dtype) / (W - 1)
    return -1 + step * (i % W).to(dtype), -1 + step * (i // W).to(dtype)


def fine_heat(f0, f1, centre, dtype=torch.float64):
    """softmax over image 1's window of (token ``centre`` of image 0's window) . (token r of image 1's) / sqrt(128)"""
    sim = (f0[:, centre].to(dtype)[:, None, :] * f1.to(dtype)).sum(-1) / CF ** 0.5
    e = torch.exp(sim - sim.max(dim=1, keepdim=True)[0])
    return e / e.sum(dim=1, keepdim=True)


def fine_expec(heat, gx, gy):
    """-> ``[K, 3]``: expectation (x, y) and std_x + std_y, every variance clamped at 1e-10"""
    ex, ey = (heat * gx).sum(1), (heat * gy).sum(1)
    vx, vy = (heat * gx * gx).sum(1) - ex * ex, (heat * gy * gy).sum(1) - ey * ey
    return torch.stack([ex, ey, vx.clamp(min=1e-10).sqrt() + vy.clamp(min=1e-10).sqrt()], 1)


def fine_match(f0, f1, mk1_c, W, scale, dtype=torch.float64):
    """``scale`` = image height / fine-map height -> ``expec [K, 3]``, ``mkpts1_f = mk1_c + expec[:, :2] (W // 2) scale``"""
    expec = fine_expec(fine_heat(f0, f1, (W * W) // 2, dtype), *fine_grid(W, dtype))
    return expec, mk1_c.to(dtype) + expec[:, :2] * (W // 2) * scale


def scaled_keypoints(mk1_c, coords, W, scale, scale1, b_ids):
    """the rounding contract of the scaled form: ``mk1_c + (coords (W // 2)) (scale scale1[b_ids])``, each product rounded to float32,
    the sum in the keypoints' dtype.  ``scale1 [B or 1, 2]`` float32, component 0 on x; ``coords [K, 2]`` are rounded to float32 first"""
    f = np.float32
    c = np.asarray(torch.as_tensor(coords).double()).astype(f)
    s1 = np.asarray(scale1, dtype=f)
    s = s1[np.asarray(b_ids)] if s1.shape[0] > 1 else np.broadcast_to(s1, (len(c), 2))
    d = (c * f(W // 2)) * (f(scale) * s)
    mk = mk1_c.numpy()
    return torch.from_numpy(mk + d.astype(mk.dtype))


def fine_match_scaled(f0, f1, mk1_c, W, scale, scale1, b_ids, dtype=torch.float64):
    """-> ``expec [K, 3]`` from the ``dtype`` heat map, ``mkpts1_f`` in the keypoints' dtype by the rounding contract"""
    expec = fine_expec(fine_heat(f0, f1, (W * W) // 2, dtype), *fine_grid(W, dtype))
    return expec, scaled_keypoints(mk1_c, expec[:, :2], W, scale, scale1, b_ids)


# ---- the cases of the device test (inputs only; float32, on the CPU) -----------------------------------------------------------------
GATHER_MAPS = {"5x6 stride 2": (5, 6, 2), "3x4 stride 4": (3, 4, 4)}                     # coarse rows, coarse columns, stride
GATHER_WINDOWS = (1, 3, 5, 7, 9, 11)


def gather_cells(hc, wc):
    """the four corners, one cell on each edge, one interior cell, twice, and one more edge cell: K = 19"""
    nine = [0, wc - 1, (hc - 1) * wc, hc * wc - 1, 1, wc, 2 * wc - 1, (hc - 1) * wc + 2, wc + 1]
    return torch.tensor(nine + nine + [wc - 2])


def gather_map(name, B=3, seed=5):
    hc, wc, stride = GATHER_MAPS[name]
    g = torch.Generator().manual_seed(seed + hc)
    return torch.randn(B, hc * stride * wc * stride, CF, generator=g)


ATTN_SHAPES = ((1, 1), (9, 9), (49, 49), (81, 81), (121, 121), (81, 121), (121, 25), (1, 128), (200, 128))
ATTN_COUNTS = (1, 7)


def attention_inputs(K, L, S, shifted):
    """``randn``; shifted: ``randn * 4 - 2``, where the exp branch and the x + 1 branch of phi both carry weight"""
    g = torch.Generator().manual_seed(1000 * L + 7 * S + K + (500000 if shifted else 0))
    q, k, v = torch.randn(K, L, CF, generator=g), torch.randn(K, S, CF, generator=g), torch.randn(K, S, CF, generator=g)
    return (q * 4 - 2, k * 4 - 2, v * 4 - 2) if shifted else (q, k, v)


LN_ROWS = (1, 2, 3, 4, 5, 1863)
LN_KINDS = ("ordinary", "equal", "mean100")
EQUAL_VALUE = 0.7


def layernorm_inputs(T, kind):
    """-> ``x, gamma, beta, res``.  ordinary: randn * 3 + 1; equal: the same with row T // 2 of equal values; mean100: 100 + randn"""
    g = torch.Generator().manual_seed(31 * T + LN_KINDS.index(kind))
    x = torch.randn(T, CF, generator=g)
    x = 100 + x if kind == "mean100" else x * 3 + 1
    if kind == "equal":
        x[T // 2] = EQUAL_VALUE
    gamma, beta = 1 + 0.2 * torch.randn(CF, generator=g), 0.2 * torch.randn(CF, generator=g)
    return x, gamma, beta, torch.randn(T, CF, generator=g)


LINEAR_ROWS = (63, 64, 65, 127, 128, 129)
LINEAR_FORMS = ((128, 128, 256, True), (256, 0, 128, False))


def linear_inputs(T, ka, kb, nout):
    g = torch.Generator().manual_seed(T + ka + nout)
    xa, xb = torch.randn(T, ka, generator=g), (torch.randn(T, kb, generator=g) if kb else None)
    return xa, xb, torch.randn(nout, ka + kb, generator=g) / (ka + kb) ** 0.5


MATCH_K = 23
ONEHOT = ("top left", "top right", "bottom left", "bottom right", "centre")
MATCH_CASES = ("random", "peak") + tuple("one-hot " + p for p in ONEHOT) + ("uniform", "equal negative")


def onehot_token(W, where):
    return {"top left": 0, "top right": W - 1, "bottom left": W * (W - 1), "bottom right": W * W - 1, "centre": (W * W) // 2}[where]


def match_inputs(W, case, K=MATCH_K):
    """-> ``f0, f1 [K, W * W, 128]``, ``mk1_c [K, 2]`` (float64; the plain form takes them as float32)"""
    WW, c = W * W, (W * W) // 2
    g = torch.Generator().manual_seed(100 * W + MATCH_CASES.index(case))
    f0, f1 = torch.randn(K, WW, CF, generator=g), torch.randn(K, WW, CF, generator=g)
    mk1 = torch.rand(K, 2, generator=g, dtype=torch.float64) * 100
    if case == "peak":                                       # one pixel right and down of the centre
        f1[:, c + W + 1] = 2.0 * f0[:, c]
    elif case.startswith("one-hot"):                         # logit 40 |f0|^2 / sqrt(128) ~ 450 against N(0, 1): one-hot in f32 and f64
        f1[:, onehot_token(W, case[len("one-hot "):])] = 40.0 * f0[:, c]
    elif case == "uniform":
        f1.zero_()
    elif case == "equal negative":                           # every logit -40 |f0|^2 / sqrt(128), the same sum for every token
        f1[:] = -40.0 * f0[:, c][:, None, :]
    return f0, f1, mk1
