"""tests/loftr_fine_reference.py without a GPU: every restatement against the oracle the suite already trusts (oracle/loftr_oracle.py,
oracle/onepose_oracle.py, ``F.layer_norm``) at every window the oracle takes, the float32 stand-ins against float64 (the ``*_STANDIN``
constants are re-derived here), seeded faults against the bounds of the device test, and the constructor's window range."""
import copy

import pytest
import torch
import torch.nn.functional as F

from oracle import loftr_oracle as lo
from oracle import onepose_oracle as orc
from onepose_st_amd import loftr
from tests import loftr_fine_reference as fr
from tests.loftr_fine_reference import BARS, excess, max_abs

F64, F32 = torch.float64, torch.float32


# ---- the restatements against the oracle ---------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", sorted(fr.GATHER_MAPS))
@pytest.mark.parametrize("W", fr.GATHER_WINDOWS)
def test_windows_equal_the_unfold(name, W):
    hc, wc, stride = fr.GATHER_MAPS[name]
    hf, wf = hc * stride, wc * stride
    feat, cells = fr.gather_map(name), fr.gather_cells(hc, wc)
    b_ids = torch.tensor([0, 2] * 10)[:len(cells)]
    nchw = feat.reshape(3, hf, wf, fr.CF).permute(0, 3, 1, 2).contiguous()
    assert len(cells) == 19 and torch.equal(fr.windows(feat, b_ids, cells, hf, wf, wc, stride, W), lo.fine_windows(nchw, b_ids, cells, (hc, wc), W))


@pytest.mark.parametrize("L,S", fr.ATTN_SHAPES)
def test_linear_attention_equals_the_oracle(L, S):
    q, k, v = (t.double() for t in fr.attention_inputs(3, L, S, shifted=True))
    want = orc.linear_attention(q.view(3, L, 8, 16), k.view(3, S, 8, 16), v.view(3, S, 8, 16)).reshape(3, L, 128)
    assert excess(fr.linear_attention(q, k, v), want, (1e-12, 1e-13)) <= 1


@pytest.mark.parametrize("kind", fr.LN_KINDS)
def test_layernorm_equals_torch(kind):
    x, gamma, beta, res = (t.double() for t in fr.layernorm_inputs(1863, kind))
    want = F.layer_norm(x, (128,), gamma, beta, 1e-5)
    assert excess(fr.layernorm(x, gamma, beta), want, (1e-11, 1e-11)) <= 1 and excess(fr.layernorm(x, gamma, beta, res), want + res, (1e-11, 1e-11)) <= 1
    if kind == "equal":
        assert torch.equal(fr.layernorm(x, gamma, beta)[1863 // 2], beta)


@pytest.mark.parametrize("case", ["random", "peak", "one-hot top right", "uniform"])
@pytest.mark.parametrize("W", fr.WINDOWS)
def test_fine_match_equals_the_oracle(W, case):
    f0, f1, mk1 = fr.match_inputs(W, case)
    hw_i, hw_f = (96, 128), (24, 32)                                   # scale 4
    want = lo.fine_matching(f0.double(), f1.double(), mk1, mk1, hw_i, hw_f)
    expec, mk1f = fr.fine_match(f0, f1, mk1, W, 4.0)
    # the oracle's grid is a float32 linspace (its error 6e-8 enters the expectation once and the std through a square root)
    assert excess(expec[:, :2], want["expec_f"][:, :2], (0, 2e-7)) <= 1 and excess(expec[:, 2], want["expec_f"][:, 2], (0, 1e-3)) <= 1
    assert excess(mk1f, want["mkpts1_f"], (0, 2e-6)) <= 1
    # the scaled form with unit scales and float64 keypoints: the plain form up to the float32 rounding of each product
    e2, m2 = fr.fine_match_scaled(f0, f1, mk1, W, 4.0, torch.ones(1, 2), torch.zeros(len(mk1), dtype=torch.long))
    assert torch.equal(e2, expec) and m2.dtype == F64 and max_abs(m2, mk1f) <= 2e-6


def test_scaled_keypoints_follow_torch_float32():
    """tests/loftr_sfm_oracle.py's formula, in torch float32: the same bits"""
    from tests import loftr_sfm_oracle as lsf
    g = torch.Generator().manual_seed(2)
    coords = torch.rand(50, 2, generator=g) * 2 - 1
    b_ids, s1 = torch.randint(0, 3, (50,), generator=g), torch.tensor([[1.25, 0.8], [0.7, 1.6], [1.1, 1.3]])
    for W in fr.WINDOWS:
        for dt in (F32, F64):
            mk = (torch.rand(50, 2, generator=g, dtype=F64) * 100).to(dt)
            for s in (s1, s1[:1]):
                want = lsf.fine_keypoints1(mk, coords, W, (96, 128), (48, 64), s, b_ids)
                got = fr.scaled_keypoints(mk, coords, W, 2.0, s, b_ids)
                assert got.dtype == dt and torch.equal(got, want)


def test_rows_linear_equals_a_matmul():
    xa, xb, w = fr.linear_inputs(65, 128, 128, 256)
    want = (torch.cat([xa, xb], 1).double() @ w.double().T).relu()
    assert torch.equal(fr.rows_linear(xa, xb, w, True), want) and (want == 0).any()
    xa, xb, w = fr.linear_inputs(65, 256, 0, 128)
    assert xb is None and torch.equal(fr.rows_linear(xa, None, w, False), xa.double() @ w.double().T)


# ---- the float32 stand-ins ----------------------------------------------------------------------------------------------------------
def _derived(measured, recorded):
    return 0.5 * recorded <= measured <= recorded


def test_standin_meets_the_bars_on_ordinary_inputs():
    """what the bars cost in plain float32: every family outside the three measured ones meets its bar.  (The row of equal values is
    left out: torch's float32 mean of 128 equal values is not that value, and 1 / sqrt(eps) = 316 multiplies what is left; the kernel's
    butterfly sum doubles at every step and is exact there.)"""
    worst = {}
    for L, S in fr.ATTN_SHAPES:
        q, k, v = fr.attention_inputs(7, L, S, shifted=False)
        worst["attention"] = max(worst.get("attention", 0), excess(fr.linear_attention(q, k, v, F32), fr.linear_attention(q, k, v), BARS["attention"]))
    for T in fr.LN_ROWS:
        for kind in ("ordinary",):
            x, gamma, beta, res = fr.layernorm_inputs(T, kind)
            worst["layernorm"] = max(worst.get("layernorm", 0), excess(fr.layernorm(x, gamma, beta, res, F32), fr.layernorm(x, gamma, beta, res), BARS["layernorm"]))
    for W in fr.WINDOWS:
        for case in fr.MATCH_CASES:
            f0, f1, mk1 = fr.match_inputs(W, case)
            (e32, m32), (e64, m64) = fr.fine_match(f0, f1, mk1.float(), W, 4.0, F32), fr.fine_match(f0, f1, mk1.float(), W, 4.0)
            worst["expec"] = max(worst.get("expec", 0), excess(e32[:, :2], e64[:, :2], BARS["expec"]))
            worst["mkpts1_f"] = max(worst.get("mkpts1_f", 0), excess(m32, m64, BARS["mkpts1_f"]))
            if not case.startswith("one-hot"):
                worst["std"] = max(worst.get("std", 0), excess(e32[:, 2], e64[:, 2], BARS["std"]))
    print("float32 stand-in, largest error in units of the bar:", {k: f"{v:.3g}" for k, v in worst.items()})
    assert max(worst.values()) <= 1


def _ln_mean100_standin():
    worst = 0.0
    for T in fr.LN_ROWS:
        x, gamma, beta, res = fr.layernorm_inputs(T, "mean100")
        for r in (None, res):
            worst = max(worst, max_abs(fr.layernorm(x, gamma, beta, r, F32), fr.layernorm(x, gamma, beta, r)))
    return worst


def _attn_shifted_standin():
    worst = 0.0
    for K in fr.ATTN_COUNTS:
        for L, S in fr.ATTN_SHAPES:
            q, k, v = fr.attention_inputs(K, L, S, shifted=True)
            worst = max(worst, max_abs(fr.linear_attention(q, k, v, F32), fr.linear_attention(q, k, v)))
    return worst


def _onehot_std_standin():
    worst = 0.0
    for W in fr.WINDOWS:
        for where in fr.ONEHOT:
            f0, f1, mk1 = fr.match_inputs(W, "one-hot " + where)
            worst = max(worst, max_abs(fr.fine_match(f0, f1, mk1, W, 4.0, F32)[0][:, 2], fr.fine_match(f0, f1, mk1, W, 4.0)[0][:, 2]))
    return worst


def test_recorded_standin_errors_are_the_measured_ones():
    ln, at, oh = _ln_mean100_standin(), _attn_shifted_standin(), _onehot_std_standin()
    print(f"float32 stand-in, largest |error|: mean-100 LayerNorm {ln:.3e}, shifted attention {at:.3e}, one-hot std {oh:.3e}")
    assert _derived(ln, fr.LN_MEAN100_STANDIN) and _derived(at, fr.ATTN_SHIFTED_STANDIN) and _derived(oh, fr.ONEHOT_STD_STANDIN)
    assert fr.LN_MEAN100_BOUND == 8 * fr.LN_MEAN100_STANDIN and fr.ATTN_SHIFTED_BOUND == 8 * fr.ATTN_SHIFTED_STANDIN
    assert fr.ONEHOT_STD_BOUND == 8 * fr.ONEHOT_STD_STANDIN


# ---- seeded faults: each lies outside the bound the device test holds the kernel to --------------------------------------------------
def test_fault_window_shifted_by_one_pixel():
    for name, (hc, wc, stride) in fr.GATHER_MAPS.items():
        hf, wf = hc * stride, wc * stride
        feat, cells, b_ids = fr.gather_map(name), fr.gather_cells(hc, wc), torch.zeros(19, dtype=torch.long)
        for W in fr.GATHER_WINDOWS:
            good = fr.windows(feat, b_ids, cells, hf, wf, wc, stride, W)
            right = fr.windows(feat.reshape(3, hf, wf, -1).roll(-1, 2).reshape(3, hf * wf, -1), b_ids, cells, hf, wf, wc, stride, W)
            down = fr.windows(feat.reshape(3, hf, wf, -1).roll(-1, 1).reshape(3, hf * wf, -1), b_ids, cells, hf, wf, wc, stride, W)
            assert not torch.equal(good, right) and not torch.equal(good, down), (name, W)


@pytest.mark.parametrize("L,S", [(81, 121), (121, 25), (1, 128), (200, 128)])
def test_fault_attention_scaled_by_the_query_length(L, S):
    """v / S and . S cancel, so a kernel with L in ONE of the two places is off by L / S or S / L"""
    q, k, v = fr.attention_inputs(7, L, S, shifted=False)
    good = fr.linear_attention(q, k, v)
    for bad in (good * L / S, good * S / L):               # . L in place of . S; v / L in place of v / S
        assert excess(bad, good, BARS["attention"]) > 100


def test_fault_one_pass_variance_on_the_large_mean_rows():
    """E[x^2] - E[x]^2 in float32 loses the variance's digits under a mean of 100; outside the family's bound, which the two-pass
    stand-in defines"""
    x, gamma, beta, _ = fr.layernorm_inputs(1863, "mean100")
    mean = x.mean(dim=1, keepdim=True)
    var = (x * x).mean(dim=1, keepdim=True) - mean * mean
    bad = (x - mean) / torch.sqrt(var + 1e-5) * gamma + beta
    err = max_abs(bad, fr.layernorm(x, gamma, beta))
    print(f"one-pass variance, float32: largest |error| {err:.3e} against the bound {fr.LN_MEAN100_BOUND:.3e}")
    assert err > 2 * fr.LN_MEAN100_BOUND
    # and on ordinary rows it would pass: only the large-mean rows hold the kernel to two passes
    x, gamma, beta, _ = fr.layernorm_inputs(1863, "ordinary")
    mean = x.mean(dim=1, keepdim=True)
    bad = (x - mean) / torch.sqrt((x * x).mean(dim=1, keepdim=True) - mean * mean + 1e-5) * gamma + beta
    assert excess(bad, fr.layernorm(x, gamma, beta), BARS["layernorm"]) <= 1


@pytest.mark.parametrize("W", fr.WINDOWS)
def test_fault_grid_step_and_centre_token(W):
    WW = W * W
    i = torch.arange(WW)
    bad_grid = (-1 + (2.0 / W) * (i % W).double(), -1 + (2.0 / W) * (i // W).double())
    caught_step, caught_centre = [], []
    for case in fr.MATCH_CASES:
        f0, f1, mk1 = fr.match_inputs(W, case)
        good, _ = fr.fine_match(f0, f1, mk1, W, 4.0)
        step = fr.fine_expec(fr.fine_heat(f0, f1, WW // 2), *bad_grid)
        centre = fr.fine_expec(fr.fine_heat(f0, f1, WW // 2 - 1), *fr.fine_grid(W))
        if excess(step[:, :2], good[:, :2], BARS["expec"]) > 100:
            caught_step.append(case)
        if excess(centre[:, :2], good[:, :2], BARS["expec"]) > 100:
            caught_centre.append(case)
    assert {"random", "peak", "one-hot bottom right", "one-hot centre", "uniform"} <= set(caught_step), caught_step
    assert {"random", "peak", "one-hot top left", "one-hot centre"} <= set(caught_centre), caught_centre


def test_fault_one_hot_std_off_the_clamp():
    """a variance clamp of 1e-8 in place of 1e-10 moves the one-hot std from 2e-5 to 2e-4: outside the family's bound"""
    assert 2e-4 - 2e-5 > 2 * fr.ONEHOT_STD_BOUND
    for W in fr.WINDOWS:
        for where in fr.ONEHOT:
            f0, f1, mk1 = fr.match_inputs(W, "one-hot " + where)
            expec, _ = fr.fine_match(f0, f1, mk1, W, 4.0)
            gx, gy = fr.fine_grid(W)
            p = fr.onehot_token(W, where)
            assert max_abs(expec[:, 0], gx[p].expand(fr.MATCH_K)) < 1e-12 and max_abs(expec[:, 1], gy[p].expand(fr.MATCH_K)) < 1e-12
            assert max_abs(expec[:, 2], torch.full((fr.MATCH_K,), 2e-5, dtype=F64)) < 1e-15


def test_uniform_heat_map_closed_form():
    for W in fr.WINDOWS:
        for case in ("uniform", "equal negative"):
            f0, f1, mk1 = fr.match_inputs(W, case)
            expec, mk1f = fr.fine_match(f0, f1, mk1, W, 4.0)
            gx, _ = fr.fine_grid(W)
            assert expec[:, :2].abs().max() < 1e-14 and max_abs(expec[:, 2], (2 * (gx * gx).mean().sqrt()).expand(fr.MATCH_K)) < 1e-14
            assert max_abs(mk1f, mk1) < 1e-12


# ---- the constructor ---------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("W", [1, 2, 4, 13])
def test_constructor_refuses_windows_outside_3_to_11_odd(W):
    cfg = copy.deepcopy(loftr.default_cfg)
    cfg["fine_window_size"] = W
    with pytest.raises(ValueError, match="odd, from 3 to 11"):
        loftr.LoFTR_for_OnePose_Plus(cfg)


@pytest.mark.parametrize("W", [3, 5, 7, 9, 11])
def test_constructor_accepts_every_odd_window_from_3_to_11(W):
    cfg = copy.deepcopy(loftr.default_cfg)
    cfg["fine_window_size"] = W
    assert loftr.LoFTR_for_OnePose_Plus(cfg).config["fine_window_size"] == W
