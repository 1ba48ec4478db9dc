"""The LoFTR matcher's fine stage on the MI355X -- the six kernels of csrc/loftr_fine.hip behind ``ophip_fine2_gather`` / ``_gather_b``,
``ophip_fine2_attention``, ``ophip_rows_layernorm128``, ``ophip_rows_linear_x3``, ``ophip_fine2_match`` / ``_match_scaled`` -- against the
float64 restatements of tests/loftr_fine_reference.py at every window size, length and edge the entry points accept, and the whole
matcher at windows 5 and 7 against oracle/loftr_oracle.py.  Every call goes through ``hip.call``; every output buffer starts as NaN.

Bounds (tests/loftr_fine_reference.py; none comes from a device).  Gather, integer outputs and the scaled form's ``mkpts1_f``: exact.
Elsewhere the bars of tests/test_gpu_loftr.py at window 9, ``BARS``, now against float64.  Three families are held to 8 times the error
of the float32 stand-in on the same inputs, measured on the CPU by tests/test_loftr_fine_reference_cpu.py, in place of their bar.

Largest error observed on the MI355X (the module prints them), beside the bound and its source ("of the bar": the largest
|error| / (atol + rtol |reference|), 1 being the bar):

    kernel     family                                    observed               bound
    gather     every window, map, batch form             bit-equal              exact
    attention  randn, every (L, S), K 1 / 7 / 300        3.9e-3 of the bar      rtol 1e-4 / atol 1e-5 (test_gpu_loftr.py)
    attention  randn * 4 - 2                             3.2e-6 absolute        2.08e-5 = 8 x 2.6e-6 (float32 stand-in)
    LayerNorm  ordinary rows, T 1 .. 1863                3.8e-2 of the bar      1e-5 / 1e-5 (test_gpu_loftr.py)
    LayerNorm  the row of equal values against beta      3.9e-3 of the bar      1e-5 / 1e-5
    LayerNorm  mean 100, std 1                           1.5e-5 absolute        1.92e-4 = 8 x 2.4e-5 (float32 stand-in)
    linear     T 63 .. 129, both forms                   0.81 of the bar        2e-4 / 2e-5 (test_gpu_loftr.py::test_rows_linear_x3)
    match      expectation, every window and heat map    1.3e-2 of the bar      1e-4 / 1e-5 (test_gpu_loftr.py)
    match      one-hot expectation against its grid pt   3.0e-8 absolute        1e-4 / 1e-5
    match      std, all but the one-hot maps             0.77 of the bar        1e-3 / 1e-3 (test_gpu_loftr.py); window 3, planted peak
    match      one-hot std (the clamp, 2e-5)             5.1e-13 absolute       4.08e-12 = 8 x 5.1e-13 (float32 stand-in)
    match      mkpts1_f, plain form                      8.3e-3 of the bar      1e-5 / 1e-4 (test_gpu_loftr.py)
    match      mkpts1_f, scaled form                     bit-equal              exact (the rounding contract on the kernel's expectation)

The float32 stand-in of the planted-peak std sits at 0.77 of its bar at window 3 too (a variance of 1e-9 taken as a difference of two
numbers near 1): the figure is f32 arithmetic, not the kernel's.  The plain form may fuse ``mk + e * scale``; with unit scales the scaled
form gives the same bits where ``W // 2`` is a power of two (windows 3, 5, 9) and lies within 9e-3 of the bar at windows 7 and 11.
"""
import copy

import numpy as np
import pytest
import torch

from oracle import loftr_oracle as lo
from onepose_st_amd import hip, loftr, packing
from onepose_st_amd.synthetic import make_synthetic_loftr_state_dict
from tests import loftr_fine_reference as fr
from tests import test_gpu_loftr as tgl
from tests.loftr_fine_reference import BARS, excess, max_abs
from tests.loftr_helpers import device_hook, oracle_hook, planted_pair

pytestmark = pytest.mark.gpu

FIGURES = {}          # family -> largest error seen (units of its bar, or absolute where the bound is absolute)


@pytest.fixture(scope="module")
def dev():
    if not torch.cuda.is_available():
        pytest.skip("needs the MI355X")
    hip.load()
    yield torch.device("cuda:0")
    for family, (value, unit) in sorted(FIGURES.items()):
        print(f"largest device error  {family:34s} {value:.3e} {unit}")


@pytest.fixture(scope="module")
def lsd():
    return make_synthetic_loftr_state_dict(0)


def nan(dev, *shape, dtype=torch.float32):
    return torch.full(shape, float("nan"), dtype=dtype, device=dev)


def note(family, value, unit):
    FIGURES[family] = (max(value, FIGURES.get(family, (0.0, unit))[0]), unit)


def within_bar(family, got, ref, bar, msg=""):
    e = excess(got, ref, BARS[bar])
    note(family, e, f"of the bar {BARS[bar]}")
    assert e <= 1, (family, msg, e)


def within_abs(family, got, ref, bound, msg=""):
    e = max_abs(got, ref)
    note(family, e, f"absolute, bound {bound:.3e}")
    assert e <= bound, (family, msg, e, bound)


P, I64 = hip.ptr, torch.int64


# ---- gather --------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", sorted(fr.GATHER_MAPS))
@pytest.mark.parametrize("W", fr.GATHER_WINDOWS)
def test_gather_is_bit_equal_at_every_window_and_border(dev, name, W):
    hc, wc, stride = fr.GATHER_MAPS[name]
    hf, wf = hc * stride, wc * stride
    feat, cells = fr.gather_map(name), fr.gather_cells(hc, wc)
    K = len(cells)
    b_ids = torch.tensor([0, 2] * K)[:K]                                       # images 0 and 2 of three
    zeros = torch.zeros(K, dtype=I64)
    dfeat, dcells, db = feat.to(dev), cells.to(dev), b_ids.to(dev)
    S = hip.stream_handle()
    out = nan(dev, K, W * W, 128)                                              # one image: image 1 of the batch
    hip.call("ophip_fine2_gather", P(dfeat[1]), hf, wf, P(dcells, I64), K, wc, stride, W, P(out), S)
    assert torch.equal(out.cpu(), fr.windows(feat[1:2], zeros, cells, hf, wf, wc, stride, W))
    out = nan(dev, K, W * W, 128)                                              # batch of three, the matches on images 0 and 2
    hip.call("ophip_fine2_gather_b", P(dfeat), hf * wf * 128, P(db, I64), hf, wf, P(dcells, I64), K, wc, stride, W, P(out), S)
    assert torch.equal(out.cpu(), fr.windows(feat, b_ids, cells, hf, wf, wc, stride, W))
    out = nan(dev, K, W * W, 128)                                              # batch stride 0: every match reads the one image
    hip.call("ophip_fine2_gather_b", P(dfeat[2]), 0, P(db, I64), hf, wf, P(dcells, I64), K, wc, stride, W, P(out), S)
    assert torch.equal(out.cpu(), fr.windows(feat[2:3], zeros, cells, hf, wf, wc, stride, W))


def test_gather_without_matches_and_refused_arguments(dev):
    hc, wc, stride = fr.GATHER_MAPS["3x4 stride 4"]
    hf, wf = hc * stride, wc * stride
    dfeat, dcells = fr.gather_map("3x4 stride 4").to(dev), fr.gather_cells(hc, wc).to(dev)
    db = torch.zeros(19, dtype=I64, device=dev)
    out = nan(dev, 19, 81, 128)
    S = hip.stream_handle()
    hip.call("ophip_fine2_gather", P(dfeat[0]), hf, wf, P(dcells, I64), 0, wc, stride, 9, P(out), S)
    hip.call("ophip_fine2_gather_b", P(dfeat), hf * wf * 128, P(db, I64), hf, wf, P(dcells, I64), 0, wc, stride, 9, P(out), S)
    assert bool(torch.isnan(out).all())                                        # K = 0: no launch, nothing written
    for W, K in ((2, 19), (13, 19), (9, -1)):
        with pytest.raises(ValueError):
            hip.call("ophip_fine2_gather", P(dfeat[0]), hf, wf, P(dcells, I64), K, wc, stride, W, P(out), S)
        with pytest.raises(ValueError):
            hip.call("ophip_fine2_gather_b", P(dfeat), hf * wf * 128, P(db, I64), hf, wf, P(dcells, I64), K, wc, stride, W, P(out), S)
    with pytest.raises(ValueError):
        hip.call("ophip_fine2_gather", None, hf, wf, P(dcells, I64), 19, wc, stride, 9, P(out), S)
    with pytest.raises(ValueError):
        hip.call("ophip_fine2_gather", P(dfeat[0]), hf, wf, P(dcells, I64), 19, wc, stride, 9, None, S)
    with pytest.raises(ValueError):
        hip.call("ophip_fine2_gather_b", P(dfeat), hf * wf * 128, None, hf, wf, P(dcells, I64), 19, wc, stride, 9, P(out), S)
    assert bool(torch.isnan(out).all())


# ---- linear attention ------------------------------------------------------------------------------------------------------------------
def _attention(dev, q, k, v):
    K, L, S = q.shape[0], q.shape[1], k.shape[1]
    dq, dk, dv = q.to(dev), k.to(dev), v.to(dev)
    msg = nan(dev, K, L, 128)
    hip.call("ophip_fine2_attention", P(dq), P(dk), P(dv), K, L, S, P(msg), hip.stream_handle())
    return msg


@pytest.mark.parametrize("L,S", fr.ATTN_SHAPES)
def test_attention_at_every_length(dev, L, S):
    for K in fr.ATTN_COUNTS:
        q, k, v = fr.attention_inputs(K, L, S, shifted=False)
        within_bar("attention, randn", _attention(dev, q, k, v), fr.linear_attention(q, k, v), "attention", (K, L, S))
        q, k, v = fr.attention_inputs(K, L, S, shifted=True)
        within_abs("attention, randn * 4 - 2", _attention(dev, q, k, v), fr.linear_attention(q, k, v), fr.ATTN_SHIFTED_BOUND, (K, L, S))


def test_attention_with_more_matches_than_compute_units(dev):
    q, k, v = fr.attention_inputs(300, 81, 81, shifted=False)
    within_bar("attention, randn", _attention(dev, q, k, v), fr.linear_attention(q, k, v), "attention", "K = 300")
    t = torch.zeros(1, 129, 128, device=dev)
    msg = nan(dev, 1, 129, 128)
    with pytest.raises(ValueError):                                            # 2 * 129 * 128 floats do not fit the LDS
        hip.call("ophip_fine2_attention", P(t), P(t), P(t), 1, 129, 129, P(msg), hip.stream_handle())
    assert bool(torch.isnan(msg).all())


# ---- LayerNorm -----------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("T", fr.LN_ROWS)
def test_layernorm_rows(dev, T):
    for kind in fr.LN_KINDS:
        x, gamma, beta, res = fr.layernorm_inputs(T, kind)
        dx, dg, db, dr = x.to(dev), gamma.to(dev), beta.to(dev), res.to(dev)
        for r, drr in ((None, None), (res, dr)):
            y = nan(dev, T, 128)
            hip.call("ophip_rows_layernorm128", P(dx), P(dg), P(db), P(drr), T, P(y), hip.stream_handle())
            ref = fr.layernorm(x, gamma, beta, r)
            if kind == "mean100":
                within_abs("LayerNorm, mean 100", y, ref, fr.LN_MEAN100_BOUND, (T, r is not None))
            else:
                within_bar("LayerNorm, " + kind, y, ref, "layernorm", (T, r is not None))
            if kind == "equal":                                                # the row of equal values: beta (+ the residual)
                want = beta.double() if r is None else beta.double() + res[T // 2].double()
                within_bar("LayerNorm, the row of equal values", y[T // 2], want, "layernorm", (T, r is not None))


# ---- linear rows -----------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("ka,kb,nout,relu", fr.LINEAR_FORMS)
@pytest.mark.parametrize("T", fr.LINEAR_ROWS)
def test_rows_linear_on_either_side_of_a_workgroup(dev, T, ka, kb, nout, relu):
    xa, xb, w = fr.linear_inputs(T, ka, kb, nout)
    wp = packing.pack_linear_x3(w).to(dev)
    da, db = xa.to(dev), (xb.to(dev) if kb else None)
    y = nan(dev, T + 1, nout)                                                  # one row more: the kernel stops at T
    hip.call("ophip_rows_linear_x3", P(da), ka, P(db), kb, T, P(wp, None), nout, int(relu), P(y), hip.stream_handle())
    within_bar("linear rows", y[:T], fr.rows_linear(xa, xb, w, relu), "linear", (T, ka, kb, nout))
    assert bool(torch.isnan(y[T]).all())


# ---- fine matching ---------------------------------------------------------------------------------------------------------------------
PX = 4.0              # image height / fine-map height in these calls


def _check_expec(W, case, expec, ref):
    within_bar("match, expectation", expec[:, :2], ref[:, :2], "expec", (W, case))
    gx, gy = fr.fine_grid(W)
    if case.startswith("one-hot"):
        p = fr.onehot_token(W, case[len("one-hot "):])
        within_bar("match, one-hot expectation vs grid point", expec[:, :2], torch.stack([gx[p], gy[p]]).expand(len(expec), 2), "expec", (W, case))
        within_abs("match, one-hot std", expec[:, 2], ref[:, 2], fr.ONEHOT_STD_BOUND, (W, case))
    else:
        within_bar("match, std", expec[:, 2], ref[:, 2], "std", (W, case))
    if case in ("uniform", "equal negative"):
        within_bar("match, expectation", expec[:, :2], torch.zeros(len(expec), 2), "expec", (W, case))
        within_bar("match, std", expec[:, 2], (2 * (gx * gx).mean().sqrt()).expand(len(expec)), "std", (W, case))


@pytest.mark.parametrize("W", fr.WINDOWS)
def test_fine_match_at_every_window(dev, W):
    for case in fr.MATCH_CASES:
        f0, f1, mk1 = fr.match_inputs(W, case)
        mk1 = mk1.float()
        ref_e, ref_m = fr.fine_match(f0, f1, mk1, W, PX)
        d0, d1, dm = f0.to(dev), f1.to(dev), mk1.to(dev)
        expec, mk1f = nan(dev, fr.MATCH_K, 3), nan(dev, fr.MATCH_K, 2)
        hip.call("ophip_fine2_match", P(d0), P(d1), P(dm), fr.MATCH_K, W, (W // 2) * PX, P(expec), P(mk1f), hip.stream_handle())
        _check_expec(W, case, expec, ref_e)
        within_bar("match, mkpts1_f (plain form)", mk1f, ref_m, "mkpts1_f", (W, case))


@pytest.mark.parametrize("kdtype", [torch.float32, torch.float64])
@pytest.mark.parametrize("W", fr.WINDOWS)
def test_fine_match_scaled_at_every_window(dev, W, kdtype):
    B = 3
    s1 = torch.tensor([[1.25, 0.8], [0.7, 1.6], [1.1, 1.3]])
    b_ids = torch.tensor([0, 2, 2, 0, 2] * 5)[:fr.MATCH_K]                     # pair 1 has no match
    ds, db = s1.to(dev), b_ids.to(dev)
    assert s1.shape[0] == B and 1 not in b_ids.tolist()
    for case in ("random", "peak", "one-hot bottom right", "uniform"):
        f0, f1, mk1 = fr.match_inputs(W, case)
        mk1 = mk1.to(kdtype)
        d0, d1, dm = f0.to(dev), f1.to(dev), mk1.to(dev)
        for bstride in (2, 0):
            scales = s1 if bstride else s1[:1]
            ref_e, ref_m = fr.fine_match_scaled(f0, f1, mk1, W, PX, scales, b_ids)
            expec, mk1f = nan(dev, fr.MATCH_K, 3), nan(dev, fr.MATCH_K, 2, dtype=kdtype)
            hip.call("ophip_fine2_match_scaled", P(d0), P(d1), P(dm, None), int(kdtype == torch.float64), P(db, I64), P(ds), bstride, fr.MATCH_K, W,
                     PX, P(expec), P(mk1f, None), hip.stream_handle())
            _check_expec(W, case, expec, ref_e)
            # bit for bit: the rounding contract on the kernel's own expectation
            want = fr.scaled_keypoints(mk1, expec[:, :2].cpu(), W, PX, scales, b_ids)
            assert mk1f.dtype == kdtype and want.dtype == kdtype and torch.equal(mk1f.cpu(), want), (W, case, bstride)
            within_bar("match, mkpts1_f (scaled form) vs the reference's expectation", mk1f, ref_m, "mkpts1_f", (W, case, bstride))
        if kdtype == torch.float32:                                            # unit scales against the plain kernel
            ones = torch.ones(1, 2, device=dev)
            e1, m1, e2, m2 = nan(dev, fr.MATCH_K, 3), nan(dev, fr.MATCH_K, 2), nan(dev, fr.MATCH_K, 3), nan(dev, fr.MATCH_K, 2)
            hip.call("ophip_fine2_match_scaled", P(d0), P(d1), P(dm, None), 0, P(db, I64), P(ones), 0, fr.MATCH_K, W, PX, P(e1), P(m1, None),
                     hip.stream_handle())
            hip.call("ophip_fine2_match", P(d0), P(d1), P(dm), fr.MATCH_K, W, (W // 2) * PX, P(e2), P(m2), hip.stream_handle())
            assert torch.equal(e1, e2), (W, case)
            # the plain form may fuse mk + e * scale, the scaled form rounds the product first: the same bits where the product is exact
            # (W // 2 a power of two, as at window 9), within the bar at windows 7 and 11
            if W // 2 in (1, 2, 4):
                assert torch.equal(m1, m2), (W, case)
            within_bar("match, mkpts1_f (scaled form, unit scales) vs the plain form", m1, m2, "mkpts1_f", (W, case))


def test_fine_match_refuses_windows_1_and_13(dev):
    t, mk = torch.zeros(2, 169, 128, device=dev), torch.zeros(2, 2, device=dev)
    ids, ones = torch.zeros(2, dtype=I64, device=dev), torch.ones(1, 2, device=dev)
    expec, mk1f = nan(dev, 2, 3), nan(dev, 2, 2)
    for W in (1, 13):
        with pytest.raises(ValueError):
            hip.call("ophip_fine2_match", P(t), P(t), P(mk), 2, W, 4.0, P(expec), P(mk1f), hip.stream_handle())
        with pytest.raises(ValueError):
            hip.call("ophip_fine2_match_scaled", P(t), P(t), P(mk, None), 0, P(ids, I64), P(ones), 0, 2, W, 4.0, P(expec), P(mk1f, None),
                     hip.stream_handle())
    assert bool(torch.isnan(expec).all()) and bool(torch.isnan(mk1f).all())


# ---- the whole matcher at other windows ------------------------------------------------------------------------------------------------
def _matcher(lsd, dev, W):
    cfg = copy.deepcopy(loftr.default_cfg)
    cfg["fine_window_size"] = W
    m = loftr.LoFTR_for_OnePose_Plus(cfg).eval()
    m.load_state_dict(lsd, strict=True)
    return m.to(dev)


@pytest.mark.parametrize("W", [5, 7])
def test_matcher_on_planted_features_against_the_oracle(lsd, dev, W):
    """tests/test_gpu_loftr.py::test_matcher_on_planted_features_against_the_oracle with the window in the config: the same assertions and bars"""
    H, Wi = 96, 128
    pair = planted_pair((H, Wi))
    img = torch.zeros(1, 1, H, Wi)
    cfg = lo.loftr_default_cfg()
    cfg["fine_window_size"] = W
    with torch.no_grad():
        ref = lo.loftr_forward(lsd, cfg, img, img, feature_hook=oracle_hook(pair))
    data = tgl._run(_matcher(lsd, dev, W), dev, img, img, device_hook(pair, dev))
    K = len(ref["i_ids"])
    close = tgl.close
    assert K >= 40 and float((ref["mconf"] - 0.2).abs().min()) > 0.05
    assert data["i_ids"].tolist() == ref["i_ids"].tolist() and data["j_ids"].tolist() == ref["j_ids"].tolist()
    assert tuple(data["hw0_c"]) == (12, 16) and tuple(data["hw1_f"]) == (48, 64) and data["bs"] == 1
    close(data["_feat_c0"], ref["feat_c0"], 2e-3, 1e-3, "coarse rows of image 0")
    close(data["_feat_c1"], ref["feat_c1"], 2e-3, 1e-3, "coarse rows of image 1")
    close(data["mconf"], ref["mconf"], 2e-3, 1e-5)
    assert torch.equal(data["mkpts0_c"].cpu(), ref["mkpts0_c"]) and torch.equal(data["mkpts1_c"].cpu(), ref["mkpts1_c"])
    assert data["_fine_f0"].shape == (K, W * W, 128) and ref["fine_f0"].shape == (K, W * W, 128)
    close(data["_fine_f0"], ref["fine_f0"], 1e-3, 5e-4, "fine transformer, image 0 windows")
    close(data["_fine_f1"], ref["fine_f1"], 1e-3, 5e-4, "fine transformer, image 1 windows")
    close(data["expec_f"][:, :2], ref["expec_f"][:, :2], 1e-3, 2e-4)
    close(data["mkpts1_f"], ref["mkpts1_f"], 1e-4, 2e-3)
    assert torch.equal(data["mkpts0_f"], data["mkpts0_c"])
    d = (data["mkpts1_f"] - data["mkpts0_f"]).cpu().numpy()
    assert np.abs(np.median(d, axis=0) - np.array([16.0, 8.0])).max() < 0.5


def test_batched_views_equal_the_per_view_loop_at_window_5(lsd, dev):
    """tests/test_gpu_loftr_full.py::test_batched_views_equal_the_per_view_loop at window 5: two views against one query, every output of
    a pair bit-identical to that pair run alone"""
    m = _matcher(lsd, dev, 5)
    H, W = 96, 128
    x0, g0, xq, gq = planted_pair((H, W), seed=30)
    g = torch.Generator().manual_seed(31)
    views = [(x0, g0), (x0 + 0.05 * torch.randn(x0.shape, generator=g), g0 + 0.05 * torch.randn(g0.shape, generator=g))]
    cl = lambda t: t[0].permute(1, 2, 0).reshape(-1, 128).contiguous()

    def batched_hook(fc0, ff0, fc1, ff1):
        assert fc0.shape[0] == 2 and fc1.shape[0] == 1
        return (torch.cat([v[0] for v in views]).to(dev), torch.stack([cl(v[1]) for v in views]).to(dev), xq.to(dev), cl(gq)[None].to(dev))
    batch = tgl._run(m, dev, torch.zeros(2, 1, H, W), torch.zeros(1, 1, H, W), batched_hook)
    singles = [tgl._run(m, dev, torch.zeros(1, 1, H, W), torch.zeros(1, 1, H, W), device_hook((v[0], v[1], xq, gq), dev)) for v in views]
    assert len(singles[0]["i_ids"]) >= 40 and len(singles[1]["i_ids"]) >= 40
    assert batch["expec_f"].shape == (len(batch["b_ids"]), 3) and batch["_fine_f0"].shape[1] == 25
    for k, one in enumerate(singles):
        sel = batch["b_ids"] == k
        assert torch.equal(batch["b_ids"][sel], torch.full_like(one["b_ids"], k))
        for key in ("i_ids", "j_ids", "mconf", "mkpts0_c", "mkpts1_c", "mkpts0_f", "mkpts1_f", "expec_f", "_fine_f0", "_fine_f1"):
            assert torch.equal(batch[key][sel], one[key]), (k, key)
        assert torch.equal(batch["conf_matrix"][k], one["conf_matrix"][0]), k
