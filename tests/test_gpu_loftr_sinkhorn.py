"""Optimal-transport (sinkhorn) coarse matching in the LoFTR matcher, on the MI355X (run with ``-m gpu``): the stage
(``ophip_coarse_match_2d_sinkhorn``) against the float64 oracle of tests/loftr_sinkhorn_oracle.py, the SuperGlue marginals on the device,
the whole matcher with each coarse attention form, batched views against the per-view loop, determinism, the detector end to end and the
empty path.  All calls go through the C ABI.

Bars: conf_matrix within 1e-4 absolute of float64 (iters = 0 leaves it unnormalised, (m + n) exp(S): relative 1e-3 there); the index lists
bit-exact.  Rows and columns whose decision sits within a relative band of 1e-4 of the threshold, of a tie or of the dustbin are excused
from both and counted; the count is printed (a handful of the ~10^4 rows and columns the runs
decide, all on random unplanted rows or columns)."""
import copy

import numpy as np
import pytest
import torch

from onepose_st_amd import detector, hip, loftr, matchcall
from onepose_st_amd.synthetic import make_synthetic_loftr_state_dict
from tests import loftr_sinkhorn_oracle as lso
from tests import test_gpu_loftr as tgl
from tests import test_gpu_loftr_full as tglf
from tests.loftr_helpers import device_hook, oracle_hook, planted_pair

pytestmark = pytest.mark.gpu

BAND = 1e-4
AMP = 6.0                 # planted features are scaled: unscaled rows give S ~ 1 and confidences far below the threshold


@pytest.fixture(scope="module")
def dev():
    assert torch.cuda.is_available(), "these tests need the MI355X"
    hip.load()
    return torch.device("cuda:0")


@pytest.fixture(scope="module")
def lsd():
    sd = dict(make_synthetic_loftr_state_dict(0))
    sd["coarse_matching.bin_score"] = torch.tensor(1.0)
    return sd


def _cfg(coarse="linear", fine="linear"):
    c = copy.deepcopy(loftr.default_cfg)
    c["coarse"]["attention"] = coarse
    c["fine"]["attention"] = fine
    c["match_coarse"]["match_type"] = "sinkhorn"
    return c


@pytest.fixture(scope="module")
def matchers(lsd, dev):
    out = {}

    def get(coarse="linear", enable_fine_matching=True):
        key = (coarse, enable_fine_matching)
        if key not in out:
            m = loftr.LoFTR_for_OnePose_Plus(_cfg(coarse), enable_fine_matching=enable_fine_matching).eval()
            m.load_state_dict(lsd, strict=True)
            out[key] = m.to(dev)
        return out[key]
    return get


# ------------------------------------------------------------------------------------------------
# the stage
# ------------------------------------------------------------------------------------------------
def _stage(dev, f0, f1, w0, w1, bin_score, iters, prefilter, thr=0.2, border=2, conf=None):
    B, L0, L1 = f0.shape[0], f0.shape[1], f1.shape[1]
    ii = torch.arange(L0)
    pts0 = torch.stack([(ii % w0).float() * 8, (ii // w0).float() * 8, torch.zeros(L0)], 1)[None].contiguous().to(dev)
    d0, d1 = f0.contiguous().to(dev), f1.contiguous().to(dev)
    conf = torch.full((B, L0, L1), float("nan"), device=dev) if conf is None else conf
    ws = torch.full((hip.load().ophip_coarse_sinkhorn_workspace_floats(B, L0, L1),), float("nan"), device=dev)
    cap = B * L0
    ids = [torch.empty(cap, dtype=torch.int64, device=dev) for _ in range(4)]
    mconf, mk0, mk1 = torch.empty(cap, device=dev), torch.empty(cap, 3, device=dev), torch.empty(cap, 2, device=dev)
    gt = torch.empty(cap, dtype=torch.bool, device=dev)
    cnt = torch.zeros(4, dtype=torch.int32, device=dev)
    matchcall.coarse_match_2d(d0, d1, pts0, w0c=w0, w1c=w1, sinkhorn=(bin_score, iters, prefilter), thr=thr, border_rm=border, scale=8.0,
                              lists=matchcall.MatchLists(*ids[:3], mconf, mk0, mk1, ids[3], gt, cnt), conf=conf, workspace=ws)
    K = int(cnt[0])
    return {"conf": conf, "ws": ws, "K": K, "b_ids": ids[0][:K].cpu(), "i_ids": ids[1][:K].cpu(), "j_ids": ids[2][:K].cpu(),
            "mconf": mconf[:K].cpu(), "m_bids": ids[3][:K].cpu(), "mkpts0": mk0[:K].cpu(), "mkpts1": mk1[:K].cpu()}


def _features(B, L0, L1, seed, amp=4.0):
    """random rows, half of the smaller grid planted (image-1 cell p(k) carries image-0 cell k) and scaled so that matches clear thr"""
    g = torch.Generator().manual_seed(seed)
    f0, f1 = torch.randn(B, L0, 256, generator=g), torch.randn(B, L1, 256, generator=g)
    for b in range(B):
        n = min(L0, L1) // 2
        src, dst = torch.randperm(L0, generator=g)[:n], torch.randperm(L1, generator=g)[:n]
        f1[b, dst] = f0[b, src] + 0.1 * torch.randn(n, 256, generator=g)
    return f0 * amp, f1 * amp


def _near(assign, conf, thr):
    """rows / columns of the float64 reference whose decision sits within BAND (relative) of the threshold, a tie or the dustbin"""
    L, S = conf.shape[1:]
    la = assign.clamp_min(1e-300).log()
    rel = lambda a, b: (a - b).abs() < BAND                       # in log space: a relative band
    top2r = la[:, :L].topk(2, dim=2)[0] if S >= 1 else None
    top2c = la[:, :, :S].topk(2, dim=1)[0]
    near_r = rel(la[:, :L, S], la[:, :L, :S].max(2)[0]) | rel(top2r[..., 0], top2r[..., 1])
    near_c = rel(la[:, L, :S], la[:, :L, :S].max(1)[0]) | rel(top2c[:, 0], top2c[:, 1])
    lc = conf.clamp_min(1e-300).log()
    near_r |= rel(lc.max(2)[0], torch.tensor(thr, dtype=conf.dtype).log())
    near_c |= rel(lc.max(1)[0], torch.tensor(thr, dtype=conf.dtype).log())
    return near_r, near_c


def _check_stage(out, f0, f1, hw0, hw1, bin_score, iters, prefilter, tag, thr=0.2):
    conf_ref, assign, _, _ = lso.sinkhorn_conf(f0, f1, bin_score, iters, prefilter)
    ref = lso.get_coarse_match(conf_ref.float(), hw0, hw1, (hw0[0] * 8, hw0[1] * 8), thr, 2)
    near_r, near_c = _near(assign, conf_ref, thr)
    n_near = int(near_r.sum()) + int(near_c.sum())
    got = out["conf"].double().cpu()
    keep = ~(near_r[:, :, None] | near_c[:, None, :])
    err = (got - conf_ref).abs()
    tol = 1e-4 + (1e-3 if iters == 0 else 0.0) * conf_ref.abs()
    bad = (err > tol) & keep
    assert not bad.any(), f"{tag}: conf_matrix off at {int(bad.sum())} entries, max error {float(err[keep].max()):.3g}"
    have = list(zip(out["b_ids"].tolist(), out["i_ids"].tolist(), out["j_ids"].tolist()))
    want = list(zip(ref["b_ids"].tolist(), ref["i_ids"].tolist(), ref["j_ids"].tolist()))
    if have != want:
        diff = set(have) ^ set(want)
        assert all(near_r[b, i] or near_c[b, j] for b, i, j in diff), f"{tag}: match lists differ outside the bands: {sorted(diff)[:6]}"
    print(f"{tag}: K = {len(want)}, rows / columns within the bands: {n_near}")
    if have == want:
        np.testing.assert_allclose(out["mconf"].numpy(), ref["mconf"].numpy(), rtol=1e-4, atol=1e-4)
    return len(want), n_near


GRIDS = [((8, 10), (9, 13)),          # L0 = 80 < L1 = 117, L1 not a multiple of 4
         ((12, 16), (8, 12)),         # L0 = 192 > L1 = 96
         ((9, 13), (9, 13)),          # 117 x 117
         ((20, 30), (18, 28))]        # 600 x 504: five row chunks, two column strips, several similarity tiles


@pytest.mark.parametrize("iters", [0, 1, 3, 10])
@pytest.mark.parametrize("B", [1, 3])
@pytest.mark.parametrize("grids", GRIDS)
def test_stage_against_the_oracle(dev, grids, B, iters):
    (h0, w0), (h1, w1) = grids
    f0, f1 = _features(B, h0 * w0, h1 * w1, seed=h0 * w1 + B + iters)
    total_near = 0
    for prefilter in (0, 1):
        for bin_score in (-1.0, 1.0, 4.0):
            out = _stage(dev, f0, f1, w0, w1, bin_score, iters, prefilter)
            K, n_near = _check_stage(out, f0, f1, (h0, w0), (h1, w1), bin_score, iters, prefilter, f"{grids} B={B} it={iters} pf={prefilter} a={bin_score}")
            total_near += n_near
            assert K >= 3 * B, "the planted pairs must match: the comparison would be vacuous"
            assert out["K"] == K
            assert torch.equal(out["m_bids"], out["b_ids"])
            assert torch.equal(out["mkpts0"][:, :2], torch.stack([out["i_ids"] % w0, out["i_ids"] // w0], 1).float() * 8)
    print(f"{grids} B={B} iters={iters}: rows / columns within the bands over all six runs: {total_near}")


def test_stage_rejects_bad_arguments(dev):
    f0, f1 = _features(1, 80, 117, seed=1)
    with pytest.raises(ValueError):
        _stage(dev, f0, f1, 10, 13, 1.0, -1, 1)
    with pytest.raises(ValueError):
        _stage(dev, f0, f1, 10, 13, 1.0, 3, 2)
    with pytest.raises(ValueError):
        _stage(dev, f0, f1, 10, 13, float("inf"), 3, 1)
    with pytest.raises(ValueError):
        _stage(dev, f0, f1, 10, 12, 1.0, 3, 1)                        # 117 is no multiple of 12


def test_marginals_on_the_device(dev):
    """50 iterations, no prefilter: with the dual potentials the call leaves in its workspace (documented layout), every real row of
    the assignment sums to 1 and the dustbin row to n, every real column to 1 and the dustbin column to m -- independent of the oracle"""
    (h0, w0), (h1, w1) = (12, 16), (9, 13)
    B, m, n, alpha = 2, h0 * w0, h1 * w1, 1.0
    f0, f1 = _features(B, m, n, seed=50, amp=1.0)               # (sharper scores converge more slowly than 50 iterations)
    out = _stage(dev, f0, f1, w0, w1, alpha, 50, 0)
    base = hip.load().ophip_coarse_workspace_floats(B, m, n)
    base += (16 - (out["ws"].data_ptr() // 4 + base) % 16) % 16
    up, vp = (m + 4) // 4 * 4, (n + 4) // 4 * 4
    ws = out["ws"].cpu().double()
    u = ws[base:base + B * up].view(B, up)[:, :m + 1]
    v = ws[base + B * up:base + B * (up + vp)].view(B, vp)[:, :n + 1]
    S = torch.einsum("blc,bsc->bls", f0.double() / 16, f1.double() / 16)
    Z = torch.full((B, m + 1, n + 1), alpha, dtype=torch.float64)
    Z[:, :m, :n] = S
    norm = -np.log(m + n)
    P = (Z + u[:, :, None] + v[:, None, :]).exp()                  # the assignment / (m + n): marginals mu, nu
    rows, cols = P.sum(2) / np.exp(norm), P.sum(1) / np.exp(norm)
    np.testing.assert_allclose(rows[:, :m].numpy(), 1.0, atol=2e-3)
    np.testing.assert_allclose(rows[:, m].numpy(), float(n), rtol=2e-3)
    np.testing.assert_allclose(cols[:, :n].numpy(), 1.0, atol=2e-3)
    np.testing.assert_allclose(cols[:, n].numpy(), float(m), rtol=2e-3)
    np.testing.assert_allclose(out["conf"].double().cpu().numpy(), (P[:, :m, :n] / np.exp(norm)).numpy(), atol=1e-4)


# ------------------------------------------------------------------------------------------------
# the matcher
# ------------------------------------------------------------------------------------------------
def _scaled(pair, amp=AMP):
    return (pair[0] * amp, pair[1], pair[2] * amp, pair[3])


@pytest.mark.parametrize("sizes", [((96, 128), (96, 128)), ((96, 128), (80, 112))])
@pytest.mark.parametrize("coarse", ["linear", "full"])
def test_matcher_on_planted_features_against_the_oracle(matchers, lsd, dev, coarse, sizes):
    hw0, hw1 = sizes
    pair = _scaled(planted_pair(hw0) if hw0 == hw1 else tglf.planted_pair_sizes(hw0, hw1))
    img0, img1 = torch.zeros(1, 1, *hw0), torch.zeros(1, 1, *hw1)
    with torch.no_grad():
        ref = lso.loftr_forward(lsd, _cfg(coarse), img0, img1, feature_hook=oracle_hook(pair))
    data = tgl._run(matchers(coarse), dev, img0, img1, device_hook(pair, dev))
    K = len(ref["i_ids"])
    assert K >= 20 and float((ref["mconf"] - 0.2).abs().min()) > 0.05
    assert data["i_ids"].tolist() == ref["i_ids"].tolist() and data["j_ids"].tolist() == ref["j_ids"].tolist()
    tgl.close(data["_feat_c0"], ref["feat_c0"], 2e-3, 1e-3, "coarse rows of image 0")
    tgl.close(data["mconf"], ref["mconf"], 2e-3, 1e-4)
    tgl.close(data["conf_matrix"], ref["conf_matrix"], 0, 2e-3, "conf_matrix")
    assert torch.equal(data["mkpts0_c"].cpu(), ref["mkpts0_c"]) and torch.equal(data["mkpts1_c"].cpu(), ref["mkpts1_c"])
    tgl.close(data["expec_f"][:, :2], ref["expec_f"][:, :2], 1e-3, 2e-4)
    tgl.close(data["mkpts1_f"], ref["mkpts1_f"], 1e-4, 2e-3)
    # coarse only: the coarse keypoints are the fine ones
    data = tgl._run(matchers(coarse, enable_fine_matching=False), dev, img0, img1, device_hook(pair, dev))
    assert data["i_ids"].tolist() == ref["i_ids"].tolist() and data["j_ids"].tolist() == ref["j_ids"].tolist()
    assert torch.equal(data["mkpts0_f"], data["mkpts0_c"]) and torch.equal(data["mkpts1_f"], data["mkpts1_c"])


def test_batched_views_equal_the_per_view_loop_and_runs_repeat(matchers, dev):
    m = matchers("linear")
    H, W = 96, 128
    x0, g0, xq, gq = _scaled(planted_pair((H, W), seed=30))
    g = torch.Generator().manual_seed(31)
    views = [(x0, g0), (x0 + 0.3 * torch.randn(x0.shape, generator=g), g0), (AMP * torch.randn(x0.shape, generator=g), torch.randn(g0.shape, generator=g))]
    cl = lambda t: t[0].permute(1, 2, 0).reshape(-1, 128).contiguous()

    def batched_hook(fc0, ff0, fc1, ff1):
        return (torch.cat([v[0] for v in views]).to(dev), torch.stack([cl(v[1]) for v in views]).to(dev), xq.to(dev), cl(gq)[None].to(dev))
    batch = tgl._run(m, dev, torch.zeros(3, 1, H, W), torch.zeros(1, 1, H, W), batched_hook)
    again = tgl._run(m, dev, torch.zeros(3, 1, H, W), torch.zeros(1, 1, H, W), batched_hook)
    for key in ("b_ids", "i_ids", "j_ids", "mconf", "conf_matrix", "mkpts1_f"):
        assert torch.equal(batch[key], again[key]), key
    singles = [tgl._run(m, dev, torch.zeros(1, 1, H, W), torch.zeros(1, 1, H, W), device_hook((v[0], v[1], xq, gq), dev)) for v in views]
    assert len(singles[0]["i_ids"]) >= 20 and len(singles[1]["i_ids"]) >= 20
    for k, one in enumerate(singles):
        sel = batch["b_ids"] == k
        for key in ("i_ids", "j_ids", "mconf", "mkpts0_c", "mkpts1_c", "mkpts0_f", "mkpts1_f", "expec_f"):
            assert torch.equal(batch[key][sel], one[key]), (k, key)
        assert torch.equal(batch["conf_matrix"][k], one["conf_matrix"][0]), k


def test_detector_end_to_end_and_the_empty_path(matchers, lsd, dev):
    """three reference views, the query carries view 1's content moved by (2, 1) cells: that view wins with a sinkhorn matcher;
    zero features give no match and the reference's empty shapes"""
    matcher = matchers("linear")
    H, W = 96, 128
    views = [np.full((H, W), 10 * (k + 1), dtype=np.uint8) for k in range(3)]
    det = detector.LocalFeatureObjectDetector(matcher, views)
    pairs = {0: _scaled(planted_pair((H, W), (0, 0), seed=20, noise=30.0)),             # views 0, 2: the copy drowns in noise
             1: _scaled(planted_pair((H, W), (2, 1), seed=21)),
             2: _scaled(planted_pair((H, W), (0, 0), seed=22, noise=30.0))}
    calls = {"n": 0}

    def hook(fc0, ff0, fc1, ff1):
        if fc0.shape[0] == 3:
            outs = [device_hook(pairs[k], dev)(None, None, None, None) for k in range(3)]
            return (torch.cat([o[0] for o in outs]), torch.stack([o[1] for o in outs]), torch.cat([o[2] for o in outs]), torch.stack([o[3] for o in outs]))
        k = calls["n"] % 3
        calls["n"] += 1
        return device_hook(pairs[k], dev)(fc0, ff0, fc1, ff1)
    matcher.feature_hook = hook
    try:
        res = det.match_worker(torch.zeros(1, 1, H, W, device=dev))
        loop = det.match_worker(torch.zeros(1, 1, H, W, device=dev), batched=False)
        for k in range(3):
            assert np.array_equal(res[k]["bbox"], loop[k]["bbox"]) and np.array_equal(np.asarray(res[k]["inliers"]), np.asarray(loop[k]["inliers"])), k
        assert res[1]["inliers"].sum() >= 20 and res[1]["inliers"].sum() > max(res[0]["inliers"].sum(), res[2]["inliers"].sum())
        assert np.abs(res[1]["bbox"] - np.array([16, 8, W + 16, H + 8])).max() <= 1
    finally:
        matcher.feature_hook = None
    L = (H // 8) * (W // 8)
    zero = (torch.zeros(1, L, 256), torch.zeros(1, 128, H // 2, W // 2), torch.zeros(1, L, 256), torch.zeros(1, 128, H // 2, W // 2))
    img = torch.zeros(1, 1, H, W)
    with torch.no_grad():
        ref = lso.loftr_forward(lsd, _cfg(), img, img, feature_hook=oracle_hook(zero))
    assert len(ref["i_ids"]) == 0
    data = tgl._run(matcher, dev, img, img, device_hook(zero, dev))
    assert len(data["i_ids"]) == 0
    assert data["expec_f"].shape == (0, 3) and data["mkpts0_f"].shape == (0, 2) and data["mkpts1_f"].shape == (0, 2)
