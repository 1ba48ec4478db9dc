"""Full (softmax) attention in the LoFTR matcher behind the detector, on the MI355X (run with ``-m gpu``): the one-stream coarse layer
(``ophip_encoder_layer_full_x3_stream``) and the window attention kernel (``ophip_fine2_full_attention``) against the CPU oracle, the
whole matcher on planted features against tests/loftr_full_oracle.py for each attention combination, batched views against the per-view
loop, the detector end to end, and the empty path.  All calls go through the C ABI.

Bars: the layer at rtol 3e-4 / atol 1e-4 (tests/test_gpu_full_attention.py::test_encoder_layer_full); the window kernel at 1e-5 / 1e-5
against float64 (test_fine_full_attention_kernel); the matcher at the bars of
tests/test_gpu_loftr.py::test_matcher_on_planted_features_against_the_oracle."""
import copy

import numpy as np
import pytest
import torch

from onepose_st_amd import hip, layercall, loftr, packing
from onepose_st_amd.synthetic import make_synthetic_loftr_state_dict
from tests import loftr_full_oracle as lfo
from tests import test_gpu_loftr as tgl
from tests.loftr_helpers import device_hook, oracle_hook, planted_pair

pytestmark = pytest.mark.gpu

COMBOS = [("full", "linear"), ("linear", "full"), ("full", "full")]


@pytest.fixture(scope="module")
def dev():
    assert torch.cuda.is_available(), "these tests need the MI355X"
    hip.load()
    return torch.device("cuda:0")


@pytest.fixture(scope="module")
def lsd():
    return make_synthetic_loftr_state_dict(0)


def _cfg(coarse, fine):
    c = copy.deepcopy(loftr.default_cfg)
    c["coarse"]["attention"] = coarse
    c["fine"]["attention"] = fine
    return c


@pytest.fixture(scope="module")
def matchers(lsd, dev):
    out = {}

    def get(coarse, fine, enable_fine_matching=True):
        key = (coarse, fine, enable_fine_matching)
        if key not in out:
            m = loftr.LoFTR_for_OnePose_Plus(_cfg(coarse, fine), enable_fine_matching=enable_fine_matching).eval()
            m.load_state_dict(lsd, strict=True)
            out[key] = m.to(dev)
        return out[key]
    return get


close = tgl.close


# ------------------------------------------------------------------------------------------------
# one-stream coarse layer
# ------------------------------------------------------------------------------------------------
def _layer(dev, w, x, src, nb, y=None, **override):
    """``nb``: the batch extent of the output and the workspace; ``override``: header arguments put in place of the planned ones (a batch
    extent, a stride the plan would not choose)"""
    L, S = x.shape[1], src.shape[1]
    y = torch.full((nb, L, 256), float("nan"), device=dev) if y is None else y
    entry, named = layercall.plan_layer_full_stream(x, src, y, wpack=w, workspace=layercall.workspace("full", nb, L, S, dev, stream_form=True))
    hip.launch(entry, dict(named, **override))
    return y


@pytest.mark.parametrize("mode", ["pair", "shared_src", "shared_x", "self"])
@pytest.mark.parametrize("B,L,S", [(1, 70, 19), (3, 130, 45), (3, 33, 200)])
def test_one_stream_layer(lsd, dev, mode, B, L, S):
    """ragged L != S (not multiples of the 32-key / 128-query tiles; S = 19 below one key tile); ``shared_*``: that input is one image
    passed with batch stride 0; ``self``: src is x"""
    if mode == "self":
        S = L
    g = torch.Generator().manual_seed(100 * B + L + S)
    nx, ns = (1 if mode == "shared_x" else B), (1 if mode == "shared_src" else B)
    x = torch.randn(nx, L, 256, generator=g)
    src = x if mode == "self" else torch.randn(ns, S, 256, generator=g)
    p = "loftr_coarse.layers.3."
    with torch.no_grad():
        ref = lfo.encoder_layer(lsd, p, x.expand(B, -1, -1).contiguous(), src.expand(B, -1, -1).contiguous())
    w = packing.pack_coarse_layer(lsd, p).to(dev)
    dx = x.to(dev)
    ds = dx if mode == "self" else src.to(dev)
    y = _layer(dev, w, dx, ds, B)
    err = (y.cpu() - ref).abs().max().item()
    print(f"one-stream {mode} B={B} L={L} S={S}: max abs err {err:.3e}")
    close(y, ref, 3e-4, 1e-4, f"{mode} layer")
    # a batch element's rows are those of a B = 1 call on its own inputs
    for b in range(1, B):
        xb, sb = dx[min(b, nx - 1)][None].contiguous(), ds[min(b, ns - 1)][None].contiguous()
        yb = _layer(dev, w, xb, xb if mode == "self" else sb, 1, x_bstride=L * 256, src_bstride=S * 256)
        assert torch.equal(yb[0], y[b]), (mode, b)
    with pytest.raises(ValueError):                    # in place
        _layer(dev, w, dx, ds, nx, y=dx, B=nx)
    with pytest.raises(ValueError):                    # a stride that overlaps rows
        _layer(dev, w, dx, ds, B, x_bstride=128)


# ------------------------------------------------------------------------------------------------
# window attention kernel
# ------------------------------------------------------------------------------------------------
def _attention_f64(q, k, v):
    K, L, S = q.shape[0], q.shape[1], k.shape[1]
    out = []
    for c in range(0, K, 100):
        qq, kk, vv = (t[c:c + 100].double().view(-1, t.shape[1], 8, 16) for t in (q, k, v))
        out.append(lfo.full_attention(qq, kk, vv).reshape(-1, L, 128))
    return torch.cat(out)


@pytest.mark.parametrize("K", [1, 7, 1000])
@pytest.mark.parametrize("L,S", [(1, 1), (9, 9), (25, 25), (81, 81), (121, 121), (81, 121), (121, 25)])
def test_window_full_attention_kernel(dev, K, L, S):
    """W in {1, 3, 5, 9, 11} with L = S = W^2, and window-against-window of two sizes, against float64"""
    g = torch.Generator().manual_seed(7 * K + 3 * L + S)
    q, k, v = torch.randn(K, L, 128, generator=g), torch.randn(K, S, 128, generator=g), torch.randn(K, S, 128, generator=g)
    want = _attention_f64(q, k, v)
    dq, dk, dv = q.to(dev), k.to(dev), v.to(dev)
    out = torch.full((K, L, 128), float("nan"), device=dev)
    hip.call("ophip_fine2_full_attention", hip.ptr(dq), hip.ptr(dk), hip.ptr(dv), K, L, S, hip.ptr(out), hip.stream_handle())
    o = out.cpu()
    assert not torch.isnan(o).any()
    err = (o.double() - want).abs().max().item()
    print(f"window attention K={K} L={L} S={S}: max abs err {err:.3e}")
    np.testing.assert_allclose(o.numpy(), want.float().numpy(), rtol=1e-5, atol=1e-5)
    if S == 1:
        assert torch.equal(o, v.expand(-1, L, -1))
    with pytest.raises(ValueError):
        hip.call("ophip_fine2_full_attention", hip.ptr(dq), hip.ptr(dk), hip.ptr(dv), K, 122, S, hip.ptr(out), hip.stream_handle())


# ------------------------------------------------------------------------------------------------
# whole matcher
# ------------------------------------------------------------------------------------------------
def planted_pair_sizes(hw0, hw1, shift_cells=(2, 1), seed=5, noise=0.1):
    """``loftr_helpers.planted_pair`` for images of different sizes: image-1 cell (y + dy, x + dx) carries image-0 cell (y, x), and
    image 1's fine map carries image 0's moved by (4 dy, 4 dx) fine pixels; the rest is unrelated noise"""
    (H0, W0), (H1, W1) = hw0, hw1
    hc0, wc0, hc1, wc1 = H0 // 8, W0 // 8, H1 // 8, W1 // 8
    dx, dy = shift_cells
    g = torch.Generator().manual_seed(seed)
    x0 = torch.randn(1, hc0 * wc0, 256, generator=g)
    x1 = torch.randn(1, hc1 * wc1, 256, generator=g)
    for y in range(hc0):
        for x in range(wc0):
            y1, x1_ = y + dy, x + dx
            if 0 <= y1 < hc1 and 0 <= x1_ < wc1:
                x1[0, y1 * wc1 + x1_] = x0[0, y * wc0 + x] + noise * torch.randn(256, generator=g)
    g0 = torch.randn(1, 128, H0 // 2, W0 // 2, generator=g)
    g1 = torch.randn(1, 128, H1 // 2, W1 // 2, generator=g)
    oy, ox = 4 * dy, 4 * dx
    h, w = min(H0 // 2, H1 // 2 - oy), min(W0 // 2, W1 // 2 - ox)
    g1[:, :, oy:oy + h, ox:ox + w] = g0[:, :, :h, :w]
    g1 = g1 + 0.5 * noise * torch.randn(g1.shape, generator=g)
    return x0, g0, x1, g1


@pytest.mark.parametrize("sizes", [((96, 128), (96, 128)), ((96, 128), (80, 112))])
@pytest.mark.parametrize("coarse,fine", COMBOS)
def test_matcher_on_planted_features_against_the_oracle(matchers, lsd, dev, coarse, fine, sizes):
    hw0, hw1 = sizes
    pair = planted_pair(hw0) if hw0 == hw1 else planted_pair_sizes(hw0, hw1)
    img0, img1 = torch.zeros(1, 1, *hw0), torch.zeros(1, 1, *hw1)
    with torch.no_grad():
        ref = lfo.loftr_forward(lsd, _cfg(coarse, fine), img0, img1, feature_hook=oracle_hook(pair))
    data = tgl._run(matchers(coarse, fine), dev, img0, img1, device_hook(pair, dev))
    K = len(ref["i_ids"])
    assert K >= 40 and float((ref["mconf"] - 0.2).abs().min()) > 0.05            # every reference confidence far from the threshold
    assert data["i_ids"].tolist() == ref["i_ids"].tolist() and data["j_ids"].tolist() == ref["j_ids"].tolist()
    assert tuple(data["hw0_c"]) == (hw0[0] // 8, hw0[1] // 8) and tuple(data["hw1_c"]) == (hw1[0] // 8, hw1[1] // 8)
    close(data["_feat_c0"], ref["feat_c0"], 2e-3, 1e-3, "coarse rows of image 0 after 8 layers")
    close(data["_feat_c1"], ref["feat_c1"], 2e-3, 1e-3, "coarse rows of image 1")
    close(data["mconf"], ref["mconf"], 2e-3, 1e-5)
    assert torch.equal(data["mkpts0_c"].cpu(), ref["mkpts0_c"]) and torch.equal(data["mkpts1_c"].cpu(), ref["mkpts1_c"])
    close(data["_fine_f0"], ref["fine_f0"], 1e-3, 5e-4, "fine transformer, image 0 windows")
    close(data["_fine_f1"], ref["fine_f1"], 1e-3, 5e-4, "fine transformer, image 1 windows")
    close(data["expec_f"][:, :2], ref["expec_f"][:, :2], 1e-3, 2e-4)
    close(data["mkpts1_f"], ref["mkpts1_f"], 1e-4, 2e-3)
    assert torch.equal(data["mkpts0_f"], data["mkpts0_c"])
    d = (data["mkpts1_f"] - data["mkpts0_f"]).cpu().numpy()
    assert np.abs(np.median(d, axis=0) - np.array([16.0, 8.0])).max() < 0.5


def test_batched_views_equal_the_per_view_loop(matchers, dev):
    """three views against ONE query (batch stride 0 in the coarse layers, the query's layer-0 self layer run once): every output of a
    pair is bit-identical to that pair run alone"""
    m = matchers("full", "full")
    H, W = 96, 128
    x0, g0, xq, gq = planted_pair((H, W), seed=30)
    g = torch.Generator().manual_seed(31)
    views = [(x0, g0),
             (x0 + 0.05 * torch.randn(x0.shape, generator=g), g0 + 0.05 * torch.randn(g0.shape, generator=g)),
             (torch.randn(x0.shape, generator=g), torch.randn(g0.shape, generator=g))]
    cl = lambda t: t[0].permute(1, 2, 0).reshape(-1, 128).contiguous()

    def batched_hook(fc0, ff0, fc1, ff1):
        assert fc0.shape[0] == 3 and fc1.shape[0] == 1
        return (torch.cat([v[0] for v in views]).to(dev), torch.stack([cl(v[1]) for v in views]).to(dev), xq.to(dev), cl(gq)[None].to(dev))
    batch = tgl._run(m, dev, torch.zeros(3, 1, H, W), torch.zeros(1, 1, H, W), batched_hook)
    singles = [tgl._run(m, dev, torch.zeros(1, 1, H, W), torch.zeros(1, 1, H, W), device_hook((v[0], v[1], xq, gq), dev)) for v in views]
    assert len(singles[0]["i_ids"]) >= 40 and len(singles[1]["i_ids"]) >= 40
    for k, one in enumerate(singles):
        sel = batch["b_ids"] == k
        assert torch.equal(batch["b_ids"][sel], torch.full_like(one["b_ids"], k))
        for key in ("i_ids", "j_ids", "mconf", "mkpts0_c", "mkpts1_c", "mkpts0_f", "mkpts1_f", "expec_f"):
            assert torch.equal(batch[key][sel], one[key]), (k, key)
        assert torch.equal(batch["conf_matrix"][k], one["conf_matrix"][0]), k
        assert torch.equal(batch["_feat_c0"][k], one["_feat_c0"][0]) and torch.equal(batch["_feat_c1"][k], one["_feat_c1"][0]), k


def test_detector_end_to_end_with_a_full_attention_matcher(matchers, dev):
    """tests/test_gpu_loftr.py::test_detector_end_to_end_on_the_device on a matcher with both encoders full: the planted view wins, the
    box, crop and K_crop follow"""
    tgl.test_detector_end_to_end_on_the_device(matchers("full", "full"), dev)


@pytest.mark.parametrize("coarse,fine", COMBOS)
def test_empty_path_and_coarse_only(matchers, lsd, dev, coarse, fine):
    """K = 0 returns the reference's empty shapes; ``enable_fine_matching=False`` returns the coarse keypoints as the fine ones"""
    H, W = 96, 128
    L = (H // 8) * (W // 8)
    zero = (torch.zeros(1, L, 256), torch.zeros(1, 128, H // 2, W // 2), torch.zeros(1, L, 256), torch.zeros(1, 128, H // 2, W // 2))
    img = torch.zeros(1, 1, H, W)
    with torch.no_grad():
        ref = lfo.loftr_forward(lsd, _cfg(coarse, fine), img, img, feature_hook=oracle_hook(zero))
    assert len(ref["i_ids"]) == 0
    data = tgl._run(matchers(coarse, fine), dev, img, img, device_hook(zero, dev))
    assert len(data["i_ids"]) == 0
    assert data["expec_f"].shape == (0, 3) and data["mkpts0_f"].shape == (0, 2) and data["mkpts1_f"].shape == (0, 2)
    pair = planted_pair((H, W))
    with torch.no_grad():
        ref = lfo.loftr_forward(lsd, _cfg(coarse, fine), img, img, feature_hook=oracle_hook(pair))
    data = tgl._run(matchers(coarse, fine, enable_fine_matching=False), dev, img, img, device_hook(pair, dev))
    assert data["i_ids"].tolist() == ref["i_ids"].tolist() and data["j_ids"].tolist() == ref["j_ids"].tolist()
    assert torch.equal(data["mkpts0_f"], data["mkpts0_c"]) and torch.equal(data["mkpts1_f"], data["mkpts1_c"])
