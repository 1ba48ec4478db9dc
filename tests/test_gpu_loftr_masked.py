"""Padding masks (mask0 / mask1) in the LoFTR matcher on the MI355X (run with ``-m gpu``): the two-mask encoder entry points against the
masked oracle layer (tests/loftr_masked_oracle.py), the matcher against the oracle with dual softmax and Sinkhorn, one pair and three
views against one shared query, through the real backbone on zero-padded images, padding invariance on the device (fine stage included)
and all-ones masks against no masks.  All calls go through the C ABI.

Bars as tests/test_gpu_loftr.py: index lists equal to the oracle's except matches whose decision sits within a narrow band of the
threshold or of a tie (set aside and counted), mconf 2e-3 relative, coarse keypoints exact, fine keypoints within 2e-3 px."""
import copy

import numpy as np
import pytest
import torch

from onepose_st_amd import hip, layercall, loftr, packing
from onepose_st_amd.synthetic import make_synthetic_loftr_state_dict
from tests import loftr_masked_oracle as lmo
from tests.loftr_helpers import planted_pair

pytestmark = pytest.mark.gpu

THR = 0.2


@pytest.fixture(scope="module")
def dev():
    if not torch.cuda.is_available():
        pytest.skip("needs the MI355X")
    hip.load()
    return torch.device("cuda:0")


@pytest.fixture(scope="module")
def lsd():
    sd = dict(make_synthetic_loftr_state_dict(0))
    sd["coarse_matching.bin_score"] = torch.tensor(1.0)
    return sd


@pytest.fixture(scope="module")
def matchers(lsd, dev):
    out = {}

    def get(match_type="dual_softmax"):
        if match_type not in out:
            cfg = copy.deepcopy(loftr.default_cfg)
            cfg["match_coarse"]["match_type"] = match_type
            m = loftr.LoFTR_for_OnePose_Plus(cfg).eval()
            sd = lsd if match_type == "sinkhorn" else {k: v for k, v in lsd.items() if k != "coarse_matching.bin_score"}
            m.load_state_dict(sd, strict=True)
            out[match_type] = m.to(dev)
        return out[match_type]
    return get


def close(a, b, rtol, atol, msg=""):
    np.testing.assert_allclose(a.detach().cpu().numpy(), b.detach().cpu().numpy(), rtol=rtol, atol=atol, err_msg=msg)


def rect_masks(B, hwp, extents):
    m = torch.zeros(B, *hwp, dtype=torch.bool)
    for b, (h, w) in enumerate(extents):
        m[b, :h, :w] = True
    return m


# ------------------------------------------------------------------------------------------------
# the encoder layer with a mask on each stream
# ------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("B,hw0,hw1", [(1, (9, 11), (8, 13)), (3, (12, 16), (10, 14))])
def test_encoder_layer_with_two_masks_against_the_oracle(lsd, dev, B, hw0, hw1):
    """self, image 0 against image 1 and image 1 against image 0, both streams masked, rectangular extents that differ per pair"""
    g = torch.Generator().manual_seed(B)
    L0, L1 = hw0[0] * hw0[1], hw1[0] * hw1[1]
    x0, x1 = torch.randn(B, L0, 256, generator=g), torch.randn(B, L1, 256, generator=g)
    ext0 = [(hw0[0] - b, hw0[1] - 2 * b - 1) for b in range(B)]
    ext1 = [(hw1[0] - 2 * b - 1, hw1[1] - b) for b in range(B)]
    m0, m1 = rect_masks(B, hw0, ext0).flatten(1), rect_masks(B, hw1, ext1).flatten(1)
    p = "loftr_coarse.layers.3."
    w = packing.pack_coarse_layer_x3w8(lsd, p).to(dev)
    d0, d1, dm0, dm1 = x0.to(dev), x1.to(dev), m0.to(dev), m1.to(dev)
    kw = dict(mode="bf16x3", wpack=w, workspace=layercall.workspace("bf16x3", B, L0, L1, dev))
    tol = dict(rtol=3e-4, atol=1e-4)
    # self
    y0, y1 = torch.full_like(d0, float("nan")), torch.full_like(d1, float("nan"))
    layercall.layer(d0, d1, y0, y1, is_cross=0, masks=(dm0, dm1), **kw)
    r0, r1 = lmo.masked_layer(lsd, p, x0, x0, m0, m0), lmo.masked_layer(lsd, p, x1, x1, m1, m1)
    assert (r0 - lmo.masked_layer(lsd, p, x0, x0)).abs().max() > 1e-2          # the masks matter
    close(y0, r0, msg="self, stream 0", **tol)
    close(y1, r1, msg="self, stream 1", **tol)
    # cross: image 0 against image 1, then image 1 against image 0 (one stream per launch)
    n0 = torch.full_like(d0, float("nan"))
    layercall.layer(d0, d1, n0, None, is_cross=1, streams=1, masks=(dm0, dm1), **kw)
    close(n0, lmo.masked_layer(lsd, p, x0, x1, m0, m1), msg="cross, image 0 against image 1", **tol)
    n1 = torch.full_like(d1, float("nan"))
    layercall.layer(d0, d1, None, n1, is_cross=1, streams=2, masks=(dm0, dm1), **kw)
    close(n1, lmo.masked_layer(lsd, p, x1, x0, m1, m0), msg="cross, image 1 against image 0", **tol)
    # one mask NULL: that stream unmasked
    layercall.layer(d0, d1, n0, None, is_cross=1, streams=1, masks=(None, dm1), **kw)
    close(n0, lmo.masked_layer(lsd, p, x0, x1, None, m1), msg="cross, mask0 NULL", **tol)
    assert torch.equal(dm0.cpu(), m0) and torch.equal(dm1.cpu(), m1)                # the masks are read only


# ------------------------------------------------------------------------------------------------
# the matcher
# ------------------------------------------------------------------------------------------------
def _cl(g):
    """[V, 128, hf, wf] -> the hook's channels-last [V, hf * wf, 128]"""
    return g.permute(0, 2, 3, 1).reshape(g.shape[0], -1, 128).contiguous()


def _hook(x0, g0, x1, g1, dev):
    if x0.shape[0] == 1:
        return lambda *a: (x0.to(dev), _cl(g0)[0].to(dev), x1.to(dev), _cl(g1)[0].to(dev))
    return lambda *a: (x0.to(dev), _cl(g0).to(dev), x1.to(dev), _cl(g1).to(dev))


def _run(m, dev, feats, hw0p, hw1p, masks, V=1, V1=1):
    m.feature_hook = _hook(*feats, dev)
    data = {"image0": torch.zeros(V, 1, 8 * hw0p[0], 8 * hw0p[1], device=dev), "image1": torch.zeros(V1, 1, 8 * hw1p[0], 8 * hw1p[1], device=dev)}
    if masks is not None:
        data["mask0"], data["mask1"] = masks[0].to(dev), masks[1].to(dev)
    try:
        m(data, _debug=True)
    finally:
        m.feature_hook = None
    return data


def _borderline(conf, b, i, j):
    """a decision within the band: conf near the threshold, or a near-tie in its row or column"""
    c = float(conf[b, i, j])
    if abs(c - THR) < 5e-3:
        return True
    row, col = conf[b, i].clone(), conf[b, :, j].clone()
    row[j], col[i] = -1, -1
    return float(row.max()) > c * (1 - 5e-3) or float(col.max()) > c * (1 - 5e-3)


def _check(data, ref, tag):
    have = list(zip(data["b_ids"].tolist(), data["i_ids"].tolist(), data["j_ids"].tolist()))
    want = list(zip(ref["b_ids"].tolist(), ref["i_ids"].tolist(), ref["j_ids"].tolist()))
    diff = set(have) ^ set(want)
    assert all(_borderline(ref["conf_matrix"], *d) for d in diff), f"{tag}: matches differ outside the band: {sorted(diff)[:6]}"
    print(f"{tag}: K = {len(want)}, set aside {len(diff)}")
    close(data["conf_matrix"], ref["conf_matrix"], 0, 5e-3, f"{tag}: conf_matrix")
    common = [k for k, t in enumerate(have) if t in set(want)]
    rk = {t: k for k, t in enumerate(want)}
    ri = [rk[have[k]] for k in common]
    ci, ri = torch.tensor(common, dtype=torch.long), torch.tensor(ri, dtype=torch.long)
    close(data["mconf"].cpu()[ci], ref["mconf"][ri], 2e-3, 1e-5, f"{tag}: mconf")
    assert torch.equal(data["mkpts0_c"].cpu()[ci], ref["mkpts0_c"][ri]) and torch.equal(data["mkpts1_c"].cpu()[ci], ref["mkpts1_c"][ri])
    close(data["mkpts1_f"].cpu()[ci], ref["mkpts1_f"][ri], 1e-4, 2e-3, f"{tag}: mkpts1_f")
    assert torch.equal(data["mkpts0_f"], data["mkpts0_c"])
    return len(want), len(diff)


def _padded_pair(seed=3, amp=1.0):
    """planted_pair on a 12 x 16 grid, padded: image 0 to 15 x 18, image 1 to 13 x 20 (random junk in the padded coarse rows, zeros in
    the padded fine maps)"""
    hw = (12, 16)
    x0, g0, x1, g1 = planted_pair((96, 128), seed=seed)
    x0, x1 = x0 * amp, x1 * amp
    hw0p, hw1p = (15, 18), (13, 20)
    gen = torch.Generator().manual_seed(seed + 100)

    def pad(x, g, hwp):
        xp = torch.randn(1, hwp[0], hwp[1], 256, generator=gen) * 2
        xp[:, :hw[0], :hw[1]] = x.view(1, hw[0], hw[1], 256)
        gp = torch.zeros(1, 128, 4 * hwp[0], 4 * hwp[1])
        gp[:, :, :4 * hw[0], :4 * hw[1]] = g
        return xp.view(1, -1, 256), gp
    p0, q0 = pad(x0, g0, hw0p)
    p1, q1 = pad(x1, g1, hw1p)
    masks = (rect_masks(1, hw0p, [hw]), rect_masks(1, hw1p, [hw]))
    return (x0, g0, x1, g1), (p0, q0, p1, q1), hw, hw0p, hw1p, masks


def _shared_query(seed=5, amp=1.0):
    """three views of different valid sizes (padded to 13 x 17) against one 12 x 16 query: view k carries query cell (y + dy, x + dx)
    at cell (y, x) of its valid grid; batch-1 mask1"""
    hw1, hw0p = (12, 16), (13, 17)
    views, shifts = ((12, 16), (10, 13), (11, 15)), ((2, 1), (1, 1), (0, 2))
    g = torch.Generator().manual_seed(seed)
    q = torch.randn(1, hw1[0] * hw1[1], 256, generator=g)
    gq = torch.randn(1, 128, 4 * hw1[0], 4 * hw1[1], generator=g)
    V = len(views)
    x0 = torch.randn(V, hw0p[0] * hw0p[1], 256, generator=g) * 2
    g0 = torch.zeros(V, 128, 4 * hw0p[0], 4 * hw0p[1])
    for k, ((h, w), (dx, dy)) in enumerate(zip(views, shifts)):
        for y in range(h):
            for x in range(w):
                if y + dy < hw1[0] and x + dx < hw1[1]:
                    x0[k, y * hw0p[1] + x] = q[0, (y + dy) * hw1[1] + x + dx] + 0.1 * torch.randn(256, generator=g)
                else:
                    x0[k, y * hw0p[1] + x] = torch.randn(256, generator=g)
        g0[k, :, :4 * h, :4 * w] = torch.roll(gq[0], shifts=(-4 * dy, -4 * dx), dims=(1, 2))[:, :4 * h, :4 * w]
    masks = (rect_masks(V, hw0p, views), torch.ones(1, *hw1, dtype=torch.bool))
    return (x0 * amp, g0, q * amp, gq), hw0p, hw1, masks


@pytest.mark.parametrize("match_type", ["dual_softmax", "sinkhorn"])
def test_matcher_one_pair_against_the_oracle(matchers, lsd, dev, match_type):
    m = matchers(match_type)
    amp = 1.0 if match_type == "dual_softmax" else 6.0
    _, padded, hw, hw0p, hw1p, masks = _padded_pair(amp=amp)
    with torch.no_grad():
        ref = lmo.forward_from_features(lsd, m.config, *padded, (8 * hw0p[0], 8 * hw0p[1]), *masks)
    data = _run(m, dev, padded, hw0p, hw1p, masks)
    K, _ = _check(data, ref, f"{match_type}, one pair")
    if match_type == "dual_softmax":
        assert K >= 40
    close(data["_feat_c0"][0, masks[0].flatten()], ref["feat_c0"][0, masks[0].flatten()], 2e-3, 1e-3, "coarse rows of image 0 (valid cells)")
    close(data["_feat_c1"][0, masks[1].flatten()], ref["feat_c1"][0, masks[1].flatten()], 2e-3, 1e-3, "coarse rows of image 1 (valid cells)")
    if match_type == "dual_softmax":
        conf = data["conf_matrix"][0].cpu()
        v0, v1 = masks[0].flatten(), masks[1].flatten()
        assert (conf[v0][:, ~v1] == 0).all() and (conf[~v0][:, v1] == 0).all()        # one padded cell: exactly 0


@pytest.mark.parametrize("match_type", ["dual_softmax", "sinkhorn"])
def test_matcher_three_views_against_a_shared_query(matchers, lsd, dev, match_type):
    m = matchers(match_type)
    amp = 1.0 if match_type == "dual_softmax" else 6.0
    feats, hw0p, hw1, masks = _shared_query(amp=amp)
    with torch.no_grad():
        ref = lmo.forward_from_features(lsd, m.config, *feats, (8 * hw0p[0], 8 * hw0p[1]), *masks)
    data = _run(m, dev, feats, hw0p, hw1, masks, V=3, V1=1)
    K, _ = _check(data, ref, f"{match_type}, three views")
    if match_type == "dual_softmax":
        assert K >= 40 and set(data["b_ids"].tolist()) == {0, 1, 2}


def test_matcher_through_the_real_backbone_on_zero_padded_images(matchers, lsd, dev):
    m = matchers()
    g = torch.Generator().manual_seed(8)
    img0 = torch.zeros(1, 1, 80, 112)
    img0[:, :, :64, :96] = torch.rand(1, 1, 64, 96, generator=g)
    img1 = torch.rand(1, 1, 64, 96, generator=g)
    m0 = rect_masks(1, (10, 14), [(8, 12)])
    m1 = torch.ones(1, 8, 12, dtype=torch.bool)
    with torch.no_grad():
        ref = lmo.loftr_forward(lsd, m.config, img0, img1, m0, m1)
    data = {"image0": img0.to(dev), "image1": img1.to(dev), "mask0": m0.to(dev), "mask1": m1.to(dev)}
    m(data)
    v0 = m0.flatten()
    close(data["conf_matrix"][0][v0.to(dev)].max(dim=1)[0], ref["conf_matrix"][0][v0].max(dim=1)[0], 2e-2, 1e-6, "row maxima of the valid rows")
    assert (data["conf_matrix"][0][~v0.to(dev)] == 0).all()                     # padded rows against an unpadded image: exactly 0
    _check(data, ref, "real backbone")


def test_padding_invariance_on_the_device(matchers, dev):
    """the same planted pair unpadded without masks and padded with masks: identical indices, keypoints within the LoFTR bars"""
    m = matchers()
    plain, padded, hw, hw0p, hw1p, masks = _padded_pair()
    a = _run(m, dev, plain, hw, hw, None)
    b = _run(m, dev, padded, hw0p, hw1p, masks)
    K = len(a["i_ids"])
    assert K >= 40
    remap = lambda ids, wp: (ids // hw[1]) * wp + ids % hw[1]
    assert b["i_ids"].tolist() == remap(a["i_ids"], hw0p[1]).tolist() and b["j_ids"].tolist() == remap(a["j_ids"], hw1p[1]).tolist()
    assert torch.equal(a["mkpts0_c"], b["mkpts0_c"]) and torch.equal(a["mkpts1_c"], b["mkpts1_c"])
    close(b["mconf"], a["mconf"], 2e-3, 1e-5, "mconf")
    close(b["expec_f"][:, :2], a["expec_f"][:, :2], 1e-3, 2e-4, "expec_f")
    close(b["mkpts1_f"], a["mkpts1_f"], 1e-4, 2e-3, "mkpts1_f")
    v0, v1 = masks[0].flatten().to(dev), masks[1].flatten().to(dev)
    close(b["conf_matrix"][0][v0][:, v1], a["conf_matrix"][0], 0, 5e-3, "conf_matrix at the valid cells")


@pytest.mark.parametrize("match_type", ["dual_softmax", "sinkhorn"])
def test_all_ones_masks_give_the_unmasked_matches(matchers, dev, match_type):
    m = matchers(match_type)
    plain, _, hw, _, _, _ = _padded_pair(amp=1.0 if match_type == "dual_softmax" else 6.0)
    ones = (torch.ones(1, *hw, dtype=torch.bool), torch.ones(1, *hw, dtype=torch.bool))
    a = _run(m, dev, plain, hw, hw, None)
    b = _run(m, dev, plain, hw, hw, ones)
    assert a["i_ids"].tolist() == b["i_ids"].tolist() and a["j_ids"].tolist() == b["j_ids"].tolist()
    close(b["mconf"], a["mconf"], 2e-3, 1e-5, "mconf")
    close(b["mkpts1_f"], a["mkpts1_f"], 1e-4, 2e-3, "mkpts1_f")
    if match_type == "dual_softmax":
        assert len(a["i_ids"]) >= 40
