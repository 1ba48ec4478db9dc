"""The SfM calls of the LoFTR matcher on the MI355X (run with ``-m gpu``): the coarse-id and sampler kernels and the per-pair-scale fine
match against the oracle of tests/loftr_sfm_oracle.py, the fine-only call on planted fine maps and through the real backbone with
feature extraction, the SfM coarse call with image scales, and determinism.  All calls go through the C ABI.

Bars: ids, clipped keypoints and nearest samples bit-exact (nearest samples of keypoints whose unnormalised coordinate lies within 1e-4
of a half-integer are excused and counted); bilinear samples within 1e-5 of the map's max |value| against ``F.grid_sample`` on the same
device map with the oracle's float32 grid; the fine stage at the bars of test_gpu_loftr's planted-feature test."""
import copy

import pytest
import torch
import torch.nn.functional as F

from oracle import loftr_oracle as lo
from onepose_st_amd import hip, loftr
from onepose_st_amd.synthetic import make_synthetic_loftr_state_dict
from tests import loftr_sfm_oracle as lsf
from tests import loftr_sinkhorn_oracle as lso
from tests.loftr_helpers import device_hook, oracle_hook, planted_pair
from tests.test_gpu_loftr import close

pytestmark = pytest.mark.gpu

REF_KEYS = {"image0", "image1", "bs", "hw0_i", "hw1_i", "hw0_c", "hw1_c", "hw0_f", "hw1_f", "m_bids", "b_ids", "i_ids", "j_ids", "mconf",
            "mkpts0_c", "mkpts1_c", "mkpts0_f", "mkpts1_f"}


@pytest.fixture(scope="module")
def dev():
    assert torch.cuda.is_available(), "these tests need the MI355X"
    hip.load()
    return torch.device("cuda:0")


@pytest.fixture(scope="module")
def lsd():
    return make_synthetic_loftr_state_dict(0)


@pytest.fixture(scope="module")
def matchers(lsd, dev):
    out = {}

    def get(enable_fine_matching=True, sinkhorn=False, thr=None):
        key = (enable_fine_matching, sinkhorn, thr)
        if key not in out:
            cfg = copy.deepcopy(loftr.default_cfg)
            sd = dict(lsd)
            if sinkhorn:
                cfg["match_coarse"]["match_type"] = "sinkhorn"
                sd["coarse_matching.bin_score"] = torch.tensor(1.0)
            if thr is not None:
                cfg["match_coarse"]["thr"] = thr
            m = loftr.LoFTR_for_OnePose_Plus(cfg, enable_fine_matching=enable_fine_matching).eval()
            m.load_state_dict(sd, strict=True)
            out[key] = m.to(dev)
        return out[key]
    return get


def _keypoints(g, K, hw_i, dtype, margin=20):
    """x over the whole width and a little beyond (clip, wrap), y from a little above the image to ``margin`` px above its bottom
    (an id past the last row would be the IndexError case)"""
    H, W = hw_i
    x = torch.rand(K, generator=g, dtype=torch.float64) * (W + 20) - 10
    y = torch.rand(K, generator=g, dtype=torch.float64) * (H - margin + 10) - 10
    return torch.stack([x, y], 1).to(dtype)


# ------------------------------------------------------------------------------------------------
# the kernels
# ------------------------------------------------------------------------------------------------
def _ids_call(dev, k0, k1, hw0_i, hw1_i, s0=None, s1=None):
    hw0_c, hw1_c = (hw0_i[0] // 8, hw0_i[1] // 8), (hw1_i[0] // 8, hw1_i[1] // 8)
    d0, d1 = k0.clone().to(dev), k1.clone().to(dev)
    K = len(k0)
    ii, jj = torch.full((K,), -7, dtype=torch.int64, device=dev), torch.full((K,), -7, dtype=torch.int64, device=dev)
    bad = torch.full((1,), 99, dtype=torch.int32, device=dev)
    ds0, ds1 = (s0.to(dev) if s0 is not None else None), (s1.to(dev) if s1 is not None else None)
    hip.call("ophip_loftr_coarse_ids", hip.ptr(d0, None), int(d0.dtype == torch.float64), hip.ptr(d1, None), int(d1.dtype == torch.float64), K,
             *hw0_i, *hw1_i, *hw0_c, *hw1_c, 8.0, hip.ptr(ds0), hip.ptr(ds1), hip.ptr(ii, torch.int64), hip.ptr(jj, torch.int64),
             hip.ptr(bad, torch.int32), hip.stream_handle())
    ref = {"mkpts0_c": k0.clone(), "mkpts1_c": k1.clone(), "hw0_i": hw0_i, "hw1_i": hw1_i, "hw0_c": hw0_c, "hw1_c": hw1_c}
    if s0 is not None:
        ref.update({"scale0": s0, "scale1": s1})
    _, ri, rj = lsf.coarse_ids(ref)
    return d0.cpu(), d1.cpu(), ii.cpu(), jj.cpu(), int(bad.item()), ref, ri, rj


@pytest.mark.parametrize("t0,t1", [(torch.float32, torch.float32), (torch.float64, torch.float64), (torch.float32, torch.float64)])
@pytest.mark.parametrize("scaled", [False, True])
def test_coarse_ids_kernel_bit_exact(dev, t0, t1, scaled):
    g = torch.Generator().manual_seed(11)
    hw0_i, hw1_i = (480, 640), (512, 384)
    k0, k1 = _keypoints(g, 3000, hw0_i, t0), _keypoints(g, 3000, hw1_i, t1)
    s0 = torch.tensor([[1.25, 0.8]]) if scaled else None
    s1 = torch.tensor([[1.1, 0.9]]) if scaled else None
    if not scaled:                         # ties: x = 8k + 4 lands on a cell's half -> round half to even; and the wrap into the next row
        k0[:64, 0] = (8 * torch.arange(64) + 4).to(t0)
        k1[:48, 1] = (8 * torch.arange(48) + 4).to(t1)
        k0[64:70, 0] = hw0_i[1] - 2
        k1[64:70, 0] = hw1_i[1] + 5
    d0, d1, ii, jj, bad, ref, ri, rj = _ids_call(dev, k0, k1, hw0_i, hw1_i, s0, s1)
    assert d0.dtype == t0 and d1.dtype == t1
    assert torch.equal(d0, ref["mkpts0_c"]) and torch.equal(d1, ref["mkpts1_c"]), "in-place clip"
    assert (d0[:, 0] >= 0).all() and (d0[:, 0] <= hw0_i[1] - 2).all() and not torch.equal(d0, k0)
    assert torch.equal(ii, ri) and torch.equal(jj, rj)
    assert bad == int(((ri < 0) | (ri >= 60 * 80)).sum() + ((rj < 0) | (rj >= 64 * 48)).sum())
    if not scaled:
        assert (ri[:64] % 80 == 2 * ((torch.arange(64) + 1) // 2)).all()            # half to even: 0.5 -> 0, 1.5 -> 2, 2.5 -> 2
        assert (ri[64:70] % 80 == 0).all()                                        # 638 / 8 = 79.75 -> 80: the next row's first cell
        assert (ri[64:70] // 80 == (d0[64:70, 1] / 8).round().long() + 1).all()


def test_coarse_ids_kernel_counts_ids_past_the_grid(dev):
    hw_i = (64, 96)
    k0 = torch.tensor([[10.0, 10.0], [94.0, 62.0], [50.0, 61.0], [94.0, 20.0]])       # 62 / 8 = 7.75 -> row 8 of 8; 61 / 8 -> 7.625
    k1 = torch.tensor([[10.0, 10.0], [3.0, 70.0], [5.0, 5.0], [5.0, 5.0]], dtype=torch.float64)
    d0, d1, ii, jj, bad, ref, ri, rj = _ids_call(dev, k0, k1, hw_i, hw_i)
    assert torch.equal(ii, ri) and torch.equal(jj, rj)
    L = 8 * 12
    assert bad == int((ri >= L).sum() + (rj >= L).sum()) == 3 and ri[1] >= L and ri[2] >= L and rj[1] >= L
    assert torch.equal(d1, ref["mkpts1_c"]) and float(d1[1, 1]) == 62.0


def _sampler_case(g, K, hw_i, C, hw_map, kdtype, nearest, scale):
    fmap = torch.randn(hw_map[0] * hw_map[1], C, generator=g) * 3
    ext = (float(scale[0, 0]) * hw_i[0], float(scale[0, 1]) * hw_i[1])
    x = torch.rand(K, generator=g, dtype=torch.float64) * (ext[1] * 1.2) - 0.1 * ext[1]            # about 20 % of the points outside
    y = torch.rand(K, generator=g, dtype=torch.float64) * (ext[0] * 1.2) - 0.1 * ext[0]
    return fmap, torch.stack([x, y], 1).to(kdtype), nearest


def _sample_jobs(dev, cases, hw_i, scale):
    sd = scale.to(dev)
    keep, jobs = [], []
    for fmap, kp, nearest, hw_map in cases:
        dm, dk = fmap.to(dev), kp.to(dev)
        out = torch.full((len(kp), fmap.shape[1]), float("nan"), device=dev)
        keep.append((dm, dk, out))
        jobs.append(hip.SampleJob(dm.data_ptr(), dk.data_ptr(), sd.data_ptr(), out.data_ptr(), hw_map[0], hw_map[1], fmap.shape[1], len(kp),
                                  hw_i[0], hw_i[1], int(kp.dtype == torch.float64), int(nearest)))
    hip.call("ophip_sample_features", (hip.SampleJob * len(jobs))(*jobs), len(jobs), hip.stream_handle())
    return keep


def _check_samples(dm, dk, out, hw_map, hw, nearest, label):
    """``dm [h * w, C]`` device map, ``dk`` keypoints, ``out`` the kernel's rows; -> near-half count (nearest)"""
    if len(dk) == 0:
        return 0
    grid = lsf.sample_grid(dk.cpu(), hw)
    ref = F.grid_sample(lsf.channels_first(dm, hw_map), grid.to(dm.device), mode="nearest" if nearest else "bilinear",
                        align_corners=True)[0, :, :, 0].t()
    assert torch.isfinite(out).all(), label
    if nearest:
        ux, uy = lsf.unnormalised(grid[0, :, 0, 0], hw_map[1]), lsf.unnormalised(grid[0, :, 0, 1], hw_map[0])
        excused = lsf.near_half(ux) | lsf.near_half(uy)
        ok = ~excused.to(out.device)
        assert torch.equal(out[ok], ref[ok]), label
        # and against the CPU oracle (the reference's own arithmetic) on the same rows
        cpu = lsf.sample_feature_from_featuremap(lsf.channels_first(dm.cpu(), hw_map), dk.cpu(), hw, "nearest")
        assert torch.equal(out[ok].cpu(), cpu[ok.cpu()]), label
        return int(excused.sum())
    bar = 1e-5 * float(dm.abs().max())
    assert float((out - ref).abs().max()) <= bar, (label, float((out - ref).abs().max()), bar)
    return 0


@pytest.mark.parametrize("K", [0, 1, 517, 20000])
def test_sampler_kernel_both_widths_in_one_launch(dev, K):
    g = torch.Generator().manual_seed(K + 1)
    hw_i = (480, 640)
    scale = torch.tensor([[1.25, 0.75]])
    hw = lsf.imghw(scale, hw_i)
    specs = [(256, (60, 80), torch.float32, True), (256, (60, 80), torch.float64, True),
             (128, (240, 320), torch.float32, False), (128, (240, 320), torch.float64, False)]
    cases = []
    for C, hw_map, kd, nearest in specs:
        fmap, kp, _ = _sampler_case(g, K, hw_i, C, hw_map, kd, nearest, scale)
        if K > 4:                         # exact half-integers and points just outside
            kp[0] = torch.tensor([0.0, 0.0], dtype=kd)
            kp[1] = torch.tensor([float(hw[1]) - 1, float(hw[0]) - 1], dtype=kd)
            kp[2] = torch.tensor([-5.0 * float(hw[1]), 3.0], dtype=kd)
            kp[3] = torch.tensor([3.0, 2.0 * float(hw[0])], dtype=kd)
        cases.append((fmap, kp, nearest, hw_map))
    keep = _sample_jobs(dev, cases, hw_i, scale)
    torch.cuda.synchronize()
    excused = 0
    for (dm, dk, out), (_, _, nearest, hw_map) in zip(keep, cases):
        assert out.shape == (K, dm.shape[1]) and out.dtype == torch.float32
        excused += _check_samples(dm, dk, out, hw_map, hw, nearest, f"C {dm.shape[1]} {dk.dtype}")
        if K > 4:
            assert (out[2:4] == 0).all(), "zero padding outside the map"
            assert torch.equal(out[0], dm[0])                                 # the corner pixel itself
    print(f"sampler K={K}: {excused} nearest samples within 1e-4 of a half-integer excused")


def test_sampler_zero_padding_and_edges(dev):
    """points beyond each side give zero rows; a bilinear point half a pixel outside weighs the missing corners with 0"""
    hw_i, scale = (64, 96), torch.tensor([[1.0, 1.0]])
    hw_map = (16, 24)
    fmap = torch.arange(16 * 24 * 128, dtype=torch.float32).reshape(16 * 24, 128) / 1000 + 1
    kp = torch.tensor([[-20.0, 30.0], [200.0, 30.0], [40.0, -20.0], [40.0, 100.0], [-1.0, 30.0], [95.5, 63.5], [0.0, 0.0]])
    cases = [(fmap, kp, False, hw_map), (fmap, kp.double(), True, hw_map)]
    keep = _sample_jobs(dev, cases, hw_i, scale)
    torch.cuda.synchronize()
    hw = lsf.imghw(scale, hw_i)
    for (dm, dk, out), (_, _, nearest, _) in zip(keep, cases):
        _check_samples(dm, dk, out, hw_map, hw, nearest, "edges")
        assert (out[:4] == 0).all()
        assert torch.equal(out[6], dm[0])


@pytest.mark.parametrize("kdtype", [torch.float32, torch.float64])
@pytest.mark.parametrize("shared", [False, True])
def test_fine_match_with_per_pair_scales(dev, kdtype, shared):
    g = torch.Generator().manual_seed(17)
    K, W, B = 300, 9, 3
    hw_i, hw_f = (96, 128), (48, 64)
    f0, f1 = torch.randn(K, 81, 128, generator=g), torch.randn(K, 81, 128, generator=g)
    f1[:, 50] += 2.0 * f0[:, 40]
    mk1 = (torch.rand(K, 2, generator=g, dtype=torch.float64) * 100).to(kdtype)
    b_ids = torch.randint(0, B, (K,), generator=g)
    s1 = torch.tensor([[1.25, 0.8]]) if shared else torch.tensor([[1.25, 0.8], [0.7, 1.6], [1.1, 1.3]])
    ref = lo.fine_matching(f0, f1, mk1.float(), mk1.float(), hw_i, hw_f)
    d0, d1, dm, db, ds = f0.to(dev), f1.to(dev), mk1.to(dev), b_ids.to(dev), s1.to(dev)
    expec, mk1f = torch.empty(K, 3, device=dev), torch.empty(K, 2, dtype=kdtype, device=dev)
    hip.call("ophip_fine2_match_scaled", hip.ptr(d0), hip.ptr(d1), hip.ptr(dm, None), int(kdtype == torch.float64), hip.ptr(db, torch.int64),
             hip.ptr(ds), 0 if shared else 2, K, W, 2.0, hip.ptr(expec), hip.ptr(mk1f, None), hip.stream_handle())
    close(expec[:, :2], ref["expec_f"][:, :2], 1e-4, 1e-5, "expectation")
    # bit-exact against the reference's formula on the kernel's own expectation
    want = lsf.fine_keypoints1(mk1, expec[:, :2].cpu(), W, hw_i, hw_f, s1, b_ids)
    assert want.dtype == kdtype and torch.equal(mk1f.cpu(), want)
    want_o = lsf.fine_keypoints1(mk1, ref["expec_f"][:, :2], W, hw_i, hw_f, s1, b_ids)
    close(mk1f, want_o, 1e-5, 1e-4, "mkpts1_f against the oracle's expectation")
    # unit scales reproduce the plain kernel exactly
    if kdtype == torch.float32:
        ones = torch.ones(1, 2, device=dev)
        hip.call("ophip_fine2_match_scaled", hip.ptr(d0), hip.ptr(d1), hip.ptr(dm, None), 0, hip.ptr(db, torch.int64), hip.ptr(ones), 0, K, W,
                 2.0, hip.ptr(expec), hip.ptr(mk1f, None), hip.stream_handle())
        e2, m2 = torch.empty(K, 3, device=dev), torch.empty(K, 2, device=dev)
        hip.call("ophip_fine2_match", hip.ptr(d0), hip.ptr(d1), hip.ptr(dm), K, W, 8.0, hip.ptr(e2), hip.ptr(m2), hip.stream_handle())
        assert torch.equal(expec, e2) and torch.equal(mk1f, m2)


# ------------------------------------------------------------------------------------------------
# the fine-only call
# ------------------------------------------------------------------------------------------------
def _fine_maps(g, hw_i):
    return torch.randn(1, 128, hw_i[0] // 2, hw_i[1] // 2, generator=g)


def _cl(gmap, dev):
    return gmap[0].permute(1, 2, 0).reshape(-1, 128).contiguous().to(dev)


def _fine_only_inputs(g, K, hw0_i, hw1_i, t0, t1, unit):
    k0, k1 = _keypoints(g, K, hw0_i, t0), _keypoints(g, K, hw1_i, t1)
    s0 = torch.tensor([[1.0, 1.0]]) if unit else torch.tensor([[1.25, 0.8]])
    s1 = torch.tensor([[1.0, 1.0]]) if unit else torch.tensor([[1.1, 0.9]])         # h factors >= 1: no id past the last row
    return k0, k1, s0, s1


@pytest.mark.parametrize("hw0_i,hw1_i,K,t1,unit", [
    ((512, 512), (512, 512), 0, torch.float32, True),
    ((512, 512), (512, 512), 1, torch.float32, False),
    ((512, 512), (512, 512), 517, torch.float64, True),
    ((480, 640), (512, 384), 517, torch.float32, False),
    ((480, 640), (512, 384), 1, torch.float64, True),
    ((480, 640), (512, 384), 5000, torch.float64, False),
])
def test_fine_only_call_on_planted_fine_maps(matchers, lsd, dev, hw0_i, hw1_i, K, t1, unit):
    g = torch.Generator().manual_seed(K + hw0_i[1])
    k0, k1, s0, s1 = _fine_only_inputs(g, K, hw0_i, hw1_i, torch.float32, t1, unit)
    g0, g1 = _fine_maps(g, hw0_i), _fine_maps(g, hw1_i)
    m = matchers()
    img0, img1 = torch.zeros(1, 1, *hw0_i, device=dev), torch.zeros(1, 1, *hw1_i, device=dev)
    dk0, dk1 = k0.to(dev), k1.to(dev)
    data = {"image0": img0, "image1": img1, "scale0": s0.to(dev), "scale1": s1.to(dev), "mkpts0_c": dk0, "mkpts1_c": dk1}
    m.feature_hook = lambda fc0, ff0, fc1, ff1: (fc0, _cl(g0, dev), fc1, _cl(g1, dev))
    try:
        m(data)
    finally:
        m.feature_hook = None
    with torch.no_grad():
        ref = lsf.fine_only_forward(lsd, lo.loftr_default_cfg(), {"hw0_i": hw0_i, "hw1_i": hw1_i, "mkpts0_c": k0.clone(), "mkpts1_c": k1.clone(),
                                                                 "scale0": s0, "scale1": s1}, g0, g1)
    assert set(data) == REF_KEYS | {"scale0", "scale1", "expec_f"}, sorted(set(data) ^ (REF_KEYS | {"scale0", "scale1", "expec_f"}))
    assert data["mconf"].dtype == torch.int64 and torch.equal(data["mconf"].cpu(), torch.ones(K, dtype=torch.int64))
    assert data["m_bids"] is data["b_ids"] and (data["b_ids"] == 0).all() and data["b_ids"].dtype == torch.int64
    assert data["mkpts0_c"] is dk0 and data["mkpts1_c"] is dk1 and data["mkpts0_f"] is dk0
    assert torch.equal(dk0.cpu(), ref["mkpts0_c"]) and torch.equal(dk1.cpu(), ref["mkpts1_c"]), "the caller's tensors come back clipped"
    assert torch.equal(data["i_ids"].cpu(), ref["i_ids"]) and torch.equal(data["j_ids"].cpu(), ref["j_ids"])
    assert data["mkpts1_f"].dtype == ref["mkpts1_f"].dtype == t1 and data["mkpts1_f"].shape == (K, 2)
    assert data["expec_f"].shape == (K, 3) and data["expec_f"].dtype == torch.float32
    assert tuple(data["hw0_c"]) == (hw0_i[0] // 8, hw0_i[1] // 8) and tuple(data["hw1_f"]) == (hw1_i[0] // 2, hw1_i[1] // 2)
    if K == 0:
        assert data["mkpts1_f"] is dk1
        return
    close(data["expec_f"][:, :2], ref["expec_f"][:, :2], 1e-3, 2e-4)
    close(data["mkpts1_f"], ref["mkpts1_f"], 1e-4, 2e-3)
    # the scaled step itself, bit-exact on the device's own expectation
    want = lsf.fine_keypoints1(ref["mkpts1_c"], data["expec_f"][:, :2].cpu(), 9, hw0_i, (hw0_i[0] // 2, hw0_i[1] // 2), s1, ref["b_ids"])
    assert torch.equal(data["mkpts1_f"].cpu(), want)


def test_fine_only_call_without_fine_matching_and_the_index_error(matchers, dev):
    g = torch.Generator().manual_seed(5)
    hw = (128, 160)
    k0, k1 = _keypoints(g, 40, hw, torch.float64), _keypoints(g, 40, hw, torch.float32)
    k0[0] = torch.tensor([200.0, 300.0], dtype=torch.float64)                   # clipped to (158, 126): row 126 / 8 -> 16 of 16
    img = torch.rand(1, 1, *hw, generator=g).to(dev)
    s = torch.tensor([[1.0, 1.0]], device=dev)
    d0, d1 = k0.to(dev), k1.to(dev)
    data = {"image0": img, "image1": img.clone(), "scale0": s, "scale1": s, "mkpts0_c": d0, "mkpts1_c": d1}
    matchers(enable_fine_matching=False)(data)                                  # no fine stage: the reference does not index, no error
    assert data["mkpts0_f"] is d0 and data["mkpts1_f"] is d1 and "expec_f" not in data and "conf_matrix" not in data
    assert d0[0].tolist() == [158.0, 126.0] and int(data["i_ids"][0]) >= 16 * 20
    data = {"image0": img, "image1": img.clone(), "scale0": s, "scale1": s, "mkpts0_c": k0.to(dev), "mkpts1_c": k1.to(dev)}
    with pytest.raises(IndexError):
        matchers()(data)


# ------------------------------------------------------------------------------------------------
# extraction through the real backbone
# ------------------------------------------------------------------------------------------------
def _check_extraction(data, hw0_i, hw1_i, s0, s1, coarse=True, fine=True):
    excused = 0
    for i, (hw_i, s) in enumerate(((hw0_i, s0), (hw1_i, s1))):
        hw = lsf.imghw(s.cpu(), hw_i)
        kp = data[f"mkpts{i}_f"]
        hw_c, hw_f = (hw_i[0] // 8, hw_i[1] // 8), (hw_i[0] // 2, hw_i[1] // 2)
        if coarse:
            out = data[f"feat_coarse_b_{i}"]
            assert out.shape == (len(kp), 256) and out.dtype == torch.float32
            excused += _check_samples(data[f"_bb_c{i}"][0], kp, out, hw_c, hw, True, f"coarse {i}")
        if fine:
            out = data[f"feat_ext{i}"]
            assert out.shape == (len(kp), 128) and out.dtype == torch.float32
            _check_samples(data[f"_bb_f{i}"][0], kp, out, hw_f, hw, False, f"fine {i}")
    return excused


def test_fine_only_call_with_extraction_through_the_real_backbone(matchers, lsd, dev):
    g = torch.Generator().manual_seed(23)
    hw0_i, hw1_i = (240, 320), (256, 224)
    img0, img1 = torch.rand(1, 1, *hw0_i, generator=g), torch.rand(1, 1, *hw1_i, generator=g)
    k0, k1, s0, s1 = _fine_only_inputs(g, 700, hw0_i, hw1_i, torch.float64, torch.float32, False)
    m = matchers()
    data = {"image0": img0.to(dev), "image1": img1.to(dev), "scale0": s0.to(dev), "scale1": s1.to(dev), "mkpts0_c": k0.to(dev),
            "mkpts1_c": k1.to(dev)}
    m(data, extract_coarse_feature=True, extract_fine_feature=True, _debug=True)
    assert {"feat_coarse_b_0", "feat_coarse_b_1", "feat_ext0", "feat_ext1"} <= set(data)
    excused = _check_extraction(data, hw0_i, hw1_i, s0, s1)
    print(f"fine-only extraction: {excused} nearest samples within 1e-4 of a half-integer excused")
    # the device's pre-encoding maps against the oracle backbone (the backbone bar of test_gpu_backbone: 1e-4 relative)
    with torch.no_grad():
        for i, img in enumerate((img0, img1)):
            fc, ff = lsf.backbone_maps(lsd, img)
            want_c, want_f = fc[0].flatten(1).t(), ff[0].flatten(1).t()
            assert float((data[f"_bb_c{i}"][0].cpu() - want_c).abs().max()) <= 1e-4 * float(want_c.abs().max())
            assert float((data[f"_bb_f{i}"][0].cpu() - want_f).abs().max()) <= 1e-4 * float(want_f.abs().max())
            # the sampler read the map BEFORE the positional encoding: map + PE table = the encoded rows of the coarse path
            pe = m._pe_table(fc.shape[2], fc.shape[3], dev).cpu()                 # the table the coarse path adds
            assert float((pe - lsf.pe_rows(fc.shape[2:])).abs().max()) <= 1e-6
            enc = data[f"_enc_c{i}"][0].cpu()
            assert float((data[f"_bb_c{i}"][0].cpu() + pe - enc).abs().max()) <= 1e-6 * float(pe.abs().max())
            assert float((data[f"_bb_c{i}"][0].cpu() - enc).abs().max()) > 0.5
            # and the sampled rows against the oracle backbone's maps
            hw = lsf.imghw(data[f"scale{i}"].cpu(), img.shape[2:])
            kp = data[f"mkpts{i}_f"].cpu()
            want = lsf.sample_feature_from_featuremap(ff, kp, hw, "bilinear")
            assert float((data[f"feat_ext{i}"].cpu() - want).abs().max()) <= 1.01e-4 * float(ff.abs().max())


def test_coarse_call_with_extraction_through_the_real_backbone(matchers, dev):
    g = torch.Generator().manual_seed(29)
    hw_i = (192, 256)
    img0, img1 = torch.rand(1, 1, *hw_i, generator=g), torch.rand(1, 1, *hw_i, generator=g)
    s0, s1 = torch.tensor([[1.25, 0.8]]), torch.tensor([[0.9, 1.1]])
    for fine in (True, False):
        m = matchers(enable_fine_matching=fine, thr=0.0)
        data = {"image0": img0.to(dev), "image1": img1.to(dev), "scale0": s0.to(dev), "scale1": s1.to(dev)}
        m(data, extract_coarse_feature=True, extract_fine_feature=True, _debug=True)
        K = len(data["b_ids"])
        assert K >= 4, K                           # random weights and images: a handful of mutual nearest neighbours at thr 0
        _check_extraction(data, hw_i, hw_i, s0, s1)
        # the coarse keypoints carry the scales as given (component 0 on x)
        want0 = lsf.scaled_coarse_keypoints(data["i_ids"].cpu(), data["b_ids"].cpu(), (24, 32), hw_i, (24, 32), s0)
        assert torch.equal(data["mkpts0_c"].cpu(), want0)


# ------------------------------------------------------------------------------------------------
# the SfM coarse call: image scales on planted features
# ------------------------------------------------------------------------------------------------
def _batched_hook(pair, dev, V, V1):
    x0, g0, x1, g1 = pair
    cl = lambda g: g[0].permute(1, 2, 0).reshape(-1, 128).contiguous().to(dev)
    return lambda fc0, ff0, fc1, ff1: (x0.expand(V, -1, -1).contiguous().to(dev), cl(g0)[None].expand(V, -1, -1).contiguous(),
                                       x1.expand(V1, -1, -1).contiguous().to(dev), cl(g1)[None].expand(V1, -1, -1).contiguous())


@pytest.mark.parametrize("V,V1", [(1, 1), (2, 1), (2, 2)])
@pytest.mark.parametrize("fine", [False, True])
def test_sfm_coarse_call_with_scales_on_planted_features(matchers, lsd, dev, V, V1, fine):
    H, W = 96, 128
    pair = planted_pair((H, W))
    img = torch.zeros(1, 1, H, W)
    with torch.no_grad():
        ref = lo.loftr_forward(lsd, lo.loftr_default_cfg(), img, img, feature_hook=oracle_hook(pair))
    s0 = torch.tensor([[1.25, 0.8], [0.6, 1.5]])[:V]
    s1 = torch.tensor([[0.9, 1.1], [1.3, 0.7]])[:V1]
    m = matchers(enable_fine_matching=fine)
    m.feature_hook = _batched_hook(pair, dev, V, V1) if V > 1 else device_hook(pair, dev)
    data = {"image0": torch.zeros(V, 1, H, W, device=dev), "image1": torch.zeros(V1, 1, H, W, device=dev), "scale0": s0.to(dev),
            "scale1": s1.to(dev)}
    try:
        m(data)
    finally:
        m.feature_hook = None
    Kr = len(ref["i_ids"])
    assert Kr >= 40 and len(data["b_ids"]) == V * Kr
    b_ids, i_ids, j_ids = data["b_ids"].cpu(), data["i_ids"].cpu(), data["j_ids"].cpu()
    assert torch.equal(b_ids, torch.arange(V).repeat_interleave(Kr))
    assert torch.equal(i_ids, ref["i_ids"].repeat(V)) and torch.equal(j_ids, ref["j_ids"].repeat(V))
    want0 = lsf.scaled_coarse_keypoints(i_ids, b_ids, (12, 16), (H, W), (12, 16), s0)
    want1 = lsf.scaled_coarse_keypoints(j_ids, b_ids, (12, 16), (H, W), (12, 16), s1)
    assert torch.equal(data["mkpts0_c"].cpu(), want0) and torch.equal(data["mkpts1_c"].cpu(), want1)
    assert "conf_matrix" in data and "gt_mask" in data
    if not fine:
        assert data["mkpts0_f"] is data["mkpts0_c"] and data["mkpts1_f"] is data["mkpts1_c"]
        return
    close(data["expec_f"][:, :2], ref["expec_f"][:, :2].repeat(V, 1), 1e-3, 2e-4)
    want = lsf.fine_keypoints1(want1, data["expec_f"][:, :2].cpu(), 9, (H, W), (H // 2, W // 2), s1, b_ids)
    assert torch.equal(data["mkpts1_f"].cpu(), want)
    want_o = lsf.fine_keypoints1(want1, ref["expec_f"][:, :2].repeat(V, 1), 9, (H, W), (H // 2, W // 2), s1, b_ids)
    close(data["mkpts1_f"], want_o, 1e-4, 2e-3)
    assert torch.equal(data["mkpts0_f"], data["mkpts0_c"])


def test_sfm_coarse_call_with_scales_sinkhorn(matchers, lsd, dev):
    H, W = 96, 128
    x0, g0, x1, g1 = planted_pair((H, W))
    pair = (x0 * 6.0, g0, x1 * 6.0, g1)            # as test_gpu_loftr_sinkhorn: unscaled rows leave the confidences below the threshold
    img = torch.zeros(1, 1, H, W)
    sd = dict(lsd)
    sd["coarse_matching.bin_score"] = torch.tensor(1.0)
    cfg = lo.loftr_default_cfg()
    cfg["match_coarse"]["match_type"] = "sinkhorn"
    with torch.no_grad():
        ref = lso.loftr_forward(sd, cfg, img, img, feature_hook=oracle_hook(pair))
    s0, s1 = torch.tensor([[1.25, 0.8]]), torch.tensor([[0.9, 1.1]])
    m = matchers(enable_fine_matching=False, sinkhorn=True)
    m.feature_hook = device_hook(pair, dev)
    data = {"image0": torch.zeros(1, 1, H, W, device=dev), "image1": torch.zeros(1, 1, H, W, device=dev), "scale0": s0.to(dev),
            "scale1": s1.to(dev)}
    try:
        m(data)
    finally:
        m.feature_hook = None
    assert len(ref["i_ids"]) >= 20 and torch.equal(data["i_ids"].cpu(), ref["i_ids"]) and torch.equal(data["j_ids"].cpu(), ref["j_ids"])
    assert torch.equal(data["mkpts0_c"].cpu(), lsf.scaled_coarse_keypoints(ref["i_ids"], ref["b_ids"], (12, 16), (H, W), (12, 16), s0))
    assert torch.equal(data["mkpts1_c"].cpu(), lsf.scaled_coarse_keypoints(ref["j_ids"], ref["b_ids"], (12, 16), (H, W), (12, 16), s1))


# ------------------------------------------------------------------------------------------------
# determinism
# ------------------------------------------------------------------------------------------------
def test_two_identical_calls_are_bit_identical(matchers, dev):
    g = torch.Generator().manual_seed(31)
    hw0_i, hw1_i = (240, 320), (256, 224)
    img0, img1 = torch.rand(1, 1, *hw0_i, generator=g).to(dev), torch.rand(1, 1, *hw1_i, generator=g).to(dev)
    k0, k1, s0, s1 = _fine_only_inputs(g, 900, hw0_i, hw1_i, torch.float32, torch.float64, False)
    outs = []
    for _ in range(2):
        data = {"image0": img0, "image1": img1, "scale0": s0.to(dev), "scale1": s1.to(dev), "mkpts0_c": k0.to(dev), "mkpts1_c": k1.to(dev)}
        matchers()(data, extract_coarse_feature=True, extract_fine_feature=True)
        outs.append(data)
    for k in ("i_ids", "j_ids", "expec_f", "mkpts0_f", "mkpts1_f", "feat_coarse_b_0", "feat_coarse_b_1", "feat_ext0", "feat_ext1"):
        assert torch.equal(outs[0][k], outs[1][k]), k
