"""Full (softmax) attention in the coarse and fine encoders on the MI355X (run with ``-m gpu``): the coarse layer entry, the flash-attention
kernel and the fine attention kernel against the CPU oracle (tests/full_attention_oracle.py), the whole path against the goldens the
reference produced with ``attention = "full"`` (both encoders; coarse only), the mixed configurations at c1, c2 with both encoders full
(pose parity, bit-reproducibility, batch independence), the object cache, and the mask semantics.

Bars: the layer at rtol 3e-4 / atol 1e-4 (those of the split-bf16 linear layer, tests/test_gpu_parity.py::test_encoder_layer_x3); the
whole path through tests/test_gpu_parity.py::_check_against in "bf16x3" (indices bit-exact outside the threshold window, keypoints
within 5e-4 px, mconf within rtol 5e-4)."""
import copy
import os

import numpy as np
import pytest
import torch

from onepose_st_amd import hip, layercall, packing
from onepose_st_amd.model import OnePosePlus_model
from onepose_st_amd.synthetic import make_synthetic_inputs
from tests import full_attention_oracle as foracle
from tests.test_gpu_parity import _check_against, _pose_parity, _run_features, close

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def dev():
    assert torch.cuda.is_available(), "these tests need the MI355X"
    hip.load()
    return torch.device("cuda:0")


def _attn_cfg(cfg, coarse, fine):
    c = copy.deepcopy(cfg)
    c["loftr_coarse"]["attention"] = coarse
    c["loftr_fine"]["attention"] = fine
    return c


@pytest.fixture(scope="module")
def fcfg(cfg):
    return _attn_cfg(cfg, "full", "full")


def _model(sd, c, dev, **extra):
    c = copy.deepcopy(c)
    c.update(extra)
    m = OnePosePlus_model(c).eval()
    m.load_state_dict(sd, strict=True)
    return m.to(dev)


@pytest.fixture(scope="module")
def fmodel(sd, fcfg, dev):
    return _model(sd, fcfg, dev)


def _b2_inputs(sd, c):
    i0 = make_synthetic_inputs(sd, n_points=333, image_hw=(96, 136), n_plant=120, seed=3, config=c, frame=0)
    i1 = make_synthetic_inputs(sd, n_points=333, image_hw=(96, 136), n_plant=120, seed=3, config=c, frame=1)
    both = {k: torch.cat([i0[k], i1[k]], 0) for k in ("keypoints3d", "descriptors3d_db", "descriptors3d_coarse_db", "feat_c", "feat_f")}
    both["image_hw"] = i0["image_hw"]
    return both


# ------------------------------------------------------------------------------------------------
# kernel and layer
# ------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("cross", [0, 1])
@pytest.mark.parametrize("B,L3,L2", [(1, 64, 32), (2, 70, 45), (3, 130, 7), (1, 5, 300), (1, 1000, 1200)])
def test_encoder_layer_full(sd, dev, cross, B, L3, L2):
    """ragged L and S (not multiples of the 32-key / 128-query tiles, S below one tile), L3d != L2d, several frames"""
    g = torch.Generator().manual_seed(4)
    x3, x2 = torch.randn(B, L3, 256, generator=g), torch.randn(B, L2, 256, generator=g)
    p = "loftr_coarse.layers.2."
    with torch.no_grad():
        if cross:
            r2, r3 = foracle.encoder_layer(sd, p, x2, x3, 8), foracle.encoder_layer(sd, p, x3, x2, 8)
        else:
            r2, r3 = foracle.encoder_layer(sd, p, x2, x2, 8), foracle.encoder_layer(sd, p, x3, x3, 8)
    w = packing.pack_coarse_layer(sd, p).to(dev)
    kw = dict(mode="full", wpack=w, is_cross=cross, workspace=layercall.workspace("full", B, L3, L2, dev))
    d3, d2 = x3.to(dev), x2.to(dev)
    y3, y2 = torch.full_like(d3, float("nan")), torch.full_like(d2, float("nan"))
    layercall.layer(d3, d2, y3, y2, **kw)
    e3, e2 = (y3.cpu() - r3).abs().max().item(), (y2.cpu() - r2).abs().max().item()
    print(f"full cross={cross} B={B} L=({L3},{L2}): max abs err 3D {e3:.3e} 2D {e2:.3e}")
    close(y3, r3, rtol=3e-4, atol=1e-4, msg="3D stream")
    close(y2, r2, rtol=3e-4, atol=1e-4, msg="2D stream")
    # a batch element's rows do not depend on its batch position
    if B > 1:
        y3b, y2b = torch.empty_like(d3[1:2]), torch.empty_like(d2[1:2])
        layercall.layer(d3[1:2].contiguous(), d2[1:2].contiguous(), y3b, y2b, **dict(kw, workspace=layercall.workspace("full", 1, L3, L2, dev)))
        assert torch.equal(y3b, y3[1:2]) and torch.equal(y2b, y2[1:2])
    with pytest.raises(ValueError):
        layercall.layer(d3, d2, d3, y2, **kw)


def _attention_f64(q, k, v):
    B, L, S = q.shape[0], q.shape[1], k.shape[1]
    q, k, v = (t.double().view(B, -1, 8, 32) for t in (q, k, v))
    return foracle.full_attention(q, k, v).reshape(B, L, 256)


@pytest.mark.parametrize("B,L,S,growing", [(1, 1, 1, False), (2, 33, 31, False), (1, 200, 97, False), (1, 129, 1000, True),
                                           (2, 64, 4800, True)])
def test_flash_attention_kernel(dev, B, L, S, growing):
    """the attention step alone against float64.  ``growing``: key norms rise along the source axis, so the running maximum grows on
    almost every tile and every rescale of the accumulator carries weight (random keys leave it near the first tile's)"""
    g = torch.Generator().manual_seed(9)
    q, k, v = torch.randn(B, L, 256, generator=g), torch.randn(B, S, 256, generator=g), torch.randn(B, S, 256, generator=g)
    if growing:
        k = k * torch.linspace(0.2, 3.0, S).view(1, S, 1)
    want = _attention_f64(q, k, v)
    qd, kd, vd = q.to(dev), k.to(dev), v.to(dev)          # (held: the kernel runs after the call returns)
    out = torch.full((B, L, 256), float("nan"), device=dev)
    hip.call("ophip_full_attention_h8d32", hip.ptr(qd), hip.ptr(kd), hip.ptr(vd), B, L, S, hip.ptr(out), hip.stream_handle())
    err = (out.cpu().double() - want).abs().max().item()
    print(f"flash B={B} L={L} S={S} growing={growing}: max abs err {err:.3e}")
    np.testing.assert_allclose(out.cpu().numpy(), want.float().numpy(), rtol=2e-4, atol=1e-4)


@pytest.mark.parametrize("L,S", [(25, 25), (1, 1), (25, 1), (1, 25)])
def test_fine_full_attention_kernel(dev, L, S):
    """window self (25 x 25), 3D self (1 x 1: the message is v exactly), window cross (25 x 1: v of the 3D token exactly), 3D cross (1 x 25)
    against the oracle's FullAttention in float64; matches at or past the device-side count are written as zeros"""
    K, live = 300, 257
    g = torch.Generator().manual_seed(5)
    q, k, v = torch.randn(K, L, 128, generator=g), torch.randn(K, S, 128, generator=g), torch.randn(K, S, 128, generator=g)
    want = foracle.full_attention(q.double().view(K, L, 8, 16), k.double().view(K, S, 8, 16), v.double().view(K, S, 8, 16)).reshape(K, L, 128)
    qd, kd, vd = q.to(dev), k.to(dev), v.to(dev)
    count = torch.tensor([live, 0, 0, 0], dtype=torch.int32, device=dev)
    out = torch.full((K, L, 128), float("nan"), device=dev)
    hip.call("ophip_fine_full_attention", hip.ptr(qd), hip.ptr(kd), hip.ptr(vd), K, L, S, hip.ptr(count, torch.int32), hip.ptr(out),
             hip.stream_handle())
    o = out.cpu()
    err = (o[:live].double() - want[:live]).abs().max().item()
    print(f"fine attention L={L} S={S}: max abs err {err:.3e}")
    np.testing.assert_allclose(o[:live].numpy(), want[:live].float().numpy(), rtol=1e-5, atol=1e-5)
    if S == 1:
        assert torch.equal(o[:live], v[:live].expand(-1, L, -1))
    assert not o[live:].any()


# ------------------------------------------------------------------------------------------------
# whole path
# ------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("case,fine", [("c1", "full"), ("b2", "full"), ("c1", "linear"), ("b2", "linear")])
def test_full_attention_against_reference_golden(fmodel, sd, cfg, dev, golden_dir, case, fine):
    c = _attn_cfg(cfg, "full", fine)
    tag = "full_attention" if fine == "full" else "full_coarse"
    g = np.load(os.path.join(golden_dir, f"{case}_{tag}_feature_boundary.npz"))
    model = fmodel if fine == "full" else _model(sd, c, dev)
    if case == "c1":
        inp = make_synthetic_inputs(sd, n_points=1000, image_hw=(240, 320), n_plant=600, seed=1, config=c)
    else:
        inp = _b2_inputs(sd, c)
    data = _run_features(model, inp, dev)
    n_sa = _check_against(data, g, "bf16x3", label=f"{case}_{tag}", want_rowmax=g["conf_rowmax"])
    err_px = float(np.abs(data["mkpts_query_f"].cpu().numpy() - g["mkpts_query_f"]).max()) if n_sa == 0 else 0.0
    assert err_px < 5e-4, err_px
    if case == "c1":
        rm = data["conf_matrix"].max(dim=2)[0][0].cpu().numpy()
        np.testing.assert_allclose(rm, g["conf_rowmax"], rtol=5e-4, atol=1e-6)
        # guard against a silent fall-back to the linear encoder: the linear golden's row maxima are far outside that tolerance
        lin = np.load(os.path.join(golden_dir, "c1_feature_boundary.npz"))["conf_rowmax"]
        assert np.abs(rm - lin).max() > 100 * (5e-4 * np.abs(lin).max() + 1e-6)
    if fine == "full":          # and to the linear fine encoder: the keypoints of the coarse-full / fine-linear fixture are far away
        half = np.load(os.path.join(golden_dir, f"{case}_full_coarse_feature_boundary.npz"))
        assert np.abs(data["mkpts_query_f"].cpu().numpy() - half["mkpts_query_f"]).max() > 100 * 5e-4


@pytest.mark.parametrize("coarse,fine", [("linear", "full"), ("full", "linear")])
def test_mixed_attention_at_c1_against_oracle(sd, cfg, dev, coarse, fine):
    c = _attn_cfg(cfg, coarse, fine)
    model = _model(sd, c, dev)
    inp = make_synthetic_inputs(sd, n_points=1000, image_hw=(240, 320), n_plant=600, seed=1, config=c)
    data = _run_features(model, inp, dev)
    with torch.no_grad():
        ref = foracle.forward_from_features(sd, c, inp, inp["feat_c"], inp["feat_f"], inp["image_hw"])
    _check_against(data, {k: ref[k].numpy() for k in ("b_ids", "i_ids", "j_ids", "m_bids", "mconf", "mkpts_3d_db", "mkpts_query_c",
                                                      "mkpts_query_f", "expec_f")}, "bf16x3", label=f"c1_{coarse}_{fine}",
                   want_rowmax=ref["conf_matrix"].max(dim=2)[0][0].numpy())


def test_c2_full_attention_against_oracle_pose_and_reproducibility(fmodel, sd, fcfg, dev):
    inp = make_synthetic_inputs(sd, n_points=7000, image_hw=(480, 640), n_plant=3000, seed=1, config=fcfg)
    data = _run_features(fmodel, inp, dev)
    torch.set_num_threads(max(1, min(16, os.cpu_count() or 1)))
    with torch.no_grad():
        ref = foracle.forward_from_features(sd, fcfg, inp, inp["feat_c"], inp["feat_f"], inp["image_hw"])
    assert len(ref["i_ids"]) > 2000
    n_sa = _check_against(data, {k: ref[k].numpy() for k in ("b_ids", "i_ids", "j_ids", "m_bids", "mconf", "mkpts_3d_db", "mkpts_query_c",
                                                             "mkpts_query_f", "expec_f")}, "bf16x3", label="c2_full_attention",
                          want_rowmax=ref["conf_matrix"].max(dim=2)[0][0].numpy())
    _pose_parity(data, ref["mkpts_3d_db"].numpy(), ref["mkpts_query_f"].numpy(), inp, "c2 full attention vs oracle", n_sa)
    del ref
    # two runs bit-identical
    again = _run_features(fmodel, inp, dev)
    for k in ("i_ids", "j_ids", "mconf", "mkpts_query_f", "conf_matrix"):
        assert torch.equal(again[k], data[k]), k
    # a B = 2 batch is bit-identical to its two frames run alone
    other = make_synthetic_inputs(sd, n_points=7000, image_hw=(480, 640), n_plant=3000, seed=1, config=fcfg, frame=1)
    alone = _run_features(fmodel, other, dev)
    both = {k: torch.cat([inp[k], other[k]], 0) for k in ("keypoints3d", "descriptors3d_db", "descriptors3d_coarse_db", "feat_c", "feat_f")}
    both["image_hw"] = inp["image_hw"]
    batch = _run_features(fmodel, both, dev)
    for b, single in ((0, data), (1, alone)):
        sel = batch["b_ids"] == b
        for k in ("i_ids", "j_ids", "mconf", "mkpts_query_f"):
            assert torch.equal(batch[k][sel], single[k]), (b, k)
        assert torch.equal(batch["conf_matrix"][b], single["conf_matrix"][0]), b


def test_object_cache_is_bit_identical(sd, fcfg, dev):
    plain = _model(sd, fcfg, dev)
    cached = _model(sd, fcfg, dev, hip_cache_object=True)
    assert cached.cache_object
    f0 = make_synthetic_inputs(sd, n_points=1000, image_hw=(240, 320), n_plant=600, seed=1, config=fcfg, frame=0)
    f1 = make_synthetic_inputs(sd, n_points=1000, image_hw=(240, 320), n_plant=600, seed=1, config=fcfg, frame=1)
    for f in (f0, f1, f0):                        # a miss, then hits of the same object on another frame and on the first again
        a, b = _run_features(plain, f, dev), _run_features(cached, f, dev)
        for k in ("i_ids", "j_ids", "mconf", "mkpts_query_f", "conf_matrix"):
            assert torch.equal(a[k], b[k]), k
    assert cached._obj_cache is not None and cached._obj_cache["y3d0"] is None          # no linear-layer rows in the entry


def test_mask_raises_like_the_reference_and_scale_alone_works(fmodel, sd, fcfg, dev, golden_dir):
    inp = _b2_inputs(sd, fcfg)
    g = np.load(os.path.join(golden_dir, "b2_masked_scaled_feature_boundary.npz"))
    d = {k: (v.to(dev) if torch.is_tensor(v) else v) for k, v in inp.items()}
    data = {k: d[k] for k in ("keypoints3d", "descriptors3d_db", "descriptors3d_coarse_db")}
    data["query_image_mask"] = torch.from_numpy(g["query_image_mask"]).to(dev)
    with pytest.raises(TypeError, match="linear_attention.py:85"):
        fmodel.forward_features(data, d["feat_c"], d["feat_f"], inp["image_hw"])
    # the oracle (the reference's FullAttention) fails the same way
    inp_m = dict(inp, query_image_mask=torch.from_numpy(g["query_image_mask"]))
    with pytest.raises(TypeError), torch.no_grad():
        foracle.forward_from_features(sd, fcfg, inp_m, inp["feat_c"], inp["feat_f"], inp["image_hw"])
    # query_image_scale alone only changes the fine scale
    scale = torch.from_numpy(g["query_image_scale"])
    data = {k: d[k] for k in ("keypoints3d", "descriptors3d_db", "descriptors3d_coarse_db")}
    data["query_image_scale"] = scale.to(dev)
    fmodel.forward_features(data, d["feat_c"], d["feat_f"], inp["image_hw"])
    inp_s = dict(inp, query_image_scale=scale)
    with torch.no_grad():
        ref = foracle.forward_from_features(sd, fcfg, inp_s, inp["feat_c"], inp["feat_f"], inp["image_hw"])
    _check_against(data, {k: ref[k].numpy() for k in ("b_ids", "i_ids", "j_ids", "m_bids", "mconf", "mkpts_3d_db", "mkpts_query_c",
                                                      "mkpts_query_f", "expec_f")}, "bf16x3", label="b2_full_attention_scaled")
