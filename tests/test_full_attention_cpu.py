"""Full (softmax) attention in the coarse and fine encoders, without a GPU: config and model construction, the rejected combinations,
the CPU oracle against the goldens the reference produced with ``attention = "full"`` (tests/golden/make_golden_full_attention.py), and the
emitted code of the attention kernels.

Oracle bars are those of tests/test_oracle_golden.py: every stage checksum, indices exact."""
import copy
import os

import numpy as np
import pytest
import torch

from onepose_st_amd.config import validate_config
from onepose_st_amd.model import OnePosePlus_model
from tests import full_attention_oracle as foracle
from tests.test_disasm_guards import device_asm  # noqa: F401  (fixture)
from tests.test_oracle_golden import _inputs, close_cs, cs


def _cfg(cfg, coarse="linear", fine="linear", **extra):
    c = copy.deepcopy(cfg)
    c["loftr_coarse"]["attention"] = coarse
    c["loftr_fine"]["attention"] = fine
    c.update(extra)
    return c


@pytest.mark.parametrize("coarse,fine", [("full", "linear"), ("linear", "full"), ("full", "full")])
def test_full_attention_model_builds_and_loads_the_same_state_dict(sd, cfg, coarse, fine):
    c = _cfg(cfg, coarse=coarse, fine=fine)
    validate_config(c)
    m = OnePosePlus_model(c).eval()
    assert (m.coarse_full, m.fine_full) == (coarse == "full", fine == "full")
    keys = set(m.state_dict().keys())
    assert len(keys) == 195 and keys == set(OnePosePlus_model(cfg).state_dict().keys())
    m.load_state_dict(sd, strict=True)


@pytest.mark.parametrize("coarse,fine", [("full", "linear"), ("linear", "full"), ("full", "full")])
@pytest.mark.parametrize("precision", ["f32", "bf16"])
def test_full_attention_needs_the_split_bf16_mode(cfg, precision, coarse, fine):
    with pytest.raises(NotImplementedError, match="bf16x3"):
        OnePosePlus_model(_cfg(cfg, coarse=coarse, fine=fine, hip_precision=precision))
    OnePosePlus_model(_cfg(cfg, hip_precision=precision))        # the linear path keeps every mode


def test_full_fine_attention_rejects_the_plain_bf16_fine_stage(cfg):
    before = os.environ.get("OPHIP_FINE_PRECISION")
    with pytest.raises(NotImplementedError, match="hip_fine_precision"):
        OnePosePlus_model(_cfg(cfg, fine="full", hip_fine_precision="bf16"))
    assert os.environ.get("OPHIP_FINE_PRECISION") == before              # rejected before the process-wide switch is touched


def test_unknown_attention_is_rejected(cfg):
    with pytest.raises(NotImplementedError):
        OnePosePlus_model(_cfg(cfg, coarse="performer"))


def test_full_attention_oracle_masked_cross_raises_like_the_reference():
    q, k, v = torch.randn(1, 5, 8, 32), torch.randn(1, 7, 8, 32), torch.randn(1, 7, 8, 32)
    with pytest.raises(TypeError):
        foracle.full_attention(q, k, v, q_mask=None, kv_mask=torch.ones(1, 7, dtype=torch.bool))
    # unmasked: a plain softmax attention (float64 restatement)
    qd, kd, vd = q.double(), k.double(), v.double()
    a = torch.softmax(torch.einsum("nlhd,nshd->nhls", qd, kd) / 32 ** 0.5, dim=-1)
    want = torch.einsum("nhls,nshd->nlhd", a, vd)
    torch.testing.assert_close(foracle.full_attention(q, k, v).double(), want, rtol=1e-5, atol=1e-6)


@pytest.mark.parametrize("case,fname,fine", [("c1", "c1_full_attention_feature_boundary.npz", "full"),
                                             ("b2", "b2_full_attention_feature_boundary.npz", "full"),
                                             ("c1", "c1_full_coarse_feature_boundary.npz", "linear"),
                                             ("b2", "b2_full_coarse_feature_boundary.npz", "linear")])
def test_full_attention_oracle_matches_reference_golden(sd, cfg, golden_dir, case, fname, fine):
    c = _cfg(cfg, coarse="full", fine=fine)
    g = np.load(os.path.join(golden_dir, fname))
    inp = _inputs(sd, c, case)
    for k in ("keypoints3d", "descriptors3d_db", "descriptors3d_coarse_db", "feat_c", "feat_f"):
        np.testing.assert_allclose(cs(inp[k]), g["in_" + k], rtol=1e-12, atol=1e-9)
    trace = {}
    with torch.no_grad():
        out = foracle.forward_from_features(sd, c, inp, inp["feat_c"], inp["feat_f"], inp["image_hw"], trace)
    close_cs(cs(trace["q2d_in"]), g["pe_out_cs"])
    close_cs(cs(trace["d3_in"].transpose(1, 2)), g["kpt_out_cs"])
    for li, (d3, d2) in enumerate(trace["coarse_layers"]):
        close_cs(cs(d2), g[f"coarse{li}_2d_cs"])
        close_cs(cs(d3), g[f"coarse{li}_3d_cs"])
        np.testing.assert_allclose(d2[0][:4, :8].numpy(), g[f"coarse{li}_2d_probe"], rtol=1e-4, atol=1e-5)
        np.testing.assert_allclose(d3[0][:4, :8].numpy(), g[f"coarse{li}_3d_probe"], rtol=1e-4, atol=1e-5)
    conf = out["conf_matrix"]
    np.testing.assert_allclose(conf.max(dim=2)[0][0].numpy(), g["conf_rowmax"], rtol=1e-4, atol=1e-6)
    np.testing.assert_allclose(conf.max(dim=1)[0][0].numpy(), g["conf_colmax"], rtol=1e-4, atol=1e-6)
    for k in ("b_ids", "i_ids", "j_ids", "m_bids"):
        np.testing.assert_array_equal(out[k].numpy(), g[k])
    for k in ("mconf", "mkpts_3d_db", "mkpts_query_c", "mkpts_query_f"):
        np.testing.assert_allclose(out[k].numpy(), g[k], rtol=1e-4, atol=2e-5, err_msg=k)
    np.testing.assert_allclose(out["expec_f"][:, :2].numpy(), g["expec_f"][:, :2], rtol=1e-4, atol=2e-5)
    close_cs(cs(trace["fine_f3_in"]), g["fine_in_f3_cs"])
    close_cs(cs(trace["fine_win_in"]), g["fine_in_win_cs"])
    close_cs(cs(trace["fine_win_out"]), g["fine1_win_cs"])
    close_cs(cs(trace["fine_f3_out"]), g["fine1_f3_cs"])
    if case == "c1":           # the issue's figures for this case: K = 555, 548 of them planted pairs
        key = lambda i, j: i.astype(np.int64) * 100000 + j
        assert len(g["i_ids"]) == 555
        assert int(np.isin(key(g["i_ids"], g["j_ids"]), key(g["planted_i"], g["planted_j"])).sum()) == 548
    # the fixture is a different computation from the linear one: its coarse layers differ from the linear golden's
    lin = np.load(os.path.join(golden_dir, "c1_feature_boundary.npz" if case == "c1" else "b2_ragged_feature_boundary.npz"))
    assert abs(lin["coarse5_3d_cs"][1] - g["coarse5_3d_cs"][1]) > 1e-3 * abs(g["coarse5_3d_cs"][1])
    if fine == "full":         # and its fine encoder is the full one: the fine outputs differ from the coarse-full / fine-linear fixture's
        half = np.load(os.path.join(golden_dir, fname.replace("full_attention", "full_coarse")))
        np.testing.assert_array_equal(half["fine_in_win_cs"], g["fine_in_win_cs"])
        assert abs(half["fine1_f3_cs"][1] - g["fine1_f3_cs"][1]) > 1e-3 * abs(g["fine1_f3_cs"][1])


@pytest.mark.parametrize("kernel,mfma", [("full_flash_kernel", True), ("fine_full_attention_kernel", False)])
def test_attention_kernels_do_not_spill(device_asm, kernel, mfma):  # noqa: F811
    ks = {k: v for k, v in device_asm.items() if kernel in k}
    assert len(ks) == 1, sorted(ks)
    for sym, ins in ks.items():
        assert any(t.startswith("v_mfma_f32_32x32x16_bf16") for t in ins) == mfma, sym
        spills = [t for t in ins if t.startswith("scratch_")]
        assert not spills, (sym, spills[:4])
