"""Optimal-transport (sinkhorn) coarse matching in the LoFTR matcher behind the detector, without a GPU: construction with each attention
form, the ``state_dict`` layout (the linear keys plus ``coarse_matching.bin_score``), the rejected configurations, the marginals of the
test-side oracle (tests/loftr_sinkhorn_oracle.py), and the emitted code of the new kernels."""
import copy

import pytest
import torch

from onepose_st_amd import loftr
from onepose_st_amd.synthetic import make_synthetic_loftr_state_dict
from tests import loftr_sinkhorn_oracle as lso
from tests.test_disasm_guards import device_asm  # noqa: F401  (fixture)


def _cfg(coarse="linear", fine="linear", **mc):
    c = copy.deepcopy(loftr.default_cfg)
    c["coarse"]["attention"] = coarse
    c["fine"]["attention"] = fine
    c["match_coarse"]["match_type"] = "sinkhorn"
    c["match_coarse"].update(mc)
    return c


@pytest.mark.parametrize("coarse,fine", [("linear", "linear"), ("full", "linear"), ("linear", "full"), ("full", "full")])
def test_sinkhorn_matcher_builds_with_each_attention_form(coarse, fine):
    m = loftr.LoFTR_for_OnePose_Plus(_cfg(coarse, fine)).eval()
    assert m.sinkhorn and (m.coarse_full, m.fine_full) == (coarse == "full", fine == "full")
    assert m.coarse_matching.bin_score.shape == () and float(m.coarse_matching.bin_score.detach()) == 1.0


def test_state_dict_is_the_linear_keys_plus_bin_score_and_loads_strictly():
    want = loftr.LoFTR_for_OnePose_Plus().state_dict()
    m = loftr.LoFTR_for_OnePose_Plus(_cfg(skh_init_bin_score=2.5)).eval()
    got = m.state_dict()
    assert set(got) == set(want) | {"coarse_matching.bin_score"}
    assert all(got[k].shape == want[k].shape for k in want)
    assert got["coarse_matching.bin_score"].dtype == torch.float32 and float(got["coarse_matching.bin_score"]) == 2.5
    sd = dict(make_synthetic_loftr_state_dict(0))
    sd["coarse_matching.bin_score"] = torch.tensor(-0.75)
    m.load_state_dict(sd, strict=True)
    assert float(m.coarse_matching.bin_score.detach()) == -0.75
    # a dual-softmax checkpoint lacks the key
    with pytest.raises(RuntimeError, match="coarse_matching.bin_score"):
        loftr.LoFTR_for_OnePose_Plus(_cfg()).load_state_dict(make_synthetic_loftr_state_dict(0), strict=True)
    # and the dual-softmax model has no such key
    with pytest.raises(RuntimeError, match="coarse_matching.bin_score"):
        loftr.LoFTR_for_OnePose_Plus().load_state_dict(sd, strict=True)


def test_rejected_configurations():
    c = _cfg()
    c["match_coarse"]["match_type"] = "optimal"
    with pytest.raises(NotImplementedError):
        loftr.LoFTR_for_OnePose_Plus(c)
    for bad in (-1, 1.5, "3", True):
        with pytest.raises(ValueError):
            loftr.LoFTR_for_OnePose_Plus(_cfg(skh_iters=bad))
    with pytest.raises(NotImplementedError):
        loftr.LoFTR_for_OnePose_Plus(_cfg(sparse_spvs=True))
    loftr.LoFTR_for_OnePose_Plus(_cfg(sparse_spvs=False, skh_iters=0))
    assert not loftr.LoFTR_for_OnePose_Plus().sinkhorn                # the default config stays dual-softmax
    assert "coarse_matching.bin_score" not in loftr.LoFTR_for_OnePose_Plus().state_dict()


@pytest.mark.parametrize("m,n,alpha", [(7, 11, 1.0), (12, 5, -1.0), (9, 13, 4.0)])
def test_oracle_meets_the_marginals_after_many_iterations(m, n, alpha):
    """real rows of the assignment sum to 1 and the dustbin row to n; real columns to 1 and the dustbin column to m"""
    g = torch.Generator().manual_seed(m * n)
    scores = torch.randn(2, m, n, generator=g, dtype=torch.float64) * 3
    P = lso.log_optimal_transport(scores, torch.tensor(alpha, dtype=torch.float64), 200).exp()
    rows, cols = P.sum(2), P.sum(1)
    assert torch.allclose(rows[:, :m], torch.ones(2, m, dtype=torch.float64), atol=1e-9)
    assert torch.allclose(rows[:, m], torch.full((2,), float(n), dtype=torch.float64), atol=1e-9)
    assert torch.allclose(cols[:, :n], torch.ones(2, n, dtype=torch.float64), atol=1e-9)
    assert torch.allclose(cols[:, n], torch.full((2,), float(m), dtype=torch.float64), atol=1e-9)


def test_oracle_prefilter_zeroes_the_rows_and_columns_the_dustbin_wins():
    g = torch.Generator().manual_seed(5)
    f0, f1 = torch.randn(1, 20, 256, generator=g), torch.randn(1, 30, 256, generator=g)
    f1[0, :10] = f0[0, :10] * 4                                         # ten planted pairs, the rest unmatched
    f0[0, :10] *= 4
    conf, assign, filter0, filter1 = lso.sinkhorn_conf(f0, f1, 1.0, 3, True)
    plain, _, _, _ = lso.sinkhorn_conf(f0, f1, 1.0, 3, False)
    assert filter0[0, 10:].all() and not filter0[0, :10].any() and filter1[0, 10:].all() and not filter1[0, :10].any()
    assert (conf[0, 10:] == 0).all() and (conf[0, :, 10:] == 0).all()
    assert torch.equal(conf[0, :10, :10], plain[0, :10, :10]) and (torch.diagonal(conf[0, :10, :10]) > 0.5).all()


def test_sinkhorn_kernels_do_not_spill(device_asm):  # noqa: F811
    ks = {k: v for k, v in device_asm.items() if "skh_" in k}
    assert len(ks) == 8, sorted(ks)               # rows (3 instances), cols (2), colcomb, final (2)
    for sym, ins in ks.items():
        spills = [t for t in ins if t.startswith("scratch_")]
        assert not spills, (sym, spills[:4])
