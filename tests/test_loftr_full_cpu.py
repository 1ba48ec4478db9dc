"""Full (softmax) attention in the LoFTR matcher behind the detector, without a GPU: construction per encoder, the ``state_dict`` layout,
the rejected forms, the test-side oracle (tests/loftr_full_oracle.py) against the published linear restatement, and the emitted code of
the window attention kernel."""
import copy

import pytest
import torch

from oracle import loftr_oracle as lo
from onepose_st_amd import loftr
from onepose_st_amd.synthetic import make_synthetic_loftr_state_dict
from tests import loftr_full_oracle as lfo
from tests.loftr_helpers import oracle_hook, planted_pair
from tests.test_disasm_guards import device_asm  # noqa: F401  (fixture)


def _cfg(coarse="linear", fine="linear"):
    c = copy.deepcopy(loftr.default_cfg)
    c["coarse"]["attention"] = coarse
    c["fine"]["attention"] = fine
    return c


@pytest.fixture(scope="module")
def lsd():
    return make_synthetic_loftr_state_dict(0)


@pytest.fixture(scope="module")
def pair_run(lsd):
    """the oracle on a planted 96 x 128 pair, per (coarse, fine) form"""
    pair = planted_pair((96, 128))
    img = torch.zeros(1, 1, 96, 128)
    out = {}

    def run(coarse, fine):
        if (coarse, fine) not in out:
            with torch.no_grad():
                out[coarse, fine] = lfo.loftr_forward(lsd, _cfg(coarse, fine), img, img, feature_hook=oracle_hook(pair))
        return out[coarse, fine]
    return run


@pytest.mark.parametrize("coarse,fine", [("full", "linear"), ("linear", "full"), ("full", "full")])
def test_full_attention_matcher_builds_and_loads_the_linear_state_dict(lsd, coarse, fine):
    m = loftr.LoFTR_for_OnePose_Plus(_cfg(coarse, fine)).eval()
    assert (m.coarse_full, m.fine_full) == (coarse == "full", fine == "full")
    want = loftr.LoFTR_for_OnePose_Plus().state_dict()
    got = m.state_dict()
    assert set(got) == set(want) and all(got[k].shape == want[k].shape for k in want)
    m.load_state_dict(lsd, strict=True)


@pytest.mark.parametrize("enc", ["coarse", "fine"])
def test_other_attention_forms_still_raise(enc):
    c = _cfg()
    c[enc]["attention"] = "sparse"
    with pytest.raises(NotImplementedError):
        loftr.LoFTR_for_OnePose_Plus(c)


def test_oracle_with_both_encoders_linear_is_the_published_restatement(lsd, pair_run):
    img = torch.zeros(1, 1, 96, 128)
    with torch.no_grad():
        ref = lo.loftr_forward(lsd, lo.loftr_default_cfg(), img, img, feature_hook=oracle_hook(planted_pair((96, 128))))
    got = pair_run("linear", "linear")
    for k in ("feat_c0", "feat_c1", "conf_matrix", "b_ids", "i_ids", "j_ids", "mconf", "fine_f0", "fine_f1", "expec_f", "mkpts1_f"):
        assert torch.equal(got[k], ref[k]), k


def test_oracle_swaps_the_attention_of_each_encoder(pair_run):
    lin, fc, ff = pair_run("linear", "linear"), pair_run("full", "linear"), pair_run("linear", "full")
    # full coarse: other coarse rows
    assert (fc["feat_c0"] - lin["feat_c0"]).abs().max() > 1e-2
    assert (fc["feat_c1"] - lin["feat_c1"]).abs().max() > 1e-2
    # full fine: the same coarse stage, other fine rows
    assert torch.equal(ff["feat_c0"], lin["feat_c0"]) and torch.equal(ff["i_ids"], lin["i_ids"])
    assert (ff["fine_f0"] - lin["fine_f0"]).abs().max() > 1e-2
    # the planted pair keeps its matches under every form
    for c, f in (("full", "linear"), ("linear", "full"), ("full", "full")):
        r = pair_run(c, f)
        assert len(r["i_ids"]) >= 40 and float((r["mconf"] - 0.2).abs().min()) > 0.05, (c, f)


def test_window_attention_kernel_does_not_spill(device_asm):  # noqa: F811
    ks = {k: v for k, v in device_asm.items() if "fine2_full_attention_kernel" in k}
    assert len(ks) == 1, sorted(ks)
    for sym, ins in ks.items():
        spills = [t for t in ins if t.startswith("scratch_")]
        assert not spills, (sym, spills[:4])
