"""Padding masks (mask0 / mask1) of the LoFTR matcher without a GPU: the masked oracle (tests/loftr_masked_oracle.py) against the
existing oracles, its padding invariance, a hand-checked mask_border_with_padding case, the input forms that raise, the new C entries in
the header, the binding and the built library."""
import copy
import ctypes
import os

import pytest
import torch

from oracle import loftr_oracle as lo
from onepose_st_amd import hip, loftr
from onepose_st_amd.synthetic import make_synthetic_loftr_state_dict
from tests import loftr_masked_oracle as lmo
from tests import loftr_sinkhorn_oracle as lso
from tests.loftr_helpers import planted_pair
from tests.test_disasm_guards import device_asm  # noqa: F401  (fixture)

NEW_ENTRIES = ("ophip_encoder_layer_x3w8_masks", "ophip_encoder_layer_x3w8_streams_masks", "ophip_coarse_match_2d_masked",
               "ophip_coarse_match_2d_sinkhorn_masked")


@pytest.fixture(scope="module")
def sd64():
    sd = make_synthetic_loftr_state_dict(0)
    sd = {k: (v.double() if v.is_floating_point() else v) for k, v in sd.items()}
    sd["coarse_matching.bin_score"] = torch.tensor(1.0, dtype=torch.float64)
    return sd


def pad_rows(x, hw, hwp, junk_seed):
    """rows [B, h * w, C] of an h x w grid -> [B, hp * wp, C], the grid in the top-left corner, random junk in the padded cells"""
    (h, w), (hp, wp) = hw, hwp
    g = torch.Generator().manual_seed(junk_seed)
    out = torch.randn(x.shape[0], hp, wp, x.shape[-1], generator=g, dtype=x.dtype) * 3
    out[:, :h, :w] = x.view(x.shape[0], h, w, -1)
    return out.view(x.shape[0], hp * wp, -1)


def grid_mask(B, hw, hwp):
    m = torch.zeros(B, *hwp, dtype=torch.bool)
    m[:, :hw[0], :hw[1]] = True
    return m


def remap(ids, w, wp):
    return (ids // w) * wp + ids % w


def test_oracle_without_masks_and_with_all_ones_masks_is_the_existing_oracle(sd64):
    cfg = lo.loftr_default_cfg()
    x0, _, x1, _ = planted_pair((96, 128))
    x0, x1 = x0.double(), x1.double()
    names = cfg["coarse"]["layer_names"]
    ref = lo.transformer_two_images(sd64, "loftr_coarse", names, 8, x0, x1)
    none = lmo.transformer_two_images(sd64, "loftr_coarse", names, 8, x0, x1)
    ones = torch.ones(1, x0.shape[1], dtype=torch.bool)
    full = lmo.transformer_two_images(sd64, "loftr_coarse", names, 8, x0, x1, ones, ones)
    assert torch.equal(none[0], ref[0]) and torch.equal(none[1], ref[1])
    assert torch.equal(full[0], ref[0]) and torch.equal(full[1], ref[1])          # phi * 1.0 and v * 1.0 are exact
    hw = (12, 16)
    m = torch.ones(1, *hw, dtype=torch.bool)
    mc = cfg["match_coarse"]
    want = lo.coarse_matching(ref[0], ref[1], hw, hw, (96, 128), mc)
    assert len(want["i_ids"]) >= 40
    for masks in ((None, None), (m, m)):
        got = lmo.coarse_matching(ref[0], ref[1], hw, hw, (96, 128), mc, *masks)
        for k in ("b_ids", "i_ids", "j_ids", "mconf", "mkpts0_c", "mkpts1_c", "conf_matrix"):
            assert torch.equal(got[k], want[k]), k
    skh = dict(mc, match_type="sinkhorn")
    want = lso.coarse_matching(ref[0], ref[1], hw, hw, (96, 128), skh, 1.0)
    for masks in ((None, None), (m, m)):
        got = lmo.coarse_matching(ref[0], ref[1], hw, hw, (96, 128), skh, *masks, bin_score=1.0)
        for k in ("b_ids", "i_ids", "j_ids", "mconf", "conf_matrix"):
            assert torch.equal(got[k], want[k]), k


def test_dual_softmax_path_is_invariant_under_padding(sd64):
    """a planted pair padded to larger grids (junk in the padded rows) with masks: the unpadded matches with remapped cell ids, and the same
    confidences at the valid cells"""
    cfg = lo.loftr_default_cfg()
    H, W = 96, 128
    hw = (H // 8, W // 8)
    x0, g0, x1, g1 = (t.double() for t in planted_pair((H, W)))
    ref = lmo.forward_from_features(sd64, cfg, x0, g0, x1, g1, (H, W), fine=False)
    K = len(ref["i_ids"])
    assert K >= 40
    hwp0, hwp1 = (hw[0] + 3, hw[1] + 2), (hw[0] + 1, hw[1] + 4)
    p0, p1 = pad_rows(x0, hw, hwp0, 1), pad_rows(x1, hw, hwp1, 2)
    z = lambda hwp: torch.zeros(1, 128, 4 * hwp[0], 4 * hwp[1], dtype=torch.float64)
    m0, m1 = grid_mask(1, hw, hwp0), grid_mask(1, hw, hwp1)
    got = lmo.forward_from_features(sd64, cfg, p0, z(hwp0), p1, z(hwp1), (8 * hwp0[0], 8 * hwp0[1]), m0, m1, fine=False)
    valid0 = m0.flatten(1)[0]
    valid1 = m1.flatten(1)[0]
    torch.testing.assert_close(got["feat_c0"][0, valid0], ref["feat_c0"][0], rtol=1e-9, atol=1e-9)
    torch.testing.assert_close(got["feat_c1"][0, valid1], ref["feat_c1"][0], rtol=1e-9, atol=1e-9)
    assert got["i_ids"].tolist() == remap(ref["i_ids"], hw[1], hwp0[1]).tolist()
    assert got["j_ids"].tolist() == remap(ref["j_ids"], hw[1], hwp1[1]).tolist()
    conf = got["conf_matrix"][0]
    torch.testing.assert_close(conf[valid0][:, valid1], ref["conf_matrix"][0], rtol=1e-9, atol=1e-12)
    # padded regions: a pair with one padded cell is 0, a pair of two padded cells 1 / (L0 L1)
    assert (conf[valid0][:, ~valid1] == 0).all() and (conf[~valid0][:, valid1] == 0).all()
    L0, L1 = conf.shape
    torch.testing.assert_close(conf[~valid0][:, ~valid1], torch.full_like(conf[~valid0][:, ~valid1], 1.0 / (L0 * L1)))
    torch.testing.assert_close(got["mconf"], ref["mconf"], rtol=1e-9, atol=1e-12)


def test_border_with_padding_by_hand():
    """border 2; grid 0 is 7 x 8 with a valid 6 x 7 corner (rows 2..3, columns 2..4 survive); grid 1 is 6 x 6 whose mask holds row 0
    only: its extent h1 = 1 < border, so the clear starts at 1 - 2 = -1, i.e. the last row only (rows 2..4 survive), and w1 = 6 keeps
    columns 2..3"""
    (h0, w0), (h1, w1) = (7, 8), (6, 6)
    m0 = torch.zeros(1, h0, w0, dtype=torch.bool)
    m0[:, :6, :7] = True
    m1 = torch.zeros(1, h1, w1, dtype=torch.bool)
    m1[:, 0] = True
    conf = torch.full((1, h0 * w0, h1 * w1), 0.01)
    plant = {"a": ((2, 2), (2, 2)), "b": ((3, 4), (4, 3)),                                # kept (b: row 4 of grid 1 survives the -1 start)
             "c": ((4, 3), (3, 2)), "d": ((3, 5), (2, 3)), "e": ((2, 3), (5, 2)),          # dropped: grid-0 row 4, column 5; grid-1 row 5
             "f": ((3, 2), (3, 4)), "g": ((1, 3), (3, 3))}                                 # dropped: grid-1 column 4; grid-0 row 1
    for (a, b) in plant.values():
        conf[0, a[0] * w0 + a[1], b[0] * w1 + b[1]] = 0.9
    out = lmo.get_coarse_match(conf, (h0, w0), (h1, w1), (8 * h0, 8 * w0), 0.2, 2, m0, m1)
    assert out["i_ids"].tolist() == [2 * w0 + 2, 3 * w0 + 4] and out["j_ids"].tolist() == [2 * w1 + 2, 4 * w1 + 3]
    # without masks the all-sides border of the padded grids decides instead: a, d and c stay (grid-0 rows 2..4, columns 2..5), b goes
    # (grid-1 row 4 is in the last two rows)
    plain = lmo.get_coarse_match(conf, (h0, w0), (h1, w1), (8 * h0, 8 * w0), 0.2, 2)
    assert plain["i_ids"].tolist() == [2 * w0 + 2, 3 * w0 + 5, 4 * w0 + 3]
    # border 0: nothing is cleared, every planted pair stays
    assert len(lmo.get_coarse_match(conf, (h0, w0), (h1, w1), (8 * h0, 8 * w0), 0.2, 0, m0, m1)["i_ids"]) == len(plant)


def _images(V=1, V1=1, H=64, W=96):
    return torch.zeros(V, 1, H, W), torch.zeros(V1, 1, H, W)


def _masks(V=1, V1=1, hw=(8, 12)):
    return torch.ones(V, *hw, dtype=torch.bool), torch.ones(V1, *hw, dtype=torch.bool)


def test_mask_forms_that_raise_and_the_well_formed_call():
    m = loftr.LoFTR_for_OnePose_Plus().eval()
    i0, i1 = _images()
    k0, k1 = _masks()
    bad = [
        {"mask0": k0},                                                                   # no partner
        {"mask1": k1},
        {"mask0": k0.to(torch.uint8), "mask1": k1.to(torch.uint8)},                      # another dtype
        {"mask0": k0.float(), "mask1": k1.float()},
        {"mask0": torch.ones(1, 64, 96, dtype=torch.bool), "mask1": torch.ones(1, 64, 96, dtype=torch.bool)},      # image resolution
        {"mask0": torch.ones(2, 8, 12, dtype=torch.bool), "mask1": k1},                  # wrong batch
        {"mask0": k0, "mask1": torch.ones(1, 8, 11, dtype=torch.bool)},                  # wrong grid
        {"mask0": k0.flatten(1), "mask1": k1.flatten(1)},                                # flattened
    ]
    for extra in bad:
        with pytest.raises(NotImplementedError):
            m({"image0": i0, "image1": i1, **extra})
    # V = 3 against one query: mask1 has image1's batch (1); a batch-3 mask1 is the wrong batch
    i0v, i1v = _images(V=3, V1=1)
    k0v, k1v = _masks(V=3, V1=3)
    with pytest.raises(NotImplementedError):
        m({"image0": i0v, "image1": i1v, "mask0": k0v, "mask1": k1v})
    # well-formed masks on CPU tensors get as far as the device check
    with pytest.raises(hip.HipLibraryError):
        m({"image0": i0, "image1": i1, "mask0": k0, "mask1": k1})
    with pytest.raises(hip.HipLibraryError):
        m({"image0": i0v, "image1": i1v, "mask0": k0v, "mask1": k1})
    # full coarse attention with masks keeps raising, with the reason in the message
    cfg = copy.deepcopy(loftr.default_cfg)
    cfg["coarse"]["attention"] = "full"
    mf = loftr.LoFTR_for_OnePose_Plus(cfg).eval()
    with pytest.raises(NotImplementedError, match="NaN"):
        mf({"image0": i0, "image1": i1, "mask0": k0, "mask1": k1})
    cfg = copy.deepcopy(loftr.default_cfg)
    cfg["fine"]["attention"] = "full"                                                    # the fine encoder is never masked
    with pytest.raises(hip.HipLibraryError):
        loftr.LoFTR_for_OnePose_Plus(cfg).eval()({"image0": i0, "image1": i1, "mask0": k0, "mask1": k1})


def test_new_entries_in_header_binding_and_library():
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    header = open(os.path.join(root, "include", "onepose_hip.h")).read()
    for name in NEW_ENTRIES:
        assert f"{name}(" in header, name
        assert name in hip.EXPORTED_SYMBOLS, name
    lib = ctypes.CDLL(hip.library_path())
    for name in NEW_ENTRIES:
        assert hasattr(lib, name), name


def test_new_encoder_instantiation_has_no_scratch(device_asm):  # noqa: F811
    hits = [k for k in device_asm if "enc_x3w8_kernel" in k]
    assert len(hits) == 6, hits                      # {attn_apply, kv_reduce} x {plain, query-masked, both streams masked}
    for k in hits:
        assert not any(t.startswith("scratch_") for t in device_asm[k]), k
    lim = [k for k in device_asm if "pad_limits_kernel" in k]
    assert len(lim) == 1

