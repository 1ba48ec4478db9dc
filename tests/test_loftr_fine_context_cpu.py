"""CPU side of ``fine_concat_coarse_feat``: the state-dict layout and the strict load, the refusals, the header and
the binding of ``libonepose_fine_context.so`` (every rejected call without a device), the test-side oracle on the planted pair, and the bar
of tests/loftr_fine_context_reference.py: the stand-in's figure re-derived, every seeded fault outside it."""
import copy
import ctypes
import os
import re

import pytest
import torch

from onepose_st_amd import cabi, fine_context, loftr, packing, sfm_coarse, sfm_fine
from onepose_st_amd.synthetic import make_synthetic_loftr_state_dict
from tests import loftr_fine_context_reference as R
from tests.loftr_helpers import planted_pair

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NEW_KEYS = {"fine_preprocess.down_proj.weight": (128, 256), "fine_preprocess.down_proj.bias": (128,),
            "fine_preprocess.merge_feat.weight": (128, 256), "fine_preprocess.merge_feat.bias": (128,)}


def config(**kw):
    cfg = copy.deepcopy(loftr.default_cfg)
    cfg["fine_concat_coarse_feat"] = True
    cfg.update(kw)
    return cfg


@pytest.fixture(scope="module")
def sd():
    return make_synthetic_loftr_state_dict(0, fine_concat_coarse_feat=True)


# ---- state dict ------------------------------------------------------------------------------------------------------------------------
def test_state_dict_layout_and_strict_load(sd, tmp_path):
    plain = make_synthetic_loftr_state_dict(0)
    assert set(sd) - set(plain) == set(NEW_KEYS) and set(plain) <= set(sd)
    assert all(torch.equal(sd[k], plain[k]) for k in plain)                      # the new tensors are drawn after every other one
    assert {k: tuple(sd[k].shape) for k in NEW_KEYS} == NEW_KEYS
    for fine in (True, False):                                                    # the published class owns them without the fine stage too
        m = loftr.LoFTR_for_OnePose_Plus(config(), enable_fine_matching=fine)
        assert set(m.state_dict()) == set(sd)
        m.load_state_dict(sd, strict=True)
        assert torch.equal(m.fine_preprocess.merge_feat.bias, sd["fine_preprocess.merge_feat.bias"])
        with pytest.raises(RuntimeError, match="fine_preprocess"):
            m.load_state_dict(plain, strict=True)
    assert set(loftr.LoFTR_for_OnePose_Plus().state_dict()) == set(plain)        # without the switch: exactly today's keys
    with pytest.raises(RuntimeError, match="fine_preprocess"):
        loftr.LoFTR_for_OnePose_Plus().load_state_dict(sd, strict=True)
    assert sfm_coarse.build_model({"matcher." + k: v for k, v in sd.items()}, config()).fine_context
    path = tmp_path / "public.ckpt"
    torch.save({"state_dict": sd}, path)
    m = loftr.build_2D_match_model({"method": "LoFTR", "weight_path": str(path), "config": config(fine_window_size=5)})
    assert m.fine_context and not m.training and m.config["fine_window_size"] == 5
    with pytest.raises(RuntimeError, match="fine_preprocess"):                    # the default config is still the reference's
        loftr.build_2D_match_model({"method": "LoFTR", "weight_path": str(path)})


def test_pack_fine_context(sd):
    wp = packing.pack_fine_context(sd)
    assert wp.dtype == torch.uint8 and wp.numel() == 2 * 2 * 128 * (256 + 128 + 128) + 4 * 256
    hi = wp[:2 * 128 * 512].view(torch.bfloat16).float()
    lo = wp[2 * 128 * 512:4 * 128 * 512].view(torch.bfloat16).float()
    wm = sd["fine_preprocess.merge_feat.weight"]
    flat = torch.cat([packing.pack_linear_frag16(m) for m in (sd["fine_preprocess.down_proj.weight"], wm[:, :128], wm[:, 128:])])
    assert torch.equal(hi, flat.to(torch.bfloat16).float()) and float((hi + lo - flat).abs().max()) < 2.0 ** -16
    bias = wp[4 * 128 * 512:].view(torch.float32)
    assert torch.equal(bias[:128], sd["fine_preprocess.down_proj.bias"]) and torch.equal(bias[128:], sd["fine_preprocess.merge_feat.bias"])
    # fragment (tile 0, k-block 1) of the window half: lane 32 h + r holds Wm[r][16 + 8 h .. 16 + 8 h + 7]
    frag = flat[128 * 256:128 * 384].view(4, 8, 64, 8)[0, 1]
    assert torch.equal(frag[32 + 5], wm[5, 24:32]) and torch.equal(frag[7], wm[7, 16:24])
    with pytest.raises(ValueError):
        packing.pack_fine_context({**sd, "fine_preprocess.down_proj.weight": torch.zeros(128, 128)})


# ---- refusals --------------------------------------------------------------------------------------------------------------------------
def test_refusals(sd):
    m = loftr.LoFTR_for_OnePose_Plus(config()).eval()
    img = torch.zeros(1, 1, 64, 96)
    with pytest.raises(NotImplementedError, match="fine_concat_coarse_feat with provided coarse matches"):
        m({"image0": img, "image1": img, "mkpts0_c": torch.zeros(3, 2), "mkpts1_c": torch.zeros(3, 2)})
    with pytest.raises(NotImplementedError, match="fine_concat_coarse_feat with provided coarse matches"):
        sfm_fine._check_matcher(m)
    with pytest.raises(NotImplementedError, match="fine_concat_coarse_feat with provided coarse matches"):
        sfm_fine.build_feature_bank(m, [img])
    sfm_fine._check_matcher(loftr.LoFTR_for_OnePose_Plus().eval())               # without the switch: as before
    cfg = config()
    cfg["coarse"]["temp_bug_fix"] = True
    with pytest.raises(NotImplementedError, match="temp_bug_fix"):
        loftr.LoFTR_for_OnePose_Plus(cfg)
    with pytest.raises(cabi.HipLibraryError):                                     # no CPU fallback
        fine_context.merge(torch.zeros(1, 9, 128), torch.zeros(1, 9, 128), torch.zeros(1, 4, 256), torch.zeros(1, 4, 256),
                           torch.zeros(1, dtype=torch.int64), torch.zeros(1, dtype=torch.int64), torch.zeros(1, dtype=torch.int64), 3,
                           packing.pack_fine_context(sd))
    with pytest.raises(TypeError, match="^x1: expected a tensor$"):
        fine_context.merge(torch.zeros(1, 9, 128), torch.zeros(1, 9, 128), torch.zeros(1, 4, 256), None,
                           torch.zeros(1, dtype=torch.int64), torch.zeros(1, dtype=torch.int64), torch.zeros(1, dtype=torch.int64), 3,
                           packing.pack_fine_context(sd))


# ---- header and binding ----------------------------------------------------------------------------------------------------------------
SYMBOLS = ("opfcx_abi_version", "opfcx_last_error", "opfcx_wpack_bytes", "opfcx_context_floats", "opfcx_merge")
MERGE_PARAMS = ("win0", "win1", "coarse0", "coarse0_bstride", "coarse1", "coarse1_bstride", "b_ids", "i_ids", "j_ids", "K", "B", "L0", "L1", "W",
                "wpack", "context", "out0", "out1", "stream")


def test_header_and_binding(tmp_path):
    entry, = cabi.EXTENSIONS
    assert tuple(entry) == ("opfcx", "ext/onepose_fine_context.h", "libonepose_fine_context.so", "OPFCX_LIB", "fine_context")
    assert entry not in cabi.LIBRARIES
    for column, taken in zip(entry, zip(*cabi.LIBRARIES)):
        assert column not in taken
    text = open(os.path.join(REPO, "include", "ext", "onepose_fine_context.h")).read()
    header = cabi.parse(text, cabi.names_of("opfcx"))
    assert tuple(header.prototypes) == SYMBOLS == fine_context.EXPORTED_SYMBOLS
    assert tuple(n for _, n in header.prototypes["opfcx_merge"].params) == MERGE_PARAMS
    assert header.defines == {"OPFCX_ABI_VERSION": 1, "OPFCX_TILE_ROWS": 64, "OPFCX_MAX_ROWS": 2 ** 30}
    assert fine_context.ABI_VERSION == 1 and fine_context.TILE_ROWS == R.TILE == 64
    assert cabi.parse(text).prototypes == {}                                      # the table's reader does not know the prefix
    assert cabi.parse("int ophip_x(int a);", None).prototypes.keys() == {"ophip_x"} == cabi.parse("int ophip_x(int a);").prototypes.keys()
    with pytest.raises(TypeError, match="takes 19 arguments"):
        fine_context.check_arity("opfcx_merge", (1, 2, 3))
    with pytest.raises(TypeError, match="missing context; unknown workspace"):
        fine_context.order("opfcx_merge", **{**{n: 0 for n in MERGE_PARAMS if n != "context"}, "workspace": 0})
    for other in os.listdir(os.path.join(REPO, "include")):                       # no other header is the place of these entry points
        if other.endswith(".h"):
            assert "opfcx_" not in open(os.path.join(REPO, "include", other)).read()
    mk = open(os.path.join(REPO, "onepose_st_amd", "csrc", "Makefile")).read()
    srcs = re.search(r"^SRCS := (.*)$", mk, re.M).group(1).split()
    assert "fine_context.hip" not in srcs and re.search(r"^FCX_SRCS := fine_context.hip$", mk, re.M)
    # the load errors
    absent = cabi.Binding(entry.header, entry.so, entry.prefix, "OPFCX_NO_SUCH_VARIABLE", names=cabi.names_of("opfcx"))
    absent.path = str(tmp_path / "libonepose_absent.so")
    with pytest.raises(cabi.HipLibraryError, match="libonepose_absent.so not found"):
        absent.load()
    no_header = cabi.Binding("ext/no_such_header.h", entry.so, entry.prefix, entry.env, names=cabi.names_of("opfcx"))
    assert no_header.exported_symbols == () and no_header.abi_version is None
    with pytest.raises(cabi.HipLibraryError, match="no_such_header.h not found"):
        no_header.load()


def test_built_library_rejects_without_a_device(sd):
    assert os.path.exists(fine_context.library_path()), "libonepose_fine_context.so: run __graft_entry__.build()"
    lib = fine_context.load()
    assert all(hasattr(lib, s) for s in SYMBOLS) and lib.opfcx_abi_version() == 1
    assert fine_context.wpack_bytes() == packing.pack_fine_context(sd).numel() == 263168
    assert lib.opfcx_context_floats(3) == 2 * 3 * 128 and lib.opfcx_context_floats(0) == 0
    p = ctypes.c_void_p(1 << 20)                                                  # never dereferenced: every call below is refused first
    good = dict(win0=p, win1=p, coarse0=p, coarse0_bstride=0, coarse1=p, coarse1_bstride=0, b_ids=p, i_ids=p, j_ids=p, K=4, B=1, L0=8, L1=8,
                W=5, wpack=p, context=p, out0=p, out1=p, stream=None)

    def refused(message, **change):
        with pytest.raises(ValueError, match=message):
            fine_context.call("opfcx_merge", *fine_context.order("opfcx_merge", **{**good, **change}))
    for name in ("win0", "win1", "coarse0", "coarse1", "b_ids", "i_ids", "j_ids", "wpack", "context", "out0", "out1"):
        refused("^opfcx_merge: opfcx_merge: null pointer$", **{name: None})
    for change in (dict(K=-1), dict(B=0), dict(L0=0), dict(L1=0)):
        refused("bad sizes", **change)
    for W in (1, 2, 4, 10, 12, 13, -3):
        refused("window: odd, from 3 to 11", W=W)
    refused("OPFCX_MAX_ROWS", K=2 ** 30 // 121 + 1, W=11)
    refused("16-byte aligned", out1=ctypes.c_void_p((1 << 20) + 4))
    for change in (dict(coarse0_bstride=-256), dict(coarse1_bstride=8 * 256 - 4), dict(B=2, coarse0_bstride=8 * 256 + 2)):
        refused("image strides", **change)


# ---- the test-side oracle ---------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("W", [5, 9])
def test_oracle_on_the_planted_pair(sd, W):
    """the precondition of the device test: K >= 40 and every confidence more than 0.05 from the threshold; without the switch's step the
    composition is ``oracle/loftr_oracle.py``'s own forward"""
    from oracle import loftr_oracle as lo
    from tests.loftr_helpers import oracle_hook

    x0, g0, x1, g1 = planted_pair((96, 128))
    cfg = config(fine_window_size=W)
    with torch.no_grad():
        ref = R.forward_from_features(sd, cfg, x0, g0, x1, g1, (96, 128))
        plain = lo.loftr_forward(sd, cfg, torch.zeros(1, 1, 96, 128), torch.zeros(1, 1, 96, 128), feature_hook=oracle_hook((x0, g0, x1, g1)))
    K = len(ref["i_ids"])
    assert K >= 40 and float((ref["mconf"] - 0.2).abs().min()) > 0.05
    assert torch.equal(ref["i_ids"], plain["i_ids"]) and torch.equal(ref["mconf"], plain["mconf"])      # the coarse path ignores the switch
    assert ref["fine_in0"].shape == (K, W * W, 128) and not torch.equal(ref["fine_f0"], plain["fine_f0"])
    assert R.row_error(ref["fine_in1"], R.reference(sd, ref["windows1"], ref["feat_c1"], ref["b_ids"], ref["j_ids"])) < 1e-5
    assert ref["expec_f"].shape == (K, 3) and torch.isfinite(ref["mkpts1_f"]).all()


# ---- the bar ---------------------------------------------------------------------------------------------------------------------------
def test_the_two_statements_agree(sd):
    for name in R.CASES:
        case = R.make_case(name)
        for a, b in zip(R.both_images(R.reference, sd, case), R.both_images(R.reference_published, sd, case)):
            assert a.dtype == torch.float64 and R.row_error(a, b) < 1e-13, name


def test_the_cases_are_the_edges():
    rows = {n: c[0] * c[0] * c[1] for n, c in R.CASES.items()}
    assert rows["w3_k7"] == 63 and rows["w3_k8"] == 72 and rows["w5_k3"] == 75 and rows["w9_k1"] == 81 and rows["w11_k1"] == 121
    assert rows["w5_k300"] > 100 * R.TILE and {c[0] for c in R.CASES.values()} == {3, 5, 9, 11}
    b3, s0, edge = R.make_case("batch3"), R.make_case("stride0"), R.make_case("edge_cells")
    assert sorted(set(b3["b_ids"].tolist())) == [0, 2] and b3["x0"].shape[0] == 3 and b3["x1"].shape[0] == 3
    assert s0["x1"].shape[0] == 1 and s0["x0"].shape[0] == 3 and sorted(set(s0["b_ids"].tolist())) == [0, 2]
    assert edge["i_ids"].tolist() == [0, 29, 0, 29] and edge["j_ids"].tolist() == [39, 0, 39, 0] and edge["b_ids"].tolist() == [0, 0, 1, 1]
    for name in R.CASES:
        c = R.make_case(name)
        assert bool((c["i_ids"] != c["j_ids"]).all()), name


def test_the_standin_figure_is_the_recorded_one(sd):
    worst = R.standin_worst(sd)
    print(f"stand-in, worst row error over the cases: {worst:.3e} (recorded {R.ROWS_STANDIN:.3e}, bar {R.ROWS_BAR:.3e})")
    assert 0.5 * R.ROWS_STANDIN <= worst <= R.ROWS_STANDIN and R.ROWS_BAR == 2 * R.ROWS_STANDIN
    # the float64 form of the stand-in: what the split alone costs, without f32 sums -- the same order of magnitude
    case = R.make_case("w5_k300")
    exact = max(R.row_error(y, r) for y, r in zip(R.both_images(R.standin, sd, case, dtype=torch.float64), R.both_images(R.reference, sd, case)))
    assert 0.25 * worst < exact <= R.ROWS_STANDIN


@pytest.mark.parametrize("fault", R.FAULTS)
def test_every_seeded_fault_lies_outside_the_bar(sd, fault):
    case = R.make_case(R.FAULT_CASE)
    ref = R.both_images(R.reference, sd, case)
    if fault == "ij":                          # i / j swapped: each image takes its context at the other image's cell
        L0, L1 = case["x0"].shape[1], case["x1"].shape[1]
        got = (R.standin(sd, case["win0"], case["x0"], case["b_ids"], case["j_ids"] % L0),
               R.standin(sd, case["win1"], case["x1"], case["b_ids"], case["i_ids"] % L1))
    else:
        got = R.both_images(R.standin, sd, case, wrong=fault)
    errors = [R.row_error(y, r) for y, r in zip(got, ref)]
    print(f"{fault}: {errors[0]:.3e} {errors[1]:.3e} against the bar {R.ROWS_BAR:.3e}")
    assert min(errors) > 100 * R.ROWS_BAR
    clean = [R.row_error(y, r) for y, r in zip(R.both_images(R.standin, sd, case), ref)]
    assert max(clean) <= R.ROWS_STANDIN
