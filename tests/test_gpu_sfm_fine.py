"""SfM fine matching over a pair list on the MI355X (run with ``-m gpu``).  The pair list is the one of
tests/sfm_fine_cases.py: five images in two size groups, seven pairs, 300 rows, scales other than one.

1. the two new kernels against what exists: ``opsff_row_ids`` against ``tests/loftr_sfm_oracle.coarse_ids`` pair by pair (ids, clipped
   keypoints, bad count and first bad row exact), ``opsff_sample_rows`` against ``ophip_sample_features`` per pair on the same maps (bit-equal);
2. batching does not change a bit: ``chunk_rows`` 64, 2^20, one that splits a pair, every pair's slice alone, and a second run;
3. the backbone's maps of an image do not depend on the batch it ran in;
4. every output equals the parent's path, one ``forward`` per pair, with ``torch.equal``;
5. errors; 6. the chain from a triangulated model to the optimiser.
Nothing is set aside anywhere.  The file fails without the feature: the module and its library do not exist."""
import copy

import numpy as np
import pytest
import torch

from onepose_st_amd import hip, loftr
from onepose_st_amd.backbone_hip import HipBackbone
from onepose_st_amd.synthetic import make_synthetic_loftr_state_dict
from tests import loftr_sfm_oracle as lsf
from tests import sfm_fine_cases as cases

pytestmark = pytest.mark.gpu

FLOAT_KEYS = ("mkpts0_c", "mkpts1_c", "mkpts0_f", "mkpts1_f", "expec_f", "feature_c0", "feature_c1", "feature0", "feature1")
PARENT_KEYS = {"mkpts0_c": "mkpts0_c", "mkpts1_c": "mkpts1_c", "mkpts0_f": "mkpts0_f", "mkpts1_f": "mkpts1_f", "expec_f": "expec_f", "i_ids": "i_ids",
               "j_ids": "j_ids", "feature_c0": "feat_coarse_b_0", "feature_c1": "feat_coarse_b_1", "feature0": "feat_ext0", "feature1": "feat_ext1"}


@pytest.fixture(scope="module")
def dev():
    assert torch.cuda.is_available(), "these tests need the MI355X"
    hip.load()
    return torch.device("cuda:0")


@pytest.fixture(scope="module")
def matchers(dev):
    lsd = make_synthetic_loftr_state_dict(0)
    out = {}
    for attention in ("linear", "full"):
        cfg = copy.deepcopy(loftr.default_cfg)
        cfg["fine"]["attention"] = attention
        m = loftr.LoFTR_for_OnePose_Plus(cfg).eval()
        m.load_state_dict(lsd, strict=True)
        out[attention] = m.to(dev)
    return out


@pytest.fixture(scope="module")
def images(dev):
    return [t.to(dev) for t in cases.images()]


@pytest.fixture(scope="module")
def bank(matchers, images, dev):
    """one bank for the whole file (the fine attention does not enter the backbone); max_batch 2: the group of three runs as 2 + 1"""
    from onepose_st_amd import sfm_fine as sf

    return sf.build_feature_bank(matchers["linear"], images, cases.scales().to(dev), max_batch=2)


def _device_pairs(dtype, dev):
    return {k: v.to(dev) for k, v in cases.pair_list(dtype).items()}


@pytest.fixture(scope="module")
def results(matchers, bank, dev):
    """``fine_match_pairs`` on the whole list, computed once per (attention, dtype) and shared (not to be written to)"""
    from onepose_st_amd import sfm_fine as sf

    cache = {}

    def get(attention, dtype):
        if (attention, dtype) not in cache:
            cache[attention, dtype] = sf.fine_match_pairs(matchers[attention], bank, _device_pairs(dtype, dev))
        return cache[attention, dtype]
    return get


def _same(a, b, label=""):
    from onepose_st_amd import sfm_fine as sf

    assert set(sf.RESULT_KEYS) <= set(a) and set(sf.RESULT_KEYS) <= set(b)
    for k in sf.RESULT_KEYS:
        assert a[k].dtype == b[k].dtype and a[k].shape == b[k].shape and torch.equal(a[k], b[k]), (label, k)


# ---- 1. the kernels -------------------------------------------------------------------------------------------------------------------
def test_bank_layout(bank, images):
    from onepose_st_amd import sfm_fine as sf

    assert bank["n_images"] == 5 and bank["bytes"] == sf.bank_bytes(cases.SIZES)
    assert [g["hw"] for g in bank["groups"]] == [(96, 128), (64, 96)] and [g["images"] for g in bank["groups"]] == [[0, 1, 3], [2, 4]]
    assert bank["image_group"].tolist() == list(cases.GROUP) and bank["image_index"].tolist() == [0, 1, 0, 2, 1]
    assert bank["image_hw"].tolist() == [list(s) for s in cases.SIZES] and bank["image_hw"].dtype == torch.int32
    assert torch.equal(bank["scales"].cpu(), cases.scales())
    for g in bank["groups"]:
        H, W = g["hw"]
        n = len(g["images"])
        assert g["fine"].shape == (n, (H // 2) * (W // 2), 128) and g["coarse"].shape == (n, (H // 8) * (W // 8), 256)
        assert g["fine"].is_contiguous() and g["coarse"].is_contiguous() and g["fine"].dtype == g["coarse"].dtype == torch.float32
        assert torch.isfinite(g["fine"]).all() and torch.isfinite(g["coarse"]).all() and float(g["fine"].abs().max()) > 0
    assert sum(g["fine"].numel() + g["coarse"].numel() for g in bank["groups"]) * 4 == bank["bytes"]


def _oracle_ids(p):
    """``coarse_ids`` pair by pair -> clipped keypoints, ids, and per row the number of its ids outside the grid"""
    sc, off = cases.scales(), p["pair_offsets"].tolist()
    k0, k1, ii, jj, bad_rows = [], [], [], [], []
    for n, (l, r, _) in enumerate(cases.PAIRS):
        a, b = off[n], off[n + 1]
        (H0, W0), (H1, W1) = cases.SIZES[l], cases.SIZES[r]
        data = {"mkpts0_c": p["mkpts0_c"][a:b].clone(), "mkpts1_c": p["mkpts1_c"][a:b].clone(), "hw0_i": (H0, W0), "hw1_i": (H1, W1),
                "hw0_c": (H0 // 8, W0 // 8), "hw1_c": (H1 // 8, W1 // 8), "scale0": sc[l:l + 1], "scale1": sc[r:r + 1]}
        _, i, j = lsf.coarse_ids(data)
        bad = ((i < 0) | (i >= (H0 // 8) * (W0 // 8))).long() + ((j < 0) | (j >= (H1 // 8) * (W1 // 8))).long()
        k0.append(data["mkpts0_c"]), k1.append(data["mkpts1_c"]), ii.append(i), jj.append(j), bad_rows.append(bad)
    return torch.cat(k0), torch.cat(k1), torch.cat(ii), torch.cat(jj), torch.cat(bad_rows)


@pytest.mark.parametrize("t0,t1", [(torch.float32, torch.float32), (torch.float64, torch.float64), (torch.float32, torch.float64)])
@pytest.mark.parametrize("planted", [False, True])
def test_row_ids_kernel_against_the_oracle_pair_by_pair(bank, dev, t0, t1, planted):
    from onepose_st_amd import sfm_fine as sf

    p = cases.pair_list(torch.float64)
    p["mkpts0_c"], p["mkpts1_c"] = p["mkpts0_c"].to(t0), p["mkpts1_c"].to(t1)
    if planted:                                   # y below image 0 (unit scale): clipped to 94, which rounds to row 12 of 12
        p["mkpts0_c"][[71, 93]] = torch.tensor([[30.0, 200.0], [126.5, 95.0]], dtype=t0)      # pair (0, 3): left image 0
        p["mkpts1_c"][[240, 250]] = torch.tensor([[5.0, 500.0], [40.0, 99.0]], dtype=t1)      # right images 0, and 1 (h factor 1.25: stays inside)
    before = (p["mkpts0_c"].clone(), p["mkpts1_c"].clone())
    d = {k: p[k].to(dev) for k in sf.PAIR_KEYS}
    m0, m1, ii, jj, ctrl = sf.row_ids(bank, d["mkpts0_c"], d["mkpts1_c"], d["row_left"], d["row_right"])
    w0, w1, wi, wj, bad = _oracle_ids(p)
    assert m0.dtype == t0 and m1.dtype == t1
    assert torch.equal(m0.cpu(), w0) and torch.equal(m1.cpu(), w1), "clipped copies"
    assert torch.equal(d["mkpts0_c"].cpu(), before[0]) and torch.equal(d["mkpts1_c"].cpu(), before[1]), "the inputs are read only"
    assert not torch.equal(w0, before[0]) and not torch.equal(w1, before[1])
    assert torch.equal(ii.cpu(), wi) and torch.equal(jj.cpu(), wj)
    nbad, first = ctrl.tolist()
    assert nbad == int(bad.sum()) == (3 if planted else 0)
    assert first == (int(torch.nonzero(bad)[0, 0]) if planted else sf.NO_ROW) and (not planted or first == 71)
    if planted:
        assert bad[71] == bad[93] == bad[240] == 1 and bad[250] == 0


def test_sampler_kernel_against_the_per_pair_sampler(bank, dev):
    """the four tables of every bucket in one launch each, against ``ophip_sample_features`` with one pair's four jobs on the same maps"""
    from onepose_st_amd import sfm_fine as sf

    for t0, t1 in ((torch.float64, torch.float32), (torch.float32, torch.float64)):
        p = cases.pair_list(torch.float64)
        g = torch.Generator().manual_seed(13)
        # the sampler's own range: the keypoints as they are, a fifth of them outside scale * (H, W)
        k0 = (p["mkpts0_c"] * 1.3 - 8 + torch.rand(300, 2, generator=g, dtype=torch.float64)).to(t0).to(dev)
        k1 = (p["mkpts1_c"] * 1.3 - 8 + torch.rand(300, 2, generator=g, dtype=torch.float64)).to(t1).to(dev)
        k0[0], k0[1] = torch.tensor([0.0, 0.0], dtype=t0), torch.tensor([127.0, 95.0], dtype=t0)          # the corners of image 0 (unit scale)
        left, right = p["row_left"].to(dev), p["row_right"].to(dev)
        outs = [torch.full((300, C), float("nan"), device=dev) for C in (256, 256, 128, 128)]
        launches = 0
        for _, _, buckets in sf.plan_chunks(300, 128, cases.bucket_keys(p)):
            for key, rows in buckets:
                consecutive = int(rows[-1]) - int(rows[0]) + 1 == len(rows)
                rows_d = None if consecutive else torch.from_numpy(rows).to(dev)
                sf.sample_rows(bank, key // 2, key % 2, k0, k1, left, right, rows_d, int(rows[0]) if consecutive else 0, len(rows), *outs)
                launches += 1
        assert launches >= 6
        off, sc = p["pair_offsets"].tolist(), bank["scales"]
        for n, (l, r, _) in enumerate(cases.PAIRS):
            a, b = off[n], off[n + 1]
            want = [torch.full((b - a, C), float("nan"), device=dev) for C in (256, 256, 128, 128)]
            jobs, keep = [], []
            for t, (img, kp, nearest) in enumerate(((l, k0, 1), (r, k1, 1), (l, k0, 0), (r, k1, 0))):
                grp = bank["groups"][cases.GROUP[img]]
                fmap = (grp["coarse"] if nearest else grp["fine"])[int(bank["image_index"][img])]
                H, W = cases.SIZES[img]
                hw = (H // 8, W // 8) if nearest else (H // 2, W // 2)
                kk, ss = kp[a:b].contiguous(), sc[img:img + 1].contiguous()
                keep += [kk, ss]
                jobs.append(hip.SampleJob(fmap.data_ptr(), kk.data_ptr(), ss.data_ptr(), want[t].data_ptr(), hw[0], hw[1], fmap.shape[1], b - a, H, W,
                                          int(kk.dtype == torch.float64), nearest))
            hip.call("ophip_sample_features", (hip.SampleJob * 4)(*jobs), 4, hip.stream_handle())
            torch.cuda.synchronize()
            for t in range(4):
                assert torch.isfinite(want[t]).all() and torch.equal(outs[t][a:b], want[t]), (n, t)
        assert (outs[0][0] == bank["groups"][0]["coarse"][0][0]).all() and (outs[2][1] == bank["groups"][0]["fine"][0][-1]).all()
        assert sum(int((o == 0).all(1).sum()) for o in outs) >= 40 and all(float(o.abs().max()) > 0 for o in outs)       # zero rows outside the maps


# ---- 2. batching ------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("attention,dtype", [("linear", torch.float64), ("full", torch.float32)])
def test_batching_does_not_change_a_bit(matchers, bank, results, dev, attention, dtype):
    from onepose_st_amd import sfm_fine as sf

    m, pairs = matchers[attention], _device_pairs(dtype, dev)
    base = results(attention, dtype)
    off = pairs["pair_offsets"].tolist()
    assert base["mkpts0_f"] is base["mkpts0_c"] and base["mkpts1_f"].dtype == dtype and base["expec_f"].shape == (300, 3)
    assert 100 not in off and 200 not in off                                  # chunk_rows 100 splits pairs
    for chunk_rows in (64, 1 << 20, 100):
        _same(sf.fine_match_pairs(m, bank, pairs, chunk_rows=chunk_rows), base, f"chunk_rows {chunk_rows}")
    _same(sf.fine_match_pairs(m, bank, pairs), base, "second run")
    parts = [sf.fine_match_pairs(m, bank, {k: pairs[k][off[n]:off[n + 1]] for k in sf.PAIR_KEYS}) for n in range(len(off) - 1)]
    _same({k: torch.cat([q[k] for q in parts]) for k in sf.RESULT_KEYS}, base, "pair by pair")
    for k in FLOAT_KEYS:
        assert torch.isfinite(base[k]).all(), k
    assert float((base["mkpts1_f"] - base["mkpts1_c"]).abs().max()) > 0


# ---- 3. the backbone's rows do not depend on the batch ----------------------------------------------------------------------------------------
@pytest.mark.parametrize("hw", [(96, 128), (64, 96)])
def test_backbone_maps_do_not_depend_on_the_batch(matchers, dev, hw):
    g = torch.Generator().manual_seed(hw[0])
    imgs = torch.rand(5, 1, *hw, generator=g).to(dev)
    Wb = matchers["linear"]._blocks(dev)["backbone"]
    bbk = HipBackbone("bf16x3")
    alone = bbk.forward(Wb, imgs[2:3].contiguous())
    first = bbk.forward(Wb, imgs[[2, 0]].contiguous())
    second = bbk.forward(Wb, imgs[[4, 2]].contiguous())
    five = bbk.forward(Wb, imgs)
    differing = []
    for name, t in (("coarse", 0), ("fine", 1)):
        for label, got in (("first of two", first[t][0]), ("second of two", second[t][1]), ("third of five", five[t][2])):
            if not torch.equal(got, alone[t][0]):
                differing.append((name, label, float((got - alone[t][0]).abs().max())))
    print("maps that differ from the image run alone:", differing)
    assert differing == []


# ---- 4. equal to the parent's path -----------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("attention,dtype", [("linear", torch.float64), ("linear", torch.float32), ("full", torch.float32)])
def test_equal_to_one_forward_per_pair(matchers, bank, results, images, dev, attention, dtype):
    m, pairs = matchers[attention], _device_pairs(dtype, dev)
    got = results(attention, dtype)
    off, sc = pairs["pair_offsets"].tolist(), bank["scales"]
    differing = []
    for n, (l, r, rows) in enumerate(cases.PAIRS):
        a, b = off[n], off[n + 1]
        data = {"image0": images[l], "image1": images[r], "scale0": sc[l:l + 1].clone(), "scale1": sc[r:r + 1].clone(),
                "mkpts0_c": pairs["mkpts0_c"][a:b].clone(), "mkpts1_c": pairs["mkpts1_c"][a:b].clone()}
        m(data, extract_coarse_feature=True, extract_fine_feature=True)            # as matchWorker calls it; clips data's keypoints in place
        for k, ref in PARENT_KEYS.items():
            assert data[ref].shape == got[k][a:b].shape and data[ref].dtype == got[k].dtype, (n, k)
            if not torch.equal(got[k][a:b], data[ref]):
                differing.append((n, k, float((got[k][a:b].double() - data[ref].double()).abs().max())))
    print("outputs that differ from the per-pair call (pair, key, max abs):", differing)
    assert differing == []
    assert [p[2] for p in cases.PAIRS].count(1) == 1 and {(cases.GROUP[p[0]], cases.GROUP[p[1]]) for p in cases.PAIRS} == {(0, 0), (0, 1), (1, 1), (1, 0)}


# ---- 5. errors ---------------------------------------------------------------------------------------------------------------------------------
def test_errors_and_the_empty_list(matchers, bank, results, dev):
    from onepose_st_amd import sfm_fine as sf

    m = matchers["linear"]
    pairs = _device_pairs(torch.float64, dev)
    before = (pairs["mkpts0_c"].clone(), pairs["mkpts1_c"].clone())
    got = sf.fine_match_pairs(m, bank, pairs, chunk_rows=128)
    _same(got, results("linear", torch.float64), "chunk_rows 128")
    assert torch.equal(pairs["mkpts0_c"], before[0]) and torch.equal(pairs["mkpts1_c"], before[1]), "the caller's tensors are unchanged"
    assert not torch.equal(got["mkpts0_c"], before[0]) and got["mkpts0_c"].data_ptr() != pairs["mkpts0_c"].data_ptr()
    # a planted keypoint outside the grid: y clipped to 94 on the unit-scale image rounds to row 12 of 12
    bad = dict(pairs, mkpts0_c=pairs["mkpts0_c"].clone(), mkpts1_c=pairs["mkpts1_c"].clone())
    bad["mkpts0_c"][71] = torch.tensor([30.0, 200.0], dtype=torch.float64)
    bad["mkpts0_c"][93] = torch.tensor([126.5, 95.0], dtype=torch.float64)
    with pytest.raises(IndexError, match=r"^2 provided coarse keypoint.*row 71 \(images 0 and 3\)"):
        sf.fine_match_pairs(m, bank, bad)
    past = dict(pairs, row_right=pairs["row_right"].clone())
    past["row_right"][120] = 5
    with pytest.raises(IndexError, match=r"row_right.*\[120\] = 5"):
        sf.fine_match_pairs(m, bank, past)
    with pytest.raises(hip.HipLibraryError):
        sf.fine_match_pairs(m, bank, {k: v.cpu() for k, v in pairs.items()})
    m.feature_hook = lambda *a: a
    try:
        with pytest.raises(NotImplementedError):
            sf.fine_match_pairs(m, bank, pairs)
        with pytest.raises(NotImplementedError):
            sf.build_feature_bank(m, [torch.zeros(1, 1, 64, 96, device=dev)])
    finally:
        m.feature_hook = None
    with pytest.raises(ValueError, match="max_bytes"):
        sf.build_feature_bank(m, [torch.zeros(1, 1, 64, 96, device=dev)], max_bytes=sf.bank_bytes([(64, 96)]) - 1)
    for dtype in (torch.float32, torch.float64):
        empty = sf.fine_match_pairs(m, bank, {k: v[:0] for k, v in _device_pairs(dtype, dev).items()})
        assert set(empty) == set(sf.RESULT_KEYS)
        for k, shape, dt in (("mkpts0_c", (0, 2), dtype), ("mkpts1_c", (0, 2), dtype), ("mkpts0_f", (0, 2), dtype), ("mkpts1_f", (0, 2), dtype),
                             ("expec_f", (0, 3), torch.float32), ("i_ids", (0,), torch.int64), ("j_ids", (0,), torch.int64),
                             ("feature_c0", (0, 256), torch.float32), ("feature_c1", (0, 256), torch.float32), ("feature0", (0, 128), torch.float32),
                             ("feature1", (0, 128), torch.float32)):
            assert tuple(empty[k].shape) == shape and empty[k].dtype == dt and empty[k].is_cuda, k


# ---- 6. the chain ------------------------------------------------------------------------------------------------------------------------------
def test_chain_from_the_triangulated_model_to_the_optimiser(matchers, dev):
    from onepose_st_amd import postopt, sfm_fine as sf, sfm_tracks as st, sfm_triangulate as tri
    from tests.sfm_triangulate_scenes import scene

    s = scene("small")
    to_dev = lambda d: {k: torch.from_numpy(np.ascontiguousarray(v)).to(dev) for k, v in d.items()}      # noqa: E731
    model = tri.triangulate(to_dev(s["merged"]), to_dev(s["cameras"]))
    plan = st.assign_tracks(model)
    pairs = st.matching_pairs(plan, model)
    I, M = model["image_ids"].numel(), pairs["mkpts0_idx"].numel()
    g = torch.Generator().manual_seed(41)
    imgs = torch.rand(I, 1, 480, 640, generator=g).to(dev)                     # the scenes' image size
    scales = torch.tensor([[1.25, 1.1]]).repeat(I, 1).to(dev)                  # h factor 1.25: no keypoint rounds past the last row of cells
    m = matchers["linear"]
    bank = sf.build_feature_bank(m, imgs, scales, max_batch=4)
    assert len(bank["groups"]) == 1 and bank["bytes"] == sf.bank_bytes([(480, 640)] * I)
    res = sf.fine_match_pairs(m, bank, pairs, chunk_rows=100)
    assert M > 100 and res["mkpts1_f"].shape == (M, 2) and res["mkpts1_f"].dtype == torch.float64
    for k in FLOAT_KEYS:
        assert torch.isfinite(res[k]).all(), k
    assert float((res["mkpts1_f"] - res["mkpts1_c"]).abs().max()) <= 4 * 2 * 1.25 + 1e-9      # inside the 9 x 9 window: 4 fine px of 2 image px, scaled
    rows = st.optimisation_rows(plan, model, pairs)
    agg, poses = st.to_optimizer_inputs(plan, model, pairs, rows, res["mkpts1_f"])
    R = rows["fine_row"].numel()
    assert agg["mkpts1_f"].shape == (R, 2) and torch.equal(agg["mkpts1_f"], res["mkpts1_f"][rows["fine_row"]])
    tracks = st.to_aggregation_inputs(plan, rows, res["feature_c0"], res["feature_c1"], res["feature0"], res["feature1"])
    assert tuple(tracks) == st.TRACK_KEYS and tracks["feature_c1"].shape == (R, 256) and tracks["feature0"].shape == (R, 128)
    cfgs = {"solver_type": "FirstOrder", "residual_mode": "geometry_error", "optimize_lr": {"depth": 3e-2}, "optim_procedure": ["depth"]}
    out = postopt.Optimizer(cfgs).start_optimize(agg, poses)
    assert out is not None
    ref = sf.to_reference_outputs(res, pairs, model, scales)
    names = st.to_reference_outputs(pairs, model)
    assert list(ref) == list(names) and len(ref) == pairs["pair_left"].numel()
    for name, entry in ref.items():
        n = len(names[name]["mkpts0_idx"])
        assert tuple(entry) == sf.REFERENCE_KEYS and len(entry) == 11
        assert np.array_equal(entry["mkpts0_idx"], names[name]["mkpts0_idx"])
        for k, width in (("mkpts0_c", 2), ("mkpts1_c", 2), ("mkpts0_f", 2), ("mkpts1_f", 2), ("feature_c0", 256), ("feature_c1", 256),
                         ("feature0", 128), ("feature1", 128)):
            assert isinstance(entry[k], np.ndarray) and entry[k].shape == (n, width), (name, k)
        assert entry["scale0"].shape == entry["scale1"].shape == (1, 2) and entry["scale0"].tolist() == [[1.25, 1.100000023841858]]
