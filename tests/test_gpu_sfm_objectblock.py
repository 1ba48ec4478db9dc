"""``onepose_st_amd/sfm_objectblock.py`` on the MI355X against ``tests/sfm_objectblock_oracle.py``, bit for bit: float64 and float32 are
compared as integer bit patterns, ids, offsets and counts exactly.  Nothing is set aside: every case first asserts on the CPU that no
pair distance lies within 1e-6 relative of the merge threshold and no box value within 1e-9 relative of 0 or v.v
(``oracle.check_conditions``), so the share of excluded points and pairs is 0.

The file fails without the feature (the module does not exist).  Seeded faults: each was built as a variant of the device library
(loaded through ``OPSFM_LIB``) or, for the one that lives in the Python module, patched there, and this file was run against it on the
MI355X.  Tests that failed (of 9; the clean build passes all 9):

* the means summed in reverse order (``mean_rows_f32`` and ``point_mean_kernel`` walk their rows backwards): hand, seeded, golden,
  long_track, realistic, kept_count_above_20000, block_joins_the_product_path
* first writer wins instead of last (``agg_winner_kernel`` keeps the minimum ordinal): hand, seeded, golden, long_track, realistic
* the track-length cut of ``select_points`` stops at ``rest < thres`` instead of the reference's ``rest <= thres`` (``get_tkl``): hand
  (track_length 3 instead of 2); the only case whose rest meets the threshold exactly
* a dropped point kept as a group (``merge_resolve_kernel`` accepts a skipped point that nobody recorded): hand, seeded, golden,
  long_track, realistic, kept_count_above_20000, new_point_without_observation, block_joins_the_product_path
* the group mean taken in float32 (``group_emit_kernel`` sums in float): hand, seeded, golden, long_track, realistic,
  kept_count_above_20000

``tests/test_sfm_objectblock_cpu.py`` shows on the CPU that the oracle with each fault differs from the oracle on the hand, seeded and
golden inputs.
"""
import numpy as np
import pytest
import torch

from tests import sfm_objectblock_oracle as orc

pytestmark = pytest.mark.gpu

TRACK_KEYS = ("assigned_image", "assigned_kpt", "row_offsets", "ref_image", "ref_kpt", "feature_c0", "feature_c1", "feature0", "feature1")
COMPARED = ("desc_coarse", "desc_fine", "written", "scores_cleared", "keypoints3d", "group_offsets", "group_members", "descriptors3d_coarse",
            "descriptors3d_fine", "scores3d")


def _bits(a):
    a = np.ascontiguousarray(a)
    return a.view({4: np.int32, 8: np.int64}[a.itemsize]) if a.dtype.kind == "f" else a


def run_device(case, dev="cuda:0"):
    from onepose_st_amd import sfm_objectblock as sob

    t = {k: torch.from_numpy(np.ascontiguousarray(v)).to(dev) for k, v in case.items() if isinstance(v, np.ndarray)}
    res = sob.build_object_block({k: t[k] for k in TRACK_KEYS}, {k: t[k] for k in ("point_ids", "xyz", "track_len")}, t["point3D_ids"],
                                 t["kpt_offsets"], bbox_corners=t.get("bbox_corners"), max_num_kp3d=case["max_num_kp3d"])
    torch.cuda.synchronize()
    out = {k: res[k].cpu().numpy() for k in COMPARED if k in res}
    out.update({k: res["features"][k].cpu().numpy() for k in ("desc_coarse", "desc_fine", "written", "scores_cleared")})
    out.update(track_length=res["track_length"], after_bbox=res["counts"]["after_bbox"], after_track_length=res["counts"]["after_track_length"])
    return out, res


def check(case, want=None):
    assert orc.check_conditions(case) == 0                                 # nothing set aside
    want = orc.vectorised_form(case) if want is None else want
    got, res = run_device(case)
    for k in ("track_length", "after_bbox", "after_track_length"):
        print(k, got[k], want[k])
        assert got[k] == want[k], k
    for k in COMPARED:
        g, w = np.asarray(got[k]), np.asarray(want[k])
        assert g.shape == w.shape and g.dtype == w.dtype, (k, g.shape, w.shape, g.dtype, w.dtype)
        diff = int((_bits(g) != _bits(w)).sum())
        print(k, g.shape, "differing elements:", diff)
        assert diff == 0, k
    return got, res


def test_hand_case():
    case = orc.hand_case()
    got, _ = check(case, orc.reference_form(case) | {"written": orc.vectorised_form(case)["written"]})
    assert got["track_length"] == 2 and got["after_track_length"] == 8 > case["max_num_kp3d"]
    assert got["group_members"].tolist() == [10, 11, 12, 14, 15, 16, 17]        # 13 is dropped


def test_seeded_small_case_and_repeat():
    case = orc.make_case(5, 300, 12, 6, 150, n_close=12, n_chains=5, cluster=8, collisions=40)
    got, _ = check(case, orc.reference_form(case) | {"written": orc.vectorised_form(case)["written"]})
    again, _ = run_device(case)
    for k in COMPARED:
        assert np.array_equal(_bits(got[k]), _bits(again[k])), k


def test_golden_case(golden_dir):
    """the device against what the reference's own functions gave (tests/golden/sfm_objectblock_small.npz)"""
    import os

    npz = np.load(os.path.join(golden_dir, "sfm_objectblock_small.npz"))
    case = orc.golden_case(npz)
    assert orc.check_conditions(case) == 0
    got, _ = run_device(case)
    bad = orc.golden_mismatches(npz, got)
    print("keys differing from the reference golden:", bad)
    assert bad == []


def test_long_track():
    case = orc.make_case(9, 400, 12, 5, 10 ** 6, n_close=8, n_chains=3, collisions=30, long_track=1300)
    assert np.diff(case["row_offsets"]).max() > 1000
    check(case)


def test_realistic_case():
    """the reference's working size: ~60 000 points before filtering, max_num_kp3d 15 000, 150 images, mean track length ~20"""
    case = orc.make_case(21, 57000, 150, 20, 15000, n_close=2500, n_chains=400, cluster=70, collisions=3000)
    got, _ = check(case)
    n0, n = got["after_track_length"], len(got["keypoints3d"])
    print("points", len(case["xyz"]), "kept", n0, "merged", n, "members", len(got["group_members"]))
    assert np.diff(got["group_offsets"]).max() >= 64 and len(got["group_members"]) < n0      # a big cluster, and dropped points


def test_kept_count_above_20000():
    case = orc.make_case(33, 23000, 40, 4, 10 ** 6, n_close=600, n_chains=100, cluster=0, box=False)
    got, _ = check(case)
    assert got["after_track_length"] > 20000


def test_box_that_rejects_everything():
    from onepose_st_amd import sfm_objectblock as sob

    case = orc.hand_case()
    t = {k: torch.from_numpy(case[k]).cuda() for k in ("point_ids", "xyz", "track_len")}
    with pytest.raises(ValueError, match="rejects every point"):
        sob.select_points(t["point_ids"], t["xyz"], t["track_len"], torch.from_numpy(case["bbox_corners"] + 100.0).cuda(), 5)


def test_new_point_without_observation():
    from onepose_st_amd import sfm_objectblock as sob

    case = orc.hand_case()
    case["point3D_ids"][[3, 8]] = -1                                       # nobody sees ids 14, 15 any more
    with pytest.raises(ValueError, match="no observation"):
        run_device(case)


def test_block_joins_the_product_path(cfg, sd):
    """build_object_block -> to_model_inputs -> OnePosePlus_model.forward_features with a planted query (synthetic's recipe: the query's
    coarse features are the block's encoded descriptors plus noise, at cells of their own): K > 0 and the indices of the CPU oracle on
    the same block."""
    from onepose_st_amd import host_math, sfm_objectblock as sob
    from onepose_st_amd.model import OnePosePlus_model
    from oracle import onepose_oracle

    case = orc.make_case(41, 500, 12, 6, 10 ** 6, n_close=10, n_chains=4, box=False, extent=0.2)
    for k in ("feature_c0", "feature_c1", "feature0", "feature1"):
        case[k] = np.random.default_rng(3).standard_normal(case[k].shape).astype(np.float32)
    _, res = run_device(case)
    block = {k: v.cpu() for k, v in sob.to_model_inputs(res).items()}
    want = orc.vectorised_form(case)
    assert np.array_equal(block["descriptors3d_coarse_db"][0].numpy(), want["descriptors3d_coarse"].astype(np.float32).T)
    N = block["keypoints3d"].shape[1]
    H, W = 96, 136
    hc, wc, C, Cf = H // 8, W // 8, 256, 128
    g = torch.Generator().manual_seed(7)
    n_plant = 120
    pi = torch.randperm(N, generator=g)[:n_plant]
    pj = torch.randperm(hc * wc, generator=g)[:n_plant]
    kn = host_math.normalize_keypoints3d(block["keypoints3d"])
    enc3d = block["descriptors3d_coarse_db"] + host_math.keypoint_mlp(sd, kn).transpose(1, 2)
    q2d = torch.randn(hc * wc, C, generator=g)
    q2d[pj] = enc3d[0, :, pi].T + 0.1 * torch.randn(n_plant, C, generator=g)
    feat_c = (q2d.T.reshape(C, hc, wc) - host_math.sinusoid_table(C, hc, wc))[None].contiguous()
    feat_f = torch.randn(1, Cf, H // 2, W // 2, generator=g)
    feat_f[0, :, 4 * (pj // wc), 4 * (pj % wc)] = block["descriptors3d_db"][0, :, pi] + 0.1 * torch.randn(Cf, n_plant, generator=g)
    model = OnePosePlus_model(cfg).eval()
    model.load_state_dict(sd, strict=True)
    model.to("cuda:0")
    data = {k: v.cuda() for k, v in block.items()}
    model.forward_features(data, feat_c.cuda(), feat_f.cuda(), (H, W))
    with torch.no_grad():
        ref = onepose_oracle.forward_from_features(sd, cfg, block, feat_c, feat_f, (H, W))
    K = len(ref["i_ids"])
    print("matches", K)
    assert K > 0
    assert torch.equal(data["i_ids"].cpu(), ref["i_ids"]) and torch.equal(data["j_ids"].cpu(), ref["j_ids"])
