"""CPU side of the SfM object block: the oracle's two forms agree, a hand-worked case, the input checks, the
header / binding, and that the GPU tests' inputs tell every seeded fault from the truth."""
import os

import numpy as np
import pytest
import torch

from onepose_st_amd import cabi, hip
from tests import sfm_objectblock_oracle as orc

REPO = os.path.abspath(os.path.join(os.path.dirname(__file__), ".."))
TRACK_KEYS = ("assigned_image", "assigned_kpt", "row_offsets", "ref_image", "ref_kpt", "feature_c0", "feature_c1", "feature0", "feature1")


def _same(a, b):
    a, b = np.asarray(a), np.asarray(b)
    return a.shape == b.shape and a.dtype == b.dtype and a.tobytes() == b.tobytes()


def test_product_module_exists_and_keeps_to_itself():
    import onepose_st_amd.sfm_objectblock as sob

    src = open(sob.__file__).read()
    assert "import oracle" not in src and "from tests" not in src and "from oracle" not in src


def test_hand_case():
    """What the hand case (``oracle.hand_case``) must give, worked by hand."""
    case = orc.hand_case()
    assert orc.check_conditions(case) == 0
    r = orc.reference_form(case)
    # stage A.  slot 4 = (1, 0): track 0's row 0 wrote feature_c1[0], then track 1's query -- the later writer -- the mean of its one row
    assert _same(r["desc_coarse"][4], case["feature_c0"][3]) and _same(r["desc_fine"][4], case["feature0"][3])
    # slot 8 = (2, 1): track 1's row, then track 2's row 4 wins
    assert _same(r["desc_coarse"][8], case["feature_c1"][4])
    # slot 0: track 0's query, column 0 = ((1 + 2^24) - 2^24) / 3 = 0 in float32 row order (1/3 in the reverse order)
    assert r["desc_coarse"][0, 0] == 0.0 and r["desc_fine"][0, 0] == 0.0
    assert r["desc_coarse"][0, 1] == np.float32(np.float32(np.float32(case["feature_c0"][0, 1] + case["feature_c0"][1, 1]) + case["feature_c0"][2, 1]) / np.float32(3))
    assert r["scores_cleared"].tolist() == [True, True, False, False, True] + [False] * 7
    assert not r["desc_coarse"][[2, 3, 5, 9, 11]].any()                    # nothing writes them
    # stage B.  id 18 is outside the box; lengths {2: 3 points, 3: 5 points}, thres = min(8, 5) = 5: after length 2 the rest is 5 <= 5, so
    # track_length = 2 and all 8 stay: more than max_num_kp3d
    assert (r["after_bbox"], r["track_length"], r["after_track_length"]) == (8, 2, 8) and case["max_num_kp3d"] == 5
    # by id: 10 | 11 + 12 (7e-4 apart) | 12: recorded, skipped | 13: 12 is recorded -> skipped, and in no group: dropped | 14 + 15 | 16 | 17
    assert r["group_members"].tolist() == [10, 11, 12, 14, 15, 16, 17] and r["group_offsets"].tolist() == [0, 1, 3, 5, 6, 7]
    assert _same(r["keypoints3d"][1], np.array([(0.2 + 0.2007) / 2, (0.2 + 0.2) / 2, (0.2 + 0.2) / 2]))
    assert _same(r["keypoints3d"][2], np.array([(0.7003 + 0.7) / 2, 0.7, 0.7]))      # id 14 is the point at 0.7003
    # stage C.  new point 1 = ids 11, 12: observations slots 7, 10 (id 11), then 6 (id 12): (1 + 2^54) - 2^54 = 0 in float64
    assert r["descriptors3d_coarse"][1, 0] == 0.0 and r["descriptors3d_fine"][1, 0] == 0.0
    assert r["descriptors3d_coarse"][1, 1] == ((float(case["feature_c1"][1, 1]) + float(case["feature_c1"][2, 1])) + float(case["feature_c1"][5, 1])) / 3
    assert r["scores3d"].shape == (5, 1) and (r["scores3d"] == 1).all()
    v = orc.vectorised_form(case)
    for k in r:
        assert _same(r[k], v[k]), k
    assert v["written"].tolist() == [True, True, False, False, True, False, True, True, True, False, True, False]


def test_oracle_equals_the_reference_golden(golden_dir):
    """both forms of the oracle against what the reference's own functions gave (tests/golden/make_golden_sfm_objectblock.py)"""
    npz = np.load(os.path.join(golden_dir, "sfm_objectblock_small.npz"))
    case = orc.golden_case(npz)
    assert orc.check_conditions(case) == 0
    assert orc.golden_mismatches(npz, orc.reference_form(case)) == []
    v = orc.vectorised_form(case)
    assert orc.golden_mismatches(npz, v) == []
    assert np.array_equal(v["written"] & v["desc_coarse"].any(axis=1), npz["desc_coarse_written"])
    for f in ("reverse_mean", "first_writer", "keep_dropped", "float32_group_mean"):
        assert orc.golden_mismatches(npz, orc.vectorised_form(case, fault=f)) != [], f


@pytest.mark.parametrize("seed,kw", [(5, dict(n_close=12, n_chains=5, cluster=8, collisions=40)), (6, dict(n_close=20, n_chains=9, cluster=5, box=False)),
                                     (7, dict(n_close=0, n_chains=0, collisions=80))])
def test_vectorised_form_equals_reference_form(seed, kw):
    case = orc.make_case(seed, 300, 12, 6, 150, **kw)
    assert orc.check_conditions(case) == 0
    r, v = orc.reference_form(case), orc.vectorised_form(case)
    for k in r:
        assert _same(r[k], v[k]), k


def test_float32_mean_is_a_running_sum():
    """np.mean over axis 0 of a float32 stack = running float32 sum in row order, one division: no pairwise summation on this axis"""
    rng = np.random.default_rng(0)
    for n in (1, 2, 7, 8, 9, 64, 129):
        x = (rng.standard_normal((n, 256)) * np.exp2(rng.integers(-8, 9, (n, 1)))).astype(np.float32)
        assert _same(np.mean(x, axis=0), orc._seq_mean(x, np.float32))
        assert _same(np.mean(x.astype(np.float64), axis=0, keepdims=True)[0], orc._seq_mean(x, np.float64))


def test_pinned_distance_is_pdist():
    from scipy.spatial.distance import pdist

    x = np.random.default_rng(1).random((200, 3)) * 1e-2
    i, j = np.triu_indices(200, 1)
    d = x[i] - x[j]
    assert _same(pdist(x, "euclidean"), np.sqrt((d[:, 0] * d[:, 0] + d[:, 1] * d[:, 1]) + d[:, 2] * d[:, 2]))


def test_inputs_discriminate_faults():
    """every seeded fault of tests/test_gpu_sfm_objectblock.py changes the oracle's answer on that file's inputs"""
    hand = orc.hand_case()
    seeded = orc.make_case(5, 300, 12, 6, 150, n_close=12, n_chains=5, cluster=8, collisions=40)
    for case, faults in ((hand, orc.FAULTS), (seeded, ("reverse_mean", "first_writer", "keep_dropped", "float32_group_mean"))):
        truth = orc.vectorised_form(case)
        for f in faults:
            bad = orc.vectorised_form(case, fault=f)
            assert any(not _same(truth[k], bad[k]) for k in truth), f


def _tensors(case):
    return {k: torch.from_numpy(np.ascontiguousarray(v)) for k, v in case.items() if isinstance(v, np.ndarray)}


def test_input_checks():
    from onepose_st_amd import sfm_objectblock as sob

    t = _tensors(orc.hand_case())
    A = [t[k] for k in TRACK_KEYS] + [t["kpt_offsets"]]
    assert sob.check_track_inputs(*A) == (3, 6, 4, 12)
    with pytest.raises(hip.HipLibraryError):
        sob.aggregate_track_features(*A)
    with pytest.raises(hip.HipLibraryError):
        sob.select_points(t["point_ids"], t["xyz"], t["track_len"], t["bbox_corners"], 5)
    with pytest.raises(hip.HipLibraryError):
        sob.average_point_features(t["point3D_ids"], torch.zeros(12, 256), torch.tensor([0, 1]), torch.tensor([10]))
    with pytest.raises(NotImplementedError):
        sob.aggregate_track_features(*A, aggregation_method="max")
    with pytest.raises(NotImplementedError):
        sob.aggregate_track_features(*A, keypoints_update_method="fine_match_keypoints")

    def track(**kw):
        return [kw.get(k, t[k]) for k in TRACK_KEYS] + [kw.get("kpt_offsets", t["kpt_offsets"])]

    with pytest.raises(ValueError):
        sob.check_track_inputs(*track(feature_c0=t["feature_c0"].double()))
    with pytest.raises(ValueError):
        sob.check_track_inputs(*track(feature1=t["feature1"][:, :64]))
    with pytest.raises(ValueError):
        sob.check_track_inputs(*track(row_offsets=torch.tensor([0, 3, 3, 6])))          # a track without rows
    with pytest.raises(ValueError):
        sob.check_track_inputs(*track(row_offsets=torch.tensor([0, 3, 4, 5])))
    with pytest.raises(ValueError):
        sob.check_track_inputs(*track(kpt_offsets=torch.tensor([0, 4, 3, 10, 12])))
    with pytest.raises(IndexError):
        sob.check_track_inputs(*track(ref_image=torch.tensor([1, 2, 4, 2, 2, 1])))
    with pytest.raises(IndexError):
        sob.check_track_inputs(*track(ref_kpt=torch.tensor([0, 0, 2, 1, 1, 2])))      # image 3 has 2 keypoints
    with pytest.raises(IndexError):
        sob.check_track_inputs(*track(assigned_kpt=torch.tensor([0, -1, 1])))

    B = (t["point_ids"], t["xyz"], t["track_len"], t["bbox_corners"], 5, 1e-3)
    assert sob.check_point_inputs(*B) == 9
    bad_xyz = t["xyz"].clone()
    bad_xyz[0, 0] = float("nan")
    for args in ((t["point_ids"], t["xyz"].float(), *B[2:]), (t["point_ids"], bad_xyz, *B[2:]), (t["point_ids"][:5], *B[1:]),
                 (torch.tensor([10, 11, 12, 13, 15, 14, 16, 17, 10]), *B[1:]), (*B[:3], t["bbox_corners"][:4], 5, 1e-3), (*B[:4], 0, 1e-3),
                 (*B[:5], 0.0), (*B[:2], -t["track_len"], *B[3:]), (t["point_ids"] - 11, *B[1:])):
        with pytest.raises(ValueError):
            sob.check_point_inputs(*args)
    assert sob.pair_chunks(15000) == (512, 30) and sob.pair_chunks(100) == (512, 1)
    chunk_len, n = sob.pair_chunks(10 ** 6)
    assert n <= sob.PAIR_MAX_CHUNKS and chunk_len * n >= 10 ** 6 and chunk_len % sob.PAIR_TILE == 0


def test_header_and_binding():
    from onepose_st_amd import sfm_objectblock as sob

    header = cabi.parse(open(os.path.join(REPO, "include", "onepose_sfm.h")).read())
    assert header.defines["OPSFM_ABI_VERSION"] == sob.ABI_VERSION == 1
    with pytest.raises(TypeError, match="takes 5 arguments"):
        sob.check_arity("opsfm_box_test", (1, 2, 3, 4))
    with pytest.raises(TypeError):
        sob.check_arity("opsfm_point_mean", tuple(range(9)))
    # the frame path's header is not the place of these entry points
    assert "opsfm_" not in open(os.path.join(REPO, "include", "onepose_hip.h")).read()


def test_built_library_exports_every_prototype():
    from onepose_st_amd import sfm_objectblock as sob

    assert os.path.exists(sob.library_path()), "libonepose_sfm.so: run __graft_entry__.build()"
    assert sob.load().opsfm_workspace_bytes(1000, 10) >= 4000
