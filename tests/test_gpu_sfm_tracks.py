"""``onepose_st_amd/sfm_tracks.py`` on the MI355X against ``tests/sfm_tracks_oracle.py``: every integer output exact, the copies of
``xys`` bit-equal, nothing set aside (``EXCLUDED`` counts what a comparison leaves out; it stays 0 and every test asserts it).  The one
float result that is not pinned bit for bit is the initial depth (numpy's matmul goes through BLAS): per slot
``|got - want| <= 8 * 2^-52 * (|K| (|R| |X| + |t|))_z`` (``oracle.depth_bound``: the forward error of the arithmetic, not a measured
number), the ``-1`` fill exact.  ``update_model`` is held to the 1e-10 of ``tests/test_gpu_postopt.py``'s test of the two functions it
composes, the optimiser chain to that file's ``rel < 1e-6``.

The file fails without the feature (the module and its library do not exist).  Seeded faults: each is a variant of the device library
(``EXTRA=-DOPSFT_FAULT_... tools/build_variant.sh <name> - sfm_tracks``, loaded through ``OPSFT_LIB``).  Tests that each fault must fail: the list is derived on the CPU, where
``tests/test_sfm_tracks_cpu.py::test_inputs_discriminate_faults`` shows that the oracle with the same fault differs on these inputs:

* ties resolved by the initial order instead of the carried order (``OPSFT_FAULT_TIE_INITIAL_ORDER``, ``select_kernel``): carried_order_tie,
  long_track
* first write wins for a duplicate keypoint (``OPSFT_FAULT_FIRST_KEYPOINT_WINS``, ``take_kernel``): hand, golden, duplicates,
  shuffled_ids_and_idle_images, long_track
* right images ordered by index instead of id (``OPSFT_FAULT_RIGHT_BY_INDEX``, ``pair_keys_kernel``): hand, golden,
  shuffled_ids_and_idle_images (the cases whose id order differs from the index order)
* last occurrence instead of first for a repeated image in a track (``OPSFT_FAULT_LAST_OCCURRENCE``, ``track_rows_kernel``): hand, golden,
  duplicates, shuffled_ids_and_idle_images, long_track
* a robbed slot of a keyframe treated as owned (``OPSFT_FAULT_ROBBED_IS_OWNED``, ``take_kernel``): every comparing test
"""
import os

import numpy as np
import pytest
import torch

from tests import sfm_tracks_oracle as orc

pytestmark = pytest.mark.gpu

EXACT = ("keyframes", "state", "is_keyframe", "assigned_image", "assigned_kpt", "pair_left", "pair_right", "pair_offsets", "mkpts0_idx",
         "fine_row", "ref_image", "ref_kpt", "n_query", "row_offsets")
BITS = ("mkpts0_c", "mkpts1_c")
EXCLUDED = 0                                                               # items any comparison below sets aside


def to_device(m, dev="cuda:0"):
    return {k: torch.from_numpy(np.ascontiguousarray(v)).to(dev) for k, v in m.items()}


def run_device(m):
    from onepose_st_amd import sfm_tracks as st

    model = to_device(m)
    plan = st.assign_tracks(model)
    pairs = st.matching_pairs(plan, model)
    rows = st.optimisation_rows(plan, model, pairs)
    torch.cuda.synchronize()
    out = {k: plan[k].cpu().numpy() for k in st.PLAN_KEYS}
    out.update({k: pairs[k].cpu().numpy() for k in st.PAIR_KEYS})
    out.update({k: rows[k].cpu().numpy() for k in st.ROW_KEYS})
    return out, (model, plan, pairs, rows)


def compare(m, got, want):
    for k in EXACT:
        g, w = np.asarray(got[k]), np.asarray(want[k])
        assert g.shape == w.shape and g.dtype == w.dtype, (k, g.shape, w.shape, g.dtype, w.dtype)
        diff = int((g != w).sum())
        print(k, g.shape, "differing elements:", diff)
        assert diff == 0, k
    for k in BITS:
        g, w = np.ascontiguousarray(got[k]), np.ascontiguousarray(want[k])
        assert g.shape == w.shape and g.dtype == w.dtype == np.float64, k
        diff = int((g.view(np.int64) != w.view(np.int64)).sum())
        print(k, g.shape, "differing bit patterns:", diff)
        assert diff == 0, k
    g, w = got["initial_depth"], want["initial_depth"]
    bound = orc.depth_bound(m, want["state"])
    err = np.abs(g - w)
    occ = want["state"] >= 0
    print("initial_depth: occupied", int(occ.sum()), "max |err|", err.max(), "max err / bound", (err[occ] / bound[occ]).max() if occ.any() else 0.0)
    assert np.array_equal(g[~occ], w[~occ]) and (w[~occ] == -1).all()      # the fill is exact
    assert (err <= bound).all()
    print("excluded items:", EXCLUDED)
    assert EXCLUDED == 0


def check(m, want=None):
    want = orc.vectorised_form(m) if want is None else want
    got, handles = run_device(m)
    compare(m, got, want)
    return got, handles


def test_hand_case():
    m = orc.hand_case()
    got, _ = check(m, orc.reference_form(m))
    assert got["keyframes"].tolist() == [1, 0] and got["assigned_kpt"].tolist() == [0, 1, 3, 2, 3]
    assert got["pair_right"].tolist() == [2, 3, 2, 0, 3] and got["fine_row"].tolist() == [2, 4, 0, 1, 6, 3]


def test_golden_case(golden_dir):
    """the device against what the reference's own classes gave (tests/golden/sfm_tracks_small.npz)"""
    npz = np.load(os.path.join(golden_dir, "sfm_tracks_small.npz"))
    m = orc.golden_model(npz)
    got, (model, plan, pairs, rows) = check(m, orc.reference_form(m))
    from tests.test_sfm_tracks_cpu import golden_mismatches
    from onepose_st_amd import sfm_tracks as st

    agg, poses = st.to_optimizer_inputs(plan, model, pairs, rows, torch.from_numpy(npz["mkpts1_f"]).cuda())
    bad = golden_mismatches(npz, m, got, {k: v.cpu().numpy() for k, v in agg.items()})
    print("keys differing from the reference golden:", bad)
    assert bad == [] and list(poses) == m["image_ids"].tolist()


def test_carried_order_tie():
    m = orc.tie_case()
    got, _ = check(m, orc.reference_form(m))
    assert got["keyframes"].tolist() == [2, 1, 0]                    # the initial order would take image 0 second


def test_duplicates():
    """points seen twice in their keyframe (both slots owned, the later keypoint assigned) and twice in another image"""
    m = orc.make_model(13, 300, 10, 5, n_dup=60)
    want = orc.reference_form(m)
    ids, cnt = np.unique(want["state"][want["state"] >= 0], return_counts=True)
    assert (cnt == 2).sum() >= 5, "no point owns two slots of its keyframe"
    assert (want["n_query"] < np.diff(m["track_offsets"]) - 1).sum() >= 5
    check(m, want)
    check(m)


def test_shuffled_ids_and_idle_images():
    """id order differs from index order; one image has no registered keypoint, some are never keyframes"""
    m = orc.make_model(5, 300, 12, 6, n_dup=25, shuffle_ids=True, empty_images=(4,))
    assert (np.diff(m["image_ids"]) < 0).any()
    want = orc.reference_form(m)
    assert not want["is_keyframe"][4] and (~want["is_keyframe"]).sum() >= 2 and (m["point3D_ids"][m["kpt_offsets"][4]:m["kpt_offsets"][5]] == -1).all()
    check(m, want)


def test_long_track():
    m = orc.make_model(9, 200, 12, 5, n_dup=10, long_track=1300)
    assert np.diff(m["track_offsets"]).max() == 1300
    check(m, orc.reference_form(m))


def test_realistic_case_and_repeat():
    """60 000 points, 150 images, mean track 20 (1.2 M elements) against the vectorised oracle; a second run is bit-identical"""
    m = orc.make_model(21, 60000, 150, 20, n_dup=500, shuffle_ids=True)
    got, _ = check(m)
    print("elements", len(m["track_image"]), "slots", len(m["point3D_ids"]), "keyframes", len(got["keyframes"]), "pair rows", len(got["mkpts0_idx"]))
    again, _ = run_device(m)
    for k in got:
        assert got[k].tobytes() == again[k].tobytes(), k


def test_optimizer_chain():
    """to_optimizer_inputs -> Optimizer.start_optimize reproduces postopt's own oracle on the oracle's rows"""
    from onepose_st_amd import postopt, sfm_tracks as st
    from tests import postopt_oracle as po

    m = orc.with_projected_keypoints(orc.make_model(31, 200, 8, 5, n_dup=10, shuffle_ids=True), noise=0.3)
    got, (model, plan, pairs, rows) = check(m)
    want = orc.vectorised_form(m)
    mk1f = want["mkpts1_c"] + 0.5 * np.random.default_rng(2).standard_normal(want["mkpts1_c"].shape)
    agg, poses = st.to_optimizer_inputs(plan, model, pairs, rows, torch.from_numpy(mk1f).cuda())
    ref = orc.optimizer_inputs(m, want, mk1f)
    for k, w in ref.items():
        g = agg[k].cpu().numpy()
        if k == "depth":
            assert g.shape == w.shape and np.abs(g - w).max() <= orc.depth_bound(m, want["state"]).max(), k
        else:
            assert g.shape == w.shape and g.tobytes() == w.astype(g.dtype).tobytes(), k
    cfgs = {"solver_type": "FirstOrder", "residual_mode": "geometry_error", "optimize_lr": {"depth": 3e-2}, "optim_procedure": ["depth"]}
    res = postopt.Optimizer(cfgs).start_optimize(agg, poses)
    ids = m["image_ids"].tolist()
    aa = torch.from_numpy(np.concatenate([postopt.convert_pose2angleAxis([m["R"][i], m["t"][i]]) for i in range(len(ids))]))
    index_of = {c: i for i, c in enumerate(ids)}
    data = {k: torch.from_numpy(np.ascontiguousarray(ref[k])) for k in ("depth", "n_query", "intrinsic0", "intrinsic1", "mkpts0_c", "mkpts1_f")}
    data.update(angle_axis_to_world=aa, left_pose_idx=torch.tensor([index_of[c] for c in ref["left_colmap_ids"].tolist()]),
                right_pose_idx=torch.tensor([index_of[c] for c in ref["right_colmap_ids"].tolist()]))
    d_ref, _, _ = po.solve_literal(data)
    rel = ((torch.from_numpy(res["depth"]) - d_ref).abs() / d_ref.abs()).max().item()
    print("depth after the optimiser: max relative difference to the oracle", rel)
    assert rel < 1e-6
    assert np.array_equal(res["point_cloud_ids"], m["point_ids"]) and np.array_equal(res["colmap_frame_ids"], m["image_ids"])
    # update_model: the two postopt functions it composes, at their test's bar
    R, t = (torch.from_numpy(a).cuda() for a in res["pose"])
    upd = st.update_model(plan, model, torch.from_numpy(res["depth"]).cuda(), R, t)
    ref_upd = orc.update_model(m, want, res["depth"][:, 0], res["pose"][0], res["pose"][1])
    for k in ("xyz", "xys"):
        err = np.abs(upd[k].cpu().numpy() - ref_upd[k]).max()
        print("update_model", k, "max |err|", err)
        assert err < 1e-10, k
    unreg = m["point3D_ids"] == -1
    assert np.array_equal(upd["xys"].cpu().numpy()[unreg], m["xys"][unreg])


def test_aggregation_chain():
    """to_aggregation_inputs -> build_object_block reproduces sfm_objectblock_oracle on the same case"""
    from onepose_st_amd import sfm_objectblock as sob, sfm_tracks as st
    from tests import sfm_objectblock_oracle as sorc

    m = orc.make_model(41, 300, 10, 5, shuffle_ids=True)
    got, (model, plan, pairs, rows) = check(m)
    want = orc.vectorised_form(m)
    M = len(want["mkpts0_idx"])
    rng = np.random.default_rng(4)
    feats = {k: rng.standard_normal((M, d)).astype(np.float32) for k, d in (("feature_c0", 256), ("feature_c1", 256), ("feature0", 128), ("feature1", 128))}
    tracks = st.to_aggregation_inputs(plan, rows, *(torch.from_numpy(feats[k]).cuda() for k in ("feature_c0", "feature_c1", "feature0", "feature1")))
    assert tuple(tracks) == st.TRACK_KEYS
    case = {k: want[k] for k in ("assigned_image", "assigned_kpt", "row_offsets", "ref_image", "ref_kpt")}
    case.update({k: v[want["fine_row"]] for k, v in feats.items()})
    case.update(kpt_offsets=m["kpt_offsets"], point3D_ids=m["point3D_ids"], point_ids=m["point_ids"], xyz=m["xyz"],
                track_len=np.diff(m["track_offsets"]).astype(np.int64), max_num_kp3d=200)
    assert sorc.check_conditions(case) == 0
    ref = sorc.vectorised_form(case)
    res = sob.build_object_block(tracks, {k: model[k] for k in ("point_ids", "xyz")} | {"track_len": torch.from_numpy(case["track_len"]).cuda()},
                                 model["point3D_ids"], model["kpt_offsets"], max_num_kp3d=200)
    for k in ("keypoints3d", "group_offsets", "group_members", "descriptors3d_coarse", "descriptors3d_fine", "scores3d"):
        assert res[k].cpu().numpy().tobytes() == ref[k].tobytes(), k
    for k in ("desc_coarse", "desc_fine", "written", "scores_cleared"):
        assert res["features"][k].cpu().numpy().tobytes() == ref[k].tobytes(), k


def test_pair_list_that_lacks_a_row():
    from onepose_st_amd import sfm_tracks as st

    model = to_device(orc.hand_case())
    plan = st.assign_tracks(model)
    pairs = st.matching_pairs(plan, model)
    broken = dict(pairs, mkpts0_idx=pairs["mkpts0_idx"].clone())
    broken["mkpts0_idx"][6] = 1                                            # pair (1, 3) now holds keypoint 1 twice and keypoint 2 never
    with pytest.raises(ValueError, match="exactly one row"):
        st.optimisation_rows(plan, model, broken)
