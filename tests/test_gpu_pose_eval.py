"""The pose evaluation on the device (``onepose_st_amd/pose_eval.py``, ``libonepose_pose_eval.so``) against its numpy restatement
(tests/pose_eval_oracle.py): every output bit for bit at the block, tile and chunk edges, the flags, the input forms, run-to-run bytes, a
non-default stream, ``to_host`` against what the reference's functions returned, ``compute_query_pose_errors`` and ``evaluate_records``.
Everything is small: at most 65 frames and 513 vertices."""
import os

import numpy as np
import pytest
import torch

from onepose_st_amd import pnp_device
from tests import pose_eval_oracle as po
from tests.pose_eval_oracle import EPS, coordinate_scale, mean_bound, pixel_scale

pytestmark = pytest.mark.gpu

DEV = "cuda:0"
REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.fixture(scope="module")
def pe():
    from onepose_st_amd import pose_eval
    pose_eval.load()
    return pose_eval


@pytest.fixture(scope="module")
def golden():
    return dict(np.load(os.path.join(REPO, "tests", "golden", "pose_eval_small.npz")))


def dev(a, dtype=None):
    return torch.from_numpy(np.ascontiguousarray(a, dtype=dtype)).to(DEV)


def same_bytes(t, a):
    """a device tensor against a numpy array: dtype, shape and every byte (NaN payloads included)"""
    got = t.cpu().numpy()
    return got.dtype == a.dtype and got.shape == a.shape and got.tobytes() == np.ascontiguousarray(a).tobytes()


def check(errs, verts, pred, gt, K=None, symmetric=False, no_pose=None, unit="m"):
    """every device output of one call against the oracle, bit for bit"""
    rot_cos, t_err, fl = po.errors(pred, gt, no_pose=no_pose, unit=unit)
    assert same_bytes(errs.flags, fl), (errs.flags.cpu().numpy(), fl)
    assert same_bytes(errs.rot_cos, rot_cos), (errs.rot_cos.cpu().numpy(), rot_cos)
    assert same_bytes(errs.t_err, t_err), (errs.t_err.cpu().numpy(), t_err)
    if verts is None:
        assert errs.add_dist is None and errs.proj2d is None
        return
    want = (po.adds if symmetric else po.add)(verts, pred, gt, fl)
    assert same_bytes(errs.add_dist, want), (errs.add_dist.cpu().numpy(), want)
    if K is None:
        assert errs.proj2d is None
    else:
        want = po.proj2d(verts, pred, gt, K, fl)
        assert same_bytes(errs.proj2d, want), (errs.proj2d.cpu().numpy(), want)


@pytest.mark.parametrize("F", [1, 3, 65])
@pytest.mark.parametrize("V", [1, 255, 256, 257, 513])
def test_bit_equal_at_block_tile_and_chunk_edges(pe, V, F):
    """V: below, at and one past the 256-vertex block (= the LDS tile of ADD-S: a second tile with one vertex), and a third block with
    one vertex; F: one frame, three (ADD-S with a pair budget of one frame per launch, and at V = 513 of one block per launch) and more
    than one 64-lane wave of frames"""
    s = po.scene(100 + V + F, F, V)
    verts, pred, gt, K = s["verts"], s["pose_pred"], s["pose_gt"], s["K"]
    d_verts, d_pred, d_gt = dev(verts), dev(pred), dev(gt)
    check(pe.pose_errors(d_pred, d_gt, model_points=d_verts, K=K), verts, pred, gt, K)
    budgets = [None] if F != 3 else [V * V, 2 * V * V] + ([256 * V, 2 * 256 * V] if V == 513 else [])
    for budget in budgets:
        check(pe.pose_errors(d_pred, d_gt, model_points=d_verts, K=K, symmetric=True, pair_budget=budget), verts, pred, gt, K, symmetric=True)
    if F == 3 and V > 1:
        with pytest.raises(ValueError, match="pair_budget outside"):
            pe.pose_errors(d_pred, d_gt, model_points=d_verts, symmetric=True, pair_budget=min(V, 256) * V - 1)


def test_identical_poses_are_exact_zeros(pe):
    s = po.scene(5, 6, 300)
    verts, gt, K = s["verts"], s["pose_gt"].copy(), s["K"]
    perm = np.array([[0.0, 1.0, 0.0], [0.0, 0.0, 1.0], [1.0, 0.0, 0.0]])
    gt[0, :, :3], gt[1, :, :3] = np.eye(3), perm                          # rotations whose squared entries sum to 3 without rounding
    for symmetric in (False, True):
        errs = pe.pose_errors(dev(gt), dev(gt), model_points=dev(verts), K=K, symmetric=symmetric)
        check(errs, verts, gt, gt, K, symmetric=symmetric)
        host = errs.unpack(errs.pack().cpu().numpy())
        assert (host["t_err"] == 0).all() and (host["add_dist"] == 0).all() and (host["proj2d"] == 0).all()
        assert host["rot_cos"][0] == 1.0 and host["rot_cos"][1] == 1.0
        # a general rotation: its rows are unit vectors to a few roundings each, and nine squares are rounded and summed
        assert (np.abs(host["rot_cos"] - 1.0) <= 32 * EPS).all()
        assert (errs.to_host()["R_errs"][:2] == 0).all()


def test_clamp_and_half_turn(pe):
    I = np.concatenate([np.eye(3), [[0.0], [0.0], [0.7]]], axis=1)
    over, half, below = I.copy(), I.copy(), I.copy()
    over[:, :3] = np.eye(3) * (1 + 2.0 ** -30)                             # the pair's trace rounds above 3
    half[:, :3] = np.diag([1.0, -1.0, -1.0])
    below[:, :3] = -np.eye(3) * (1 + 2.0 ** -30)                           # the cosine's argument is below -1: NaN on the host
    pred, gt = np.stack([over, half, below, I]), np.stack([over, I, over, I])
    assert (pred[0, :, :3] * gt[0, :, :3]).sum() > 3.0
    errs = pe.pose_errors(dev(pred), dev(gt))
    check(errs, None, pred, gt)
    host = errs.to_host()
    assert host["R_errs"][0] == 0.0 and host["R_errs"][1] == 180.0 and np.isnan(host["R_errs"][2]) and host["R_errs"][3] == 0.0
    assert list(host["flags"]) == [0, 0, 0, 0]
    assert pe.aggregate_metrics(host)["5cm@5degree"] == 0.5               # NaN fails the threshold


@pytest.mark.parametrize("symmetric", [False, True])
def test_no_pose_and_non_finite_frames_between_valid_ones(pe, symmetric):
    s = po.scene(9, 7, 257)
    verts, pred, gt, K = s["verts"], s["pose_pred"].copy(), s["pose_gt"].copy(), s["K"]
    pred[1, 2, 3] = np.nan
    gt[3, 0, 0] = np.inf
    pred[5, 1, 1] = -np.inf
    no_pose = np.array([0, 0, 1, 0, 0, 1, 0])
    status = dev(np.where(no_pose, pnp_device.STATUS_NO_POSE | pnp_device.STATUS_NEEDS_MORE, pnp_device.STATUS_NEEDS_MORE), np.int32)
    errs = pe.pose_errors(dev(pred), dev(gt), status=status, model_points=dev(verts), K=K, symmetric=symmetric)
    check(errs, verts, pred, gt, K, symmetric=symmetric, no_pose=no_pose)
    host = errs.to_host(diameter=10.0)
    flagged = np.array([0, 1, 1, 1, 0, 1, 0], bool)
    assert list(host["flags"]) == [0, pe.BAD_INPUT, pe.NO_POSE, pe.BAD_INPUT, 0, pe.NO_POSE | pe.BAD_INPUT, 0]
    for k in ("R_errs", "t_errs", "add_dist", "proj2D_metric"):
        assert np.isinf(host[k][flagged]).all() and np.isfinite(host[k][~flagged]).all(), k
    assert list(host["ADD_metric"]) == list(~flagged)


def test_duplicate_vertices_under_symmetric(pe):
    s = po.scene(11, 3, 300)
    verts, pred, gt = s["verts"].copy(), s["pose_pred"], s["pose_gt"]
    verts[100:200] = verts[0:100]                                         # every one of them twice: equal distances, one minimum
    verts[299] = verts[0]
    check(pe.pose_errors(dev(pred), dev(gt), model_points=dev(verts), symmetric=True), verts, pred, gt, symmetric=True)
    same = np.repeat(verts[:1], 260, axis=0)                              # one point 260 times: two tiles of the same vertex
    errs = pe.pose_errors(dev(pred), dev(gt), model_points=dev(same), symmetric=True)
    check(errs, same, pred, gt, symmetric=True)
    plain = pe.pose_errors(dev(pred), dev(gt), model_points=dev(same))
    assert np.abs(errs.add_dist.cpu().numpy() - plain.add_dist.cpu().numpy()).max() <= 8 * EPS * plain.add_dist.max().item()


def test_input_forms(pe):
    """K per frame (tensor and array), [F, 4, 4] tables on either side, the units, host arrays for pose_gt and the model"""
    s = po.scene(13, 5, 257)
    verts, pred, gt, K = s["verts"], s["pose_pred"], s["pose_gt"], s["K"]
    Ks = np.stack([K * np.array([[1 + 0.01 * f], [1 - 0.01 * f], [1.0]]) for f in range(5)])
    check(pe.pose_errors(dev(pred), dev(gt), model_points=dev(verts), K=dev(Ks)), verts, pred, gt, Ks)
    check(pe.pose_errors(dev(pred), gt, model_points=verts, K=Ks, symmetric=True), verts, pred, gt, Ks, symmetric=True)
    bottom = np.broadcast_to(np.array([[[0.0, 0.0, 0.0, 1.0]]]), (5, 1, 4))
    pred4, gt4 = np.concatenate([pred, bottom], axis=1), np.concatenate([gt, np.full((5, 1, 4), np.nan)], axis=1)   # the fourth row is never read
    check(pe.pose_errors(dev(pred4), dev(gt4), model_points=dev(verts), K=K), verts, pred, gt, K)
    check(pe.pose_errors(dev(pred4), dev(gt), model_points=dev(verts), K=K, symmetric=True), verts, pred, gt, K, symmetric=True)
    for unit in ("m", "cm", "mm"):
        check(pe.pose_errors(dev(pred), dev(gt), unit=unit), None, pred, gt, unit=unit)
    check(pe.pose_errors(dev(pred.astype(np.float32)), dev(gt)), None, pred.astype(np.float32).astype(np.float64), gt)
    with pytest.raises(ValueError, match=r"K: \[3, 3\] shared"):
        pe.pose_errors(dev(pred), dev(gt), model_points=dev(verts), K=Ks[:4])
    with pytest.raises(ValueError, match="same number of frames"):
        pe.pose_errors(dev(pred), dev(gt[:4]))


def test_device_poses_as_input(pe):
    s = po.scene(17, 4, 255)
    verts, pred, gt, K = s["verts"], s["pose_pred"], s["pose_gt"], s["K"]
    status = np.array([0, pnp_device.STATUS_NO_POSE, pnp_device.STATUS_NEEDS_MORE, 0], np.int32)
    poses = pnp_device.DevicePoses(dev(pred), dev(np.full(4, 9, np.int32)), dev(status), dev(np.ones(8, np.uint8)), dev(np.zeros((4, 2), np.int32)))
    errs = pe.pose_errors(poses, dev(gt), model_points=dev(verts), K=K)
    check(errs, verts, pred, gt, K, no_pose=[0, 1, 0, 0])
    with pytest.raises(ValueError, match="status comes with the DevicePoses"):
        pe.pose_errors(poses, dev(gt), status=dev(status))


def test_two_runs_and_a_side_stream_give_the_same_bytes(pe):
    s = po.scene(19, 9, 513)
    verts, pred, gt, K = s["verts"], s["pose_pred"], s["pose_gt"], s["K"]
    d = (dev(pred), dev(gt))
    kw = dict(model_points=dev(verts), K=dev(K), symmetric=True)
    first = pe.pose_errors(*d, **kw).pack().cpu().numpy()
    assert np.array_equal(first, pe.pose_errors(*d, **kw).pack().cpu().numpy())
    torch.cuda.synchronize()
    side = torch.cuda.Stream(device=DEV)
    errs = pe.pose_errors(*d, stream=side, **kw)
    side.synchronize()
    assert np.array_equal(first, errs.pack().cpu().numpy())
    check(errs, verts, pred, gt, K, symmetric=True)


def test_to_host_against_the_reference(pe, golden):
    verts, pred, gt, K = golden["verts"], golden["pose_pred"], golden["pose_gt"], golden["K"]
    diameter, V = float(golden["diameter"]), len(golden["verts"])
    S, Spx = coordinate_scale(verts, pred, gt), pixel_scale(verts, K, pred, gt)
    for unit in ("m", "cm", "mm"):
        host = pe.pose_errors(dev(pred), dev(gt), unit=unit).to_host()
        ref_r, ref_t = golden[f"R_errs_{unit}"], golden[f"t_errs_{unit}"]
        assert (np.abs(host["R_errs"] - ref_r) <= np.rad2deg(16 * 2.0 ** -53 / np.sin(np.deg2rad(ref_r)))).all()
        assert (np.abs(host["t_errs"] - ref_t) <= 4 * EPS * ref_t).all()
        assert set(host) == {"R_errs", "t_errs", "flags"}
    host = pe.pose_errors(dev(pred), dev(gt), model_points=dev(verts), K=K).to_host(diameter=diameter, percentage=float(golden["percentage"]))
    assert (np.abs(host["add_dist"] - golden["add_mean"]) <= mean_bound(S, V, golden["add_mean"])).all()
    assert (np.abs(host["proj2D_metric"] - golden["proj2d"]) <= mean_bound(Spx, V, golden["proj2d"])).all()
    assert np.array_equal(host["ADD_metric"], golden["add"])
    agg = pe.aggregate_metrics(host)
    assert list(agg) == [str(k) for k in golden["aggregate_keys"]] and np.array_equal(np.array(list(agg.values())), golden["aggregate_values"])
    sym = pe.pose_errors(dev(pred), dev(gt), model_points=dev(verts), symmetric=True).to_host(diameter=diameter)
    assert (np.abs(sym["add_dist"] - golden["adds_mean"]) <= mean_bound(S, V, golden["adds_mean"])).all()
    assert np.array_equal(sym["ADD_metric"], golden["adds"]) and "proj2D_metric" not in sym


def test_compute_query_pose_errors_on_a_planted_batch(pe):
    """two frames of 80 planted matches each: the call against ``pnp_device.ransac_pnp`` followed by the oracle on its poses"""
    s = po.scene(23, 2, 300)
    verts, gt, K = s["verts"], s["pose_gt"], s["K"]
    g = np.random.default_rng(4)
    pts3d = g.uniform(-0.08, 0.08, size=(2, 80, 3)).astype(np.float32)
    mk2d = np.concatenate([po.project(K, gt[b], pts3d[b]) for b in range(2)]).astype(np.float32)
    Ks, K_origin = np.stack([K, K]), np.stack([K * np.array([[2.0], [2.0], [1.0]])] * 2)
    data = {"mkpts_query_f": dev(mk2d), "mkpts_3d_db": dev(pts3d.reshape(-1, 3)), "m_bids": dev(np.repeat([0, 1], 80), np.int64)}
    cfg = {"point_cloud_rescale": 1000, "pnp_reprojection_error": 7, "model_unit": "m", "use_pycolmap_ransac": True, "eval_ADD_metric": True}
    gt4 = np.concatenate([gt, np.broadcast_to(np.array([[[0.0, 0.0, 0.0, 1.0]]]), (2, 1, 4))], axis=1)
    poses, errs = pe.compute_query_pose_errors(data, Ks, dev(gt4, np.float32), cfg, model_points=verts, diameter=0.25, K_origin=K_origin)
    again = pnp_device.ransac_pnp(Ks, data["mkpts_query_f"], data["mkpts_3d_db"], b_ids=data["m_bids"], frames=2, scale=1000, pnp_reprojection_error=7)
    assert same_bytes(poses.pose, again.pose.cpu().numpy()) and same_bytes(poses.status, again.status.cpu().numpy())
    pred = poses.pose.cpu().numpy()
    check(errs, verts, pred, gt4.astype(np.float32).astype(np.float64), K_origin)
    host = errs.to_host()
    assert (host["flags"] == 0).all() and (host["R_errs"] < 0.1).all() and (host["t_errs"] < 0.1).all()            # planted: float32 pixels only
    assert list(host["ADD_metric"]) == [True, True] and (host["proj2D_metric"] < 1.0).all()
    with pytest.raises(NotImplementedError, match="adaptive policy"):
        pe.compute_query_pose_errors(data, Ks, dev(gt4), {**cfg, "use_pycolmap_ransac": False})


def test_evaluate_records(pe):
    s = po.scene(29, 5, 257)
    verts, pred, gt, K = s["verts"], s["pose_pred"], s["pose_gt"], s["K"]
    records = [{"pose": pred[f], "inliers": np.arange(12), "pose_refined": gt[f], "inliers_refined": np.arange(20)} for f in range(5)]
    records[2]["pose"], records[2]["inliers"] = np.eye(4)[:3], np.array([], dtype=np.int64)                          # the loop's record of a lost frame
    records[4]["pose"] = np.concatenate([pred[4], [[0.0, 0.0, 0.0, 1.0]]])
    out = pe.evaluate_records(records, gt, model_points=verts, K=K, diameter=0.2, device=DEV)
    no_pose = np.array([0, 0, 1, 0, 0])
    table = pred.copy()
    table[2] = np.eye(4)[:3]
    rot_cos, t_err, fl = po.errors(table, gt, no_pose=no_pose)
    assert np.array_equal(out["flags"], fl) and np.array_equal(out["t_errs"], t_err)
    assert np.array_equal(out["R_errs"], np.where(fl != 0, np.inf, po.angles(rot_cos)))
    assert np.array_equal(out["add_dist"], po.add(verts, table, gt, fl)) and np.array_equal(out["proj2D_metric"], po.proj2d(verts, table, gt, K, fl))
    assert np.array_equal(out["ADD_metric"], out["add_dist"] < 0.2 * 0.1) and not out["ADD_metric"][2]
    assert out["aggregate"] == pe.aggregate_metrics({k: out[k] for k in ("R_errs", "t_errs", "ADD_metric", "proj2D_metric")})
    assert set(out["aggregate"]) == {"1cm@1degree", "3cm@3degree", "5cm@5degree", "ADD metric", "proj2D metric"}
    refined = pe.evaluate_records(records, gt, key="pose_refined", device=DEV)
    assert (refined["t_errs"] == 0).all() and (refined["flags"] == 0).all() and set(refined["aggregate"]) == {"1cm@1degree", "3cm@3degree", "5cm@5degree"}
    assert refined["aggregate"]["5cm@5degree"] == 1.0
