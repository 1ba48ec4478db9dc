"""SfM depth refinement on the MI355X (run with ``-m gpu``): the prep and step kernels of ``csrc/postopt.hip`` against the CPU float64
oracle of tests/postopt_oracle.py (the reference's residual, autograd and ``torch.optim.Adam``), the device early stop, determinism,
``Optimizer.start_optimize`` and the two point kernels.

Bars.  Per-row residuals of the prep + first evaluation within 1e-8 px and l_0 within rel 1e-12; depths of the first 20 steps within
rel 1e-11.  Full runs: the same step count (after checking that the oracle's relative decrease never lies within 1e-7 of the 1e-4
threshold from the first step the rule may stop at up to its stop step), final residual within rel 1e-8 and depths within rel 1e-6.
Measured on the CPU for both seeds, the oracle against itself on the kernels' folded form ``h(d) = d * a + b``, and against a restatement
of the kernels' analytic gradient and Adam, differ by at most 7e-15 (final residual, relative) and 3e-15 (depths): Adam near the optimum
can amplify last-bit differences of the residual, so the bars keep six to eight orders of magnitude of room for the device's libm and
summation order.  Point kernels within 1e-10 of numpy float64."""
import warnings

import numpy as np
import pytest
import torch

from onepose_st_amd import hip, postopt
from onepose_st_amd.synthetic import make_synthetic_sfm_tracks
from tests import postopt_oracle as po

pytestmark = pytest.mark.gpu

ROW_KEYS = ("depth", "n_query", "intrinsic0", "intrinsic1", "mkpts0_c", "mkpts1_f", "left_pose_idx", "right_pose_idx",
            "angle_axis_to_world")


@pytest.fixture(scope="module")
def dev():
    assert torch.cuda.is_available(), "these tests need the MI355X"
    hip.load()
    return torch.device("cuda:0")


@pytest.fixture(scope="module")
def seeds():
    return {s: make_synthetic_sfm_tracks(s) for s in (0, 1)}


def refine(data, dev, **kw):
    return postopt.refine_depths(*(data[k].to(dev) for k in ROW_KEYS), **kw)


def rel(a, b):
    a, b = torch.as_tensor(a, dtype=torch.float64).cpu(), torch.as_tensor(b, dtype=torch.float64).cpu()
    return ((a - b).abs() / b.abs().clamp_min(1e-300)).max().item()


def test_prep_and_first_evaluation_match_the_oracle(dev, seeds):
    data = seeds[0]
    check_first_evaluation(refine(data, dev, max_steps=1, return_residuals=True), data)


def check_first_evaluation(out, data):
    """``out``: a one-step run with residuals; the prep kernel's fold and the first evaluation against the oracle"""
    p0, p1, idx = po.expand_inputs(data)
    want = po.depth_residual(data["depth"][idx], p0, p1, data["intrinsic0"], data["intrinsic1"], data["mkpts0_c"], data["mkpts1_f"])
    err = (out["residuals"].cpu() - want).abs().max().item()
    assert err < 1e-8, err
    l0 = torch.sum(0.5 * want * want).item()
    assert out["steps"] == 1 and abs(out["initial_residual"] - l0) <= 1e-12 * l0, (out["initial_residual"], l0)


def test_first_20_steps_follow_the_oracle(dev):
    data = make_synthetic_sfm_tracks(1, depth_noise=0.15)            # far enough from the optimum that no step k <= 20 may stop
    _, losses, traj = po.solve_literal(data, max_steps=20, record=True)
    assert len(losses) == 20
    for k in range(1, 21):
        out = refine(data, dev, max_steps=k)
        assert out["steps"] == k
        assert rel(out["depth"], traj[k - 1]) < 1e-11, (k, rel(out["depth"], traj[k - 1]))
        assert rel(out["loss"], losses[:k]) < 1e-12, k


@pytest.mark.parametrize("seed", [0, 1])
def test_full_run_matches_the_oracle(dev, seeds, seed):
    data = seeds[seed]
    d_ref, losses, _ = po.solve_literal(data)
    ratios = po.stop_ratios(losses)
    first = int(1000 * 0.2) + 1
    for i in range(first, len(losses)):
        assert abs(ratios[i] - 1e-4) >= 1e-7, (i, ratios[i])      # the stop step is not a rounding case
    out = refine(data, dev)
    assert out["steps"] == len(losses), (out["steps"], len(losses))
    assert abs(out["initial_residual"] - losses[0]) <= 1e-12 * losses[0]
    assert abs(out["final_residual"] - losses[-1]) <= 1e-8 * losses[-1], (out["final_residual"], losses[-1])
    assert rel(out["depth"], d_ref) < 1e-6, rel(out["depth"], d_ref)
    nq = data["n_query"]
    assert (nq[:3] == 1).all() and nq[3] >= 1000                    # single-row tracks and a long one are in the run
    assert rel(out["depth"][:4], d_ref[:4]) < 1e-6


def test_single_row_and_long_tracks(dev):
    data = make_synthetic_sfm_tracks(4, n_frames=6, n_tracks=3, mean_len=2, n_single=1, long_len=1500)
    data["n_query"][2] = 1
    L = int(data["n_query"].sum())
    for k in ("intrinsic0", "intrinsic1", "mkpts0_c", "mkpts1_f", "left_pose_idx", "right_pose_idx"):
        data[k] = data[k][:L]
    _, losses, traj = po.solve_literal(data, max_steps=30, record=True)
    out = refine(data, dev, max_steps=30)
    assert out["steps"] == len(losses)
    assert rel(out["depth"], traj[-1]) < 1e-11


def test_problem_at_its_optimum_runs_every_step(dev):
    # identity poses and intrinsics, keypoints at the principal point: every residual is exactly 0 at any depth, so every loss is 0 and
    # every relative decrease is 0 / 0 = NaN, which never stops the solver
    P, nq = 5, torch.tensor([1, 3, 64, 65, 200])
    L = int(nq.sum())
    eye = torch.eye(3, dtype=torch.float64).expand(L, 3, 3).contiguous()
    zeros2 = torch.zeros(L, 2, dtype=torch.float64)
    idx = torch.zeros(L, dtype=torch.int64)
    depth = torch.linspace(1.0, 3.0, P, dtype=torch.float64)[:, None]
    out = postopt.refine_depths(depth.to(dev), nq.to(dev), eye.to(dev), eye.to(dev), zeros2.to(dev), zeros2.to(dev), idx.to(dev),
                                idx.to(dev), torch.zeros(2, 6, dtype=torch.float64, device=dev))
    assert out["steps"] == 1000
    assert (out["loss"] == 0).all()
    assert torch.equal(out["depth"].cpu(), depth)


def test_small_max_steps_stop_where_the_rule_predicts(dev, seeds):
    data = dict(seeds[0])
    data["depth"] = refine(data, dev, max_steps=300)["depth"].cpu()     # start near the optimum: fresh Adam moments overshoot early
    hist = refine(data, dev, max_steps=1000)["loss"].cpu()
    ratios = po.stop_ratios(hist.tolist())
    for M in (2, 5, 10, 20, 40):
        want = M
        for i in range(1, min(M, len(ratios))):
            if ratios[i] < 1e-4 and i > M * 0.2:
                want = i + 1
                break
        assert want <= len(ratios)
        out = refine(data, dev, max_steps=M)
        assert out["steps"] == want, (M, out["steps"], want)
        assert torch.equal(out["loss"].cpu(), hist[:want])


def test_two_runs_are_bit_identical(dev, seeds):
    a = refine(seeds[1], dev, return_residuals=True)
    b = refine(seeds[1], dev, return_residuals=True)
    assert a["steps"] == b["steps"]
    assert torch.equal(a["depth"], b["depth"]) and torch.equal(a["loss"], b["loss"]) and torch.equal(a["residuals"], b["residuals"])


def test_start_optimize_returns_the_reference_dict(dev, seeds):
    data = seeds[0]
    agg = {k: data[k].to(dev) for k in ("depth", "n_query", "intrinsic0", "intrinsic1", "mkpts0_c", "mkpts1_c", "mkpts1_f",
                                         "left_colmap_ids", "right_colmap_ids", "point_cloud_id")}
    cfgs = {"solver_type": "FirstOrder", "residual_mode": "geometry_error", "optimize_lr": {"depth": 3e-2}, "optim_procedure": ["depth"],
            "num_workers": 1, "batch_size": 2000, "image_i_f_scale": 2, "verbose": False}
    with warnings.catch_warnings(record=True) as caught:
        warnings.simplefilter("always")
        res = postopt.Optimizer(cfgs).start_optimize(agg, data["frame_poses"])
    assert not [w for w in caught if "DeepLM" in str(w.message)]
    assert set(res) == {"pose", "colmap_frame_ids", "depth", "point_cloud_ids"}
    d_ref, losses, _ = po.solve_literal(data)
    assert res["depth"].shape == (data["depth"].shape[0], 1) and res["depth"].dtype == np.float64
    assert rel(torch.from_numpy(res["depth"]), d_ref) < 1e-6
    R, t = res["pose"]
    aa = data["angle_axis_to_world"]
    assert np.abs(R - po.so3_exp_map(aa[:, :3]).numpy()).max() < 1e-12 and np.array_equal(t, aa[:, 3:6].numpy())
    assert np.abs(R - data["R"].numpy()).max() < 1e-12
    assert np.array_equal(res["colmap_frame_ids"], np.array(list(data["frame_poses"].keys())))
    assert np.array_equal(res["point_cloud_ids"], data["point_cloud_id"].numpy())
    with pytest.warns(UserWarning, match="DeepLM"):
        res2 = postopt.Optimizer(dict(cfgs, solver_type="SecondOrder")).start_optimize(agg, data["frame_poses"])
    assert np.array_equal(res2["depth"], res["depth"])


def test_points_from_depth_and_projection_match_numpy(dev, seeds):
    data = seeds[1]
    P = data["depth"].shape[0]
    first = torch.cumsum(data["n_query"], 0) - data["n_query"]
    kp, fr = data["mkpts0_c"][first], data["left_pose_idx"][first]
    K, R, t = data["K"], data["R"], data["t"]
    got = postopt.points_from_depth(kp.to(dev), data["depth"].to(dev), fr.to(dev), K.to(dev), R.to(dev), t.to(dev)).cpu().numpy()
    want = np.empty((P, 3))
    for i in range(P):
        f = int(fr[i])
        T = np.concatenate([np.concatenate([R[f].numpy(), t[f].numpy()[:, None]], 1), [[0, 0, 0, 1]]], 0)
        Ti = np.linalg.inv(T)
        kh = (np.concatenate([kp[i].numpy()[None], np.ones((1, 1))], -1) * data["depth"][i].numpy()).T
        want[i] = (Ti[:3, :3] @ (np.linalg.inv(K[f].numpy()) @ kh) + Ti[:3, 3][:, None])[:, 0]
    assert np.abs(got - want).max() < 1e-10
    fr2 = torch.randint(0, K.shape[0], (P,), generator=torch.Generator().manual_seed(2))
    X = torch.from_numpy(want)
    got2 = postopt.project_points(X.to(dev), fr2.to(dev), K.to(dev), R.to(dev), t.to(dev)).cpu().numpy()
    want2 = np.empty((P, 2))
    for i in range(P):
        f = int(fr2[i])
        c = R[f].numpy() @ want[i][:, None] + t[f].numpy()[:, None]
        h = (K[f].numpy() @ c).T
        want2[i] = (h[:, :2] / (h[:, [2]] + 1e-4))[0]
    assert np.abs(got2 - want2).max() < 1e-10
