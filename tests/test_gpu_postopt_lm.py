"""The second-order (Levenberg-Marquardt) depth solver on the MI355X (run with ``-m gpu``): ``csrc/postopt_lm.hip`` through
``postopt.refine_depths_lm`` against the numpy float64 restatement of tests/postopt_lm_oracle.py.

Bars.  Trajectories (``max_iters`` 1..4 from starts at 0.4x and 1.6x the true depth, where steps are rejected): iteration and rejection
counts and status equal, depth and lambda within rel 1e-11, the bar of the first-order solver's 20-step test.  Full runs: every track
CONVERGED; depths within rel ``2 * step_tol`` (either side may stop one sub-tolerance step apart: a step below ``step_tol`` relative is
where the loop ends, so the two ends differ by at most one such step each way); iteration counts at most 1 apart and equal on all but
0.5 % of the tracks (the oracle against its own 1e-12-perturbed run differs on 0 of 200 and at most 1 of 8 200); totals within rel 1e-12 of the oracle's
sums; the final total at most the first-order solver's cost at its own depths.  Residuals within 1e-8 px of the restatement at the
device's depths (the bar of the first-order solver's first evaluation).  Starts stay below 2.5x the true depth: beyond it the
algorithm itself can run off (the cost is bounded as d -> infinity)."""
import warnings

import numpy as np
import pytest
import torch

from onepose_st_amd import hip, postopt, postopt_lm
from onepose_st_amd.synthetic import make_synthetic_sfm_tracks
from tests import postopt_lm_oracle as lm
from tests import postopt_oracle as po

pytestmark = pytest.mark.gpu

ROW_KEYS = ("depth", "n_query", "intrinsic0", "intrinsic1", "mkpts0_c", "mkpts1_f", "left_pose_idx", "right_pose_idx",
            "angle_axis_to_world")
PER_ROW = ("intrinsic0", "intrinsic1", "mkpts0_c", "mkpts1_c", "mkpts1_f", "left_pose_idx", "right_pose_idx", "left_colmap_ids",
           "right_colmap_ids")
PER_TRACK = ("depth", "depth_true", "n_query", "point_cloud_id", "points")
OUT_KEYS = ("depth", "iterations", "rejects", "status", "lambda", "initial_cost", "final_cost")
STEP_TOL = lm.DEFAULTS["step_tol"]


@pytest.fixture(scope="module")
def dev():
    assert torch.cuda.is_available(), "these tests need the MI355X"
    hip.load()
    postopt_lm.load()
    return torch.device("cuda:0")


def refine_lm(data, dev, **kw):
    return postopt.refine_depths_lm(*(data[k].to(dev) for k in ROW_KEYS), **kw)


def host(out):
    return {k: (v.cpu().numpy() if torch.is_tensor(v) else v) for k, v in out.items()}


def rel(a, b):
    a, b = np.asarray(a, dtype=np.float64), np.asarray(b, dtype=np.float64)
    return float((np.abs(a - b) / np.maximum(np.abs(b), 1e-300)).max())


def select(data, tracks, counts):
    """the tracks ``tracks`` of a synthetic dict, each cut to its first ``counts[i]`` rows"""
    nq = data["n_query"]
    first = torch.cumsum(nq, 0) - nq
    assert all(int(nq[t]) >= c >= 1 for t, c in zip(tracks, counts))
    rows = torch.cat([torch.arange(int(first[t]), int(first[t]) + c) for t, c in zip(tracks, counts)])
    out = dict(data)
    for k in PER_ROW:
        out[k] = data[k][rows].clone()
    for k in PER_TRACK:
        out[k] = data[k][torch.tensor(tracks)].clone()
    out["n_query"] = torch.tensor(counts, dtype=torch.int64)
    return out


def check_full_run(data, dev, **kw):
    """the full-run bars of the module docstring; -> (device outputs on the host, oracle outputs)"""
    want = lm.solve(data, **kw)
    assert (want["status"] == lm.CONVERGED).all()                   # the case is one the algorithm itself solves
    got = host(refine_lm(data, dev, return_residuals=True, **kw))
    P = want["status"].shape[0]
    print("P", P, "iterations max", got["iterations"].max(), "rejects", int(got["rejects"].sum()), "depth rel", rel(got["depth"], want["depth"]),
          "iteration counts that differ", int((got["iterations"] != want["iterations"]).sum()),
          "totals rel", rel(got["initial_residual"], want["initial_residual"]), rel(got["final_residual"], want["final_residual"]))
    assert (got["status"] == postopt_lm.CONVERGED).all(), np.unique(got["status"], return_counts=True)
    assert got["depth"].shape == (P, 1) and rel(got["depth"], want["depth"]) <= 2 * STEP_TOL
    diff = np.abs(got["iterations"].astype(np.int64) - want["iterations"])
    assert diff.max() <= 1 and (diff != 0).sum() <= 0.005 * P, (diff.max(), (diff != 0).sum())
    assert got["steps"] == got["iterations"].max()
    assert rel(got["initial_residual"], want["initial_residual"]) <= 1e-12
    assert rel(got["final_residual"], want["final_residual"]) <= 1e-12
    r_at, _ = lm.residuals(got["depth"][:, 0], lm.fold(data))
    assert np.abs(got["residuals"] - r_at).max() < 1e-8
    return got, want


@pytest.mark.parametrize("seed,factor", [(0, 0.4), (3, 1.6)])
def test_trajectory_follows_the_oracle(dev, seed, factor):
    data = make_synthetic_sfm_tracks(seed)
    data["depth"] = factor * data["depth_true"]
    assert lm.solve(data)["rejects"].sum() > 0                      # the start is far enough that steps are rejected
    for k in range(1, 5):
        want, got = lm.solve(data, max_iters=k), host(refine_lm(data, dev, max_iters=k))
        for key in ("iterations", "rejects", "status"):
            assert np.array_equal(got[key], want[key]), (k, key, np.nonzero(got[key] != want[key]))
        assert want["iterations"].max() == k and got["steps"] == k
        assert rel(got["depth"], want["depth"]) <= 1e-11, (k, rel(got["depth"], want["depth"]))
        assert rel(got["lambda"], want["lambda"]) <= 1e-11, k


@pytest.mark.parametrize("seed,noise", [(0, 0.03), (1, 0.03), (1, 0.15)])
def test_full_run_matches_the_oracle(dev, seed, noise):
    data = make_synthetic_sfm_tracks(seed, depth_noise=noise)
    got, _ = check_full_run(data, dev)
    nq = data["n_query"]
    assert (nq[:3] == 1).all() and nq[3] >= 1000                    # single-row tracks and a long one are in the run
    # against the first-order solver on the same inputs: its cost at its own depths, evaluated by this solver's first evaluation
    first = postopt.refine_depths(*(data[k].to(dev) for k in ROW_KEYS))
    at_first = refine_lm(dict(data, depth=first["depth"].cpu()), dev, max_iters=0)["initial_residual"]
    print("final residual: second order", got["final_residual"], "first order", at_first, "after", first["steps"], "steps")
    assert got["final_residual"] <= at_first


def test_row_count_edges(dev):
    # 64 rows is the last track that lives in registers, 65 the first through the rows workspace, 128 / 129 one and two strides of it
    base = make_synthetic_sfm_tracks(4, n_frames=6, n_tracks=60, mean_len=100, n_single=1, long_len=1500)
    counts, nq, tracks = [1, 2, 63, 64, 65, 128, 129, 1500], base["n_query"].tolist(), []
    for c in counts:                                                # the shortest unused track that has the rows
        tracks.append(min((t for t in range(len(nq)) if nq[t] >= c and t not in tracks), key=lambda t: nq[t]))
    check_full_run(select(base, tracks, counts), dev)


def test_one_track(dev):
    base = make_synthetic_sfm_tracks(4, n_frames=6, n_tracks=8, mean_len=6, n_single=1, long_len=0)
    t = int(base["n_query"].argmax())
    check_full_run(select(base, [t], [int(base["n_query"][t])]), dev)


def test_more_tracks_than_waves_in_the_grid(dev):
    data = make_synthetic_sfm_tracks(0, n_tracks=8200, mean_len=2, long_len=0, depth_noise=0.1)      # 8 200 > 4 x 2 048
    check_full_run(data, dev)


def test_degenerate_problem_is_left_untouched(dev):
    # identity poses and intrinsics, keypoints at the principal point: every residual and every Jacobian entry is exactly 0
    P, nq = 5, torch.tensor([1, 3, 64, 65, 200])
    L = int(nq.sum())
    eye = torch.eye(3, dtype=torch.float64).expand(L, 3, 3).contiguous()
    zeros2 = torch.zeros(L, 2, dtype=torch.float64)
    idx = torch.zeros(L, dtype=torch.int64)
    depth = torch.linspace(1.0, 3.0, P, dtype=torch.float64)[:, None]
    out = postopt.refine_depths_lm(depth.to(dev), nq.to(dev), eye.to(dev), eye.to(dev), zeros2.to(dev), zeros2.to(dev), idx.to(dev),
                                   idx.to(dev), torch.zeros(2, 6, dtype=torch.float64, device=dev))
    assert (out["status"] == postopt_lm.DEGENERATE).all() and (out["iterations"] == 0).all() and (out["rejects"] == 0).all()
    assert torch.equal(out["depth"].cpu(), depth)
    assert out["steps"] == 0 and out["initial_residual"] == 0.0 and out["final_residual"] == 0.0


def test_a_nan_row_stops_its_own_track_only(dev):
    data = make_synthetic_sfm_tracks(1, depth_noise=0.15)
    clean = host(refine_lm(data, dev))
    nq = data["n_query"]
    t = next(i for i in range(4, nq.shape[0]) if 2 <= int(nq[i]) <= 64)          # a track that lives in registers
    bad = dict(data, mkpts1_f=data["mkpts1_f"].clone())
    bad["mkpts1_f"][int(nq[:t].sum()) + 1, 1] = float("nan")
    got = host(refine_lm(bad, dev))
    assert got["status"][t] == postopt_lm.DEGENERATE and got["iterations"][t] == 0 and got["rejects"][t] == 0
    assert got["depth"][t, 0] == data["depth"][t, 0].item()
    keep = np.arange(nq.shape[0]) != t
    for k in OUT_KEYS:
        assert got[k][keep].tobytes() == clean[k][keep].tobytes(), k
    # the same in the long track, which goes through the rows workspace
    bad = dict(data, mkpts1_f=data["mkpts1_f"].clone())
    bad["mkpts1_f"][int(nq[:3].sum()) + 700, 0] = float("nan")
    got = host(refine_lm(bad, dev))
    assert got["status"][3] == postopt_lm.DEGENERATE and got["depth"][3, 0] == data["depth"][3, 0].item()
    keep = np.arange(nq.shape[0]) != 3
    for k in OUT_KEYS:
        assert got[k][keep].tobytes() == clean[k][keep].tobytes(), k


def test_two_runs_are_bit_identical(dev):
    data = make_synthetic_sfm_tracks(1, depth_noise=0.15)
    a, b = (host(refine_lm(data, dev, return_residuals=True)) for _ in range(2))
    for k in (*OUT_KEYS, "residuals"):
        assert a[k].tobytes() == b[k].tobytes(), k
    assert (a["initial_residual"], a["final_residual"], a["steps"]) == (b["initial_residual"], b["final_residual"], b["steps"])


def second_order_cfgs():
    return {"solver_type": "SecondOrder", "residual_mode": "geometry_error", "optimize_lr": {"depth": 3e-2}, "optim_procedure": ["depth"],
            "num_workers": 1, "batch_size": 2000, "image_i_f_scale": 2, "verbose": False, "hip_second_order": True}


def test_start_optimize_runs_the_second_order_solver(dev):
    data = make_synthetic_sfm_tracks(0)
    agg = {k: data[k].to(dev) for k in ("depth", "n_query", "intrinsic0", "intrinsic1", "mkpts0_c", "mkpts1_c", "mkpts1_f",
                                         "left_colmap_ids", "right_colmap_ids", "point_cloud_id")}
    opt = postopt.Optimizer(second_order_cfgs())
    with warnings.catch_warnings(record=True) as caught:
        warnings.simplefilter("always")
        res = opt.start_optimize(agg, data["frame_poses"])
    assert not [w for w in caught if "DeepLM" in str(w.message)]
    assert set(res) == {"pose", "colmap_frame_ids", "depth", "point_cloud_ids"}
    direct = refine_lm(data, dev)
    assert res["depth"].shape == (data["depth"].shape[0], 1) and res["depth"].dtype == np.float64
    assert np.array_equal(res["depth"], direct["depth"].cpu().numpy())
    assert opt.steps == [direct["steps"]] and opt.solver_type == "SecondOrder"
    assert (opt.initial_residual, opt.final_residual) == (direct["initial_residual"], direct["final_residual"])
    R, t = res["pose"]
    aa = data["angle_axis_to_world"]
    assert np.abs(R - po.so3_exp_map(aa[:, :3]).numpy()).max() < 1e-12 and np.array_equal(t, aa[:, 3:6].numpy())
    assert np.array_equal(res["colmap_frame_ids"], np.array(list(data["frame_poses"].keys())))
    assert np.array_equal(res["point_cloud_ids"], data["point_cloud_id"].numpy())


def test_optimizer_chain_from_the_track_rows(dev):
    """sfm_tracks' rows -> to_optimizer_inputs -> Optimizer with the second-order solver, on the scene of test_gpu_sfm_tracks.py"""
    from onepose_st_amd import sfm_tracks as st
    from tests import sfm_tracks_oracle as orc

    m = orc.with_projected_keypoints(orc.make_model(31, 200, 8, 5, n_dup=10, shuffle_ids=True), noise=0.3)
    model = {k: torch.from_numpy(np.ascontiguousarray(v)).to(dev) for k, v in m.items()}
    plan = st.assign_tracks(model)
    pairs = st.matching_pairs(plan, model)
    rows = st.optimisation_rows(plan, model, pairs)
    want = orc.vectorised_form(m)
    mk1f = want["mkpts1_c"] + 0.5 * np.random.default_rng(2).standard_normal(want["mkpts1_c"].shape)
    agg, poses = st.to_optimizer_inputs(plan, model, pairs, rows, torch.from_numpy(mk1f).to(dev))
    opt = postopt.Optimizer(second_order_cfgs())
    with warnings.catch_warnings(record=True) as caught:
        warnings.simplefilter("always")
        res = opt.start_optimize(agg, poses)
    assert not [w for w in caught if "DeepLM" in str(w.message)]
    ref = orc.optimizer_inputs(m, want, mk1f)
    ids = m["image_ids"].tolist()
    aa = torch.from_numpy(np.concatenate([postopt.convert_pose2angleAxis([m["R"][i], m["t"][i]]) for i in range(len(ids))]))
    index_of = {c: i for i, c in enumerate(ids)}
    data = {k: torch.from_numpy(np.ascontiguousarray(ref[k])) for k in ("depth", "n_query", "intrinsic0", "intrinsic1", "mkpts0_c", "mkpts1_f")}
    data.update(angle_axis_to_world=aa, left_pose_idx=torch.tensor([index_of[c] for c in ref["left_colmap_ids"].tolist()]),
                right_pose_idx=torch.tensor([index_of[c] for c in ref["right_colmap_ids"].tolist()]))
    oracle = lm.solve(data)
    assert (oracle["status"] == lm.CONVERGED).all()
    assert res["depth"].shape == oracle["depth"].shape and rel(res["depth"], oracle["depth"]) <= 2 * STEP_TOL
    assert np.array_equal(res["point_cloud_ids"], m["point_ids"]) and np.array_equal(res["colmap_frame_ids"], m["image_ids"])
    direct = refine_lm({**data, "depth": agg["depth"].cpu()}, dev)
    assert np.array_equal(res["depth"], direct["depth"].cpu().numpy()) and opt.steps == [direct["steps"]]
    # the two starts differ by the device's rounding of the initial depth and both ends lie within step_tol of the optimum, where the
    # cost is stationary: the totals differ in second order of that
    assert abs(opt.final_residual - oracle["final_residual"]) <= 1e-9 * oracle["final_residual"]
