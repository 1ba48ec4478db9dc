"""Device PnP on the GPU: every stage of ``libonepose_pnp_device.so`` against the numpy oracle (``tests/pnp_device_oracle.py``), the whole
solve against the host solver, and ``SequenceRunner(pnp="device")`` against ``pnp="host"``.  Sizes stay small (trials <= 1 024, n <= 400
per stage test); the c1 frames of the end-to-end test are the CPU test's.
"""
import os
import sys

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import pnp_device_oracle as orc  # noqa: E402

from onepose_st_amd import frameloop as fl  # noqa: E402
from onepose_st_amd import pnp  # noqa: E402

pytestmark = pytest.mark.gpu
REPROJ = 5.0
POSE_BAR = 1e-4


@pytest.fixture(scope="module")
def pd():
    if not torch.cuda.is_available():
        pytest.skip("needs the MI355X")
    from onepose_st_amd import pnp_device
    pnp_device.load()
    return pnp_device


def dev_t(a, dtype=None):
    return torch.as_tensor(np.ascontiguousarray(a), dtype=dtype).to("cuda:0")


def scene(n, seed, outliers=0.25, K=None):
    """n matches of a random pose: 0.3 px noise, a share of gross outliers -> (K, pts2d f32, pts3d f32, pose)"""
    g = np.random.default_rng(seed)
    K = np.array([[600.0, 0.5, 320.0], [0, 610.0, 240.0], [0, 0, 1]]) if K is None else K
    X = g.uniform(-0.1, 0.1, size=(n, 3))
    ax = g.normal(size=3)
    R = orc.rodrigues(ax / np.linalg.norm(ax) * g.uniform(0.1, 0.7))
    t = np.array([0.0, 0.0, 0.5]) + 0.02 * g.normal(size=3)
    cam = X @ R.T + t
    uv = (K @ cam.T).T
    uv = uv[:, :2] / uv[:, 2:3] + 0.3 * g.normal(size=(n, 2))
    bad = g.random(n) < outliers
    uv[bad] += g.uniform(20, 80, size=(int(bad.sum()), 2))
    return K, uv.astype(np.float32), X.astype(np.float32), np.concatenate([R, t[:, None]], axis=1)


def same_poses(a, b):
    """two DevicePoses bit for bit (pose, counts, status and the mask)"""
    return all(torch.equal(x, y) for x, y in ((a.pose, b.pose), (a.n_inliers, b.n_inliers), (a.status, b.status), (a.inlier_mask, b.inlier_mask)))


# ---- sample ------------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("n", [4, 5, 64, 65])
def test_sample_indices_are_exact(pd, n):
    rng = np.array([[0, n], [n, n + 3], [n + 3, 2 * n + 3]], dtype=np.int32)      # F = 3: n rows, 3 rows (no trials), n rows
    for seed in (1, 2 ** 64 - 5):
        got = pd.stages.sample(dev_t(rng), 300, seed).cpu().numpy()
        want = orc.sample(rng, 300, seed)
        assert np.array_equal(got, want)
        assert (got[1] == -1).all() and got[0].min() >= 0 and got[0].max() < n


# ---- p3p ---------------------------------------------------------------------------------------------------------------------------------------
def test_p3p_matches_the_oracle_root_for_root(pd):
    """The CPU test's 200 samples, one trial each: the root counts equal the oracle's and every pose lies within 10 x e_p3p
    (``orc.E_P3P`` = 2.62e-08, the oracle's distance to the host library measured on the CPU): both sides are float64 restatements of
    one algorithm and differ by rounding only (here: the device's cbrt / cos / acos), hence one decade of margin.
    Measured on the MI355X: 2.23e-09."""
    samples = orc.p3p_samples()
    T = len(samples)
    rows = np.zeros((3 * T, 8))
    for i, (ray, X, _) in enumerate(samples):
        rows[3 * i:3 * i + 3, :3], rows[3 * i:3 * i + 3, 5:7] = X, ray
    idx = np.arange(3 * T, dtype=np.int32).reshape(1, T, 3)
    rng = np.array([[0, 3 * T]], dtype=np.int32)
    hyps, nsol = pd.stages.p3p(dev_t(rows), dev_t(rng), dev_t(idx))
    hyps, nsol = hyps.cpu().numpy()[0], nsol.cpu().numpy()[0]
    worst = 0.0
    for i, (ray, X, _) in enumerate(samples):
        want = orc.p3p_one(ray, X)
        assert nsol[i] == len(want), i
        for k, ps in enumerate(want):
            worst = max(worst, orc.pose_distance(hyps[4 * i + k], ps))
        assert np.isnan(hyps[4 * i + len(want):4 * i + 4]).all()                  # unused slots are marked
    print(f"p3p kernel vs oracle: largest relative pose difference {worst:.3e} (bound {10 * orc.E_P3P:.2e})")
    assert worst <= 10 * orc.E_P3P
    # samples the kernel must refuse: out of the frame, repeated rows (a degenerate triangle)
    bad = np.array([[[0, 1, 3 * T], [-1, 1, 2], [5, 5, 6]]], dtype=np.int32)
    h2, n2 = pd.stages.p3p(dev_t(rows), dev_t(rng), dev_t(bad))
    assert n2.cpu().tolist() == [[0, 0, 0]] and torch.isnan(h2).all()


# ---- score -------------------------------------------------------------------------------------------------------------------------------------
def score_case(n):
    """-> (K [3, 9-able], pts2d, pts3d, b_ids, hyps [3, H, 3, 4], ranges, rows) of the score test at frame size n"""
    sizes = (n, 0, 65)
    K = np.stack([scene(4, 0)[0], np.eye(3), np.array([[500.0, 0, 300.0], [0, 500.0, 200.0], [0, 0, 1]])])
    p2, p3, b_ids, hyp_list = [], [], [], []
    for f, m in enumerate(sizes):
        _, a, b, pose = scene(max(m, 4), 100 * n + f, K=K[f])
        p2.append(a[:m]); p3.append(b[:m]); b_ids.append(np.full(m, f, dtype=np.int64))
        hs = [pose, np.full((3, 4), np.nan), pose * np.array([1, 1, 1, -1.0])]
        if m >= 3:
            rows_f = orc.prep(K[f], a[:m], b[:m], m, None, 1)
            hs += pnp.p3p(rows_f[:3, 5:7], rows_f[:3, :3])
            hs += pnp.p3p(rows_f[m - 3:, 5:7], rows_f[m - 3:, :3])
        hyp_list.append(hs)
    H = max(len(h) for h in hyp_list)
    hyps = np.full((3, H, 3, 4), np.nan)
    for f, hs in enumerate(hyp_list):
        hyps[f, :len(hs)] = np.stack(hs)
    p2, p3, b_ids = np.concatenate(p2), np.concatenate(p3), np.concatenate(b_ids)
    cap = len(p2)
    rng = orc.ranges(b_ids, cap, cap, 3)
    rows = orc.prep(K, p2, p3, cap, b_ids, 3)
    thr2 = REPROJ * REPROJ
    for f in (0, 2):                                            # no (hypothesis, row) at the threshold: the counts are then a property of the data
        fin = np.isfinite(hyps[f].reshape(H, 12)).all(axis=1)
        _, e2 = orc.residuals(hyps[f][fin], rows[rng[f, 0]:rng[f, 1]], orc._intr(K, f))
        assert np.nanmin(np.abs(e2 - thr2)) > 1e-9 * thr2
    return K, p2, p3, b_ids, hyps, rng, rows


@pytest.mark.parametrize("n", [4, 63, 64, 65, 300])
def test_score_counts_exact_and_costs_to_rounding(pd, n):
    """F = 3 with ragged ranges (n rows, an empty frame, 65 rows; 300 is above the kernel's LDS chunk of 256 rows); the hypotheses are
    the test's: host P3P poses of the frame's first rows, the true pose, a NaN pose, a pose behind the camera."""
    assert n == 300 or n <= pd.SCORE_CHUNK
    K, p2, p3, b_ids, hyps, rng, rows = score_case(n)
    cap, H = len(p2), hyps.shape[1]
    want_cnt, want_cost = orc.score(rows, rng, K, hyps, REPROJ)
    count = dev_t(np.array([cap], dtype=np.int32))
    d_rng = pd.stages.ranges(dev_t(b_ids), count, cap, 3)
    d_rows = pd.stages.prep(dev_t(K), dev_t(p2), dev_t(p3), count, dev_t(b_ids), 3)
    assert np.array_equal(d_rng.cpu().numpy(), rng) and np.array_equal(d_rows.cpu().numpy(), rows)       # stage 1, bit for bit
    cnt, cost = pd.stages.score(d_rows, d_rng, dev_t(K), dev_t(hyps), REPROJ)
    cnt, cost = cnt.cpu().numpy(), cost.cpu().numpy()
    assert np.array_equal(cnt, want_cnt)
    assert want_cnt[0, 0] >= 0.5 * n and (want_cnt[:, 1] == 0).all() and (want_cnt[:, 2] == 0).all()      # true pose, NaN, behind the camera
    assert np.array_equal(np.isinf(cost), np.isinf(want_cost)) and np.isinf(cost[:, 1]).all()
    fin = np.isfinite(want_cost)
    rel = np.abs(cost[fin] - want_cost[fin]) / np.maximum(np.abs(want_cost[fin]), 1e-300)
    print(f"n = {n}: largest relative cost difference {rel.max():.2e}")
    assert rel.max() <= 1e-12


# ---- select ------------------------------------------------------------------------------------------------------------------------------------
def test_select_ties_and_needs_more(pd):
    """Crafted (count, cost) tables over three workgroup blocks of 1 024 hypotheses: a tie in count decided by cost across a block
    boundary, a tie in count and cost decided by the index across a boundary, a frame without a candidate; the needs_more bit against
    the formula on both sides of its threshold."""
    F, H, n = 4, 2500, 100
    assert H > 2 * pd.SELECT_BLOCK
    g = np.random.default_rng(3)
    cnt = g.integers(1, 40, size=(F, H)).astype(np.int32)
    cost = g.uniform(100, 200, size=(F, H))
    cnt[0, [5, 1030, 2049]] = 50; cost[0, [5, 1030, 2049]] = (120.0, 119.5, 119.75)         # count tie: the lowest cost wins, in block 1
    cnt[1, [1023, 1024, 2047]] = 50; cost[1, [1023, 1024, 2047]] = 77.0                    # count and cost tie: the lowest index wins
    cnt[1, 3] = 50; cost[1, 3] = 77.5
    cnt[2] = 0                                                                              # no candidate
    cnt[3, 2499] = 100; cost[3, 2499] = 500.0                                               # the count decides before the cost; last slot
    want_best = np.array([1030, 1023, -1, 2499], dtype=np.int32)
    K, p2, p3, pose = scene(F * n, 5, outliers=0.0)
    b_ids = np.repeat(np.arange(F), n).astype(np.int64)
    rng = orc.ranges(b_ids, F * n, F * n, F)
    rows = orc.prep(K, p2, p3, F * n, b_ids, F)
    hyps = np.tile(pose, (F, H, 1, 1))
    count = dev_t(np.array([F * n], dtype=np.int32))
    # needed_for(50 of 100) = ceil(log(0.01) / log(0.875)) = 35, and the quotient is not close to an integer
    q = np.log(0.01) / np.log(0.875)
    assert orc.needed_for(50, n, 0.99) == 35 and abs(q - round(q)) > 1e-6
    for trials, more in ((35, False), (34, True)):
        w_best, w_n, w_status, w_mask = orc.select(cnt, cost, rows, rng, K, hyps, REPROJ, 0.99, trials)
        assert np.array_equal(w_best, want_best)
        assert bool(w_status[0] & orc.STATUS_NEEDS_MORE) == more and w_status[2] == orc.STATUS_NO_POSE | orc.STATUS_NEEDS_MORE and w_status[3] == 0
        best, n_in, status, mask = pd.stages.select(dev_t(cnt), dev_t(cost), dev_t(rows), dev_t(rng), count, dev_t(K), dev_t(hyps), REPROJ, 0.99, trials)
        assert np.array_equal(best.cpu().numpy(), w_best)
        assert np.array_equal(n_in.cpu().numpy(), w_n) and np.array_equal(status.cpu().numpy(), w_status)
        assert np.array_equal(mask.cpu().numpy(), w_mask) and w_mask[:n].all() and not w_mask[2 * n:3 * n].any()


# ---- end to end ----------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("hard", [False, True], ids=["planted", "hard"])
def test_end_to_end_matches_the_host_solver(pd, hard):
    """The CPU test's two c1 frames, 1 024 trials: the inlier set of the host solver, status 0, the pose within the pose bar.
    Measured on the MI355X (seeds 1, 2, 3): planted 3.5e-12, 3.4e-12, 1.6e-11; hard 2.1e-13, 2.1e-13, 2.2e-11; against the oracle's pose
    (seed 3) 5.6e-17 and 1.8e-10."""
    K, p2, p3, _ = orc.c1_frame(hard, orc.FRAME_SEED)
    h_pose, _, h_inl = pnp.ransac_PnP(K, p2, p3, pnp_reprojection_error=REPROJ, use_pycolmap_ransac=True, seed=1)
    for seed in (1, 2, 3):
        out = pd.ransac_pnp(K, dev_t(p2), dev_t(p3), pnp_reprojection_error=REPROJ, trials=1024, seed=seed)
        (pose, homo, inl), = out.to_host()
        assert out.status.cpu().tolist() == [0] and out.n_inliers.cpu().tolist() == [len(h_inl)]
        assert np.array_equal(inl, h_inl) and np.array_equal(homo[:3], pose) and np.array_equal(homo[3], [0, 0, 0, 1])
        d = orc.pose_distance(pose, h_pose)
        print(f"{'hard' if hard else 'planted'} frame, seed {seed}: device pose vs host {d:.2e}")
        assert d < POSE_BAR
    o = orc.solve(K, p2, p3, reproj=REPROJ, trials=1024, seed=3)
    assert np.array_equal(np.nonzero(o["mask"])[0], inl)
    print(f"device pose vs oracle (seed 3): {orc.pose_distance(pose, o['pose'][0]):.2e}")
    assert orc.pose_distance(pose, o["pose"][0]) < POSE_BAR


@pytest.fixture(scope="module")
def matcher():
    if not torch.cuda.is_available():
        pytest.skip("needs the MI355X")
    from onepose_st_amd.config import default_config
    from onepose_st_amd.model import OnePosePlus_model
    from onepose_st_amd.synthetic import make_synthetic_state_dict
    cfg = default_config()
    sd = make_synthetic_state_dict(0, cfg)
    model = OnePosePlus_model(cfg).eval()
    model.load_state_dict(sd, strict=True)
    return model.to("cuda:0"), sd, cfg


@pytest.mark.parametrize("staged", [False, True], ids=["frame_call", "staged"])
@pytest.mark.parametrize("hard", [False, True], ids=["planted", "hard"])
def test_enqueue_after_a_pending_frame(pd, matcher, hard, staged):
    """The same two frames through the real matcher: ``enqueue_after`` on the ``PendingFrame``'s capacity-sized buffers before
    ``finish()`` equals ``ransac_pnp`` on the finished frame's matches bit for bit (``staged``: the launch-by-launch form of the frame,
    whose buffers are tensors of their own; otherwise the one-call frame's block).  Measured: 551 matches / 548 inliers (planted) and
    303 / 184 (hard), the host solver's sets, poses within 9.2e-12 of the host's."""
    from onepose_st_amd.synthetic import CONFIG_SIZES, HARD_PROFILE, make_synthetic_inputs
    model, sd, cfg = matcher
    n, hw, plant = CONFIG_SIZES["c1"]
    inp = make_synthetic_inputs(sd, n_points=n, image_hw=hw, n_plant=plant, seed=orc.FRAME_SEED, config=cfg, **(HARD_PROFILE if hard else {}))
    data = {k: inp[k].to("cuda:0") for k in ("keypoints3d", "descriptors3d_db", "descriptors3d_coarse_db")}
    K = inp["K"].numpy()
    pf = model.enqueue_features(data, inp["feat_c"].to("cuda:0"), inp["feat_f"].to("cuda:0"), inp["image_hw"], want_fine_debug=staged)
    assert (pf._slot is None) == staged
    early = pd.enqueue_after(pf, K, pnp_reprojection_error=REPROJ, trials=1024)
    pf.finish()
    n_matches = data["mkpts_3d_db"].shape[0]
    assert n_matches > 300 and early.inlier_mask.shape[0] == pf.cap > n_matches
    late = pd.ransac_pnp(K, data["mkpts_query_f"].contiguous(), data["mkpts_3d_db"].contiguous(), pnp_reprojection_error=REPROJ, trials=1024)
    (p_e, _, i_e), = early.to_host()
    (p_l, _, i_l), = late.to_host()
    assert np.array_equal(p_e, p_l) and np.array_equal(i_e, i_l) and early.status_host.tolist() == late.status_host.tolist() == [0]
    assert torch.equal(early.inlier_mask[:n_matches], late.inlier_mask) and not early.inlier_mask[n_matches:].any()
    h_pose, _, h_inl = pnp.ransac_PnP(K, data["mkpts_query_f"].cpu().numpy(), data["mkpts_3d_db"].cpu().numpy(), pnp_reprojection_error=REPROJ,
                                      use_pycolmap_ransac=True)
    print(f"real matcher, {n_matches} matches: {len(i_e)} device inliers, {len(h_inl)} host inliers, pose distance {orc.pose_distance(p_e, h_pose):.2e}")
    assert orc.pose_distance(p_e, inp["pose_gt"].numpy()) < 0.05 and len(i_e) >= 0.5 * n_matches           # a pose of this frame, not of another


# ---- edges -------------------------------------------------------------------------------------------------------------------------------------
def test_too_few_rows_give_no_pose(pd):
    K, p2, p3, _ = scene(8, 1)
    for n in (0, 3):
        out = pd.ransac_pnp(K, dev_t(p2[:n]), dev_t(p3[:n]), trials=64)
        (pose, _, inl), = out.to_host()
        assert out.status.cpu().tolist() == [pd.STATUS_NO_POSE] and out.n_inliers.cpu().tolist() == [0]
        assert np.array_equal(pose, orc.IDENTITY) and len(inl) == 0
    # a device-side count below 4 in a larger table
    out = pd.ransac_pnp(K, dev_t(p2), dev_t(p3), count=dev_t(np.array([3], dtype=np.int32)), trials=64)
    assert out.status.cpu().tolist() == [pd.STATUS_NO_POSE] and np.array_equal(out.to_host()[0][0], orc.IDENTITY)


def test_capacity_tail_count_clamp_and_repeatability(pd):
    n, cap = 150, 400
    K, p2, p3, _ = scene(n, 2)
    exact = pd.ransac_pnp(K, dev_t(p2), dev_t(p3), trials=512, seed=4)
    again = pd.ransac_pnp(K, dev_t(p2), dev_t(p3), trials=512, seed=4)
    assert same_poses(exact, again) and exact.status.cpu().tolist() == [0]                  # two runs, bit for bit
    t2, t3 = np.full((cap, 2), np.nan, dtype=np.float32), np.full((cap, 3), np.nan, dtype=np.float32)
    t2[:n], t3[:n] = p2, p3
    padded = pd.ransac_pnp(K, dev_t(t2), dev_t(t3), count=dev_t(np.array([n], dtype=np.int32)), trials=512, seed=4)
    assert torch.equal(padded.pose, exact.pose) and torch.equal(padded.n_inliers, exact.n_inliers) and torch.equal(padded.status, exact.status)
    assert torch.equal(padded.inlier_mask[:n], exact.inlier_mask) and not padded.inlier_mask[n:].any()
    assert np.array_equal(padded.to_host()[0][2], exact.to_host()[0][2])
    # a count above the capacity is clamped to it (valid buffers, judged by the result)
    over = pd.ransac_pnp(K, dev_t(p2), dev_t(p3), count=dev_t(np.array([n + 1000], dtype=np.int32)), trials=512, seed=4)
    assert same_poses(over, exact)
    under = pd.ransac_pnp(K, dev_t(p2), dev_t(p3), count=dev_t(np.array([-7], dtype=np.int32)), trials=512, seed=4)
    assert under.status.cpu().tolist() == [pd.STATUS_NO_POSE]


def test_frames_do_not_interfere(pd):
    """F = 3 with an empty frame in the middle equals three calls that hold one frame's rows each, bit for bit.  The draw of a trial is
    a function of (seed, frame, trial), so a call that holds frame f alone keeps it at index f (the other frames of that call are empty).
    Rows whose b_ids lie outside [0, F) belong to no frame: adding some in front and behind changes nothing."""
    sizes = (120, 0, 77)
    Ks = np.stack([scene(4, 0)[0], np.eye(3), np.array([[500.0, 0, 300.0], [0, 500.0, 200.0], [0, 0, 1]])])
    parts = [scene(max(m, 4), 40 + f, K=Ks[f]) for f, m in enumerate(sizes)]
    p2 = np.concatenate([p[1][:m] for p, m in zip(parts, sizes)])
    p3 = np.concatenate([p[2][:m] for p, m in zip(parts, sizes)])
    b_ids = np.concatenate([np.full(m, f, dtype=np.int64) for f, m in enumerate(sizes)])
    kw = dict(frames=3, trials=512, seed=6, pnp_reprojection_error=REPROJ)
    both = pd.ransac_pnp(dev_t(Ks), dev_t(p2), dev_t(p3), b_ids=dev_t(b_ids), **kw)
    assert both.status.cpu().tolist() == [0, pd.STATUS_NO_POSE, 0]
    res = both.to_host()
    assert np.array_equal(res[1][0], orc.IDENTITY) and len(res[1][2]) == 0
    for f in (0, 2):
        sel = b_ids == f
        one = pd.ransac_pnp(dev_t(Ks), dev_t(p2[sel]), dev_t(p3[sel]), b_ids=dev_t(b_ids[sel]), **kw)
        assert torch.equal(one.pose[f], both.pose[f]) and one.n_inliers[f] == both.n_inliers[f] and one.status[f] == both.status[f]
        assert torch.equal(one.inlier_mask, both.inlier_mask[torch.as_tensor(sel)])
        assert np.array_equal(one.to_host()[f][2], res[f][2]) and len(res[f][2]) >= 0.5 * sizes[f]
        assert orc.pose_distance(res[f][0], parts[f][3]) < 0.05
    # foreign rows: ids below 0 in front, ids >= F behind (the table stays ascending)
    junk2, junk3 = np.full((5, 2), 1e30, dtype=np.float32), np.full((5, 3), np.nan, dtype=np.float32)
    f2, f3 = np.concatenate([junk2, p2, junk2]), np.concatenate([junk3, p3, junk3])
    fb = np.concatenate([np.full(5, -3, dtype=np.int64), b_ids, np.array([3, 3, 4, 2 ** 40, 2 ** 62], dtype=np.int64)])
    foreign = pd.ransac_pnp(dev_t(Ks), dev_t(f2), dev_t(f3), b_ids=dev_t(fb), **kw)
    assert torch.equal(foreign.pose, both.pose) and torch.equal(foreign.status, both.status) and torch.equal(foreign.n_inliers, both.n_inliers)
    assert torch.equal(foreign.inlier_mask[5:-5], both.inlier_mask) and not foreign.inlier_mask[:5].any() and not foreign.inlier_mask[-5:].any()


def test_entry_refuses_bad_arguments_before_any_launch(pd):
    K, p2, p3, _ = scene(16, 1)
    d2, d3 = dev_t(p2), dev_t(p3)
    with pytest.raises(ValueError, match="frames > 1 needs b_ids"):
        pd.ransac_pnp(K, d2, d3, frames=2)
    count, Kd = dev_t(np.array([16], dtype=np.int32)), dev_t(K.reshape(1, 9))
    ws = torch.empty(pd.load().oppnpd_workspace_bytes(16, 1, 64), dtype=torch.uint8, device="cuda:0")
    pose, n_in, st, mask = (torch.zeros(12, dtype=torch.float64, device="cuda:0"), torch.zeros(1, dtype=torch.int32, device="cuda:0"),
                            torch.full((1,), -9, dtype=torch.int32, device="cuda:0"), torch.zeros(16, dtype=torch.uint8, device="cuda:0"))
    P = lambda t: t.data_ptr()      # noqa: E731

    def solve(cap=16, F=1, b=None, trials=64, conf=0.99, nbytes=None, reproj=5.0, scale=1.0):
        pd.call("oppnpd_solve", P(d2), P(d3), P(count), cap, b, F, P(Kd), 1, scale, reproj, conf, trials, 1, P(ws), ws.numel() if nbytes is None else nbytes,
                P(pose), P(n_in), P(st), P(mask), None)
    for bad, msg in ((dict(trials=0), "table sizes"), (dict(trials=65537), "table sizes"), (dict(cap=0), "table sizes"), (dict(F=2), "one frame"),
                     (dict(conf=1.0), "confidence"), (dict(nbytes=64), "workspace too small"), (dict(reproj=0.0), "reproj_err_px"),
                     (dict(scale=float("nan")), "scale")):
        with pytest.raises(ValueError, match=msg):
            solve(**bad)
    torch.cuda.synchronize()
    assert st.cpu().tolist() == [-9]                                # nothing was launched
    solve()
    torch.cuda.synchronize()
    assert st.cpu().tolist() == [0]


# ---- the sequence loop -----------------------------------------------------------------------------------------------------------------------------
class _FakeModel:
    """``tests/test_frameloop.py``'s stand-in for the matcher, with its matches left on the device"""

    def __init__(self, pts3d, poses, K):
        self.pts3d, self.poses, self.K, self.t, self.fail_at, self.trans = pts3d, poses, K, 0, set(), None

    def __call__(self, data):
        pose = self.poses[self.t]
        cam = pose[:, :3] @ self.pts3d.T + pose[:, 3:4]
        uv = self.K @ cam
        uv = (uv[:2] / uv[2:]).T
        uvc = (self.trans @ np.concatenate([uv, np.ones((len(uv), 1))], axis=1).T).T[:, :2]
        n = 4 if self.t in self.fail_at else len(uv)
        data["mkpts_3d_db"] = torch.tensor(self.pts3d[:n], dtype=torch.float32).to("cuda:0")
        data["mkpts_query_f"] = torch.tensor(uvc[:n], dtype=torch.float32).to("cuda:0")
        self.t += 1


def test_sequence_runner_device_pnp_follows_the_host_loop(pd):
    """The short synthetic sequence of ``test_frameloop.py`` (five frames, frame 2 loses the track) with ``pnp="device"`` and
    ``pnp="host"``: the same boxes and re-detection flags, poses within the pose bar (measured: 4.7e-09 - 5.5e-09, and 2.6e-08 on the
    four-match frame 2)."""
    g = np.random.default_rng(1)
    K = np.array([[900.0, 0, 320.0], [0, 900.0, 240.0], [0, 0, 1]])
    pts = g.uniform(-0.08, 0.08, size=(200, 3))
    bbox3d = 0.1 * np.array([[i, j, k] for i in (-1, 1) for j in (-1, 1) for k in (-1, 1)], dtype=np.float64)
    poses = []
    for t in range(5):
        a = 0.05 * t
        R = np.array([[np.cos(a), -np.sin(a), 0], [np.sin(a), np.cos(a), 0], [0, 0, 1]])
        poses.append(np.concatenate([R, [[0.01 * t], [0.0], [0.8]]], axis=1))
    block = {k: v.to("cuda:0") for k, v in (("keypoints3d", torch.zeros(1, 200, 3)), ("descriptors3d_db", torch.zeros(1, 128, 200)),
                                           ("descriptors3d_coarse_db", torch.zeros(1, 256, 200)))}
    runs = {}
    for mode in ("host", "device"):
        fake = _FakeModel(pts, poses, K)
        fake.fail_at = {2}
        calls = []

        def detector(frame, t):
            calls.append(t)
            return fl.project_bbox(K, poses[t], bbox3d)

        def crop_fn(dev_frame, bbox, S):
            fake.trans = fl.crop_geometry(bbox, K, S)[1]
            return torch.zeros(1, 1, S, S)

        recs = fl.SequenceRunner(fake, block, K, bbox3d, detector, crop_fn=crop_fn, pnp=mode).run([np.zeros((480, 640), np.uint8)] * 5)
        runs[mode] = (recs, calls)
    (h, h_calls), (d, d_calls) = runs["host"], runs["device"]
    assert h_calls == d_calls == [0, 3]
    for t, (a, b) in enumerate(zip(h, d)):
        assert a["redetected"] == b["redetected"] and np.array_equal(a["bbox"], b["bbox"]) and a["num_matches"] == b["num_matches"]
        assert np.array_equal(a["inliers"], b["inliers"]) and (len(a["inliers"]) >= 150 or t == 2)
        dist = orc.pose_distance(b["pose"], a["pose"])
        print(f"frame {t}: device pose vs host {dist:.2e}, {len(b['inliers'])} inliers")
        assert dist < POSE_BAR
