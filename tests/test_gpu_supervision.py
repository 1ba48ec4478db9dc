"""The supervised signals on the device (``onepose_st_amd/supervision.py``, ``libonepose_supervision.so``) against their numpy restatement
(tests/supervision_oracle.py): the ground truth and the fine targets bit for bit, the losses within a bound built from the oracle's own
spread under a change of summation order and the ulp bound of the device's float64 ``log`` / ``pow``, run-to-run bytes, and the chain
behind ``forward_features``.  Everything is small: M = 35 x 37 = 1 295 cells (no multiple of 64 or 256), at most 1 000 rows.

The ulp bound: the ROCm installation carries no statement of the accuracy of its float64 ``log`` and ``pow`` (no document under its tree
names one), so 4 ulp per call is ASSUMED, as DESIGN.md section 6s says."""
import numpy as np
import pytest
import torch

from tests import supervision_oracle as oracle

pytestmark = pytest.mark.gpu

DEV = "cuda:0"
HW = (280, 296)
W_C, M = 37, 35 * 37
ASSUMED_ULP = 4
EPS = 2.0 ** -52


@pytest.fixture(scope="module")
def sup():
    from onepose_st_amd import supervision
    supervision.load()
    return supervision


def dev(a, dtype=None):
    return torch.from_numpy(np.ascontiguousarray(a, dtype=dtype)).to(DEV)


def same_bytes(t, a):
    got = t.cpu().numpy()
    return got.dtype == a.dtype and got.shape == a.shape and got.tobytes() == np.ascontiguousarray(a).tobytes()


def check_gt(got, want):
    for key in ("gt_j", "gt_xy", "gt_i", "n_gt"):
        assert same_bytes(getattr(got, key), want[key]), (key, getattr(got, key).cpu().numpy(), want[key])


def run_gt(sup, s, counts=None, kp=None):
    return sup.ground_truth(dev(s["keypoints3d"]) if kp is None else kp, dev(s["point_ids"]), s["pose_gt"], s["K"], s["image_hw"],
                            counts=None if counts is None else dev(counts, np.int32))


# ---- 1. the ground truth ------------------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def scene3():
    """three frames with the planted rows, the last one exact; its oracle ground truth"""
    s = oracle.scene(21, B=3, N=130, A=96, image_hw=HW, exact_frame=True)
    return s, oracle.ground_truth(s["keypoints3d"], s["point_ids"], None, s["pose_gt"], s["K"], HW)


def test_ground_truth_planted_rows_bit_for_bit(sup, scene3):
    s, want = scene3
    got = run_gt(sup, s)
    check_gt(got, want)
    assert got.hw_c == (35, 37) and got.shape == (3, 130, M)
    ids = s["point_ids"][0]
    assert want["gt_j"][0, ids[0]] >= 0 and want["gt_j"][0, ids[1]] == -1         # two points, one cell: the first stays
    assert ids[2] == ids[3] and want["gt_j"][0, ids[2]] >= 0                      # the same point twice
    assert all(want["gt_j"][0, ids[r]] == -1 for r in range(4, 9)) and want["gt_j"][0, ids[9]] % W_C == 0     # the four sides
    assert want["gt_j"][0, ids[10]] >= 0                                          # BEHIND the camera, inside: ground truth
    assert ids[11] == -1 and ids[12] == 135                                       # ids out of range: dropped
    ids = s["point_ids"][2]                                                       # exact halves go to even
    assert [int(want["gt_j"][2, ids[r]]) for r in range(13, 17)] == [8 * 37 + 6, 9 * 37 + 6, 4 * 37 + 15, 6 * 37 + 16]
    again = run_gt(sup, s)                                                        # two runs, identical bytes
    for key in ("gt_j", "gt_xy", "gt_i", "n_gt"):
        assert same_bytes(getattr(again, key), getattr(got, key).cpu().numpy())
    conf_gt, loc_gt = got.to_dense()                                              # the dense form and back
    o_conf, o_loc = oracle.to_dense(want["gt_j"], want["gt_xy"], M)
    assert same_bytes(conf_gt, o_conf) and same_bytes(loc_gt, o_loc)
    check_gt(sup.GroundTruth.from_dense(conf_gt, loc_gt, (35, 37)), want)


def test_ground_truth_counts_and_sentinels(sup, scene3):
    s, _ = scene3
    counts = np.array([0, 1, 96], np.int32)
    want = oracle.ground_truth(s["keypoints3d"], s["point_ids"], counts, s["pose_gt"], s["K"], HW)
    assert want["n_gt"][0] == 0 and want["n_gt"][1] <= 1 and want["n_gt"][2] > 20
    dirty = dict(s, point_ids=s["point_ids"].copy())
    dirty["point_ids"][0, :] = 2 ** 40 + 7                                        # rows at or past the count are never read
    dirty["point_ids"][1, 1:] = -2 ** 40
    check_gt(run_gt(sup, dirty, counts), want)
    over = np.array([-5, 200, 3], np.int32)                                       # clamped into [0, A]
    check_gt(run_gt(sup, s, over), oracle.ground_truth(s["keypoints3d"], s["point_ids"], over, s["pose_gt"], s["K"], HW))


def test_ground_truth_shared_object_and_one_point(sup):
    s = oracle.scene(22, B=3, N=130, A=96, image_hw=HW, shared=True)
    want = oracle.ground_truth(s["keypoints3d"], s["point_ids"], None, s["pose_gt"], s["K"], HW)
    assert want["min_margin"] >= 1e-3 and want["n_gt"].min() > 10
    check_gt(run_gt(sup, s), want)                                                # [1, N, 3]
    check_gt(run_gt(sup, s, kp=dev(s["keypoints3d"]).expand(3, -1, -1)), want)    # a stride-0 expand
    check_gt(sup.ground_truth(dev(s["keypoints3d"]), dev(s["point_ids"]), dev(s["pose_gt"]), dev(s["K"][0]), HW),  # device tables, one K
             oracle.ground_truth(s["keypoints3d"], s["point_ids"], None, s["pose_gt"], s["K"][0], HW))
    one = {"keypoints3d": np.array([[[0.01, -0.02, 0.03]]], np.float32), "point_ids": np.array([[0, 0, 5]]), "pose_gt": s["pose_gt"][:1],
           "K": s["K"][:1], "image_hw": HW}
    want = oracle.ground_truth(one["keypoints3d"], one["point_ids"], None, one["pose_gt"], one["K"], HW)
    assert want["n_gt"].tolist() == [1]
    check_gt(run_gt(sup, one), want)


# ---- 2. the fine targets ------------------------------------------------------------------------------------------------------------------
def matches_of(gt, rng, extra=10):
    b, i = np.nonzero(gt["gt_j"] >= 0)
    on = np.stack([b, i, gt["gt_j"][b, i]], axis=1)
    off = on[::2].copy()
    off[:, 2] = (off[:, 2] + 1) % M
    nb, ni = np.nonzero(gt["gt_j"] < 0)
    none = np.stack([nb, ni, rng.integers(0, M, len(nb))], axis=1)[:extra]
    m = np.concatenate([on, off, none]).astype(np.int64)
    return m[np.lexsort((m[:, 1], m[:, 0]))]


@pytest.mark.parametrize("scaled", [False, True], ids=["plain", "scaled"])
def test_fine_targets_bit_for_bit(sup, scene3, scaled):
    s, want = scene3
    gt = run_gt(sup, s)
    m = matches_of(want, np.random.default_rng(5))
    cap = len(m)
    assert cap > 100
    scale = np.array([[1.25, 0.75], [1.0, 1.5], [0.5, 1.0]], np.float32) if scaled else None
    b_ids, i_ids, j_ids = (dev(m[:, k]) for k in range(3))
    for count in (None, 0, 1, cap, -3, cap + 9):
        out = torch.full((cap, 2), 777.0, device=DEV)
        got = sup.fine_targets(b_ids, i_ids, j_ids, gt, W_C, count=count, scale=None if scale is None else dev(scale), out=out)
        e = oracle.fine_targets(m[:, 0], m[:, 1], m[:, 2], count, want["gt_j"], want["gt_xy"], W_C, scale=scale)
        n = len(e)
        assert n == (cap if count is None else min(max(count, 0), cap))
        assert same_bytes(got[:n], e) and bool((got[n:] == 777.0).all())         # rows at or past the count are not written
    on = want["gt_j"][m[:, 0], m[:, 1]] == m[:, 2]
    assert on.sum() > 40 and (~on).sum() > 40
    if not scaled:
        # the reference's `else fine_scale`: on the ground truth and still outside the window, except in the image's first cells
        assert (np.abs(e[on]).max(axis=1) > 1.0).mean() > 0.9
    data = {"b_ids": b_ids, "i_ids": i_ids, "j_ids": j_ids, "q_hw_c": (35, 37), "ground_truth": gt}
    if scaled:
        data["query_image_scale"] = dev(scale)
    sup.fine_supervision(data, {"OnePosePlus": {"loftr_backbone": {"resolution": [8, 2]}, "loftr_fine": {"window_size": 5}}})
    assert same_bytes(data["expec_f_gt"], e)
    assert sup.fine_targets(b_ids[:0], i_ids[:0], j_ids[:0], gt, W_C).shape == (0, 2)


# ---- 3. the focal loss --------------------------------------------------------------------------------------------------------------------
def focal_bound(fwd, rev, key, calls):
    """16 x the oracle's spread under the reversed order + ``calls`` library calls per term at the assumed ulp bound"""
    return 16 * abs(fwd[key] - rev[key]) + calls * ASSUMED_ULP * EPS * abs(fwd[key])


def check_focal(got, conf, gt_j, **kw):
    fwd, rev = oracle.coarse_loss(conf, gt_j, **kw), oracle.coarse_loss(conf, gt_j, reverse=True, **kw)
    host = got.to_host()
    assert host["n_pos"] == fwd["n_pos"] and host["n_neg"] == fwd["n_neg"]
    calls = 1 if kw.get("gamma", 2.0) == 2.0 else 2
    for key in ("pos_sum", "neg_sum", "loss_c"):
        if np.isnan(fwd[key]):
            assert np.isnan(host[key]), key
            continue
        bound = focal_bound(fwd, rev, key, calls)
        print(f"{key}: device {host[key]!r} oracle {fwd[key]!r} |diff| {abs(host[key] - fwd[key]):.3e} bound {bound:.3e} "
              f"(spread {abs(fwd[key] - rev[key]):.3e})")
        assert abs(host[key] - fwd[key]) <= bound, key
    return host


def random_conf(rng, B, N, Mx, gt_j):
    conf = np.exp(rng.uniform(np.log(1e-9), np.log(0.5), (B, N, Mx))).astype(np.float32)
    b, i = np.nonzero((gt_j >= 0) & (gt_j < Mx))
    conf[b, i, gt_j[b, i]] = rng.uniform(0.05, 0.95, len(b)).astype(np.float32)
    return conf


def sparse_gt(sup, gt_j, Mx):
    B, N = gt_j.shape
    return sup.GroundTruth(dev(gt_j), torch.zeros(B, N, 2, device=DEV), torch.zeros(B, Mx, dtype=torch.int64, device=DEV),
                           torch.zeros(B, dtype=torch.int32, device=DEV), (1, Mx))


@pytest.mark.parametrize("B,N,Mx", [(1, 1, M), (3, 130, M), (1, 1000, 1200)], ids=["one_row", "batch", "c1"])
@pytest.mark.parametrize("gamma", [2.0, 1.5])
def test_coarse_loss(sup, B, N, Mx, gamma):
    rng = np.random.default_rng(B * 1000 + N)
    gt_j = np.where(rng.uniform(size=(B, N)) < 0.6, rng.integers(0, Mx, (B, N)), -1).astype(np.int64)
    conf = random_conf(rng, B, N, Mx, gt_j)
    conf[0, 0, :5] = [0.0, 3e-7, 1.0, 0.9999995, 1e-6]      # 0, below the clamp, 1.0, above the upper clamp, at the clamp: in one row
    gt = sparse_gt(sup, gt_j, Mx)
    kw = dict(gamma=gamma, alpha=0.25, pos_weight=1.0, neg_weight=1.0)
    first = sup.coarse_loss(dev(conf), gt, **kw)
    check_focal(first, conf, gt_j, **kw)
    # a non-contiguous batch and row stride: the matrix inside a larger one
    big = torch.full((B, N + 3, Mx + 5), 0.5, device=DEV)
    big[:, :N, :Mx] = dev(conf)
    view = big[:, :N, :Mx]
    assert view.stride() == ((N + 3) * (Mx + 5), Mx + 5, 1)
    second = sup.coarse_loss(view, gt, **kw)
    assert second._keep[0].data_ptr() == big.data_ptr()                          # read where it lies: no copy
    assert same_bytes(second.sums, first.sums.cpu().numpy()) and same_bytes(second.counts, first.counts.cpu().numpy())      # identical bytes


def test_coarse_loss_branches_and_nan(sup):
    rng = np.random.default_rng(9)
    none = np.full((3, 130), -1, np.int64)
    conf = random_conf(rng, 3, 130, M, none)
    host = check_focal(sup.coarse_loss(dev(conf), sparse_gt(sup, none, M), neg_weight=0.5), conf, none, neg_weight=0.5)     # no positive at all
    assert host["n_pos"] == 0 and host["pos_sum"] == 0.0
    one = np.array([[[0.25]]], np.float32)                                       # N = M = 1, its one element positive: no negative
    host = check_focal(sup.coarse_loss(dev(one), sparse_gt(sup, np.zeros((1, 1), np.int64), 1), pos_weight=2.0), one, np.zeros((1, 1), np.int64),
                       pos_weight=2.0)
    assert host["n_neg"] == 0 and host["neg_sum"] == 0.0 and host["loss_c"] > 0
    gt_j = np.where(rng.uniform(size=(3, 130)) < 0.5, rng.integers(0, M, (3, 130)), -1).astype(np.int64)
    conf = random_conf(rng, 3, 130, M, gt_j)
    conf[1, 7, 300:305] = [0.0, 3e-7, 1.0, 0.9999995, np.nan]                     # all five in one row: NaN propagates, the counts stay exact
    host = check_focal(sup.coarse_loss(dev(conf), sparse_gt(sup, gt_j, M)), conf, gt_j)
    assert np.isnan(host["loss_c"]) and host["n_pos"] == int((gt_j >= 0).sum())
    far = gt_j.copy()
    far[0, 0] = M + 3                                                             # a cell outside the matrix is no positive
    check_focal(sup.coarse_loss(dev(conf[:1]), sparse_gt(sup, far[:1], M)), conf[:1], far[:1])


# ---- 4. the fine loss ---------------------------------------------------------------------------------------------------------------------
def check_fine(sup, e, g, count=None, training=False, thr=1.0):
    loss_f, n_correct, status = sup.fine_loss(dev(e), dev(g), count=count, correct_thr=thr, training=training)
    fwd = oracle.fine_loss(e, g, count=count, correct_thr=thr, training=training)
    rev = oracle.fine_loss(e, g, count=count, correct_thr=thr, training=training, reverse=True)
    assert int(status.item()) == fwd["status"] and int(n_correct.item()) == fwd["n_correct"]
    got = float(loss_f.item())
    if np.isnan(fwd["loss_f"]):
        assert np.isnan(got)
    else:
        bound = 16 * abs(fwd["loss_f"] - rev["loss_f"])                          # + - * / only: no library call, no ulp term
        print(f"loss_f: device {got!r} oracle {fwd['loss_f']!r} |diff| {abs(got - fwd['loss_f']):.3e} bound {bound:.3e}")
        assert abs(got - fwd["loss_f"]) <= bound
    return fwd


@pytest.mark.parametrize("cap", [1, 1000])
def test_fine_loss(sup, cap):
    rng = np.random.default_rng(cap)
    e = np.concatenate([rng.uniform(-0.6, 0.6, (cap, 2)), rng.uniform(0.05, 0.9, (cap, 1))], axis=1).astype(np.float32)
    g = rng.uniform(-1.6, 1.6, (cap, 2)).astype(np.float32)
    g[0] = (0.3, -0.2)
    e[-1, 2] = 0.0                                                                # a std below the clamp
    assert check_fine(sup, e, g)["status"] == oracle.OK
    assert check_fine(sup, e, g, training=True)["status"] == oracle.OK
    for count in (1, cap // 2 + 1, cap + 5, -2):
        check_fine(sup, e, g, count=count)
    far = np.full((cap, 2), 3.0, np.float32)
    assert check_fine(sup, e, far)["status"] == oracle.NONE                       # eval: NONE
    assert check_fine(sup, e, far, training=True)["status"] == oracle.FORCED      # the training corner case
    assert check_fine(sup, e, far, count=0, training=True)["status"] == oracle.EMPTY
    g[0, 0] = np.nan
    check_fine(sup, e, g)                                                         # a NaN target is not correct


# ---- the chain ----------------------------------------------------------------------------------------------------------------------------
LOSS_CONFIG = {"coarse_type": "focal", "coarse_weight": 1.0, "focal_alpha": 0.25, "focal_gamma": 2.0, "pos_weight": 1.0, "neg_weight": 1.0,
               "fine_type": "l2_with_std", "fine_weight": 0.5, "fine_correct_thr": 1.0}


def test_chain_behind_forward_features(sup, monkeypatch):
    from onepose_st_amd.config import default_config
    from onepose_st_amd.model import OnePosePlus_model
    from onepose_st_amd.synthetic import make_synthetic_inputs, make_synthetic_state_dict
    cfg = default_config()
    sd = make_synthetic_state_dict(0, cfg)
    model = OnePosePlus_model(cfg).eval()
    model.load_state_dict(sd, strict=True)
    model.to(DEV)
    inp = make_synthetic_inputs(sd, n_points=400, image_hw=(96, 136), n_plant=150, seed=11, config=cfg)

    def features():
        data = {k: inp[k].to(DEV) for k in ("keypoints3d", "descriptors3d_db", "descriptors3d_coarse_db")}
        model.forward_features(data, inp["feat_c"].to(DEV), inp["feat_f"].to(DEV), inp["image_hw"])
        return data
    plain, data = features(), features()
    before = {k: v.clone() for k, v in data.items() if isinstance(v, torch.Tensor)}
    pose = np.eye(4)
    pose[:3] = inp["pose_gt"].numpy()
    ids = np.arange(400, dtype=np.int64)[None]
    gt = sup.ground_truth(data["keypoints3d"], dev(ids), pose[None], inp["K"].numpy(), inp["image_hw"])
    want = oracle.ground_truth(inp["keypoints3d"].numpy(), ids, None, pose[None], inp["K"].numpy(), inp["image_hw"])
    check_gt(gt, want)
    assert want["n_gt"][0] > 100
    data["ground_truth"] = gt
    data["query_image_scale"] = torch.ones(1, 2, device=DEV)                      # as a data loader gives it: the coarse scale is then 8
    sup.fine_supervision(data, {"OnePosePlus": cfg})
    loss = sup.Loss(LOSS_CONFIG).eval()
    reads = []
    real_cpu = torch.Tensor.cpu
    monkeypatch.setattr(torch.Tensor, "cpu", lambda t, *a, **k: (reads.append(t.numel()), real_cpu(t, *a, **k))[1])
    for name in ("item", "tolist"):
        monkeypatch.setattr(torch.Tensor, name, lambda t, *a, _n=name, **k: pytest.fail(f"Tensor.{_n}() in Loss.forward"))
    loss(data)
    monkeypatch.undo()
    assert reads == [8 + 8 + 4 + 8]                                               # ONE packed read-back: loss_c, loss_f, status, loss
    m = np.stack([data[k].cpu().numpy() for k in ("b_ids", "i_ids", "j_ids")], axis=1)
    assert len(m) > 50
    e_gt = oracle.fine_targets(m[:, 0], m[:, 1], m[:, 2], None, want["gt_j"], want["gt_xy"], 17, scale=np.ones((1, 2), np.float32))
    assert same_bytes(data["expec_f_gt"], e_gt)
    conf, expec_f = data["conf_matrix"].cpu().numpy(), data["expec_f"].cpu().numpy()
    coarse, coarse_rev = (oracle.coarse_loss(conf, want["gt_j"], reverse=r) for r in (False, True))
    fine, fine_rev = (oracle.fine_loss(expec_f, e_gt, reverse=r) for r in (False, True))
    assert fine["status"] == oracle.OK and fine["n_correct"] > 20
    total, total_rev = (oracle.total_loss(c["loss_c"], f, 1.0, 0.5) for c, f in ((coarse, fine), (coarse_rev, fine_rev)))
    scalars = data["loss_scalars"]
    assert set(scalars) == {"loss_c", "loss_f", "loss"} and all(isinstance(v, float) for v in scalars.values())
    for key in ("loss_c", "loss_f", "loss"):
        bound = 16 * abs(total[key] - total_rev[key]) + ASSUMED_ULP * EPS * abs(total[key])
        print(f"{key}: device {scalars[key]!r} oracle {total[key]!r} bound {bound:.3e}")
        assert abs(scalars[key] - total[key]) <= bound, key
    assert data["loss"].dtype == torch.float64 and data["loss"].is_cuda and float(data["loss"]) == scalars["loss"]
    # every key the model wrote is what a run without the supervision leaves
    for k, v in plain.items():
        if isinstance(v, torch.Tensor):
            assert torch.equal(v, data[k]) and torch.equal(before[k], data[k]), k
        elif isinstance(v, (int, float, str, tuple)):        # sizes and flags (torch.Size is a tuple)
            assert data[k] == v, k
    assert set(data) - set(plain) == {"ground_truth", "query_image_scale", "expec_f_gt", "loss", "loss_scalars"}
    # the dense keys of a reference data loader give the same losses
    conf_gt, loc_gt = gt.to_dense()
    dense = {k: v for k, v in data.items() if k in plain or k == "query_image_scale"}
    dense.update(conf_matrix_gt=conf_gt, fine_location_matrix_gt=loc_gt)
    sup.fine_supervision(dense, {"OnePosePlus": cfg})
    sup.Loss(LOSS_CONFIG).eval()(dense)
    assert torch.equal(dense["expec_f_gt"], data["expec_f_gt"]) and dense["loss_scalars"] == scalars
