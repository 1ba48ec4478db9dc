"""The loss backward on the device (``onepose_st_amd/loss_backward.py``, ``libonepose_loss_backward.so``) against its numpy float64
restatement (tests/loss_backward_oracle.py): the coarse gradients within the precision bar that tests/test_loss_backward_cpu.py derives from
a float32 split-bf16 stand-in over these very cases (tests/loss_backward_cases.py), identical bytes run to run and batch to halves, the fine
gradients within one float32 rounding, and the chain behind the training-mode forward.  Every buffer of a call sits on a guarded arena
(tests/guarded.py); outputs are NaN-filled with spare rows that must stay NaN.  Everything is small: at most 2 x 300 x 1 295."""
import numpy as np
import pytest
import torch

from tests import guarded
from tests import loss_backward_cases as cases
from tests import loss_backward_oracle as oracle

pytestmark = pytest.mark.gpu

DEV = "cuda:0"
SPARE = 3


@pytest.fixture(scope="module")
def bwd():
    from onepose_st_amd import loss_backward
    loss_backward.load()
    assert (loss_backward.OWNED_ROWS, loss_backward.SWEPT_ROWS) == (cases.R, cases.S)
    return loss_backward


def sparse_gt(arena, gt_j, gt_i):
    from onepose_st_amd import supervision
    B, N = gt_j.shape
    return supervision.GroundTruth(arena.put(torch.from_numpy(gt_j).to(DEV), name="gt_j"), torch.zeros(B, N, 2, device=DEV),
                                   arena.put(torch.from_numpy(gt_i).to(DEV), name="gt_i"), torch.zeros(B, dtype=torch.int32, device=DEV),
                                   (1, gt_i.shape[1]))


def spare_out(arena, shape, name):
    """A NaN-filled output of ``shape`` with SPARE more rows behind it -> (the output, the spare rows)"""
    rows = int(np.prod(shape[:-1]))
    whole = arena.typed((rows + SPARE, shape[-1]), torch.float32, name=name)
    return whole[:rows].view(*shape), whole[rows:]


def run_coarse(bwd, case, kw):
    """-> (grad0, grad1) as numpy; the arena is checked, the spare rows are still NaN, every written value is finite"""
    B, N = case["gt_j"].shape
    M = case["gt_i"].shape[1]
    need = 20 * B * (N + M + 64) * cases.C + 24 * guarded.GUARD          # features and gradients 8, the workspace 8 bytes per row and channel
    arena = guarded.Arena(DEV, need)
    f0, f1 = arena.put(torch.from_numpy(case["feat0"]).to(DEV), name="feat0"), arena.put(torch.from_numpy(case["feat1"]).to(DEV), name="feat1")
    gt = sparse_gt(arena, case["gt_j"], case["gt_i"])
    (g0, s0), (g1, s1) = spare_out(arena, (B, N, cases.C), "grad0"), spare_out(arena, (B, M, cases.C), "grad1")
    with guarded.guarded_empty(arena, 0xFF, [bwd]):            # the workspace: poisoned, on the arena
        got = bwd.coarse_grads(f0, f1, gt, temperature=cases.TEMPERATURE, out=(g0, g1), **kw)
    torch.cuda.synchronize()
    assert got[0] is g0 and got[1] is g1
    arena.check()
    assert bool(torch.isnan(s0).all()) and bool(torch.isnan(s1).all())
    a0, a1 = g0.cpu().numpy(), g1.cpu().numpy()
    assert np.isfinite(a0).all() and np.isfinite(a1).all()
    return a0, a1


_WANT = {}


def want_of(name):
    """The case and its float64 oracle, computed once and shared"""
    if name not in _WANT:
        args, kw = cases.COARSE_CASES[name]
        case = cases.coarse_case(**args)
        _WANT[name] = (case, kw, oracle.coarse_grads(case["feat0"], case["feat1"], case["gt_j"], cases.TEMPERATURE, **kw))
    return _WANT[name]


# ---- 1. the coarse gradient ---------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", list(cases.COARSE_CASES))
def test_coarse_parity_within_the_bar(bwd, name):
    case, kw, want = want_of(name)
    assert want["pos_margin"] >= 0.01 and want["hi_margin"] >= 1e-9           # the condition on the inputs (chosen on the CPU)
    g0, g1 = run_coarse(bwd, case, kw)
    e0, e1 = oracle.frame_error(g0, want["grad0"]), oracle.frame_error(g1, want["grad1"])
    print(f"{name}: frame_error grad0 {e0:.3e} grad1 {e1:.3e} (bar {cases.COARSE_BAR:.1e}); max |grad0| {np.abs(want['grad0']).max():.3e}")
    assert e0 <= cases.COARSE_BAR and e1 <= cases.COARSE_BAR, (e0, e1)


def test_coarse_what_the_cases_are_there_for(bwd):
    """What the parity cases hold, on the float64 oracle: positives below 1e-6 (no direct gradient), confident positives and confident
    negatives, one positive above 1 - 1e-6, a batch without a positive, a frame without one in a batch that has some"""
    _, _, big = want_of("c1_like")
    conf, pos = big["conf"], big["is_pos"]
    assert (conf[pos] < 1e-6).sum() > 10 and (conf[pos] > 0.5).sum() > 100 and (conf[~pos] > 0.1).sum() > 10
    _, _, pushed = want_of("pushed")
    assert (pushed["conf"][pushed["is_pos"]] > oracle.HI).sum() == 1
    _, _, none = want_of("no_positive")
    assert none["n_pos"] == 0 and np.abs(none["grad0"]).max() > 0
    case, _, one = want_of("one_empty_frame")
    assert (case["gt_j"][1] < 0).all() and (case["gt_j"][0] >= 0).any() and np.abs(one["grad0"][1]).max() > 0


def test_coarse_identical_bytes(bwd):
    args = dict(seed=21, B=2, N=cases.R + 3, M=2 * cases.S + 5)
    case = cases.coarse_case(**args)
    assert (case["gt_j"][0] >= 0).sum() == (case["gt_j"][1] >= 0).sum() > 0         # the halves have the same n_pos
    first, again = run_coarse(bwd, case, {}), run_coarse(bwd, case, {})
    for a, b in zip(first, again):
        assert a.tobytes() == b.tobytes()
    for b in range(2):                                                              # a frame alone, its weights halved: the same bytes
        half = {k: v[b:b + 1] for k, v in case.items()}
        g0, g1 = run_coarse(bwd, half, dict(pos_weight=0.5, neg_weight=0.5))
        assert g0.tobytes() == first[0][b:b + 1].tobytes() and g1.tobytes() == first[1][b:b + 1].tobytes()


# ---- 2. the fine gradient -----------------------------------------------------------------------------------------------------------------
def run_fine(bwd, case, count, training=True, scale=1.0):
    cap, WW = case["feat_f1"].shape[:2]
    arena = guarded.Arena(DEV, 12 * cap * (WW + 1) * cases.CF + 16 * guarded.GUARD)
    ins = {k: arena.put(torch.from_numpy(v).to(DEV), name=k) for k, v in case.items()}
    g0, g1 = arena.typed((cap, cases.CF), torch.float32, name="grad_f0"), arena.typed((cap, WW, cases.CF), torch.float32, name="grad_f1")
    cnt = None if count is None else arena.put(torch.tensor([count], dtype=torch.int32, device=DEV), name="count")
    with guarded.guarded_empty(arena, 0xFF, [bwd]):
        got = bwd.fine_grads(ins["feat_f0"], ins["feat_f1"], ins["expec_f"], ins["expec_f_gt"], count=cnt, training=training, scale=scale, out=(g0, g1))
    torch.cuda.synchronize()
    arena.check()
    return g0.cpu().numpy(), g1.cpu().numpy(), int(got[2].item()), int(got[3].item())


def check_fine(got, want, n):
    g0, g1, n_correct, status = got
    assert (n_correct, status) == (want["n_correct"], want["status"])
    assert np.isnan(g0[n:]).all() and np.isnan(g1[n:]).all()                        # rows at or past the count are never written
    assert np.isfinite(g0[:n]).all() and np.isfinite(g1[:n]).all()
    for k in range(n):
        for g, w in ((g0[k], want["grad_f0"][k]), (g1[k], want["grad_f1"][k])):
            assert np.abs(g - w).max() <= cases.FINE_RTOL * np.abs(w).max(), (k, np.abs(g - w).max(), np.abs(w).max())


@pytest.mark.parametrize("W", [3, 5, 11])
@pytest.mark.parametrize("cap", [1, 255, 256, 257])
def test_fine_parity(bwd, cap, W):
    case = cases.fine_case(100 * cap + W, cap, W)
    if cap == 1:
        case["expec_f_gt"][0] = (0.3, -0.4)
    count = cap if cap == 1 else cap - 2                                            # a device count below the capacity
    want = oracle.fine_grads(**case, count=count, scale=0.5)
    correct = np.abs(case["expec_f_gt"][:count]).max(axis=1) < 1.0
    assert want["status"] == oracle.OK and want["n_correct"] == correct.sum() and (cap == 1 or 0 < correct.sum() < count)
    assert all((np.abs(want["grad_f0"][k]).max() > 0) == bool(correct[k]) for k in range(count))
    check_fine(run_fine(bwd, case, count, scale=0.5), want, count)


def test_fine_statuses(bwd):
    far = cases.fine_case(7, 70, 5, far=True)
    forced = oracle.fine_grads(**far, count=66, training=True)
    assert forced["status"] == oracle.FORCED and forced["n_correct"] == 1
    assert np.abs(forced["grad_f0"][0]).max() > 0 and not forced["grad_f0"][1:].any() and not forced["grad_f1"][1:].any()
    check_fine(run_fine(bwd, far, 66, training=True), forced, 66)
    none = oracle.fine_grads(**far, count=66, training=False)
    assert none["status"] == oracle.NONE and not none["grad_f0"].any()
    check_fine(run_fine(bwd, far, 66, training=False), none, 66)
    empty = oracle.fine_grads(**far, count=0, training=True)
    assert empty["status"] == oracle.EMPTY
    check_fine(run_fine(bwd, far, 0, training=True), empty, 0)
    whole = cases.fine_case(8, 40, 5)                                               # no count: every row
    check_fine(run_fine(bwd, whole, None), oracle.fine_grads(**whole), 40)


# ---- 3. the chain -------------------------------------------------------------------------------------------------------------------------
LOSS_CONFIG = {"coarse_type": "focal", "coarse_weight": 1.0, "focal_alpha": 0.25, "focal_gamma": 2.0, "pos_weight": 1.0, "neg_weight": 1.0,
               "fine_type": "l2_with_std", "fine_weight": 0.5, "fine_correct_thr": 1.0}
HW, NP, SEED = (32, 40), 64, 3                                                      # tests/test_gpu_train_forward.py's small scene


def test_the_chain_behind_the_training_forward(bwd):
    from onepose_st_amd import supervision
    from onepose_st_amd.config import default_config
    from onepose_st_amd.model import OnePosePlus_model
    from onepose_st_amd.synthetic import make_synthetic_inputs, make_synthetic_state_dict
    cfg = default_config()
    cfg["coarse_matching"]["border_rm"] = 0
    cfg["coarse_matching"]["train"].update(train_coarse_percent=0.3, train_pad_num_gt_min=4)
    cfg.update(hip_train_forward=True, hip_train_seed=SEED)
    sd = make_synthetic_state_dict(0, cfg)
    frames = [make_synthetic_inputs(sd, n_points=NP, image_hw=HW, n_plant=16, seed=11, config=cfg, frame=f) for f in range(2)]
    feat_c, feat_f = (torch.cat([f[k] for f in frames]).to(DEV) for k in ("feat_c", "feat_f"))
    pose = np.stack([np.eye(4)] * 2)
    for b, f in enumerate(frames):
        pose[b, :3] = f["pose_gt"].numpy()
    ids = torch.from_numpy(np.stack([np.arange(NP, dtype=np.int64)] * 2)).to(DEV)
    gt = supervision.ground_truth(frames[0]["keypoints3d"].to(DEV), ids, pose, frames[0]["K"].numpy(), HW)

    def run(keep):
        model = OnePosePlus_model({**cfg, "hip_keep_features": keep})
        model.load_state_dict(sd, strict=True)
        model.to(DEV).train()
        data = {k: frames[0][k].to(DEV) for k in ("keypoints3d", "descriptors3d_db", "descriptors3d_coarse_db")}
        data["ground_truth"] = gt
        data["query_image_scale"] = torch.ones(2, 2, device=DEV)    # (with it fine_supervision's coarse scale is the coarse one: correct rows)
        model.enqueue_features(data, feat_c, feat_f, HW).finish()
        supervision.fine_supervision(data, {"OnePosePlus": cfg})
        supervision.Loss(LOSS_CONFIG).train()(data)
        return data

    plain, kept = run(False), run(True)
    assert set(kept) - set(plain) == {"feat_c0", "feat_c1", "feat_f0", "feat_f1"}     # without the key, no new entry
    for key in plain:
        if isinstance(plain[key], torch.Tensor):
            assert torch.equal(plain[key], kept[key]), key
    with pytest.raises(KeyError, match="hip_keep_features"):
        bwd.backward(plain, LOSS_CONFIG, {"OnePosePlus": cfg})
    T = kept["expec_f"].shape[0]
    assert kept["feat_c0"].shape == (2, NP, 256) and kept["feat_c1"].shape == (2, 20, 256)
    assert kept["feat_f0"].shape == (T, 128) and kept["feat_f1"].shape == (T, 25, 128) and T == 12
    bwd.backward(kept, LOSS_CONFIG, {"OnePosePlus": cfg}, grad=2.0)
    host = {k: kept[k].cpu().numpy() for k in ("feat_c0", "feat_c1", "feat_f0", "feat_f1", "expec_f", "expec_f_gt")}
    coarse = oracle.coarse_grads(host["feat_c0"], host["feat_c1"], gt.gt_j.cpu().numpy(), cfg["coarse_matching"]["dual_softmax"]["temperature"],
                                 scale=2.0 * LOSS_CONFIG["coarse_weight"])
    print(f"chain: pos_margin {coarse['pos_margin']:.3g} hi_margin {coarse['hi_margin']:.3g} n_pos {coarse['n_pos']}")
    assert coarse["pos_margin"] >= 0.01 and coarse["hi_margin"] >= 1e-9
    for key, want in (("grad_feat_c0", coarse["grad0"]), ("grad_feat_c1", coarse["grad1"])):
        err = oracle.frame_error(kept[key].cpu().numpy(), want)
        print(f"chain: {key} frame_error {err:.3e}")
        assert err <= cases.COARSE_BAR, (key, err)
    fine = oracle.fine_grads(host["feat_f0"], host["feat_f1"], host["expec_f"], host["expec_f_gt"], scale=2.0 * LOSS_CONFIG["fine_weight"])
    assert fine["status"] == oracle.OK and fine["n_correct"] >= 4
    check_fine((kept["grad_feat_f0"].cpu().numpy(), kept["grad_feat_f1"].cpu().numpy(), fine["n_correct"], fine["status"]), fine, T)
