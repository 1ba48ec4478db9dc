"""The supervised signals (``onepose_st_amd/supervision.py``, include/ext/onepose_supervision.h) without a GPU: the
numpy oracle (``tests/supervision_oracle.py``) against what the reference itself computed (``tests/golden/supervision_small.npz``, recipe
``tests/golden/make_supervision_golden.py``), the seeded faults the oracle must notice, and the binding's header-driven parts."""
import ctypes
import os
import re

import numpy as np
import pytest
import torch

from onepose_st_amd import cabi, hip, supervision
from tests import supervision_oracle as oracle

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

# The bars, each 4 x what was measured on the CPU when the golden was made (DESIGN.md section 6s has the figures):
# the written-order float32 projection against torch's ``R @ X + t`` / ``K @`` on the golden's scene: 3.0517578e-05 px (one ulp at 256 px)
XY_BAR = 4 * 3.0517578e-05
# the float64 losses against the reference's float32 ones: 9.892872e-07 relative, on loss_c.  Not summation noise alone: the golden's
# conf_matrix holds 1.0 and 0.9999995, and the reference's float32 clamp leaves 1 - c = 1.0132790e-06 where float64 leaves 1.0e-06
LOSS_BAR = 4 * 9.892872e-07


@pytest.fixture(scope="module")
def golden():
    g = dict(np.load(os.path.join(REPO, "tests", "golden", "supervision_small.npz")))
    g["hw"] = tuple(int(v) for v in g["image_hw"])
    g["gt"] = oracle.ground_truth(g["keypoints3d"], g["point_ids"], None, g["pose_gt"], g["K"], g["hw"])
    return g


def test_golden_is_the_seeded_scene(golden):
    from tests.golden import make_supervision_golden as recipe
    s, gt, conf, matches, expec_f, scale = recipe.make_inputs(oracle)
    for key in ("keypoints3d", "point_ids", "pose_gt", "K"):
        assert np.array_equal(s[key], golden[key]), key
    assert np.array_equal(conf, golden["conf_matrix"]) and np.array_equal(matches, golden["matches"])
    assert np.array_equal(expec_f, golden["expec_f"]) and np.array_equal(scale, golden["scale"])
    first = oracle.ground_truth(s["keypoints3d"][:1], s["point_ids"][:1], None, s["pose_gt"][:1], s["K"][:1], s["image_hw"])
    assert first["min_margin"] >= 1e-3                                           # the frame that is not exact: no decision can flip


def test_oracle_tables_against_the_reference(golden):
    gt, where = golden["gt"], golden["ref_gt_where"]
    B, N = gt["gt_j"].shape
    M = gt["gt_i"].shape[1]
    assert M == 35 * 37 and len(where) > 60
    want_j = np.full((B, N), -1, np.int64)
    want_j[where[:, 0], where[:, 1]] = where[:, 2]
    assert len(set(map(tuple, where[:, :2]))) == len(where)                       # a row of the dense matrix has at most one entry
    assert np.array_equal(gt["gt_j"], want_j)
    want_i = np.full((B, M), -1, np.int64)
    want_i[where[:, 0], where[:, 2]] = where[:, 1]
    assert np.array_equal(gt["gt_i"], want_i)
    assert np.array_equal(gt["n_gt"], np.bincount(where[:, 0], minlength=B))
    diff = np.abs(gt["gt_xy"][where[:, 0], where[:, 1]] - golden["ref_gt_xy"]).max()
    print(f"max |gt_xy - reference| = {diff:.3e} px (bar {XY_BAR:.3e})")
    assert diff <= XY_BAR
    assert np.all(gt["gt_xy"][gt["gt_j"] < 0] == -50)
    # the planted rows did what they are there for
    ids = golden["point_ids"][0]
    assert gt["gt_j"][0, ids[0]] >= 0 and gt["gt_j"][0, ids[1]] == -1             # two points, one cell: the first stays
    assert gt["gt_j"][0, ids[2]] >= 0 and ids[2] == ids[3]                        # the same point twice
    assert all(gt["gt_j"][0, ids[r]] == -1 for r in range(4, 9))                  # out of each side, and rounded out
    assert gt["gt_j"][0, ids[9]] % 37 == 0                                        # outside, rounded in: column 0
    assert gt["gt_j"][0, ids[10]] >= 0                                            # BEHIND the camera: the reference has no depth test
    ids = golden["point_ids"][1]                                                  # the exact frame: halves go to even
    # x 5.5 -> 6, x 6.5 -> 6, y 4.5 -> 4, y 5.5 -> 6
    assert [int(gt["gt_j"][1, ids[r]]) for r in range(13, 17)] == [8 * 37 + 6, 9 * 37 + 6, 4 * 37 + 15, 6 * 37 + 16]
    # the dense form, by the module's own to_dense, on CPU tensors
    sparse = supervision.GroundTruth(*(torch.from_numpy(gt[k]) for k in ("gt_j", "gt_xy", "gt_i", "n_gt")), (35, 37))
    conf_gt, loc_gt = sparse.to_dense()
    assert conf_gt.dtype == torch.int16 and loc_gt.dtype == torch.float32 and tuple(loc_gt.shape) == (B, N, M, 2)
    assert np.array_equal(torch.nonzero(conf_gt == 1).numpy(), where) and int(conf_gt.sum()) == len(where)
    assert np.abs(loc_gt[where[:, 0], where[:, 1], where[:, 2]].numpy() - golden["ref_gt_xy"]).max() <= XY_BAR
    o_conf, o_loc = oracle.to_dense(gt["gt_j"], gt["gt_xy"], M)
    assert np.array_equal(conf_gt.numpy(), o_conf) and np.array_equal(loc_gt.numpy(), o_loc)
    back = supervision.GroundTruth.from_dense(conf_gt, loc_gt, (35, 37))
    for k in ("gt_j", "gt_xy", "gt_i", "n_gt"):
        assert np.array_equal(getattr(back, k).numpy(), gt[k]), k
    with pytest.raises(ValueError, match="budget_bytes"):
        sparse.to_dense(budget_bytes=1000)


@pytest.mark.parametrize("name", ["plain", "scaled"])
def test_oracle_targets_and_losses_against_the_reference(golden, name):
    g, gt, m = golden, golden["gt"], golden["matches"]
    scale = g["scale"] if name == "scaled" else None
    e = oracle.fine_targets(m[:, 0], m[:, 1], m[:, 2], None, gt["gt_j"], gt["gt_xy"], 37, scale=scale)
    diff = np.abs(e - g[f"ref_expec_f_gt_{name}"]).max()
    print(f"{name}: max |expec_f_gt - reference| = {diff:.3e} (bar {XY_BAR:.3e})")
    assert diff <= XY_BAR
    coarse = oracle.coarse_loss(g["conf_matrix"], gt["gt_j"])
    assert coarse["n_pos"] == len(g["ref_gt_where"]) and coarse["n_pos"] + coarse["n_neg"] == g["conf_matrix"].size
    worst = 0.0
    for mode in ("eval", "train"):
        fine = oracle.fine_loss(g["expec_f"], e, training=mode == "train")
        assert fine["min_margin"] >= 1e-3
        # without an image scale the reference's coarse scale is the fine one: every target is far outside the window
        assert fine["status"] == (oracle.OK if name == "scaled" else oracle.NONE if mode == "eval" else oracle.FORCED)
        total = oracle.total_loss(coarse["loss_c"], fine)
        for key, got in total.items():
            ref = float(g[f"ref_{key}_{name}_{mode}"])
            worst = max(worst, abs(got - ref) / abs(ref))
    print(f"{name}: largest relative difference of a loss to the reference's float32 = {worst:.3e} (bar {LOSS_BAR:.3e})")
    assert worst <= LOSS_BAR


def test_oracle_corner_case_against_the_reference(golden):
    g = golden
    far = np.full((len(g["matches"]), 2), 3.0, np.float32)
    ev = oracle.fine_loss(g["expec_f"], far, training=False)
    assert ev["status"] == oracle.NONE and np.isnan(ev["loss_f"]) and np.isnan(g["ref_loss_f_none_eval"])        # the reference returns None
    tr = oracle.fine_loss(g["expec_f"], far, training=True)
    assert tr["status"] == oracle.FORCED and tr["n_correct"] == 1
    assert abs(tr["loss_f"] - float(g["ref_loss_f_none_train"])) <= LOSS_BAR * tr["loss_f"]
    assert oracle.fine_loss(g["expec_f"], far, count=0, training=True)["status"] == oracle.EMPTY
    assert oracle.fine_loss(g["expec_f"], far, count=0, training=False)["status"] == oracle.NONE


def test_block_sum_is_the_written_order():
    rng = np.random.default_rng(0)
    for n in (1, 255, 256, 257, 1295):
        t = rng.uniform(0, 1, n) * 10.0 ** rng.integers(-8, 8, n)
        lanes = [0.0] * 256
        for k in range(n):                                                       # one element after another, by hand
            lanes[k % 256] = lanes[k % 256] + t[k]
        s = 128
        while s:
            lanes = [lanes[k] + lanes[k + s] for k in range(s)]
            s //= 2
        assert oracle.block_sum(t) == lanes[0]
    t = rng.uniform(0.1, 1.0, (8, 1295))
    assert np.any(oracle.block_sum(t) != oracle.block_sum(t, reverse=True))      # the order is part of the result
    assert np.array_equal(oracle.block_sum(t), [oracle.block_sum(row) for row in t])


def _halfway_scene():
    """(12, 12) pixels, one cell: a point at (0, 8) gives j == M"""
    kp = np.array([[[0 - 6, 8 - 6, 64], [0 - 6, 0 - 6, 64]]], np.float32)
    K = np.array([[64.0, 0, 6], [0, 64, 6], [0, 0, 1]])
    return kp, np.array([[0, 1]]), np.eye(4)[None], K


def test_seeded_faults_change_an_output(golden):
    g, gt, m = golden, golden["gt"], golden["matches"]
    args = (g["keypoints3d"], g["point_ids"], None, g["pose_gt"], g["K"], g["hw"])
    for fault, frame in (("depth_test", 0), ("half_away", 1), ("last_wins", 0)):
        bad = oracle.ground_truth(*args, faults={fault})
        assert not np.array_equal(bad["gt_j"][frame], gt["gt_j"][frame]), fault
        assert np.array_equal(bad["gt_j"][1 - frame], gt["gt_j"][1 - frame]) or fault == "last_wins", fault
    kp, ids, pose, K = _halfway_scene()
    good, bad = (oracle.ground_truth(kp, ids, None, pose, K, (12, 12), faults=f) for f in ((), {"j_gt_M"}))
    assert good["n_gt"].tolist() == [1] and good["gt_j"].tolist() == [[-1, 0]] and bad["n_gt"].tolist() == [2]
    e = oracle.fine_targets(m[:, 0], m[:, 1], m[:, 2], None, gt["gt_j"], gt["gt_xy"], 37)
    assert not np.array_equal(e, oracle.fine_targets(m[:, 0], m[:, 1], m[:, 2], None, gt["gt_j"], gt["gt_xy"], 37, faults={"coarse_scale_8"}))
    coarse = oracle.coarse_loss(g["conf_matrix"], gt["gt_j"])
    for fault in ("no_clamp", "per_frame_means"):
        assert oracle.coarse_loss(g["conf_matrix"], gt["gt_j"], faults={fault})["loss_c"] != coarse["loss_c"], fault
    es = oracle.fine_targets(m[:, 0], m[:, 1], m[:, 2], None, gt["gt_j"], gt["gt_xy"], 37, scale=g["scale"])
    assert oracle.fine_loss(g["expec_f"], es)["loss_f"] != oracle.fine_loss(g["expec_f"], es, faults={"w_not_normalised"})["loss_f"]


def test_oracle_counts_nan_and_branches():
    conf = np.array([[[0.0, 3e-7, 1.0, 0.9999995, 0.5]]], np.float32)
    none = oracle.coarse_loss(conf, np.array([[-1]]))
    assert none["n_pos"] == 0 and none["pos_sum"] == 0.0 and none["loss_c"] == none["neg_sum"] / 5
    one = oracle.coarse_loss(np.array([[[0.25]]], np.float32), np.array([[0]]), pos_weight=2.0)
    assert one["n_neg"] == 0 and one["loss_c"] == 2.0 * (((-0.25) * (0.75 * 0.75)) * np.log(0.25))
    conf[0, 0, 1] = np.nan
    assert np.isnan(oracle.coarse_loss(conf, np.array([[4]]))["loss_c"])
    assert oracle.coarse_loss(conf[:, :, 2:], np.array([[2]]), gamma=1.5)["pos_sum"] == ((-0.25) * np.power(0.5, 1.5)) * np.log(0.5)
    s = oracle.scene(3, B=3, N=40, A=20)
    counted = oracle.ground_truth(s["keypoints3d"], s["point_ids"], np.array([0, 1, 99]), s["pose_gt"], s["K"], s["image_hw"])
    assert counted["n_gt"][0] == 0 and counted["n_gt"][1] == 1 and counted["n_gt"][2] >= 4
    assert oracle.fine_targets([0], [0], [5], -3, counted["gt_j"], counted["gt_xy"], 37).shape == (0, 2)


# ---- header and binding ----------------------------------------------------------------------------------------------------------------
SYMBOLS = ("opsup_abi_version", "opsup_last_error", "opsup_ground_truth", "opsup_fine_targets", "opsup_coarse_loss", "opsup_fine_loss")
PARAMS = {
    "opsup_ground_truth": ("keypoints3d", "kp_bstride", "point_ids", "counts", "pose_gt", "K", "k_shared", "B", "N", "A", "H", "W", "stride",
                           "owner", "gt_j", "gt_xy", "gt_i", "n_gt", "stream"),
    "opsup_fine_targets": ("b_ids", "i_ids", "j_ids", "count", "cap", "gt_j", "gt_xy", "B", "N", "w_c", "coarse_res", "fine_res", "radius",
                           "scale", "expec_f_gt", "stream"),
    "opsup_coarse_loss": ("conf", "conf_bstride", "conf_rstride", "gt_j", "B", "N", "M", "alpha", "gamma", "pos_weight", "neg_weight",
                          "partials", "sums", "counts", "stream"),
    "opsup_fine_loss": ("expec_f", "expec_f_gt", "count", "cap", "correct_thr", "training", "loss_f", "n_correct", "status", "stream"),
}


def test_header_and_binding(tmp_path):
    entry, = cabi.ADDONS
    assert tuple(entry) == ("opsup", "ext/onepose_supervision.h", "libonepose_supervision.so", "OPSUP_LIB", "supervision")
    for table in (cabi.LIBRARIES, cabi.EXTENSIONS):                               # disjoint, column by column
        assert entry not in table
        for column, taken in zip(entry, zip(*table)):
            assert column not in taken
    text = open(os.path.join(REPO, "include", "ext", "onepose_supervision.h")).read()
    header = cabi.parse(text, cabi.names_of("opsup"))
    assert tuple(header.prototypes) == SYMBOLS == supervision.EXPORTED_SYMBOLS
    for name, params in PARAMS.items():
        assert tuple(n for _, n in header.prototypes[name].params) == params, name
    assert header.defines == {"OPSUP_ABI_VERSION": 1, "OPSUP_BLOCK": 256, "OPSUP_MAX_BATCH": 65535, "OPSUP_MAX_ROWS": 2 ** 24, "OPSUP_OK": 0,
                              "OPSUP_NONE": 1, "OPSUP_FORCED": 2, "OPSUP_EMPTY": 3}
    assert (supervision.OK, supervision.NONE, supervision.FORCED, supervision.EMPTY) == (oracle.OK, oracle.NONE, oracle.FORCED, oracle.EMPTY)
    assert supervision.BLOCK == oracle.BLOCK and supervision.ABI_VERSION == 1
    assert cabi.parse(text).prototypes == {}                                      # the table's reader does not know the prefix
    with pytest.raises(TypeError, match="takes 10 arguments"):
        supervision.check_arity("opsup_fine_loss", (1, 2, 3))
    with pytest.raises(TypeError, match="missing status; unknown flags"):
        supervision.order("opsup_fine_loss", **{**{n: 0 for n in PARAMS["opsup_fine_loss"] if n != "status"}, "flags": 0})
    for other in os.listdir(os.path.join(REPO, "include")):                       # no other header is the place of these entry points
        if other.endswith(".h"):
            assert "opsup_" not in open(os.path.join(REPO, "include", other)).read()
    mk = open(os.path.join(REPO, "onepose_st_amd", "csrc", "Makefile")).read()
    assert re.search(r"^SUP_SRCS := supervision.hip$", mk, re.M) and re.search(r"^SUP_FLAGS := -ffp-contract=off$", mk, re.M)
    assert "reduce_f64.h" in re.search(r"^SUP_HDRS := (.*)$", mk, re.M).group(1).split()
    assert len(re.findall(r"^\$\(eval \$\(call satellite,SUP,sup,supervision\)\)$", mk, re.M)) == 1
    src = open(os.path.join(REPO, "onepose_st_amd", "supervision.py")).read()
    assert not re.search(r"^\s*(from|import)\s+(oracle|tests)\b", src, re.M)     # the product does not import oracle or tests
    absent = cabi.Binding(entry.header, entry.so, entry.prefix, "OPSUP_NO_SUCH_VARIABLE", names=cabi.names_of("opsup"))
    absent.path = str(tmp_path / "libonepose_absent.so")
    with pytest.raises(cabi.HipLibraryError, match="libonepose_absent.so not found"):
        absent.load()
    no_header = cabi.Binding("ext/no_such_header.h", entry.so, entry.prefix, entry.env, names=cabi.names_of("opsup"))
    assert no_header.exported_symbols == () and no_header.abi_version is None
    with pytest.raises(cabi.HipLibraryError, match="no_such_header.h not found"):
        no_header.load()


def test_built_library_rejects_before_any_launch():
    assert os.path.exists(supervision.library_path()), "libonepose_supervision.so: run __graft_entry__.build()"
    lib = supervision.load()
    assert all(hasattr(lib, s) for s in SYMBOLS) and lib.opsup_abi_version() == 1
    p = ctypes.c_void_p(1 << 20)                                                  # never dereferenced: every call below is refused first
    good = {
        "opsup_ground_truth": dict(keypoints3d=p, kp_bstride=0, point_ids=p, counts=None, pose_gt=p, K=p, k_shared=1, B=1, N=4, A=4, H=16, W=16,
                                   stride=8, owner=p, gt_j=p, gt_xy=p, gt_i=p, n_gt=p, stream=None),
        "opsup_fine_targets": dict(b_ids=p, i_ids=p, j_ids=p, count=None, cap=4, gt_j=p, gt_xy=p, B=1, N=4, w_c=2, coarse_res=8, fine_res=2,
                                   radius=2, scale=None, expec_f_gt=p, stream=None),
        "opsup_coarse_loss": dict(conf=p, conf_bstride=16, conf_rstride=4, gt_j=p, B=1, N=4, M=4, alpha=0.25, gamma=2.0, pos_weight=1.0,
                                  neg_weight=1.0, partials=p, sums=p, counts=p, stream=None),
        "opsup_fine_loss": dict(expec_f=p, expec_f_gt=p, count=None, cap=4, correct_thr=1.0, training=0, loss_f=p, n_correct=p, status=p,
                                stream=None),
    }

    def refused(name, message, **change):
        with pytest.raises(ValueError, match=message):
            supervision.call(name, *supervision.order(name, **{**good[name], **change}))
    for name, args in good.items():
        for key, value in args.items():
            if value is p:
                refused(name, f"^{name}: {name}: null pointer$", **{key: None})
    refused("opsup_ground_truth", "B outside", B=0)
    refused("opsup_ground_truth", "B outside", B=65536)
    refused("opsup_ground_truth", "N and A", A=0)
    refused("opsup_ground_truth", "image: stride", stride=0)
    refused("opsup_ground_truth", "image: stride", H=4)
    refused("opsup_ground_truth", "kp_bstride", kp_bstride=11)
    refused("opsup_fine_targets", "cap outside", cap=0)
    refused("opsup_fine_targets", "at least 1", radius=0)
    refused("opsup_coarse_loss", "N and M", M=0)
    refused("opsup_coarse_loss", "strides", conf_rstride=3)
    refused("opsup_coarse_loss", "finite", gamma=float("nan"))
    refused("opsup_fine_loss", "cap outside", cap=2 ** 24 + 1)
    refused("opsup_fine_loss", "correct_thr", correct_thr=float("nan"))


def test_python_api_refusals():
    cfg = {"coarse_type": "focal", "coarse_weight": 1.0, "focal_alpha": 0.25, "focal_gamma": 2.0, "pos_weight": 1.0, "neg_weight": 1.0,
           "fine_type": "l2_with_std", "fine_weight": 1.0, "fine_correct_thr": 1.0}
    with pytest.raises(NotImplementedError, match="coarse_type"):
        supervision.Loss({**cfg, "coarse_type": "cross_entropy"})
    with pytest.raises(NotImplementedError, match="fine_type"):
        supervision.Loss({**cfg, "fine_type": "l2"})
    loss = supervision.Loss(cfg)
    assert loss.training and not loss.eval().training and loss.train().training
    with pytest.raises(NotImplementedError, match="mask0"):
        loss.forward({"mask0": torch.ones(1, 2, 2)})
    kp, ids, pose, K = torch.zeros(1, 4, 3), torch.zeros(1, 3, dtype=torch.int64), np.eye(4)[None], np.eye(3)
    with pytest.raises(NotImplementedError, match="query_image_scale other than 1"):
        supervision.ground_truth(kp, ids, pose, K, (16, 16), scale=torch.tensor([[1.0, 0.5]]))
    for call in (lambda: supervision.ground_truth(kp, ids, pose, K, (16, 16), scale=[1.0, 1.0]),
                 lambda: supervision.fine_loss(torch.zeros(2, 3), torch.zeros(2, 2)),
                 lambda: supervision.coarse_loss(torch.zeros(1, 4, 4), supervision.GroundTruth(ids, kp, ids, ids, (2, 2))),
                 lambda: supervision.fine_targets(ids[0], ids[0], ids[0], supervision.GroundTruth(ids, kp, ids, ids, (2, 2)), 2)):
        with pytest.raises(hip.HipLibraryError, match=re.escape(hip.NO_CPU_FALLBACK)):
            call()
    with pytest.raises(TypeError, match="^point_ids: expected a tensor$"):
        supervision.ground_truth(kp, [[0]], pose, K, (16, 16))
    with pytest.raises(ValueError, match="needs at least one match"):
        supervision.fine_loss(torch.zeros(0, 3), torch.zeros(0, 2), training=True)
    with pytest.raises(ValueError, match=r"expec_f: float32 \[cap, 3\]"):
        supervision.fine_loss(torch.zeros(2, 2), torch.zeros(2, 2))
    assert set(vars(supervision.stages)) >= {"ground_truth", "fine_targets", "coarse_loss", "fine_loss"}
