"""The training-mode forward on the device (``onepose_st_amd/train_forward.py``, ``libonepose_train_forward.so``, the model's
``hip_train_forward``) against its numpy restatement (tests/train_forward_oracle.py) and the reference's own outputs
(tests/golden/train_forward_small.npz): every comparison is exact, so there is no tolerance here.  Everything is small: at most 65 537
rows (the second round of the block scan), lists of 18 rows, a model at N = 64 on a 32 x 40 image."""
import os

import numpy as np
import pytest
import torch

from tests import train_forward_oracle as oracle
from tests.golden import make_train_forward_golden as recipe

pytestmark = pytest.mark.gpu

DEV = "cuda:0"
REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
T, G = 18, recipe.G
KEYS = ("b_ids", "i_ids", "j_ids", "mconf", "mkpts_3d", "mkpts_c", "gt_mask")
ATTR = {"mkpts_3d": "mk3d", "mkpts_c": "mkc"}


@pytest.fixture(scope="module")
def trn():
    from onepose_st_amd import train_forward
    train_forward.load()
    return train_forward


@pytest.fixture(scope="module")
def golden():
    return dict(np.load(os.path.join(REPO, "tests", "golden", "train_forward_small.npz")))


def dev(a, dtype=None):
    return torch.from_numpy(np.ascontiguousarray(a, dtype=dtype)).to(DEV)


def same_bytes(t, a):
    got = t.cpu().numpy()
    return got.dtype == a.dtype and got.shape == a.shape and got.tobytes() == np.ascontiguousarray(a).tobytes()


def sparse_gt(gt_j, M, hw_c=None):
    from onepose_st_amd import supervision
    B, N = gt_j.shape
    return supervision.GroundTruth(dev(gt_j, np.int64), torch.zeros(B, N, 2, device=DEV), torch.full((B, M), -1, dtype=torch.int64, device=DEV),
                                   torch.zeros(B, dtype=torch.int32, device=DEV), hw_c or (1, M))


# ---- 1. the ground-truth rows -------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("B,N", [(1, 1), (3, 85), (2, 128), (1, 257), (1, 65537)], ids=lambda v: str(v))
def test_gt_list_bit_for_bit(trn, B, N):
    M, rows = 4, B * N
    rng = np.random.default_rng(rows)
    edges = [r for k in range(1, rows // 256 + 1) for r in (256 * k - 1, 256 * k) if r < rows] + [0, rows - 1]
    for kind in ("random", "edges_only", "all_but_edges", "all", "none"):
        flat = {"random": np.where(rng.uniform(size=rows) < 0.4, rng.integers(0, M, rows), -1), "edges_only": np.full(rows, -1),
                "all_but_edges": rng.integers(0, M, rows), "all": rng.integers(0, M, rows), "none": np.full(rows, -1)}[kind].astype(np.int64)
        if kind in ("random", "edges_only"):
            flat[edges] = 1                                                      # ground-truth rows on both sides of every block edge
        if kind == "all_but_edges":
            flat[edges] = -1
        if kind == "none" and rows > 2:
            flat[1], flat[2] = M, -5                                             # a cell outside the grid is no ground truth
        want, n = oracle.gt_list(flat.reshape(B, N), M)
        got = trn.gt_list(sparse_gt(flat.reshape(B, N), M))
        assert got.rows.dtype == torch.int32 and tuple(got.rows.shape) == (rows,) and int(got.total.item()) == n, kind
        assert same_bytes(got.rows[:n], want), kind
        assert n == {"all": rows, "none": 0}.get(kind, n)


# ---- 2. the padded list -------------------------------------------------------------------------------------------------------------------
def case_of(golden, name):
    return {k[len(name) + 2:]: v for k, v in golden.items() if k.startswith(name + "__")}


def pred_of(c):
    return {"b_ids": c["pred_b_ids"], "i_ids": c["pred_i_ids"], "j_ids": c["pred_j_ids"], "mconf": c["pred_mconf"],
            "mkpts_3d": c["pred_mkpts_3d_db"], "mkpts_c": c["pred_mkpts_query_c"]}


def device_lists(pred, cap=None, count=None):
    """the predicted lists inside buffers of ``cap`` rows whose other rows hold values that must never be read"""
    from onepose_st_amd.matchcall import MatchLists
    P = len(pred["b_ids"])
    cap = P if cap is None else cap
    ids = [torch.full((cap,), 2 ** 40 + 11, dtype=torch.int64, device=DEV) for _ in range(3)]
    fl = [torch.full(shape, float("nan"), device=DEV) for shape in ((cap,), (cap, 3), (cap, 2))]
    for t, k in zip(ids + fl, ("b_ids", "i_ids", "j_ids", "mconf", "mkpts_3d", "mkpts_c")):
        t[:P] = dev(pred[k]).reshape(t[:P].shape)
    return MatchLists(*ids, *fl, None, None, None if count is None else torch.tensor([count, 77, 77, 77], dtype=torch.int32, device=DEV))


def sentinel_out(rows):
    from onepose_st_amd.matchcall import MatchLists
    ids = [torch.full((rows,), -777, dtype=torch.int64, device=DEV) for _ in range(3)]
    fl = [torch.full(shape, 777.0, device=DEV) for shape in ((rows,), (rows, 3), (rows, 2))]
    return MatchLists(*ids, *fl, ids[0], torch.full((rows,), True, device=DEV), torch.full((1,), -777, dtype=torch.int32, device=DEV))


def untouched(out, start):
    return all(bool((getattr(out, k)[start:] == -777).all()) for k in ("b_ids", "i_ids", "j_ids")) and bool(out.gt_mask[start:].all()) \
        and all(bool((getattr(out, k)[start:] == 777.0).all()) for k in ("mconf", "mk3d", "mkc"))


def run_case(trn, c, cap=None, count=None, step=None, out=None, gt_j=None):
    gt_j = c["gt_j"] if gt_j is None else gt_j
    kw = dict(T=T, G=G, seed=recipe.SEED, step=int(c["step"]) if step is None else step, w_c=recipe.HW_C[1], scale=recipe.HW_I[0] / recipe.HW_C[0],
              query_scale=dev(c["scale"]) if "scale" in c else None)
    got = trn.pad_matches(device_lists(pred_of(c), cap, count), sparse_gt(gt_j, recipe.M, recipe.HW_C), dev(c["keypoints3d"]), out=out, **kw)
    want = oracle.pad_matches(pred_of(c), None, gt_j, c["keypoints3d"], recipe.M, kw["w_c"], T, G, kw["seed"], kw["step"], kw["scale"], c.get("scale"))
    return got, want


def check_rows(got, want):
    assert (int(got.lists.count[0]), int(got.n_keep), int(got.status)) == (want["count"], want["n_keep"], want["status"])
    for key in KEYS:
        assert same_bytes(getattr(got.lists, ATTR.get(key, key))[:T], want[key]), key


@pytest.mark.parametrize("name", list(recipe.CASES))
def test_the_fixture_through_the_device(trn, golden, name):
    """every key equal to the reference's; the predicted lists lie in buffers of B * N rows behind a device count, as the model's do"""
    c = case_of(golden, name)
    P = len(c["pred_b_ids"])
    got, want = run_case(trn, c, cap=recipe.B * recipe.N, count=P)
    check_rows(got, want)
    n = int(got.n_keep)
    assert n == min(P, T - G) and got.lists.m_bids is got.lists.b_ids
    ref = {"b_ids": got.lists.b_ids, "i_ids": got.lists.i_ids, "j_ids": got.lists.j_ids, "gt_mask": got.lists.gt_mask, "m_bids": got.lists.b_ids[:n],
           "mkpts_3d_db": got.lists.mk3d[:n], "mkpts_query_c": got.lists.mkc[:n], "mconf": got.lists.mconf[:n]}
    for key in recipe.KEYS:
        assert same_bytes(ref[key], c[f"ref_{key}"]), (name, key)
    if P:                                                                        # P equal to the capacity, with and without a count
        for count in (None, P, P + 9):
            check_rows(run_case(trn, c, cap=P, count=count)[0], want)
    else:                                                                        # an empty list, and a negative count
        check_rows(run_case(trn, c)[0], want)
        check_rows(run_case(trn, c, cap=4, count=-3)[0], want)


def test_no_ground_truth_writes_no_row(trn, golden):
    c = case_of(golden, "p14")
    out = sentinel_out(T + 7)
    got, want = run_case(trn, c, out=out, gt_j=np.full_like(c["gt_j"], -1))
    assert want == {"count": 0, "n_keep": 13, "status": oracle.NO_GT}
    assert (int(out.count[0]), int(got.n_keep), int(got.status)) == (0, 13, trn.NO_GT) and got.lists is out
    assert untouched(out, 0)
    far = np.full_like(c["gt_j"], -1)
    far[1, 3] = recipe.M                                                         # a cell outside the grid alone: still none
    assert int(run_case(trn, c, gt_j=far)[0].status) == trn.NO_GT


def test_steps_rows_past_T_and_identical_bytes(trn, golden):
    c = case_of(golden, "p40")
    first, w0 = run_case(trn, c, step=0, out=sentinel_out(T + 7))
    check_rows(first, w0)
    assert untouched(first.lists, T)                                             # rows past T of an over-sized buffer stay as they were
    again, _ = run_case(trn, c, step=0, out=sentinel_out(T + 7))
    for key in KEYS:                                                             # the same step twice: identical bytes
        a, b = (getattr(x.lists, ATTR.get(key, key)) for x in (first, again))
        assert a.cpu().numpy().tobytes() == b.cpu().numpy().tobytes(), key
    other, w1 = run_case(trn, c, step=1)
    check_rows(other, w1)
    assert not np.array_equal(w0["sources"], w1["sources"]) and not np.array_equal(w0["gt_picks"], w1["gt_picks"])
    assert not torch.equal(other.lists.i_ids[:T], first.lists.i_ids[:T])
    last, w2 = run_case(trn, c, step=oracle.MAX_STEP - 1)
    check_rows(last, w2)
    big = trn.pad_matches(device_lists(pred_of(c)), sparse_gt(c["gt_j"], recipe.M), dev(c["keypoints3d"]), T=T, G=G, seed=2 ** 64 - 1, step=5,
                          w_c=6, scale=8.0)                                      # the seed's arithmetic is modulo 2^64
    check_rows(big, oracle.pad_matches(pred_of(c), None, c["gt_j"], c["keypoints3d"], recipe.M, 6, T, G, 2 ** 64 - 1, 5, 8.0))
    shared = trn.pad_matches(device_lists(pred_of(c)), sparse_gt(c["gt_j"], recipe.M), dev(c["keypoints3d"][:1]), T=T, G=G, seed=3, step=5,
                             w_c=6, scale=8.0)                                   # one object for every frame
    check_rows(shared, oracle.pad_matches(pred_of(c), None, c["gt_j"], c["keypoints3d"][:1], recipe.M, 6, T, G, 3, 5, 8.0))
    with pytest.raises(ValueError, match="0 < G < T"):
        trn.pad_matches(device_lists(pred_of(c)), sparse_gt(c["gt_j"], recipe.M), dev(c["keypoints3d"]), T=5, G=5, seed=0, step=0, w_c=6, scale=8.0)


# ---- 3. the model -------------------------------------------------------------------------------------------------------------------------
LOSS_CONFIG = {"coarse_type": "focal", "coarse_weight": 1.0, "focal_alpha": 0.25, "focal_gamma": 2.0, "pos_weight": 1.0, "neg_weight": 1.0,
               "fine_type": "l2_with_std", "fine_weight": 0.5, "fine_correct_thr": 1.0}
HW, NP, SEED = (32, 40), 64, 3
LIST_KEYS = ("b_ids", "i_ids", "j_ids", "gt_mask", "m_bids", "mkpts_3d_db", "mkpts_query_c", "mconf", "expec_f", "mkpts_query_f")


@pytest.mark.parametrize("attention,percent,scaled", [("linear", 0.3, True), ("full", 0.9, False)], ids=["linear-picks-scaled", "full-keep_all"])
def test_model_training_forward(trn, attention, percent, scaled):
    from onepose_st_amd import matchcall, supervision
    from onepose_st_amd.config import default_config
    from onepose_st_amd.model import OnePosePlus_model, _current_stream
    from onepose_st_amd.synthetic import make_synthetic_inputs, make_synthetic_state_dict
    cfg = default_config()
    cfg["loftr_fine"]["attention"] = attention
    cfg["coarse_matching"]["border_rm"] = 0
    cfg["coarse_matching"]["train"].update(train_coarse_percent=percent, train_pad_num_gt_min=4)
    cfg.update(hip_train_forward=True, hip_train_seed=SEED)
    sd = make_synthetic_state_dict(0, cfg)
    model = OnePosePlus_model(cfg).eval()
    model.load_state_dict(sd, strict=True)
    model.to(DEV)
    frames = [make_synthetic_inputs(sd, n_points=NP, image_hw=HW, n_plant=16, seed=11, config=cfg, frame=f) for f in range(2)]
    feat_c, feat_f = (torch.cat([f[k] for f in frames]).to(DEV) for k in ("feat_c", "feat_f"))
    B, M, w_c = 2, 20, 5
    pose = np.stack([np.eye(4)] * 2)
    for b, f in enumerate(frames):
        pose[b, :3] = f["pose_gt"].numpy()
    ids = np.stack([np.arange(NP, dtype=np.int64)] * 2)
    gt = supervision.ground_truth(frames[0]["keypoints3d"].to(DEV), dev(ids), pose, frames[0]["K"].numpy(), HW)
    gt_j = gt.gt_j.cpu().numpy()
    assert (gt_j >= 0).sum(axis=1).min() > 5

    def features(ground_truth=gt, finish=True):
        data = {k: frames[0][k].to(DEV) for k in ("keypoints3d", "descriptors3d_db", "descriptors3d_coarse_db")}
        data["ground_truth"] = ground_truth
        if scaled:
            data["query_image_scale"] = torch.ones(B, 2, device=DEV)
        pend = model.enqueue_features(data, feat_c, feat_f, HW)
        return pend.finish() if finish else pend

    ev = features()
    P = len(ev["b_ids"])
    Tm = trn.train_rows(B, NP, M, percent)
    n_keep = min(P, Tm - 4)
    assert (P > Tm - 4) == (percent == 0.3) and P > 8 and Tm == {0.3: 12, 0.9: 36}[percent]        # the picks, and the keep-all branch
    assert ev["conf_matrix"].shape == (B, NP, M) and model.train_calls == 0

    model.train()
    tr = features()
    assert model.train_calls == 1
    for key, rows in (("b_ids", Tm), ("i_ids", Tm), ("j_ids", Tm), ("gt_mask", Tm), ("expec_f", Tm), ("m_bids", n_keep), ("mkpts_3d_db", n_keep),
                      ("mkpts_query_c", n_keep), ("mconf", n_keep), ("mkpts_query_f", n_keep)):
        assert tr[key].shape[0] == rows and tr[key].dtype == ev[key].dtype and tr[key].shape[1:] == ev[key].shape[1:], key
    assert isinstance(tr["conf_matrix"], torch.Tensor) and torch.equal(tr["conf_matrix"], ev["conf_matrix"]) and tr["W"] == 5
    pred = {"b_ids": ev["b_ids"], "i_ids": ev["i_ids"], "j_ids": ev["j_ids"], "mconf": ev["mconf"], "mkpts_3d": ev["mkpts_3d_db"],
            "mkpts_c": ev["mkpts_query_c"]}
    pred = {k: v.cpu().numpy() for k, v in pred.items()}
    want = oracle.pad_matches(pred, None, gt_j, frames[0]["keypoints3d"].numpy(), M, w_c, Tm, 4, SEED, 0, 8.0, np.ones((B, 2), np.float32) if scaled else None)
    src = want["sources"]
    for key, pk in (("b_ids", "b_ids"), ("i_ids", "i_ids"), ("j_ids", "j_ids"), ("mconf", "mconf"), ("mkpts_query_c", "mkpts_c"), ("mkpts_3d_db", "mkpts_3d")):
        assert same_bytes(tr[key][:n_keep], pred[pk][src]), key                 # the eval forward's rows that the oracle's picks name
    for key in ("b_ids", "i_ids", "j_ids", "gt_mask"):
        assert same_bytes(tr[key], want[key]), key
    assert same_bytes(tr["m_bids"], want["b_ids"][:n_keep]) and int(tr["gt_mask"].sum()) == Tm - n_keep

    # the fine stage over all T rows: run by the test on the training lists
    fi = model._frame_inputs({k: tr[k] for k in ("keypoints3d", "descriptors3d_db", "descriptors3d_coarse_db")} |
                             ({"query_image_scale": tr["query_image_scale"]} if scaled else {}), feat_c, feat_f, HW)
    main = _current_stream(fi.dev)
    _, _, ff, ff_strides = model._input_stage(fi, feat_c, feat_f, main, (str(fi.dev), main.cuda_stream), False, False)
    expec, mkf = torch.full((Tm, 3), 7.0, device=DEV), torch.full((Tm, 2), 7.0, device=DEV)
    lists = dict(b_ids=tr["b_ids"], i_ids=tr["i_ids"], j_ids=tr["j_ids"], count=torch.tensor([Tm], dtype=torch.int32, device=DEV))
    mkc = dev(want["mkpts_c"])
    if attention == "linear":
        names = model.loftr_fine.layer_names
        matchcall.fine_refine(ff, ff_strides, fi.hf, fi.wf, fi.desc_fine_d, **lists, mkpts_c=mkc, max_matches=Tm, wpack=fi.W["fine_bf16"], nlayers=len(names),
                              cross_bits=sum(1 << i for i, n in enumerate(names) if n == "cross"), encoder_enable=1, nsplit=3, wc=w_c,
                              stride=fi.hf // fi.hc, fine_scale=2 * (HW[0] / fi.hf), expec_f=expec, mkpts_f=mkf, dbg_win=None, dbg_f3=None,
                              query_scale=fi.qscale)
    else:
        model._fine_full_stage(fi, dict(lists, mkc=mkc, mk2d=mkf, cap=Tm), ff, ff_strides, fi.hf // fi.hc, float(HW[0] / fi.hf), expec)
    assert torch.equal(tr["expec_f"], expec) and torch.equal(tr["mkpts_query_f"], mkf[:n_keep])
    assert bool(torch.isfinite(expec).all()) and not bool((expec == 7.0).any())

    # the supervision and the loss on the result: finite, and identical over two runs after reseed
    def loss_of(data):
        supervision.fine_supervision(data, {"OnePosePlus": cfg})
        supervision.Loss(LOSS_CONFIG).train()(data)
        assert data["expec_f_gt"].shape == (Tm, 2) and all(np.isfinite(v) for v in data["loss_scalars"].values())
        return data["loss_scalars"]
    first = loss_of(tr)
    model.reseed(SEED)
    tr2 = features()
    assert model.train_calls == 1 and loss_of(tr2) == first
    for key in LIST_KEYS + ("expec_f_gt",):
        assert torch.equal(tr[key], tr2[key]), key
    tr3 = features()                                                              # the next call draws others
    assert model.train_calls == 2 and not torch.equal(tr3["i_ids"], tr["i_ids"])

    # without the padding the eval lists are returned as they are
    cfg["coarse_matching"]["train"]["train_padding"] = False
    plain = features()
    cfg["coarse_matching"]["train"]["train_padding"] = True
    for key in LIST_KEYS + ("conf_matrix",):
        assert torch.equal(plain[key], ev[key]), key
    # a batch with no ground truth raises at finish()
    none = supervision.GroundTruth(torch.full_like(gt.gt_j, -1), gt.gt_xy, gt.gt_i, gt.n_gt, gt.hw_c)
    pend = features(none, finish=False)
    with pytest.raises(ValueError, match="^no ground-truth match in the batch$"):
        pend.finish()
    # and eval afterwards gives the eval forward's bytes: no state leaks
    model.eval()
    calls = model.train_calls
    back = features()
    assert model.train_calls == calls
    for key in LIST_KEYS + ("conf_matrix",):
        assert torch.equal(back[key], ev[key]), key
