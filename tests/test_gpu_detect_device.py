"""Device detection on the GPU: every stage of ``libonepose_detect.so`` against the numpy oracle (``tests/detect_device_oracle.py``) --
ranges, samples, counts, winners, masks, boxes and the vote exact, the affinities and the state's geometry bit for bit --, the host
estimator on the planted scenes, the detector end to end and ``SequenceRunner(detect="device")``.  Everything is small: at most 15 views
of at most 300 rows, 256 or 300 trials where the default is not the point."""
import os
import sys

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import detect_device_oracle as orc  # noqa: E402
import track_device_oracle as trk_orc  # noqa: E402
from loftr_helpers import device_hook, planted_pair  # noqa: E402

from onepose_st_amd import frameloop as fl  # noqa: E402

pytestmark = pytest.mark.gpu
S = 512


@pytest.fixture(scope="module")
def dd():
    if not torch.cuda.is_available():
        pytest.skip("needs the MI355X")
    from onepose_st_amd import detect_device
    detect_device.load()
    return detect_device


@pytest.fixture(scope="module")
def td():
    if not torch.cuda.is_available():
        pytest.skip("needs the MI355X")
    from onepose_st_amd import track_device
    track_device.load()
    return track_device


def dev_t(a, dtype=None):
    return torch.as_tensor(np.ascontiguousarray(a), dtype=dtype).to("cuda:0")


def bits(a):
    return np.ascontiguousarray(a, dtype=np.float64).view(np.uint64)


def host(t):
    return t.cpu().numpy()


def run_vote(dd, sc, **kw):
    """``detect_device.vote`` on a scene -> the outputs on the host, in the form of ``orc.detect``"""
    kw.setdefault("crop_size", S)
    d = dd.vote(dev_t(sc["mk0"]), dev_t(sc["mk1"]), dev_t(sc["b_ids"]), dev_t(sc["view_hw"]), orc.QUERY_HW, dev_t(orc.SCENE_K), **kw)
    return dict(ranges=host(d.ranges), affine=host(d.affine), boxes=host(d.boxes), n_inliers=host(d.n_inliers), status=host(d.status),
                mask=host(d.inlier_mask), winner=int(host(d.winner)[0]), state=d.state.to_host()), d


def same_state(got, want):
    return (np.array_equal(got[0], want[0]) and got[0].dtype == np.int32 and got[1] == want[1] and np.array_equal(bits(got[2]), bits(want[2]))
            and np.array_equal(bits(got[3]), bits(want[3])))


def same_outputs(got, want):
    assert np.array_equal(got["ranges"], want["ranges"])
    assert np.array_equal(got["n_inliers"], want["n_inliers"]) and np.array_equal(got["status"], want["status"])
    assert np.array_equal(got["mask"], want["mask"]) and np.array_equal(got["boxes"], want["boxes"]) and got["boxes"].dtype == np.int32
    assert np.array_equal(bits(got["affine"]), bits(want["affine"]))
    assert got["winner"] == want["winner"] and same_state(got["state"], want["state"])


# ---- ranges and sample ---------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("seed", [1, 2 ** 64 - 5])
def test_ranges_and_samples_equal_the_oracle(dd, seed):
    """rows per view 5, 0 (an empty view between two others), 6, 64, 65; three rows of no view in front (id -1) and five behind (ids 5, 7),
    ``count`` inside those five; 300 trials leave a partial block of trials"""
    rows, V, trials = (5, 0, 6, 64, 65), 5, 300
    ids = np.concatenate([np.full(3, -1), *[np.full(n, v) for v, n in enumerate(rows)], [5, 5, 7, 7, 7]]).astype(np.int64)
    cap, count = len(ids), len(ids) - 2
    g = np.random.default_rng(3)
    mk0, mk1 = g.uniform(0, 600, (cap, 2)).astype(np.float32), g.uniform(0, 600, (cap, 2)).astype(np.float32)
    want_r = orc.ranges(ids, count, cap, V)
    assert want_r.tolist() == [[3, 8], [8, 8], [8, 14], [14, 78], [78, 143]]
    cnt_d = dev_t(np.array([count], dtype=np.int32))
    got_r = dd.stages.ranges(dev_t(ids), cnt_d, cap, V)
    smp, cnt = dd.stages.score(dev_t(mk0), dev_t(mk1), got_r, trials, seed)
    assert np.array_equal(host(got_r), want_r) and got_r.dtype == torch.int32
    want_s = orc.sample(want_r, trials, seed)
    assert np.array_equal(host(smp), want_s) and (want_s[:2] == -1).all() and (want_s[2:] >= 0).all()
    assert np.array_equal(host(cnt), orc.score(mk0, mk1, want_r, want_s)) and not host(cnt)[:2].any()
    # every row: count = NULL; a count beyond the capacity is clamped to it
    all_rows = orc.ranges(ids, None, cap, V)
    assert np.array_equal(host(dd.stages.ranges(dev_t(ids), None, cap, V)), all_rows)
    assert np.array_equal(host(dd.stages.ranges(dev_t(ids), dev_t(np.array([cap + 100], dtype=np.int32)), cap, V)), all_rows)
    assert np.array_equal(host(dd.stages.ranges(dev_t(ids), dev_t(np.array([-4], dtype=np.int32)), cap, V)), np.zeros((V, 2), np.int32))


@pytest.mark.parametrize("seed", [1, 2 ** 64 - 5])
def test_ranges_and_sampler_are_the_pnp_librarys(dd, seed):
    """One range rule and one sampler in both libraries (``csrc/device_loop.h``): on an ascending table of 4, 5, 64, 65 and 257 rows per
    id, ``pnp_device``'s and this library's ranges are equal tables, and the draws of ``oppnpd_sample`` and of the fused
    ``opdet_score`` are equal and the oracle's -- all integers, compared exactly.  Every id keeps at least 4 rows, so both floors (4
    there, max(min_matches, 3) = 3 here) let every trial run; 4 and 5 rows step past the earlier picks, 64 / 65 cross a wave, 257 a
    staging chunk, 300 trials the 256-trial workgroup.  ``count``: NULL (every row; ``oppnpd_ranges`` takes no NULL and gets the
    capacity), the capacity, and one that cuts the last id short."""
    from onepose_st_amd import pnp_device
    rows, trials = (4, 5, 64, 65, 257), 300
    G = len(rows)
    ids = np.concatenate([np.full(n, g) for g, n in enumerate(rows)]).astype(np.int64)
    cap = len(ids)
    gen = np.random.default_rng(5)
    mk0, mk1 = dev_t(gen.uniform(0, 600, (cap, 2)).astype(np.float32)), dev_t(gen.uniform(0, 600, (cap, 2)).astype(np.float32))
    for count in (None, cap, cap - 100):
        n = cap if count is None else count
        r_pnp = pnp_device.stages.ranges(dev_t(ids), dev_t(np.array([n], dtype=np.int32)), cap, G)
        r_det = dd.stages.ranges(dev_t(ids), None if count is None else dev_t(np.array([count], dtype=np.int32)), cap, G)
        want_r = orc.pnp_orc.ranges(ids, n, cap, G)
        assert torch.equal(r_pnp, r_det) and r_det.dtype == torch.int32 and np.array_equal(host(r_det), want_r)
        assert (want_r[:, 1] - want_r[:, 0]).tolist() == [*rows[:-1], rows[-1] - (cap - n)]
        s_pnp = pnp_device.stages.sample(r_pnp, trials, seed)
        s_det, _ = dd.stages.score(mk0, mk1, r_det, trials, seed, min_matches=0)
        assert torch.equal(s_pnp, s_det) and s_det.dtype == torch.int32
        assert np.array_equal(host(s_det), orc.pnp_orc.sample(want_r, trials, seed)) and (host(s_det) >= 0).all()


# ---- score and select ----------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("trials", [1, 256, 300])
@pytest.mark.parametrize("rows", [(6,), (257,), (255, 256, 257), (256, 6, 255)], ids=lambda r: "x".join(map(str, r)))
def test_counts_winner_and_mask_equal_the_oracle(dd, rows, trials):
    """the chunk edge (255, 256, 257 rows), the smallest view that runs trials (6), one trial, one full block and a partial second block"""
    sc = orc.planted_scene(rows, 40 + len(rows))
    V, cap = len(rows), len(sc["mk0"])
    mk0, mk1, ids = dev_t(sc["mk0"]), dev_t(sc["mk1"]), dev_t(sc["b_ids"])
    count = dev_t(np.array([cap], dtype=np.int32))
    rng = dd.stages.ranges(ids, count, cap, V)
    smp, cnt = dd.stages.score(mk0, mk1, rng, trials, 1)
    best, n_in, status, mask = dd.stages.select(mk0, mk1, rng, count, smp, cnt)
    w_rng = orc.ranges(sc["b_ids"], cap, cap, V)
    w_smp = orc.sample(w_rng, trials, 1)
    w_cnt = orc.score(sc["mk0"], sc["mk1"], w_rng, w_smp)
    w_best, w_in, w_status, w_mask = orc.select(sc["mk0"], sc["mk1"], w_rng, cap, w_smp, w_cnt)
    assert np.array_equal(host(smp), w_smp) and np.array_equal(host(cnt), w_cnt) and host(cnt).shape == (V, trials)
    assert np.array_equal(host(best), w_best) and np.array_equal(host(n_in), w_in) and np.array_equal(host(status), w_status)
    assert np.array_equal(host(mask), w_mask) and [int(w_mask[sc["b_ids"] == v].sum()) for v in range(V)] == w_in.tolist()
    if trials >= 256:
        assert (w_in >= 3).all() and (w_best >= 0).all()


# ---- fit, box and vote ---------------------------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def big(dd):
    """V = 15, 40 to 300 rows per view, 256 trials: the device's outputs, the oracle's, and a second identical call"""
    sc = orc.planted_scene(orc.BIG_ROWS, 21)
    got, d = run_vote(dd, sc, trials=256)
    again, _ = run_vote(dd, sc, trials=256)
    want = orc.detect(sc["mk0"], sc["mk1"], sc["b_ids"], sc["view_hw"], orc.QUERY_HW, orc.SCENE_K, S, trials=256)
    return sc, got, again, want, d


def test_fit_box_and_vote_equal_the_oracle(dd, td, big):
    sc, got, _, want, d = big
    same_outputs(got, want)
    assert want["winner"] == int(np.argmax(want["n_inliers"])) and (want["n_inliers"] >= 0.65 * np.array(orc.BIG_ROWS)).all()
    assert not (want["status"] & orc.STATUS_NO_MODEL).any()
    by_set_box = td.set_box(got["boxes"][got["winner"]], dev_t(orc.SCENE_K), S).to_host()
    assert same_state(got["state"], by_set_box)
    # the stage entries give what the one call gives
    mk0, mk1, rng = dev_t(sc["mk0"]), dev_t(sc["mk1"]), d.ranges
    count = dev_t(np.array([len(sc["mk0"])], dtype=np.int32))
    smp, cnt = dd.stages.score(mk0, mk1, rng, 256, 1)
    best, n_in, status, mask = dd.stages.select(mk0, mk1, rng, count, smp, cnt)
    affine, boxes = dd.stages.fit_box(mk0, mk1, rng, dev_t(sc["view_hw"]), orc.QUERY_HW, n_in, status, mask)
    winner, st = dd.stages.vote(boxes, n_in, status, orc.QUERY_HW, dev_t(orc.SCENE_K), S)
    assert torch.equal(affine, d.affine) and torch.equal(boxes, d.boxes) and torch.equal(n_in, d.n_inliers) and torch.equal(status, d.status)
    assert torch.equal(mask, d.inlier_mask) and torch.equal(winner, d.winner) and same_state(st.to_host(), d.state.to_host())      # (the block has 4 bytes of padding)
    votes, w = d.to_host()                                                           # match_worker's dict
    assert w == want["winner"] and sorted(votes) == list(range(15))
    for v in range(15):
        assert votes[v]["bbox"].tolist() == want["boxes"][v].tolist()
        assert votes[v]["inliers"].shape == (orc.BIG_ROWS[v], 1) and int(votes[v]["inliers"].sum()) == want["n_inliers"][v]


def test_two_identical_calls_agree_bit_for_bit(big):
    _, got, again, _, _ = big
    for k in ("ranges", "boxes", "n_inliers", "status", "mask"):
        assert np.array_equal(got[k], again[k]), k
    assert np.array_equal(bits(got["affine"]), bits(again["affine"])) and got["winner"] == again["winner"] and same_state(got["state"], again["state"])


@pytest.mark.parametrize("name", orc.RULES)
def test_rules_on_the_device(dd, name):
    """the too-small view, the collinear view, two identical views, a negative corner, a corner beyond int32, a degenerate winner"""
    sc = orc.rule_scene(name)
    got, _ = run_vote(dd, sc, trials=256)
    orc.check_rule(name, got)
    same_outputs(got, orc.detect(sc["mk0"], sc["mk1"], sc["b_ids"], sc["view_hw"], orc.QUERY_HW, orc.SCENE_K, S, trials=256))


def test_no_rows_at_all_votes_the_centre_box_of_view_0(dd):
    empty = dict(mk0=np.zeros((0, 2), np.float32), mk1=np.zeros((0, 2), np.float32), b_ids=np.zeros(0, np.int64),
                 view_hw=np.array([orc.QUERY_HW] * 3, dtype=np.int32))
    got, _ = run_vote(dd, empty)
    centre = orc.centre_box(orc.QUERY_HW).tolist()
    assert got["winner"] == 0 and got["state"][0].tolist() == centre and got["boxes"].tolist() == [centre] * 3
    assert got["status"].tolist() == [orc.STATUS_NO_MODEL] * 3 and not got["n_inliers"].any() and got["state"][1] == 0


# ---- against the host ----------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("rows,seed", orc.HOST_SCENES)
def test_device_against_the_host_estimator(dd, rows, seed):
    """the planted scenes of the CPU file at the default 2048 trials: the host's inlier set, the corners within 1e-3 px (measured on the
    MI355X: at most 3.07e-12 px)"""
    from onepose_st_amd import pnp
    sc = orc.planted_scene(rows, seed)
    got, _ = run_vote(dd, sc)
    orc.assert_scene_condition(sc, got["affine"])
    for v, n in enumerate(rows):
        sel = sc["b_ids"] == v
        A, inl = pnp.estimate_affine2d(sc["mk0"][sel], sc["mk1"][sel])
        assert A is not None and np.array_equal(inl[:, 0], got["mask"][sel]) and int(inl.sum()) == got["n_inliers"][v]
        worst = max(abs(a - b) for p, q in zip(orc.corners_through(A.reshape(6), sc["view_hw"][v]), orc.corners_through(got["affine"][v], sc["view_hw"][v]))
                    for a, b in zip(p, q))
        print(f"rows {n}: {int(inl.sum())} inliers, corners through the device's and the host's affinity differ by {worst:.2e} px")
        assert worst < orc.CORNER_BAR and got["status"][v] == 0


# ---- arguments -----------------------------------------------------------------------------------------------------------------------------------
def test_entries_refuse_bad_arguments_before_any_launch(dd, td):
    sc = orc.planted_scene((40, 50), 2)
    cap, V, trials = 90, 2, 256
    t = dict(mk0=dev_t(sc["mk0"]), mk1=dev_t(sc["mk1"]), b_ids=dev_t(sc["b_ids"]), count=dev_t(np.array([cap], dtype=np.int32)),
             view_hw=dev_t(sc["view_hw"]), K=dev_t(orc.SCENE_K.reshape(9)))
    i32 = lambda n: torch.full((n,), -9, dtype=torch.int32, device="cuda:0")      # noqa: E731
    o = dict(ranges=i32(2 * V), samples=i32(3 * V * trials), cnt=i32(V * trials), best=i32(V), n_inliers=i32(V), status=i32(V), boxes=i32(4 * V),
             winner=i32(1), box=i32(4), flag=i32(1), inlier_mask=torch.full((cap,), 9, dtype=torch.uint8, device="cuda:0"),
             affine=torch.full((V, 6), -9.0, dtype=torch.float64, device="cuda:0"), K_crop=torch.full((9,), -9.0, dtype=torch.float64, device="cuda:0"),
             trans=torch.full((9,), -9.0, dtype=torch.float64, device="cuda:0"),
             workspace=torch.full((dd.load().opdet_workspace_bytes(cap, V, trials),), 7, dtype=torch.uint8, device="cuda:0"))
    ptrs = {k: v.data_ptr() for k, v in {**t, **o}.items()}
    base = dict(ptrs, cap=cap, V=V, trials=trials, H=480, W=640, S=S, min_matches=6, reproj_thr=6.0, confidence=0.99, seed=1,
                workspace_bytes=o["workspace"].numel(), stream=None)
    protos = dd._BINDING.header.prototypes
    entries = ("opdet_ranges", "opdet_score", "opdet_select", "opdet_fit_box", "opdet_vote", "opdet_detect")

    def call(name, **change):
        a = {**base, **change}
        dd.call(name, *[a[p] for _, p in protos[name].params])

    def refused(name, match, **change):
        if set(change) <= {p for _, p in protos[name].params}:
            with pytest.raises(ValueError, match=match):
                call(name, **change)
            return 1
        return 0

    n = 0
    for name in entries:
        for change, match in ((dict(V=0), "table sizes"), (dict(V=dd.MAX_VIEWS + 1), "table sizes"), (dict(cap=0), "table sizes"),
                              (dict(cap=dd.MAX_ROWS + 1), "table sizes"), (dict(trials=0), "trials"), (dict(trials=dd.MAX_TRIALS + 1), "trials"),
                              (dict(S=0), "crop size"), (dict(S=td.MAX_CROP + 1), "crop size"), (dict(reproj_thr=0.0), "reproj_thr"),
                              (dict(reproj_thr=-6.0), "reproj_thr"), (dict(reproj_thr=float("nan")), "reproj_thr"), (dict(confidence=1.0), "confidence"),
                              (dict(confidence=0.0), "confidence"), (dict(min_matches=-1), "min_matches"), (dict(H=0), "query size"), (dict(W=0), "query size"),
                              (dict(workspace_bytes=o["workspace"].numel() - 1), "workspace too small")):
            if name == "opdet_vote" and "cap" in change:
                continue
            n += refused(name, match, **change)
        for c, p in protos[name].params:
            if c.endswith("*") and p not in ("count", "stream"):                        # count = NULL means every row
                n += refused(name, "null pointer", **{p: None})
    assert n > 100
    assert dd.load().opdet_workspace_bytes(cap, 0, trials) == 0 and dd.load().opdet_workspace_bytes(cap, V, dd.MAX_TRIALS + 1) == 0
    with pytest.raises(TypeError, match="takes 6 arguments"):
        dd.call("opdet_ranges", ptrs["b_ids"], ptrs["count"], cap, V, ptrs["ranges"])
    with pytest.raises(ValueError, match="crop_size"):
        dd.vote(t["mk0"], t["mk1"], t["b_ids"], t["view_hw"], orc.QUERY_HW, t["K"], crop_size=0)
    torch.cuda.synchronize()
    for k, v in o.items():                                                              # nothing was launched
        assert bool((v == (7 if k == "workspace" else 9 if k == "inlier_mask" else -9)).all()), k
    call("opdet_detect")
    torch.cuda.synchronize()
    assert o["flag"].cpu().tolist() == [0] and o["winner"].cpu().tolist() == [1] and int(o["n_inliers"].cpu()[1]) >= 30
    assert bool((o["inlier_mask"] <= 1).all()) and bool((o["boxes"] != -9).any())


# ---- the detector end to end ---------------------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def matcher():
    if not torch.cuda.is_available():
        pytest.skip("needs the MI355X")
    from onepose_st_amd import loftr
    from onepose_st_amd.synthetic import make_synthetic_loftr_state_dict
    m = loftr.LoFTR_for_OnePose_Plus().eval()
    m.load_state_dict(make_synthetic_loftr_state_dict(0), strict=True)
    return m.to("cuda:0")


VIEW_H, VIEW_W = 96, 128
DET_K = np.array([[300.0, 0, 64], [0, 300.0, 48], [0, 0, 1]])


@pytest.fixture()
def planted_detector(matcher):
    """``test_gpu_loftr.py``'s planted three-view setup: the query carries view 1's content moved by (2, 1) coarse cells"""
    from onepose_st_amd import detector
    dev = torch.device("cuda:0")
    views = [np.full((VIEW_H, VIEW_W), 10 * (k + 1), dtype=np.uint8) for k in range(3)]
    pairs = {0: planted_pair((VIEW_H, VIEW_W), (0, 0), seed=20, noise=3.0), 1: planted_pair((VIEW_H, VIEW_W), (2, 1), seed=21),
             2: planted_pair((VIEW_H, VIEW_W), (0, 0), seed=22, noise=3.0)}
    calls = {"n": 0}

    def hook(fc0, ff0, fc1, ff1):
        if fc0.shape[0] == 3:                        # the batched call
            outs = [device_hook(pairs[k], dev)(None, None, None, None) for k in range(3)]
            return (torch.cat([o[0] for o in outs]), torch.stack([o[1] for o in outs]), torch.cat([o[2] for o in outs]), torch.stack([o[3] for o in outs]))
        k = calls["n"] % 3
        calls["n"] += 1
        return device_hook(pairs[k], dev)(fc0, ff0, fc1, ff1)
    matcher.feature_hook = hook
    try:
        yield detector.LocalFeatureObjectDetector(matcher, views, vote="device"), calls
    finally:
        matcher.feature_hook = None


def test_detector_end_to_end_with_the_device_vote(dd, td, planted_detector):
    det, calls = planted_detector
    dev = torch.device("cuda:0")
    query = torch.zeros(1, 1, VIEW_H, VIEW_W, device=dev)
    d = det.match_worker_device(query)
    assert calls["n"] == 0                                                              # ONE batched matcher call
    votes, winner = d.to_host()
    host_votes = det.match_worker(query)
    n_in = d.n_inliers.cpu().tolist()
    print(f"device vote: inliers {n_in}, boxes {d.boxes.cpu().tolist()}; host vote: {[int(np.asarray(host_votes[k]['inliers']).sum()) for k in range(3)]}")
    assert winner == 1 and n_in[1] >= 40 and n_in[1] > max(n_in[0], n_in[2])
    want = np.array([16, 8, VIEW_W + 16, VIEW_H + 8])
    assert np.abs(votes[1]["bbox"] - want).max() <= 1
    frame = torch.zeros(VIEW_H, VIEW_W, dtype=torch.uint8, device=dev)
    state = det.detect_state(frame, dev_t(DET_K), 64)
    assert isinstance(state, td.TrackState)
    got = state.to_host()
    assert np.array_equal(got[0], votes[1]["bbox"]) and same_state(got, td.set_box(votes[1]["bbox"], dev_t(DET_K), 64).to_host())
    assert same_state(got, trk_orc.box_set(votes[1]["bbox"], DET_K, 64))


# ---- the loop ------------------------------------------------------------------------------------------------------------------------------------
class _DeviceFakeModel:
    """``test_gpu_track_device.py``'s stand-in matcher: the object points through the true pose of frame ``data["frame_index"]`` and the
    crop's ``trans``; four matches on a failing frame"""

    def __init__(self, pts3d, poses, K):
        self.pts3d, self.poses, self.K = dev_t(pts3d), dev_t(np.stack(poses)), dev_t(K)
        self.fail_at, self.seen = set(), []

    def __call__(self, data):
        t = data["frame_index"]
        pose = self.poses[t]
        cam = pose[:, :3] @ self.pts3d.T + pose[:, 3:4]
        uv = self.K @ cam
        uv = torch.cat([uv[:2] / uv[2:], torch.ones_like(uv[2:])])
        uvc = (data["crop_trans"] @ uv).T[:, :2]
        n = 4 if t in self.fail_at else self.pts3d.shape[0]
        data["mkpts_3d_db"] = self.pts3d[:n].float()
        data["mkpts_query_f"] = uvc[:n].float()
        self.seen.append(t)


class _StubDetector:
    """``__call__`` and ``detect_state`` yield the same box: ``project_bbox`` of the true pose of the frame, whose number is its grey value"""

    def __init__(self, td, K, poses):
        self.td, self.K, self.poses, self.calls, self.states = td, K, poses, [], []

    def box(self, t):
        return fl.project_bbox(self.K, self.poses[t], trk_orc.CUBE)

    def __call__(self, frame, t):
        self.calls.append(t)
        return self.box(t)

    def detect_state(self, frame_u8_dev, K_dev, crop_size):
        t = int(frame_u8_dev[0, 0].item())
        self.states.append(t)
        return self.td.set_box(self.box(t), K_dev, crop_size)


@pytest.fixture(scope="module")
def loop_runs(td):
    """six frames, frame 2 loses the track: ``detect="host"`` and ``detect="device"`` at lookahead 1 and 2"""
    from onepose_st_amd import pnp_device
    pnp_device.load()
    g = np.random.default_rng(1)
    K, poses = trk_orc.SEQ_K, trk_orc.sequence_poses(6)
    pts = g.uniform(-0.08, 0.08, size=(200, 3))
    block = {k: v.to("cuda:0") for k, v in (("keypoints3d", torch.zeros(1, 200, 3)), ("descriptors3d_db", torch.zeros(1, 128, 200)),
                                           ("descriptors3d_coarse_db", torch.zeros(1, 256, 200)))}
    frames = [np.full((480, 640), t, np.uint8) for t in range(6)]
    runs = {}
    for detect in ("host", "device"):
        for la in (1, 2):
            fake, stub = _DeviceFakeModel(pts, poses, K), _StubDetector(td, K, poses)
            fake.fail_at = {2}
            recs = fl.SequenceRunner(fake, block, K, trk_orc.CUBE, stub, pnp="device", track="device", lookahead=la, detect=detect).run(frames)
            runs[detect, la] = (recs, stub.calls, stub.states)
    return runs


def same_records(a, b):
    assert len(a) == len(b)
    for x, y in zip(a, b):
        assert all(np.array_equal(bits(x[k]), bits(y[k])) for k in ("pose", "K_crop", "trans"))
        assert np.array_equal(x["inliers"], y["inliers"]) and np.array_equal(x["bbox"], y["bbox"]) and x["bbox"].dtype == y["bbox"].dtype == np.int32
        assert x["num_matches"] == y["num_matches"] and x["redetected"] == y["redetected"]


@pytest.mark.parametrize("lookahead", [1, 2])
def test_loop_with_a_stub_detector_equals_the_host_detection_bit_for_bit(loop_runs, lookahead):
    (h, h_calls, h_states), (d, d_calls, d_states) = loop_runs["host", lookahead], loop_runs["device", lookahead]
    assert h_calls == [0, 3] and h_states == [] and d_calls == [] and d_states == [0, 3]           # __call__ is never invoked
    assert [r["redetected"] for r in d] == [True, False, False, True, False, False] and all(len(r["inliers"]) >= 150 for t, r in enumerate(d) if t != 2)
    same_records(h, d)


def test_loop_records_do_not_depend_on_the_lookahead(loop_runs):
    same_records(loop_runs["device", 1][0], loop_runs["device", 2][0])


def test_loop_runs_the_real_detector_and_matcher(td, planted_detector):
    """The planted detector in front of the real 2D-3D matcher: random frames hold no object, so every frame is detected anew; every
    record carries the detected box, and ``__call__`` -- the host vote -- is never reached"""
    from onepose_st_amd.config import default_config
    from onepose_st_amd.model import OnePosePlus_model
    from onepose_st_amd.synthetic import make_synthetic_inputs, make_synthetic_state_dict
    det, calls = planted_detector
    dev = torch.device("cuda:0")
    cfg = default_config()
    sd = make_synthetic_state_dict(0, cfg)
    model = OnePosePlus_model(cfg).eval()
    model.load_state_dict(sd, strict=True)
    model.to(dev)
    obj = make_synthetic_inputs(sd, n_points=300, image_hw=(64, 64), n_plant=0, seed=4, config=cfg)
    block = {k: obj[k].to(dev) for k in ("keypoints3d", "descriptors3d_db", "descriptors3d_coarse_db")}
    g = np.random.default_rng(5)
    frames = [g.integers(0, 256, size=(VIEW_H, VIEW_W), dtype=np.uint8) for _ in range(2)]
    det.match_worker = None                                                             # the host vote must not be reached
    recs = fl.SequenceRunner(model, block, DET_K, trk_orc.CUBE, det, crop_size=128, pnp="device", track="device", lookahead=2, detect="device").run(frames)
    assert len(recs) == 2 and calls["n"] == 0
    for r in recs:
        b = r["bbox"]
        print(f"real detector in the loop: box {b.tolist()}, {r['num_matches']} matches, redetected {r['redetected']}")
        assert b[2] > b[0] and b[3] > b[1] and b.dtype == np.int32 and r["redetected"] is True
        assert np.abs(b - np.array([16, 8, VIEW_W + 16, VIEW_H + 8])).max() <= 1
        want_K, want_t = fl.crop_geometry(b, DET_K, 128)
        assert np.allclose(r["K_crop"], want_K, rtol=1e-12) and np.allclose(r["trans"], want_t, rtol=1e-12)
