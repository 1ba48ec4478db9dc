"""Device tracking on the GPU: the box entries of ``libonepose_track.so`` against the Python oracle (``tests/track_device_oracle.py``) bit
for bit, the crop against ``frameloop.crop_query`` bit for bit, the chain matcher -> pose -> next box without a read-back, and
``SequenceRunner(pnp="device", track="device")`` against ``track="host"`` at every ``lookahead``.  Everything is small: one-workgroup
kernels, crops of at most 64 x 64, six-frame sequences.
"""
import os
import sys

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import pnp_device_oracle as pnp_orc  # noqa: E402
import track_device_oracle as orc  # noqa: E402

from onepose_st_amd import frameloop as fl  # noqa: E402

pytestmark = pytest.mark.gpu
POSE_BAR = 1e-4
S = 512
PREV_BOX = [11, 22, 333, 444]


@pytest.fixture(scope="module")
def td():
    if not torch.cuda.is_available():
        pytest.skip("needs the MI355X")
    from onepose_st_amd import track_device
    track_device.load()
    return track_device


@pytest.fixture(scope="module")
def pd():
    if not torch.cuda.is_available():
        pytest.skip("needs the MI355X")
    from onepose_st_amd import pnp_device
    pnp_device.load()
    return pnp_device


def dev_t(a, dtype=None):
    return torch.as_tensor(np.ascontiguousarray(a), dtype=dtype).to("cuda:0")


def bits(a):
    return np.ascontiguousarray(a, dtype=np.float64).view(np.uint64)


def fake_poses(pd, poses, n_inliers=150, status=0):
    """a DevicePoses holding the given poses, as the solver would have left them"""
    F = len(poses)
    full = lambda v: torch.full((F,), v, dtype=torch.int32, device="cuda:0")      # noqa: E731
    return pd.DevicePoses(dev_t(np.stack(poses)), full(n_inliers), full(status), torch.zeros(1, dtype=torch.uint8, device="cuda:0"),
                          torch.zeros(F, 2, dtype=torch.int32, device="cuda:0"))


def read_states(td, states):
    """one read-back for a list of states -> [(box, flag, K_crop, trans)]"""
    raw = torch.stack([s.blob for s in states]).cpu().numpy()
    return [td.TrackState.unpack(r) for r in raw]


def same_state(got, want):
    return (np.array_equal(got[0], want[0]) and got[0].dtype == np.int32 and got[1] == want[1] and np.array_equal(bits(got[2]), bits(want[2]))
            and np.array_equal(bits(got[3]), bits(want[3])))


# ---- the box entries ---------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", ["sequence", "random"])
def test_box_entries_equal_the_oracle_bit_for_bit(td, pd, name):
    """``box_from_pose`` on the CPU test's poses (twelve of the sequence recipe, 200 seeded random ones): box and flag exact, K_crop and
    trans bit-equal; ``box_set`` on the same boxes at two crop sizes"""
    K, poses = (orc.SEQ_K, orc.sequence_poses(12)) if name == "sequence" else (orc.RND_K, orc.random_poses(200, 7))
    Kd, cube = dev_t(K), dev_t(orc.CUBE)
    prev = td.set_box(PREV_BOX, Kd, S)
    dp = fake_poses(pd, poses)
    got = read_states(td, [td.next_box(dp, prev, Kd, cube, frame=f, min_inliers=20, crop_size=S) for f in range(len(poses))])
    boxes = []
    for f, pose in enumerate(poses):
        want = orc.box_from_pose(K, pose, 150, 0, orc.CUBE, PREV_BOX, 0, 20, S)
        assert want[1] == 0 and np.array_equal(want[0], fl.project_bbox(K, pose, orc.CUBE))
        assert same_state(got[f], want), (f, got[f], want)
        boxes.append(want[0])
    for size in (S, 33):
        got = read_states(td, [td.set_box(b, Kd, size) for b in boxes[:12]])
        for b, g in zip(boxes, got):
            assert same_state(g, orc.box_set(b, K, size)), (b, size)
    assert same_state(read_states(td, [prev])[0], orc.box_set(PREV_BOX, K, S))


ON_PLANE = np.concatenate([np.eye(3), [[0.0], [0.0], [0.1]]], axis=1)            # the z = -0.1 corners have depth 0
FLAG_CASES = {
    "inliers_19": (dict(n_inliers=19), orc.LOST_POSE),
    "inliers_20": (dict(n_inliers=20), 0),
    "no_pose": (dict(status=orc.STATUS_NO_POSE), orc.LOST_POSE),
    "needs_more": (dict(status=orc.STATUS_NEEDS_MORE), orc.NEEDS_HOST),
    "box_collapses": (dict(pose=orc.FAR_POSE, K=orc.HALF_K), orc.LOST_BOX),
    "corner_on_camera_plane": (dict(pose=ON_PLANE), orc.LOST_BOX),
    "prev_flag_set": (dict(prev_flag=orc.LOST_BOX), orc.STALE),
}


@pytest.mark.parametrize("case", sorted(FLAG_CASES))
def test_every_flag_and_the_carried_box(td, pd, case):
    kw, want_flag = FLAG_CASES[case]
    a = dict(K=orc.SEQ_K, pose=orc.sequence_poses(3)[2], n_inliers=150, status=0, prev_flag=0)
    a.update(kw)
    Kd, cube = dev_t(a["K"]), dev_t(orc.CUBE)
    prev = td.set_box(PREV_BOX, Kd, S)
    prev.flag.fill_(a["prev_flag"])
    dp = fake_poses(pd, [a["pose"]], a["n_inliers"], a["status"])
    got, = read_states(td, [td.next_box(dp, prev, Kd, cube, min_inliers=20, crop_size=S)])
    want = orc.box_from_pose(a["K"], a["pose"], a["n_inliers"], a["status"], orc.CUBE, PREV_BOX, a["prev_flag"], 20, S)
    assert want[1] == want_flag and got[1] == want_flag
    assert same_state(got, want)
    if want_flag:                                               # the carried box and the geometry of the carried box
        assert got[0].tolist() == PREV_BOX
        carried = orc.geometry(PREV_BOX, a["K"], S)
        assert np.array_equal(bits(got[2]), bits(carried[0])) and np.array_equal(bits(got[3]), bits(carried[1]))
    else:
        assert got[0].tolist() != PREV_BOX


# ---- the crop ----------------------------------------------------------------------------------------------------------------------------------
CROP_BOXES = {"inside": (5, 4, 40, 30), "left": (-9, 6, 21, 29), "top": (8, -7, 37, 20), "right": (30, 5, 70, 33), "bottom": (10, 20, 44, 51),
              "outside": (60, 45, 90, 70), "width_1": (17, 3, 18, 30), "tall": (20, 2, 29, 36), "wide": (2, 12, 50, 19)}


@pytest.fixture(scope="module")
def crop_frame():
    if not torch.cuda.is_available():
        pytest.skip("needs the MI355X")
    return torch.from_numpy(np.random.default_rng(3).integers(0, 256, size=(37, 53), dtype=np.uint8)).to("cuda:0")


@pytest.mark.parametrize("size", [8, 33, 64])
def test_crop_equals_crop_query_bit_for_bit(td, crop_frame, size):
    """37 x 53 frame; 33 leaves partial 32 x 8 thread tiles"""
    Kd = dev_t(orc.SEQ_K)
    for name, box in CROP_BOXES.items():
        got = td.crop(crop_frame, td.set_box(box, Kd, size), size)
        want = fl.crop_query(crop_frame, box, size)
        assert got.shape == (1, 1, size, size) and torch.equal(got, want), name
        assert (name == "outside") == (not bool(want.any())), name
    empty = td.set_box((5, 4, 40, 30), Kd, size)
    for box in ((9, 4, 9, 30), (5, 30, 40, 4), (-2 ** 31, 0, 2 ** 31 - 1, 10)):          # empty, inverted, wider than OPTRK_MAX_BOX_SIDE
        empty.box.copy_(dev_t(np.array(box, dtype=np.int32)))
        out = td.crop(crop_frame, empty, size)
        assert not bool(out.any()) and out.shape == (1, 1, size, size)


# ---- arguments -----------------------------------------------------------------------------------------------------------------------------------
def test_entries_refuse_bad_arguments_before_any_launch(td, pd, crop_frame):
    Kd, cube = dev_t(orc.SEQ_K.reshape(9)), dev_t(orc.CUBE)
    st = td.set_box(PREV_BOX, Kd, S)
    dp = fake_poses(pd, orc.sequence_poses(1))
    box = torch.full((4,), -9, dtype=torch.int32, device="cuda:0")
    flag = torch.full((1,), -9, dtype=torch.int32, device="cuda:0")
    Kc, tr = torch.zeros(9, dtype=torch.float64, device="cuda:0"), torch.zeros(9, dtype=torch.float64, device="cuda:0")
    out = torch.full((8, 8), -9.0, dtype=torch.float32, device="cuda:0")
    P = lambda t: t.data_ptr()      # noqa: E731

    def box_set(b=(1, 2, 30, 40), size=S, **null):
        a = dict(K=P(Kd), box=P(box), flag=P(flag), K_crop=P(Kc), trans=P(tr))
        a.update(null)
        td.call("optrk_box_set", *b, a["K"], size, a["box"], a["flag"], a["K_crop"], a["trans"], None)

    def from_pose(size=S, min_inliers=20, **null):
        a = dict(K=P(Kd), pose=P(dp.pose), n_inliers=P(dp.n_inliers), status=P(dp.status), bbox3d=P(cube), prev_box=P(st.box), prev_flag=P(st.flag),
                 box=P(box), flag=P(flag), K_crop=P(Kc), trans=P(tr))
        a.update(null)
        td.call("optrk_box_from_pose", a["K"], a["pose"], a["n_inliers"], a["status"], a["bbox3d"], a["prev_box"], a["prev_flag"], min_inliers, size,
                a["box"], a["flag"], a["K_crop"], a["trans"], None)

    def crop(H=37, W=53, size=8, **null):
        a = dict(image=P(crop_frame), box=P(st.box), out=P(out))
        a.update(null)
        td.call("optrk_crop", a["image"], H, W, a["box"], size, a["out"], None)

    for name in ("K", "box", "flag", "K_crop", "trans"):
        with pytest.raises(ValueError, match="null pointer"):
            box_set(**{name: None})
    for b in ((5, 2, 5, 40), (1, 40, 30, 40), (9, 2, 5, 40)):
        with pytest.raises(ValueError, match="empty box"):
            box_set(b=b)
    for size in (0, -3, td.MAX_CROP + 1):
        with pytest.raises(ValueError, match="crop size"):
            box_set(size=size)
        with pytest.raises(ValueError, match="crop size"):
            from_pose(size=size)
        with pytest.raises(ValueError, match="bad sizes"):
            crop(size=size)
    for name in ("K", "pose", "n_inliers", "status", "bbox3d", "prev_box", "prev_flag", "box", "flag", "K_crop", "trans"):
        with pytest.raises(ValueError, match="null pointer"):
            from_pose(**{name: None})
    with pytest.raises(ValueError, match="min_inliers"):
        from_pose(min_inliers=-1)
    for name in ("image", "box", "out"):
        with pytest.raises(ValueError, match="null pointer"):
            crop(**{name: None})
    for hw in (dict(H=0), dict(W=0)):
        with pytest.raises(ValueError, match="bad sizes"):
            crop(**hw)
    with pytest.raises(ValueError, match="empty box"):
        td.set_box((4, 4, 4, 9), Kd, S)
    with pytest.raises(TypeError, match="takes 7 arguments"):
        td.call("optrk_crop", P(crop_frame), 37, 53, P(st.box), 8, P(out))
    torch.cuda.synchronize()
    assert flag.cpu().tolist() == [-9] and box.cpu().tolist() == [-9] * 4 and bool((out == -9.0).all())        # nothing was launched
    from_pose()
    crop()
    torch.cuda.synchronize()
    assert flag.cpu().tolist() == [0] and box.cpu().tolist() != [-9] * 4 and bool((out >= 0).all())


# ---- the chain through the real matcher ------------------------------------------------------------------------------------------------------------
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


def test_chain_without_a_read_back_through_the_real_matcher(td, pd, matcher):
    """The planted c1 frame: ``enqueue_after(pend, state.K_crop)`` and ``next_box`` before ``finish()``.  The state is ``set_box`` of the
    box [0, 0, S, S] at crop size S, whose trans is the identity, so ``state.K_crop`` holds K's own doubles and the pose must equal
    ``enqueue_after(pend, K)`` bit for bit; the next box is ``project_bbox`` of the pose that is read back afterwards."""
    from onepose_st_amd.synthetic import CONFIG_SIZES, make_synthetic_inputs
    model, sd, cfg = matcher
    n, hw, plant = CONFIG_SIZES["c1"]
    inp = make_synthetic_inputs(sd, n_points=n, image_hw=hw, n_plant=plant, seed=pnp_orc.FRAME_SEED, config=cfg)
    data = {k: inp[k].to("cuda:0") for k in ("keypoints3d", "descriptors3d_db", "descriptors3d_coarse_db")}
    K = inp["K"].numpy().astype(np.float64)
    pts = inp["keypoints3d"][0].numpy().astype(np.float64)
    lo, hi = pts.min(axis=0), pts.max(axis=0)
    bbox3d = np.array([[x, y, z] for x in (lo[0], hi[0]) for y in (lo[1], hi[1]) for z in (lo[2], hi[2])])
    Kd, cube = dev_t(K), dev_t(bbox3d)
    state = td.set_box((0, 0, 640, 640), Kd, 640)
    pf = model.enqueue_features(data, inp["feat_c"].to("cuda:0"), inp["feat_f"].to("cuda:0"), inp["image_hw"])
    chained = pd.enqueue_after(pf, state.K_crop, pnp_reprojection_error=5.0, trials=1024)
    nxt = td.next_box(chained, state, Kd, cube, min_inliers=20, crop_size=640)
    plain = pd.enqueue_after(pf, K, pnp_reprojection_error=5.0, trials=1024)
    pf.finish()                                                                            # nothing was read before this line
    assert np.array_equal(bits(state.K_crop.cpu().numpy()), bits(K)) and np.array_equal(state.trans.cpu().numpy(), np.eye(3))
    assert torch.equal(chained.pose, plain.pose) and torch.equal(chained.n_inliers, plain.n_inliers) and torch.equal(chained.status, plain.status)
    assert torch.equal(chained.inlier_mask, plain.inlier_mask)
    (pose, _, inl), = chained.to_host()
    box, flag, K_crop, trans = nxt.to_host()
    want = fl.project_bbox(K, pose, bbox3d)
    print(f"chain: {len(inl)} inliers, next box {box.tolist()} (project_bbox: {want.tolist()}), flag {flag}")
    assert len(inl) >= 300 and chained.status_host.tolist() == [0]
    assert flag == 0 and np.array_equal(box, want) and want[2] > want[0] and want[3] > want[1]
    assert same_state((box, flag, K_crop, trans), orc.box_from_pose(K, pose, len(inl), 0, bbox3d, (0, 0, 640, 640), 0, 20, 640))


# ---- the loop ------------------------------------------------------------------------------------------------------------------------------------
class _DeviceFakeModel:
    """``test_gpu_pnp_device.py``'s stand-in matcher with the projection done by torch on the device: the object points through the
    true pose of frame ``data["frame_index"]`` and the crop's ``trans`` (``data["crop_trans"]`` with device tracking, else what the
    loop's ``crop_fn`` recorded); four matches on a failing frame"""

    def __init__(self, pts3d, poses, K):
        self.pts3d, self.poses, self.K = dev_t(pts3d), dev_t(np.stack(poses)), dev_t(K)
        self.fail_at, self.trans, self.t, self.seen = set(), None, 0, []

    def __call__(self, data):
        t = data.get("frame_index", self.t)
        trans = data["crop_trans"] if "crop_trans" in data else dev_t(self.trans)
        pose = self.poses[t]
        cam = pose[:, :3] @ self.pts3d.T + pose[:, 3:4]
        uv = self.K @ cam
        uv = torch.cat([uv[:2] / uv[2:], torch.ones_like(uv[2:])])
        uvc = (trans @ uv).T[:, :2]
        n = 4 if t in self.fail_at else self.pts3d.shape[0]
        data["mkpts_3d_db"] = self.pts3d[:n].float()
        data["mkpts_query_f"] = uvc[:n].float()
        self.seen.append(t)
        self.t = t + 1


@pytest.fixture(scope="module")
def loop_runs(td, pd):
    """six frames, frame 2 loses the track: ``track="host"`` and ``track="device"`` at lookahead 1, 2, 3 (all with ``pnp="device"``)"""
    g = np.random.default_rng(1)
    K = orc.SEQ_K
    pts = g.uniform(-0.08, 0.08, size=(200, 3))
    poses = orc.sequence_poses(6)
    block = {k: v.to("cuda:0") for k, v in (("keypoints3d", torch.zeros(1, 200, 3)), ("descriptors3d_db", torch.zeros(1, 128, 200)),
                                           ("descriptors3d_coarse_db", torch.zeros(1, 256, 200)))}
    frames = [np.zeros((480, 640), np.uint8)] * 6
    runs = {}
    for mode in ("host", 1, 2, 3):
        fake = _DeviceFakeModel(pts, poses, K)
        fake.fail_at = {2}
        calls = []

        def detector(frame, t):
            calls.append(t)
            return fl.project_bbox(K, poses[t], orc.CUBE)

        def crop_fn(dev_frame, bbox, size):
            fake.trans = fl.crop_geometry(bbox, K, size)[1]
            return torch.zeros(1, 1, size, size)

        kw = dict(track="host") if mode == "host" else dict(track="device", lookahead=mode)
        recs = fl.SequenceRunner(fake, block, K, orc.CUBE, detector, crop_fn=crop_fn, pnp="device", **kw).run(frames)
        runs[mode] = (recs, calls, fake.seen)
    return runs


@pytest.mark.parametrize("lookahead", [1, 2, 3])
def test_device_tracked_loop_follows_the_host_tracked_loop(loop_runs, lookahead):
    """Detector calls [0, 3]; boxes, re-detection flags, match counts and inlier sets of the host-tracked loop; poses within the pose bar
    (the matches of the two loops differ by the float32 rounding of points that went through trans matrices equal to 1e-12).
    Measured on the MI355X: see DESIGN.md section 6m."""
    (h, h_calls, _), (d, d_calls, seen) = loop_runs["host"], loop_runs[lookahead]
    assert h_calls == d_calls == [0, 3] and len(d) == len(h) == 6
    assert seen[-1] == 5 and len(seen) == 6 + min(lookahead - 1, 3)               # what was speculated past frame 2 ran again
    assert [r["redetected"] for r in d] == [True, False, False, True, False, False]
    for t, (a, b) in enumerate(zip(h, d)):
        assert a["redetected"] == b["redetected"] and np.array_equal(a["bbox"], b["bbox"]) and a["num_matches"] == b["num_matches"]
        assert np.array_equal(a["inliers"], b["inliers"]) and (len(b["inliers"]) >= 150 or t == 2)
        dist = pnp_orc.pose_distance(b["pose"], a["pose"])
        rel = max(float((np.abs(b[k] - a[k]) / np.maximum(np.abs(a[k]), 1e-300)).max()) for k in ("K_crop", "trans"))
        print(f"lookahead {lookahead}, frame {t}: device-tracked pose vs host-tracked {dist:.2e}, {len(b['inliers'])} inliers, K_crop / trans rel {rel:.1e}")
        assert dist < POSE_BAR and rel <= 1e-12
        assert b["bbox"].dtype == np.int32 and b["K_crop"].shape == (3, 3) and b["trans"].shape == (3, 3)


def test_records_do_not_depend_on_the_lookahead(loop_runs):
    base = loop_runs[1][0]
    for la in (2, 3):
        for a, b in zip(base, loop_runs[la][0]):
            assert all(np.array_equal(bits(a[k]), bits(b[k])) for k in ("pose", "K_crop", "trans"))
            assert np.array_equal(a["inliers"], b["inliers"]) and np.array_equal(a["bbox"], b["bbox"])
            assert a["num_matches"] == b["num_matches"] and a["redetected"] == b["redetected"]


def test_device_tracked_loop_runs_the_real_model(td, pd, matcher):
    """``test_sequence_runner_on_device_runs_the_real_model``'s setup with ``track="device", lookahead=2``: random frames hold no object,
    so every frame rewinds and the detector is called for each; the records equal the host-tracked run's (K_crop and trans, which that
    run forms with numpy's matrix product, to the 1e-12 of a three-term sum's rounding order)"""
    from onepose_st_amd.synthetic import make_synthetic_inputs
    model, sd, cfg = matcher
    dev = torch.device("cuda:0")
    obj = make_synthetic_inputs(sd, n_points=300, image_hw=(64, 64), n_plant=0, seed=4, config=cfg)
    block = {k: obj[k].to(dev) for k in ("keypoints3d", "descriptors3d_db", "descriptors3d_coarse_db")}
    K = np.array([[500.0, 0, 160.0], [0, 500.0, 120.0], [0, 0, 1]])
    g = np.random.default_rng(5)
    frames = [g.integers(0, 256, size=(240, 320), dtype=np.uint8) for _ in range(3)]
    runs = {}
    for mode, kw in (("host", {}), ("device", dict(track="device", lookahead=2))):
        calls = []

        def detector(frame, t):
            calls.append(t)
            return [40, 30, 200, 190]

        runs[mode] = (fl.SequenceRunner(model, block, K, orc.CUBE, detector, crop_size=128, pnp="device", **kw).run(frames), calls)
    (h, h_calls), (d, d_calls) = runs["host"], runs["device"]
    assert h_calls == d_calls == [0, 1, 2] and len(d) == len(h) == 3
    for a, b in zip(h, d):
        assert np.array_equal(a["pose"], b["pose"]) and np.array_equal(a["inliers"], b["inliers"]) and len(b["inliers"]) == 0
        assert np.array_equal(a["bbox"], b["bbox"]) and a["num_matches"] == b["num_matches"] and a["redetected"] == b["redetected"] is True
        for k in ("K_crop", "trans"):
            rel = float((np.abs(b[k] - a[k]) / np.maximum(np.abs(a[k]), 1e-300)).max())
            print(f"{k}: device vs host-tracked record, largest relative difference {rel:.1e}")
            assert rel <= 1e-12
