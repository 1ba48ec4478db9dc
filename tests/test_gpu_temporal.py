"""The temporal refinement on the device (``onepose_st_amd/temporal.py``, ``libonepose_temporal.so``) against its numpy restatement
(tests/temporal_oracle.py): pyramid, tracker, collect and inject bit for bit, the count rules, run-to-run bytes, ``refine_sequence``
against the same stages composed by hand and against the oracle chain, and ``SequenceRunner(refine="device")``.  Everything is small: at
most 120 x 160 frames, 64 points, six frames."""
import numpy as np
import pytest
import torch

from onepose_st_amd import frameloop as fl, hip
from tests import pnp_device_oracle as pnp_orc
from tests import temporal_oracle as to

pytestmark = pytest.mark.gpu

POSE_BAR = 1e-4                  # DESIGN.md section 2, as in tests/test_gpu_pnp_device.py
DEV = "cuda:0"


@pytest.fixture(scope="module")
def tm():
    from onepose_st_amd import temporal
    temporal.load()
    return temporal


def dev(a, dtype=None):
    return torch.from_numpy(np.ascontiguousarray(a, dtype=dtype)).to(DEV)


def same_bytes(t, a):
    """a device tensor against a numpy array: dtype, shape and every byte (NaN payloads included)"""
    got = t.cpu().numpy()
    return got.dtype == a.dtype and got.shape == a.shape and got.tobytes() == np.ascontiguousarray(a).tobytes()


def frame_of(shape, seed):
    return np.random.default_rng(seed).integers(0, 256, size=shape, dtype=np.uint8)


# ---- pyramid ----------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("H,W,levels", [(37, 53, 4), (2, 2, 1), (120, 160, 3), (16, 70, 2)])
def test_pyramid_is_bit_equal(tm, H, W, levels):
    """odd sizes at every level (37 x 53 -> 19 x 27 -> 10 x 14 -> 5 x 7), the smallest frame, the test scene's size, and a level wider
    than one 64-column tile with a partial second one"""
    frame = frame_of((H, W), 3) if (H, W) != (120, 160) else to.scene("shift")[0]
    want = to.pyramid(frame, levels)
    pyr = tm.build_pyramid(dev(frame), levels)
    assert pyr.data.numel() == to.pyramid_bytes(H, W, levels)
    for l in range(levels):
        assert same_bytes(pyr.level(l), want[l]), l
    again = tm.build_pyramid(dev(frame), levels)
    shifted = torch.cat([torch.zeros(1, dtype=torch.uint8, device=DEV), dev(frame).reshape(-1)])[1:].view(H, W)
    assert shifted.data_ptr() % 4 == 1 and shifted.is_contiguous()     # a frame the 4-byte loads of level 0 cannot take
    odd = tm.build_pyramid(shifted, levels)
    for l in range(levels):
        assert torch.equal(again.level(l), pyr.level(l)) and torch.equal(odd.level(l), pyr.level(l))


# ---- track ------------------------------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def scenes(tm):
    """both planted scenes with their host and device pyramids at 1 and 3 levels, built once"""
    out = {}
    for kind in ("shift", "similarity"):
        src, dst, pts = to.planted_scene(kind)
        out[kind] = {"pts": pts, "pts_dev": dev(pts)}
        for L in (1, 3):
            out[kind][L] = (to.pyramid(src, L), to.pyramid(dst, L), tm.build_pyramid(dev(src), L), tm.build_pyramid(dev(dst), L))
    return out


def assert_tracks_equal(got, want, rows=slice(None)):
    assert np.array_equal(got.flags.cpu().numpy()[rows], want["flags"][rows])
    assert np.array_equal(got.iterations.cpu().numpy()[rows], want["iterations"][rows])
    assert got.pts.cpu().numpy()[rows].tobytes() == want["pts"][rows].tobytes()
    assert got.fb_error.cpu().numpy()[rows].tobytes() == want["fb_error"][rows].tobytes()


@pytest.mark.parametrize("levels", [1, 3])
@pytest.mark.parametrize("window", [5, 15, 21])
@pytest.mark.parametrize("max_iters", [1, 2, 30])
@pytest.mark.parametrize("kind", ["shift", "similarity"])
def test_track_is_bit_equal(tm, scenes, kind, max_iters, window, levels):
    """64 points, one per planted flag among them: flags and iteration counts equal, ``pts`` and ``fb_error`` bit-equal -- every operation
    is correctly rounded and the order is fixed"""
    s = scenes[kind]
    S, D, Sd, Dd = s[levels]
    want = to.track(S, D, s["pts"], window=window, max_iters=max_iters)
    got = tm.track(Sd, Dd, s["pts_dev"], window=window, max_iters=max_iters)
    assert_tracks_equal(got, want)
    if (levels, window, max_iters) == (3, 15, 30):
        seen = np.bitwise_or.reduce(want["flags"])
        assert seen & to.DEGENERATE and seen & to.OUT_OF_IMAGE and seen & to.FB_FAIL and seen & to.BAD_INPUT and (want["flags"] == 0).sum() >= 30
    again = tm.track(Sd, Dd, s["pts_dev"], window=window, max_iters=max_iters)
    for a, b in ((got.pts, again.pts), (got.fb_error, again.fb_error)):
        assert torch.equal(a.view(torch.int64), b.view(torch.int64))
    assert torch.equal(got.flags, again.flags) and torch.equal(got.iterations, again.iterations)


def test_track_without_the_check_and_with_a_guess(tm, scenes):
    s = scenes["shift"]
    S, D, Sd, Dd = s[1]
    guess = s["pts"] + np.array(to.SHIFT) + 0.4                     # one level reaches the truth from 0.4 px away, not from 6.3 px
    want = to.track(S, D, s["pts"], guess=guess, window=15, fb_threshold=None)
    got = tm.track(Sd, Dd, s["pts_dev"], guess=dev(guess), window=15, fb_threshold=None)
    assert_tracks_equal(got, want)
    assert np.isnan(want["fb_error"]).all() and not (want["flags"] & to.FB_FAIL).any()


def test_track_pose_projection_guess(tm):
    """rows with a usable projection start from it, the others from ``p`` (or the caller's guess): at one level the first kind reaches
    the truth and the second cannot"""
    src, dst, pts, truth = to.scene("shift")                        # the scene without the planted patches
    S, D, Sd, Dd = to.pyramid(src, 1), to.pyramid(dst, 1), tm.build_pyramid(dev(src), 1), tm.build_pyramid(dev(dst), 1)
    pts, truth = pts[:16], pts[:16] + np.array(to.SHIFT)
    K = np.array([[2.0, 0.0, 1.0], [0.0, 2.0, -1.0], [0.0, 0.0, 1.0]])
    pose = np.concatenate([np.eye(3), [[0.5], [0.25], [1.0]]], axis=1)
    z = 3.0                                                         # cam = scale * (X + t); u = K cam / cam_z
    X = np.stack([(truth[:, 0] - 1.0) / 2.0 * z - 0.5, (truth[:, 1] + 1.0) / 2.0 * z - 0.25, np.full(16, z - 1.0)], axis=1).astype(np.float32)
    X[12] = [0.0, 0.0, -5.0]                                        # behind the camera
    X[13] = [1e4, 0.0, 2.0]                                         # projects outside the image
    X[14] = [np.nan, 0.0, 2.0]
    X[15] = [0.0, 0.0, -1.0]                                        # cam_z = 0: a non-finite projection
    want = to.track(S, D, pts, pts_3d=X, pose=pose, K=K, scale=2.0, window=15)
    got = tm.track(Sd, Dd, dev(pts), pts_3d=dev(X), pose=dev(pose), K=dev(K), scale=2.0, window=15)
    assert_tracks_equal(got, want)
    plain = to.track(S, D, pts, window=15)
    for k in ("pts", "flags", "iterations", "fb_error"):
        assert want[k][12:].tobytes() == plain[k][12:].tobytes()   # the four rows without a usable projection started from p
    err = np.linalg.norm(want["pts"][:12] - truth[:12], axis=1)
    assert (want["flags"][:12] == 0).all() and err.max() < 0.06, (want["flags"][:12], err)
    assert not np.array_equal(want["pts"][:12], plain["pts"][:12])
    with_guess = to.track(S, D, pts, guess=truth, pts_3d=X, pose=pose, K=K, scale=2.0, window=15)
    got = tm.track(Sd, Dd, dev(pts), guess=dev(truth), pts_3d=dev(X), pose=dev(pose), K=dev(K), scale=2.0, window=15)
    assert_tracks_equal(got, with_guess)
    assert (with_guess["flags"][12:] == 0).all()


@pytest.mark.parametrize("count", [0, 10, 64, 1000, -3])
def test_track_count_handling(tm, scenes, count):
    """a count above the capacity is clamped, 0 (and a negative one) runs clean, rows at or past the count keep their sentinel"""
    s = scenes["shift"]
    S, D, Sd, Dd = s[3]
    fill = (-7.5, -9, -9, -7.5)
    want = to.track(S, D, s["pts"], count=count, window=5, fill=fill)
    out = tm.Tracks(torch.full((64, 2), fill[0], dtype=torch.float64, device=DEV), torch.full((64,), fill[1], dtype=torch.int32, device=DEV),
                    torch.full((64,), fill[2], dtype=torch.int32, device=DEV), torch.full((64,), fill[3], dtype=torch.float64, device=DEV))
    got = tm.track(Sd, Dd, s["pts_dev"], count=torch.tensor([count], dtype=torch.int32, device=DEV), window=5, out=out)
    assert got is out
    assert_tracks_equal(got, want)
    n = max(0, min(count, 64))
    assert (want["flags"][n:] == -9).all() and (want["pts"][n:] == -7.5).all()


# ---- collect and inject -------------------------------------------------------------------------------------------------------------------
def table_case(seed, cap=200):
    g = np.random.default_rng(seed)
    K = np.array([[900.0, 0, 320.0], [0, 900.0, 240.0], [0, 0, 1]])
    _, trans = fl.crop_geometry([203, 117, 398, 345], K, 512)
    trans[2, :2] = [1e-5, -2e-5]                                      # a general 3 x 3: the homogeneous divide matters
    return {"trans": trans, "p2": g.uniform(0, 512, (cap, 2)).astype(np.float32), "p3": g.normal(size=(cap, 3)).astype(np.float32),
            "mask": (g.uniform(size=cap) < 0.6).astype(np.uint8), "g": g}


@pytest.mark.parametrize("count,use_mask", [(None, True), (137, True), (200, False), (0, True), (999, False)])
def test_collect_is_exact(tm, count, use_mask):
    c = table_case(1)
    mask = c["mask"] if use_mask else None
    want_q, want_3, k = to.collect(c["p2"], c["p3"], c["trans"], count=count, mask=mask)
    cnt = None if count is None else torch.tensor([count], dtype=torch.int32, device=DEV)
    runs = [tm.collect(dev(c["p2"]), dev(c["p3"]), dev(c["trans"]), count=cnt, mask=None if mask is None else dev(mask)) for _ in range(2)]
    q = runs[0]
    assert int(q.count.item()) == k
    assert same_bytes(q.pts[:k], want_q) and same_bytes(q.pts_3d[:k], want_3)
    assert torch.equal(runs[1].count, q.count) and torch.equal(runs[1].pts[:k].view(torch.int64), q.pts[:k].view(torch.int64))
    assert torch.equal(runs[1].pts_3d[:k], q.pts_3d[:k])


def test_inject_is_exact_with_three_sources(tm):
    """capacity 200 with 3 sources of 200 / 130 / 77 rows; the second has no row left (every flag lost), the third a count below its
    capacity; a lost row's NaN point is never read into the table"""
    c = table_case(2)
    g = c["g"]
    lost = np.array([0, to.FLAG_MAX_ITERS, to.DEGENERATE, to.OUT_OF_IMAGE, to.FB_FAIL, to.BAD_INPUT, to.FB_FAIL | to.FLAG_MAX_ITERS], np.int32)
    sources_np, sources_dev = [], []
    for cap, count, all_lost in ((200, None, False), (130, None, True), (77, 50, False)):
        flags = lost[g.integers(2, 7, cap)] if all_lost else lost[g.integers(0, 7, cap)]
        pts = g.uniform(0, 640, (cap, 2))
        pts[(flags & to.LOST & ~to.FB_FAIL) != 0] = np.nan
        p3 = g.normal(size=(cap, 3)).astype(np.float32)
        sources_np.append((p3, pts, flags, count))
        cnt = None if count is None else torch.tensor([count], dtype=torch.int32, device=DEV)
        sources_dev.append((tm.Queries(dev(pts), dev(p3), cnt), tm.Tracks(dev(pts), dev(flags), None, None, count=cnt)))
    for own_count in (163, 0, 200):
        want2, want3, k = to.inject(c["p2"], c["p3"], own_count, sources_np, c["trans"])
        cnt = torch.tensor([own_count], dtype=torch.int32, device=DEV)
        runs = [tm.inject(dev(c["p2"]), dev(c["p3"]), cnt, sources_dev, dev(c["trans"])) for _ in range(2)]
        out2, out3, n = runs[0]
        assert int(n.item()) == k and out2.shape == (200 + 200 + 130 + 77, 2)
        assert same_bytes(out2[:k], want2) and same_bytes(out3[:k], want3)
        assert not torch.isnan(out2[:k]).any()
        assert torch.equal(runs[1][2], n) and torch.equal(runs[1][0][:k], out2[:k]) and torch.equal(runs[1][1][:k], out3[:k])
    only = to.inject(c["p2"], c["p3"], 163, [sources_np[1]], c["trans"])
    assert only[2] == 163                                             # a source with no selected rows contributes nothing
    out2, out3, n = tm.inject(dev(c["p2"]), dev(c["p3"]), torch.tensor([163], dtype=torch.int32, device=DEV), [sources_dev[1]], dev(c["trans"]))
    assert int(n.item()) == 163 and same_bytes(out2[:163], only[0])
    none2, none3, n0 = tm.inject(dev(c["p2"]), dev(c["p3"]), None, [], dev(c["trans"]))
    assert int(n0.item()) == 200 and same_bytes(none2, c["p2"]) and same_bytes(none3, c["p3"])


# ---- the chain ----------------------------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def plane(tm):
    """six frames of the textured plane; per frame 40 planted matches (the plane's points under the true pose, through the crop) and 30 %
    wrong ones on top, and the first pass's device pose with its inlier mask"""
    from onepose_st_amd import pnp_device
    g = np.random.default_rng(4)
    K, poses = to.PLANE_K, to.plane_poses(6)
    frames = [to.plane_frame(p) for p in poses]
    K_crop, trans = fl.crop_geometry([14, 2, 110, 94], K, 256)
    entries, host = [], []
    for t, pose in enumerate(poses):
        X = np.concatenate([g.uniform(-0.045, 0.045, (40, 2)), np.zeros((40, 1))], axis=1)
        uv = to.project(K, pose, X)
        good = to.map_to_crop(trans, uv) + g.normal(scale=0.1, size=(40, 2))
        X = np.concatenate([X, np.concatenate([g.uniform(-0.045, 0.045, (12, 2)), np.zeros((12, 1))], axis=1)])
        p2 = np.concatenate([good, g.uniform(0, 256, (12, 2))]).astype(np.float32)
        order = g.permutation(52)
        p2, p3 = p2[order], X[order].astype(np.float32)
        e = {"pts_2d": dev(p2), "pts_3d": dev(p3), "K_crop": dev(K_crop), "trans": dev(trans)}
        first = pnp_device.ransac_pnp(e["K_crop"], e["pts_2d"], e["pts_3d"], scale=1000, pnp_reprojection_error=7, trials=64)
        e["mask"], e["pose"] = first.inlier_mask, first.pose[0]
        entries.append(e)
        host.append({"p2": p2, "p3": p3, "mask": first.inlier_mask.cpu().numpy(), "planted": np.sort(np.argsort(order)[:40])})
    return {"K": K, "K_crop": K_crop, "trans": trans, "poses": poses, "frames": frames, "entries": entries, "host": host}


CHAIN = dict(temp_thresh=2, levels=3, window=11, trials=64)


def test_refine_sequence_equals_the_stages_composed_by_hand(tm, plane):
    from onepose_st_amd import pnp_device
    seq = tm.refine_sequence(plane["frames"], plane["entries"], plane["K"], **CHAIN)
    assert [f is None for f in seq.frames] == [True, True, False, False, False, False]
    pyrs = [tm.build_pyramid(dev(f), 3) for f in plane["frames"]]
    qs = [tm.collect(e["pts_2d"], e["pts_3d"], e["trans"], mask=e["mask"]) for e in plane["entries"]]
    for t in range(2, 6):
        e, f = plane["entries"][t], seq.frames[t]
        sources = [(qs[s], tm.track(pyrs[s], pyrs[t], qs[s].pts, count=qs[s].count, window=11)) for s in (t - 2, t - 1)]
        p2, p3, n = tm.inject(e["pts_2d"], e["pts_3d"], None, sources, e["trans"])
        poses = pnp_device.ransac_pnp(e["K_crop"], p2, p3, count=n, scale=1000, pnp_reprojection_error=7, trials=64)
        k = int(n.item())
        kept = sum(int(((tr.flags[:int(q.count.item())] & tm.LOST) == 0).sum().item()) for q, tr in sources)
        assert k == 52 + kept and kept >= 40, (k, kept)               # own rows + the tracked rows that were not lost
        assert torch.equal(f["count"], n) and torch.equal(f["pts_2d"][:k], p2[:k]) and torch.equal(f["pts_3d"][:k], p3[:k])
        assert torch.equal(f["poses"].pose.view(torch.int64), poses.pose.view(torch.int64))
        assert torch.equal(f["poses"].inlier_mask[:k], poses.inlier_mask[:k]) and torch.equal(f["poses"].status, poses.status)
        for (_, a), b in zip(sources, f["tracks"]):
            assert torch.equal(a.flags[:40], b.flags[:40])
    host = seq.to_host()
    assert host[0] is None and host[1] is None and host[2]["count"] == int(seq.frames[2]["count"].item())


def test_refine_sequence_with_the_pose_guess(tm, plane):
    """``pose_guess``: a carried point starts from the projection of its 3D point under frame ``t``'s first-pass pose and the full-frame
    ``K``; the first refined frame against the same calls made by hand"""
    seq = tm.refine_sequence(plane["frames"][:3], plane["entries"][:3], plane["K"], pose_guess=True, **CHAIN)
    e = plane["entries"][2]
    pyrs = [tm.build_pyramid(dev(f), 3) for f in plane["frames"][:3]]
    sources = []
    for s in (0, 1):
        q = tm.collect(plane["entries"][s]["pts_2d"], plane["entries"][s]["pts_3d"], plane["entries"][s]["trans"], mask=plane["entries"][s]["mask"])
        sources.append((q, tm.track(pyrs[s], pyrs[2], q.pts, count=q.count, pts_3d=q.pts_3d, pose=e["pose"], K=dev(plane["K"]), window=11)))
    p2, p3, n = tm.inject(e["pts_2d"], e["pts_3d"], None, sources, e["trans"])
    k = int(n.item())
    f = seq.frames[2]
    assert k > 52 + 40 and torch.equal(f["count"], n) and torch.equal(f["pts_2d"][:k], p2[:k]) and torch.equal(f["pts_3d"][:k], p3[:k])
    plain = tm.track(pyrs[0], pyrs[2], sources[0][0].pts, count=sources[0][0].count, window=11)
    assert not torch.equal(plain.iterations[:40], sources[0][1].iterations[:40])       # the guess was used: the iterations ran differently
    with pytest.raises(ValueError, match="pose_guess needs"):
        tm.refine_sequence(plane["frames"][:3], plane["entries"][:3], None, pose_guess=True, **CHAIN)


def test_refined_poses_meet_the_pose_bar_against_the_oracle_chain(tm, plane):
    """temporal_oracle + pnp_device_oracle on the same first-pass masks: the injected tables are equal byte for byte, so the poses differ
    by the device solver's own rounding only (the bar of tests/test_gpu_pnp_device.py) and the inlier sets are equal"""
    got = tm.refine_sequence(plane["frames"], plane["entries"], plane["K"], **CHAIN)
    host = got.to_host()
    pyr = [to.pyramid(f, 3) for f in plane["frames"]]
    qs = [to.collect(h["p2"], h["p3"], plane["trans"], mask=h["mask"]) for h in plane["host"]]
    for t in range(2, 6):
        h = plane["host"][t]
        sources = []
        for s in (t - 2, t - 1):
            tr = to.track(pyr[s], pyr[t], qs[s][0], window=11)
            sources.append((qs[s][1], tr["pts"], tr["flags"], None))
        p2, p3, k = to.inject(h["p2"], h["p3"], None, sources, plane["trans"])
        assert host[t]["count"] == k
        assert same_bytes(got.frames[t]["pts_2d"][:k], p2) and same_bytes(got.frames[t]["pts_3d"][:k], p3)
        want = pnp_orc.solve(plane["K_crop"], p2, p3, scale=1000.0, reproj=7.0, trials=64)
        dist = pnp_orc.pose_distance(host[t]["pose"], want["pose"][0])
        true = pnp_orc.pose_distance(host[t]["pose"], plane["poses"][t])
        print(f"frame {t}: {k} rows, {len(host[t]['inliers'])} inliers, refined pose vs oracle chain {dist:.2e}, vs the planted pose {true:.2e}")
        assert dist < POSE_BAR
        assert np.array_equal(host[t]["inliers"], np.nonzero(want["mask"][:k])[0])
        assert set(h["planted"]) <= set(host[t]["inliers"].tolist()) and len(host[t]["inliers"]) > 40 + 40


class _PlaneModel:
    """stand-in matcher on the device: the plane's points through the true pose of the frame and the crop the loop chose"""

    def __init__(self, pts3d, poses, K):
        self.pts3d, self.poses, self.K, self.trans, self.t = dev(pts3d), dev(np.stack(poses)), dev(K), None, 0

    def __call__(self, data):
        t = data.get("frame_index", self.t)
        trans = data["crop_trans"] if "crop_trans" in data else dev(self.trans)
        pose = self.poses[t]
        uv = self.K @ (pose[:, :3] @ self.pts3d.T + pose[:, 3:4])
        uv = torch.cat([uv[:2] / uv[2:], torch.ones_like(uv[2:])])
        data["mkpts_3d_db"], data["mkpts_query_f"] = self.pts3d.float(), (trans @ uv).T[:, :2].float()
        self.t = t + 1


@pytest.mark.parametrize("mode", ["host", 1, 3])
def test_sequence_runner_refine_changes_no_existing_key(tm, plane, mode):
    """``refine="device"`` after the host-tracked loop and after the device-tracked loop at lookahead 1 and 3: every key of a
    ``refine=None`` run bit-identical; frames 0-1 repeat the first pass, frames 2-5 carry a refined pose of their own frame"""
    g = np.random.default_rng(9)
    K, poses, frames = plane["K"], plane["poses"], plane["frames"]
    pts = np.concatenate([g.uniform(-0.045, 0.045, (60, 2)), np.zeros((60, 1))], axis=1)
    box3d = 0.05 * np.array([[i, j, k * 0.2] for i in (-1, 1) for j in (-1, 1) for k in (-1, 1)], dtype=np.float64)
    block = {k: v.to(DEV) for k, v in (("keypoints3d", torch.zeros(1, 60, 3)), ("descriptors3d_db", torch.zeros(1, 128, 60)),
                                       ("descriptors3d_coarse_db", torch.zeros(1, 256, 60)))}
    runs = {}
    for refine in (None, "device"):
        fake = _PlaneModel(pts, poses, K)

        def crop_fn(dev_frame, bbox, size):
            fake.trans = fl.crop_geometry(bbox, K, size)[1]
            return torch.zeros(1, 1, size, size)

        kw = dict(track="host") if mode == "host" else dict(track="device", lookahead=mode)
        runs[refine] = fl.SequenceRunner(fake, block, K, box3d, lambda frame, t: fl.project_bbox(K, poses[t], box3d), crop_size=128,
                                         crop_fn=crop_fn, pnp="device", refine=refine, temp_thresh=2,
                                         refine_options=dict(levels=3, window=11), **kw).run(frames)
    old = {"pose", "inliers", "bbox", "K_crop", "trans", "num_matches", "redetected"}
    for t, (a, b) in enumerate(zip(runs[None], runs["device"])):
        assert set(a) == old and set(b) == old | {"pose_refined", "inliers_refined", "refined"}
        for k in old:
            assert np.asarray(a[k]).tobytes() == np.asarray(b[k]).tobytes() and np.asarray(a[k]).dtype == np.asarray(b[k]).dtype, (t, k)
        assert b["refined"] == (t >= 2)
        if t < 2:
            assert b["pose_refined"] is b["pose"] and b["inliers_refined"] is b["inliers"]
        else:
            d = pnp_orc.pose_distance(b["pose_refined"], poses[t])
            print(f"{mode}, frame {t}: {len(b['inliers_refined'])} refined inliers of {b['num_matches']} own rows + carried ones, vs the planted pose {d:.2e}")
            assert d < 0.05 and len(b["inliers_refined"]) > b["num_matches"]           # a pose of this frame, with carried rows among its inliers


# ---- arguments ----------------------------------------------------------------------------------------------------------------------------
def test_entries_refuse_bad_arguments_before_any_launch(tm):
    frame = dev(frame_of((24, 32), 0))
    pyr, pts = tm.build_pyramid(frame, 2), torch.zeros(4, 2, dtype=torch.float64, device=DEV)
    for bad in (dict(window=10), dict(window=33), dict(max_iters=0), dict(eps=0.0), dict(min_eig=-1.0), dict(fb_threshold=-1.0), dict(scale=0.0)):
        with pytest.raises(ValueError):
            tm.track(pyr, pyr, pts, **bad)
    with pytest.raises(ValueError, match="levels=6"):
        tm.build_pyramid(frame, 6)                                    # 24 x 32 -> 12 x 16 -> 6 x 8 -> 3 x 4 -> 2 x 2 at level 4, 1 x 1 at level 5
    assert tm.build_pyramid(frame, 5).level(4).shape == (2, 2)
    with pytest.raises(ValueError, match="mismatched pyramids"):
        tm.track(pyr, tm.build_pyramid(frame, 3), pts)
    with pytest.raises(ValueError, match="mismatched pyramids"):
        tm.track(pyr, tm.build_pyramid(dev(frame_of((24, 34), 0)), 2), pts)
    with pytest.raises(ValueError):
        tm.track(pyr, pyr, pts.float())
    with pytest.raises(ValueError, match="all three or none"):
        tm.track(pyr, pyr, pts, pts_3d=torch.zeros(4, 3, device=DEV))
    with pytest.raises(hip.HipLibraryError):
        tm.track(pyr, pyr, pts.cpu())
    with pytest.raises(hip.HipLibraryError):
        tm.build_pyramid(frame.cpu())
    with pytest.raises(hip.HipLibraryError):
        tm.collect(torch.zeros(4, 2), torch.zeros(4, 3, device=DEV), np.eye(3))
    with pytest.raises(hip.HipLibraryError):
        tm.inject(torch.zeros(4, 2, device=DEV), torch.zeros(4, 3), None, [], np.eye(3))
    with pytest.raises(ValueError):
        tm.collect(torch.zeros(4, 2, device=DEV), torch.zeros(5, 3, device=DEV), np.eye(3))
    with pytest.raises(ValueError, match="temp_thresh"):
        tm.refine_sequence([], [], temp_thresh=9)
