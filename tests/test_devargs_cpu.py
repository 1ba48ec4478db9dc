"""``devargs``: the argument checks the device-loop modules share and the codec of their packed read-back.  The
byte layouts are written out by hand here, on CPU tensors; nothing is compiled or enqueued."""
import os
import re

import numpy as np
import pytest
import torch

from onepose_st_amd import detect_device, devargs, hip, pnp_device, pose_eval, temporal

PKG = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "onepose_st_amd")
NO_CPU = "the HIP path needs device tensors (no CPU fallback)"


def raw(*arrays):
    return np.frombuffer(b"".join(np.ascontiguousarray(a).tobytes() for a in arrays), dtype=np.uint8).copy()       # writable


def make_poses(F, cap, ranges, status, seed=0, cls=pnp_device.DevicePoses):
    rng = np.random.default_rng(seed)
    pose = rng.standard_normal((F, 3, 4))
    mask = (np.arange(cap) % 3 != 1).astype(np.uint8)
    host = dict(pose=pose, status=np.asarray(status, np.int32), ranges=np.asarray(ranges, np.int32), mask=mask)
    dp = cls(torch.from_numpy(pose), torch.full((F,), 3, dtype=torch.int32), torch.from_numpy(host["status"]), torch.from_numpy(mask),
             torch.from_numpy(host["ranges"]))
    return dp, host


# ---- the byte layouts ------------------------------------------------------------------------------------------------------------------
def test_device_poses_pack_and_unpack():
    dp, h = make_poses(2, 5, [[0, 3], [3, 5]], [pnp_device.STATUS_NEEDS_MORE, pnp_device.STATUS_NO_POSE])
    state, flag = np.arange(168, dtype=np.uint8)[::-1].copy(), np.array([7], np.int32)
    packed = dp.pack(extra=(torch.from_numpy(state), torch.from_numpy(flag).view(torch.uint8)))
    want = raw(h["pose"], h["status"], h["ranges"], h["mask"], state, flag)
    assert packed.dtype == torch.uint8 and packed.numel() == 96 * 2 + 4 * 2 + 8 * 2 + 5 + 168 + 4
    assert np.array_equal(packed.numpy(), want)
    assert dp.packed_bytes == 96 * 2 + 4 * 2 + 8 * 2 + 5 and dp.pack().numel() == dp.packed_bytes
    out, (got_state, got_flag) = dp.unpack(want, (168, 4))
    assert np.array_equal(dp.status_host, h["status"])
    assert np.array_equal(got_state, state) and got_flag.view(np.int32)[0] == 7
    assert len(out) == 2
    for f, (p, homo, inl) in enumerate(out):
        assert np.array_equal(p, h["pose"][f]) and np.array_equal(homo[:3], h["pose"][f]) and np.array_equal(homo[3], [0, 0, 0, 1])
        assert inl.dtype == np.int64
    assert out[0][2].tolist() == [0, 2] and out[1][2].tolist() == []         # mask 1 0 1 | 1 0: frame 1 has no pose
    want[:] = 0                                                                 # the results are copies of the read-back buffer
    assert np.array_equal(out[0][0], h["pose"][0]) and np.array_equal(dp.status_host, h["status"]) and got_state[0] == 167
    plain = dp.unpack(dp.pack().numpy())
    assert len(plain) == 2 and np.array_equal(plain[1][0], h["pose"][1])
    assert [np.array_equal(a[0], b[0]) and a[2].tolist() == b[2].tolist() for a, b in zip(dp.to_host(), plain)] == [True, True]


def test_device_detection_to_host():
    V, cap = 3, 4
    boxes = np.arange(12, dtype=np.int32).reshape(V, 4) * 11 - 5
    status = np.array([0, detect_device.STATUS_NO_MODEL, 0], np.int32)
    ranges = np.array([[0, 3], [3, 4], [4, 4]], np.int32)                       # the last view has no rows
    mask, winner = np.array([1, 0, 1, 1], np.uint8), np.array([2], np.int32)
    det = detect_device.DeviceDetection(None, torch.from_numpy(boxes), torch.zeros(V, dtype=torch.int32), torch.zeros(V, 6, dtype=torch.float64),
                                        torch.from_numpy(status), torch.from_numpy(winner), torch.from_numpy(mask), torch.from_numpy(ranges))
    fields = (det.boxes, det.status, det.ranges, det.winner, det.inlier_mask)
    packed = devargs.pack(fields).numpy()
    assert np.array_equal(packed, raw(boxes, status, ranges, winner, mask)) and packed.size == 16 * V + 4 * V + 8 * V + 4 + cap
    votes, win = det.to_host()
    assert win == 2 and isinstance(win, int) and sorted(votes) == [0, 1, 2]
    assert np.array_equal(det.status_host, status)
    for v in range(V):
        assert np.array_equal(votes[v]["bbox"], boxes[v]) and votes[v]["bbox"].dtype == np.int32
    assert votes[0]["inliers"].shape == (3, 1) and votes[0]["inliers"].dtype == np.uint8 and votes[0]["inliers"].ravel().tolist() == [1, 0, 1]
    assert votes[1]["inliers"].shape == (0,)                                   # no model: the empty array of the host vote
    assert votes[2]["inliers"].shape == (0, 1)                                 # a model (status 0) over an empty range


@pytest.mark.parametrize("have", [(), ("add_dist",), ("add_dist", "proj2d")], ids=["no_model", "model", "model_and_K"])
def test_device_pose_errors_pack_and_unpack(have):
    F = 3
    host = {n: np.arange(F, dtype=np.float64) * (k + 1.5) - 1 for k, n in enumerate(("rot_cos", "t_err", "add_dist", "proj2d"))}
    flags = np.array([0, pose_eval.NO_POSE, pose_eval.BAD_INPUT], np.int32)
    t = {n: torch.from_numpy(a) if n in ("rot_cos", "t_err") + have else None for n, a in host.items()}
    err = pose_eval.DevicePoseErrors(t["rot_cos"], t["t_err"], t["add_dist"], t["proj2d"], torch.from_numpy(flags))
    names = ("rot_cos", "t_err") + have
    want = raw(*[host[n] for n in names], flags)
    assert want.size == 8 * F * len(names) + 4 * F and np.array_equal(err.pack().numpy(), want)
    got = err.unpack(want)
    assert list(got) == list(names) + ["flags"]
    assert all(np.array_equal(got[n], host[n]) and got[n].dtype == np.float64 for n in names)
    assert np.array_equal(got["flags"], flags) and got["flags"].dtype == np.int32
    want[:] = 0
    assert np.array_equal(got["t_err"], host["t_err"])                          # copies
    out = err.to_host(diameter=1.0)
    assert np.array_equal(out["t_errs"], host["t_err"]) and ("add_dist" in out) == bool(have) and ("proj2D_metric" in out) == (len(have) == 2)


def refined_sequence(cls=pnp_device.DevicePoses):
    frames, hosts = [None], []
    for k, cap in enumerate((5, 9)):
        dp, h = make_poses(1, cap, [[0, cap - k]], [0 if k == 0 else pnp_device.STATUS_NEEDS_MORE], seed=k + 1, cls=cls)
        hosts.append(h)
        frames.append({"poses": dp, "count": torch.tensor([cap - k], dtype=torch.int32)})
    return temporal.RefinedSequence(frames), hosts


def check_refined(seq, hosts):
    got = seq.to_host()
    assert got[0] is None and len(got) == 3
    for g, h in zip(got[1:], hosts):
        b, e = h["ranges"][0]
        assert np.array_equal(g["pose"], h["pose"][0]) and g["status"] == int(h["status"][0]) and g["count"] == e
        assert g["inliers"].tolist() == np.nonzero(h["mask"][b:e])[0].tolist()


def test_refined_sequence_slices_by_the_poses_own_size():
    seq, hosts = refined_sequence()
    packed = seq.pack()
    assert np.array_equal(packed.numpy(), raw(*[x for h, cap in zip(hosts, (5, 9)) for x in
                                                (h["pose"], h["status"], h["ranges"], h["mask"], np.array([h["ranges"][0, 1]], np.int32))]))
    assert packed.numel() == sum(f["poses"].packed_bytes + 4 for f in seq.frames if f is not None)
    check_refined(seq, hosts)
    assert temporal.RefinedSequence([None, None]).to_host() == [None, None]

    class LongerPoses(pnp_device.DevicePoses):                                  # one field more in the packed layout
        def _packed(self):
            return (*super()._packed(), self.n_inliers)

    seq, hosts = refined_sequence(LongerPoses)
    assert seq.frames[1]["poses"].packed_bytes == 96 + 4 + 8 + 5 + 4
    check_refined(seq, hosts)


def test_codec():
    tensors = [torch.arange(6, dtype=torch.float64).reshape(2, 3), torch.tensor([3], dtype=torch.int32), torch.arange(5, dtype=torch.uint8),
               torch.arange(4, dtype=torch.float32).reshape(2, 2).t()]         # the last one is not contiguous
    packed = devargs.pack(tensors)
    assert packed.dtype == torch.uint8 and np.array_equal(packed.numpy(), raw(*[t.numpy() for t in tensors]))
    layout = devargs.packed_layout(tensors)
    assert layout == [(np.dtype(np.float64), (2, 3), 48), (np.dtype(np.int32), (1,), 4), (np.dtype(np.uint8), (5,), 5), (np.dtype(np.float32), (2, 2), 16)]
    assert devargs.packed_bytes(tensors) == 73 == packed.numel()
    arrays, end = devargs.unpack(np.concatenate([np.zeros(3, np.uint8), packed.numpy(), np.zeros(2, np.uint8)]), layout, offset=3)
    assert end == 76 and all(np.array_equal(a, t.numpy()) and a.dtype == l[0] for a, t, l in zip(arrays, tensors, layout))


# ---- the helpers -----------------------------------------------------------------------------------------------------------------------
def test_count_arg():
    assert devargs.count_arg(None, "cpu") is None
    for got, want in ((devargs.count_arg(None, "cpu", default=7), 7), (devargs.count_arg(3, "cpu"), 3), (devargs.count_arg(3, "cpu", default=7), 3)):
        assert got.dtype == torch.int32 and tuple(got.shape) == (1,) and int(got) == want
    c = torch.tensor([4], dtype=torch.int32)
    assert devargs.count_arg(c, "cpu") is c and devargs.count_arg(c, "cpu", default=9) is c
    for bad in (torch.tensor([4]), torch.tensor([4, 5], dtype=torch.int32)):
        with pytest.raises(ValueError, match="^count: one int32 on the device$"):
            devargs.count_arg(bad, "cpu")


def test_mat64_and_k_table():
    eye = [[1, 0, 0], [0, 1, 0], [0, 0, 1]]
    m = devargs.mat64("trans", eye, [(3, 3)], "cpu")
    assert m.dtype == torch.float64 and m.is_contiguous() and m.tolist() == [[1.0, 0, 0], [0, 1.0, 0], [0, 0, 1.0]]
    f32 = torch.arange(12, dtype=torch.float32).reshape(4, 3).t()
    m = devargs.mat64("pose", f32, [(3, 4)], "cpu")
    assert m.dtype == torch.float64 and m.is_contiguous() and torch.equal(m, f32.double())
    f64 = torch.eye(3, dtype=torch.float64)
    assert devargs.mat64("K", f64, [(3, 3)], "cpu") is f64                      # as it is
    with pytest.raises(ValueError, match=r"^pose: \[3, 4\]$"):
        devargs.mat64("pose", f64, [(3, 4)], "cpu")
    assert devargs.mat64("poses", torch.zeros(5, 4, 4), [(None, 3, 4), (None, 4, 4)], "cpu", "[F, 3, 4] or [F, 4, 4]").shape == (5, 4, 4)
    for bad in (torch.zeros(3, 4), torch.zeros(5, 4, 3)):
        with pytest.raises(ValueError, match=r"^poses: \[F, 3, 4\] or \[F, 4, 4\]$"):
            devargs.mat64("poses", bad, [(None, 3, 4), (None, 4, 4)], "cpu", "[F, 3, 4] or [F, 4, 4]")

    K, shared = devargs.k_table(eye, 4, "cpu")
    assert shared == 1 and K.dtype == torch.float64 and tuple(K.shape) == (1, 9) and K.is_contiguous()
    per_frame = torch.arange(36, dtype=torch.float32).reshape(4, 3, 3)
    for exact in (False, True):
        K, shared = devargs.k_table(per_frame, 4, "cpu", exact=exact)
        assert shared == 0 and K.dtype == torch.float64 and tuple(K.shape) == (4, 9) and torch.equal(K, per_frame.double().reshape(4, 9))
        with pytest.raises(ValueError, match=r"^K: \[3, 3\] shared, or \[3, 3, 3\]$"):
            devargs.k_table(per_frame, 3, "cpu", exact=exact)
    flat = torch.arange(9, dtype=torch.float64)
    assert devargs.k_table(flat, 2, "cpu")[1] == 1 and devargs.k_table(per_frame.reshape(4, 9), 4, "cpu")[1] == 0       # what reshapes is taken
    for loose in (flat, per_frame.reshape(4, 9)):
        with pytest.raises(ValueError, match=r"^K: \[3, 3\] shared, or \[4, 3, 3\]$"):
            devargs.k_table(loose, 4, "cpu", exact=True)


def test_point_tables():
    a, b = torch.zeros(4, 2), torch.zeros(4, 3)
    got = devargs.point_tables("pts_2d", a, 2, "pts_3d", b, 3, max_rows=4, min_rows=1)
    assert got[0] is a and got[1] is b
    strided = torch.zeros(2, 4).t()
    assert devargs.point_tables("a", strided, 2, "b", b, 3)[0].is_contiguous()
    for bad_a, bad_b in ((torch.zeros(3, 2), b), (torch.zeros(4, 3), b), (a, torch.zeros(4, 2)), (torch.zeros(8), b)):
        with pytest.raises(ValueError, match=r"^pts_2d \[cap, 2\] and pts_3d \[cap, 3\] must have the same length$"):
            devargs.point_tables("pts_2d", bad_a, 2, "pts_3d", bad_b, 3)
    with pytest.raises(ValueError, match=r"^own_2d \[cap, 2\] and own_3d \[cap, 3\] must have the same length, at least 1$"):
        devargs.point_tables("own_2d", torch.zeros(0, 2), 2, "own_3d", torch.zeros(0, 3), 3, min_rows=1)
    assert devargs.point_tables("a", torch.zeros(0, 2), 2, "b", torch.zeros(0, 3), 3)[0].shape == (0, 2)
    with pytest.raises(ValueError, match=r"^mkpts0 and mkpts1: \[cap, 2\], the same length$"):
        devargs.point_tables("mkpts0", a, 2, "mkpts1", torch.zeros(5, 2), 2)
    for bad_a, bad_b in ((a.double(), b), (a, b.half())):
        with pytest.raises(ValueError, match="^pts_2d and pts_3d: float32$"):
            devargs.point_tables("pts_2d", bad_a, 2, "pts_3d", bad_b, 3)
    with pytest.raises(ValueError, match="^at most 3 rows$"):
        devargs.point_tables("pts_2d", a, 2, "pts_3d", b, 3, max_rows=3)
    with pytest.raises(ValueError, match="float32"):                           # the dtype is reported before the number of rows
        devargs.point_tables("pts_2d", a.double(), 2, "pts_3d", b, 3, max_rows=3)


def test_at_least_one_row():
    a, b, count, ids = torch.ones(2, 2), torch.ones(2, 3), torch.tensor([2], dtype=torch.int32), torch.zeros(2, dtype=torch.int64)
    got = devargs.at_least_one_row(a, b, count, ids)
    assert got[0] is a and got[1] is b and got[2] is count and got[3] is ids
    assert devargs.at_least_one_row(a, b)[2:] == (None, None)
    a0, b0, c0, i0 = devargs.at_least_one_row(torch.ones(0, 2), torch.ones(0, 3), count, torch.zeros(0, dtype=torch.int64))
    assert (a0.dtype, tuple(a0.shape), b0.dtype, tuple(b0.shape)) == (torch.float32, (1, 2), torch.float32, (1, 3)) and not a0.any() and not b0.any()
    assert c0.dtype == torch.int32 and c0.tolist() == [0] and i0.dtype == torch.int64 and i0.tolist() == [0]
    a0, b0, c0, i0 = devargs.at_least_one_row(torch.ones(0, 2), torch.ones(0, 2))
    assert tuple(b0.shape) == (1, 2) and c0.tolist() == [0] and i0 is None      # no b_ids in, none out; the count is still zero


def test_need_tensors_and_need_device():
    t = torch.zeros(1)
    hip.need_tensors([("a", t), ("b", t)])                                     # CPU tensors are tensors
    hip.need_tensors(iter([("a", t)]))
    with pytest.raises(TypeError, match="^b: expected a tensor$"):
        hip.need_tensors([("a", t), ("b", [1.0]), ("c", None)])
    with pytest.raises(hip.HipLibraryError, match=re.escape(NO_CPU)):
        hip.need_device(iter([("a", t)]))
    with pytest.raises(hip.HipLibraryError, match=re.escape(NO_CPU)):
        hip.on_device([t])
    hip.on_device([])
    with pytest.raises(TypeError, match="^b: expected a tensor$"):              # every type before any device
        hip.need_device([("a", t), ("b", 3)])
    assert hip.NO_CPU_FALLBACK == NO_CPU
    with pytest.raises(hip.HipLibraryError, match=re.escape(NO_CPU)):
        hip.ptr(t)


def test_callers_keep_their_order_of_refusals():
    """One call with two things wrong reports what it reported before the helpers"""
    a, b = torch.zeros(4, 2), torch.zeros(4, 3)
    with pytest.raises(hip.HipLibraryError, match=re.escape(NO_CPU)):          # pnp_device: the device before the shapes
        pnp_device.ransac_pnp(np.eye(3), a, b[:3])
    with pytest.raises(ValueError, match="the same length"):                    # detect_device: the shapes before the device
        detect_device.vote(a, a[:3], torch.zeros(4, dtype=torch.int64), [[8, 8]], (8, 8), np.eye(3))
    with pytest.raises(ValueError, match="^count: one int32 on the device$"):
        detect_device.vote(a, a, torch.zeros(4, dtype=torch.int64), [[8, 8]], (8, 8), np.eye(3), count=torch.tensor([4]))
    with pytest.raises(hip.HipLibraryError, match=re.escape(NO_CPU)):
        detect_device.vote(a, a, torch.zeros(4, dtype=torch.int64), [[8, 8]], (8, 8), np.eye(3), count=4)
    with pytest.raises(hip.HipLibraryError, match=re.escape(NO_CPU)):          # temporal, pose_eval: the device first
        temporal.collect(a, b[:3], np.eye(3))
    with pytest.raises(hip.HipLibraryError, match=re.escape(NO_CPU)):
        pose_eval.pose_errors(torch.zeros(2, 3, 3), np.zeros((2, 3, 4)))


# ---- one home each ---------------------------------------------------------------------------------------------------------------------
def package_sources():
    out = {}
    for name in sorted(os.listdir(PKG)):
        if name.endswith(".py"):
            with open(os.path.join(PKG, name)) as f:
                out[name] = f.read()
    return out


def test_every_shared_sentence_has_one_home():
    texts = package_sources()
    homes = lambda needle: [(n, t.count(needle)) for n, t in texts.items() if needle in t]
    assert homes(NO_CPU) == [("hip.py", 1)]
    assert homes("count: one int32 on the device") == [("devargs.py", 1)]
    assert homes("the library wants a table of at least one row") == [("devargs.py", 1)]
    assert homes(": expected a tensor") == [("hip.py", 1)]
    for name in ("pnp_device.py", "detect_device.py", "temporal.py", "pose_eval.py", "frameloop.py"):
        assert "devargs." in texts[name], name
        found = re.findall(r"o \+= \d+ \*|\* 108\b|\[o:o \+ \d+ \*", texts[name])     # a packed read-back cut by a byte count written by hand
        assert not found, (name, found)
