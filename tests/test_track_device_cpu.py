"""The device tracking's oracle (``tests/track_device_oracle.py``) against the host loop's ``frameloop.project_bbox`` /
``crop_geometry`` and the flag rules of include/onepose_track.h, without a GPU; the binding's header-driven parts as well."""
import os
import sys

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import track_device_oracle as orc  # noqa: E402

from onepose_st_amd import frameloop as fl  # noqa: E402
from onepose_st_amd import hip, pnp_device, track_device  # noqa: E402

S = 512


def _edge(ext):
    """how close a projected extremum comes to an integer: where truncation could turn on one rounding"""
    return float(np.min(np.abs(ext - np.rint(ext))))


@pytest.mark.parametrize("name, K, poses, margin", [("sequence", orc.SEQ_K, orc.sequence_poses(12), 0.018), ("random", orc.RND_K, orc.random_poses(200, 7), 8.7e-4)],
                         ids=["sequence", "random"])
def test_oracle_box_equals_project_bbox(name, K, poses, margin):
    """0 mismatches on the twelve sequence poses and on 200 seeded random ones; no projected extremum is at a rounding edge (the
    distances to the nearest integer recorded with the inputs: 0.018 and 8.7e-4 -- these inputs must not get closer than half of that)"""
    closest = np.inf
    for pose in poses:
        box, ext = orc.projected_box(K, pose, orc.CUBE)
        assert box is not None and box.dtype == np.int32
        assert np.array_equal(box, fl.project_bbox(K, pose, orc.CUBE))
        closest = min(closest, _edge(ext))
    print(f"{name}: {len(poses)} poses, 0 box mismatches, closest projected extremum to an integer {closest:.2e}")
    assert closest > 0.5 * margin


def test_oracle_geometry_against_crop_geometry():
    """K_crop / trans within 1e-12 relative of ``crop_geometry`` (a matrix product whose three-term sums may round in another order) on
    every box of the two pose sets and a few crop sizes"""
    worst = 0.0
    for K, poses in ((orc.SEQ_K, orc.sequence_poses(12)), (orc.RND_K, orc.random_poses(200, 7))):
        for pose in poses:
            box, _ = orc.projected_box(K, pose, orc.CUBE)
            for size in (512, 128, 33):
                Kc, tr = orc.geometry(box, K, size)
                wKc, wtr = fl.crop_geometry(box, K, size)
                for got, want in ((Kc, wKc), (tr, wtr)):
                    rel = np.abs(got - want) / np.maximum(np.abs(want), 1e-300)
                    worst = max(worst, float(rel.max()))
    print(f"oracle K_crop / trans vs crop_geometry: largest relative difference {worst:.2e}")
    assert worst <= 1e-12


def _case(**kw):
    a = dict(K=orc.SEQ_K, pose=orc.sequence_poses(3)[2], n_inliers=150, status=0, bbox3d=orc.CUBE, prev_box=[11, 22, 333, 444], prev_flag=0,
             min_inliers=20, S=S)
    a.update(kw)
    return orc.box_from_pose(**a)


def test_flag_bits_one_at_a_time_and_the_carried_box():
    prev = np.array([11, 22, 333, 444], dtype=np.int32)
    box, flag, Kc, tr = _case()
    assert flag == 0 and np.array_equal(box, fl.project_bbox(orc.SEQ_K, orc.sequence_poses(3)[2], orc.CUBE)) and not np.array_equal(box, prev)
    assert np.array_equal(Kc, orc.geometry(box, orc.SEQ_K, S)[0])
    collapsed = dict(pose=orc.FAR_POSE, K=orc.HALF_K)                                # every corner lands in the principal point's pixel
    on_plane = np.concatenate([np.eye(3), [[0.0], [0.0], [0.1]]], axis=1)            # the z = -0.1 corners have depth 0
    for kw, want in ((dict(n_inliers=19), orc.LOST_POSE), (dict(n_inliers=20), 0), (dict(status=orc.STATUS_NO_POSE), orc.LOST_POSE),
                     (dict(status=orc.STATUS_NEEDS_MORE), orc.NEEDS_HOST), (collapsed, orc.LOST_BOX), (dict(pose=on_plane), orc.LOST_BOX),
                     (dict(prev_flag=orc.LOST_POSE), orc.STALE), (dict(prev_flag=orc.STALE), orc.STALE),
                     (dict(status=orc.STATUS_NO_POSE | orc.STATUS_NEEDS_MORE, prev_flag=2), orc.LOST_POSE | orc.NEEDS_HOST | orc.STALE),
                     (dict(collapsed, n_inliers=3), orc.LOST_POSE)):           # LOST_BOX is tested only when no other bit is set
        box, flag, Kc, tr = _case(**kw)
        assert flag == want, kw
        if want:
            carried = orc.geometry(prev, kw.get("K", orc.SEQ_K), S)
            assert np.array_equal(box, prev) and np.array_equal(Kc, carried[0]) and np.array_equal(tr, carried[1]), kw
    assert not np.isfinite(orc.project(orc.SEQ_K, on_plane, orc.CUBE)).all()
    uv = orc.project(orc.HALF_K, orc.FAR_POSE, orc.CUBE)
    assert np.isfinite(uv).all() and (uv.astype(np.int32) == [320, 240]).all()         # x1 == x0 and y1 == y0
    huge = np.concatenate([np.eye(3), [[1e9], [0.0], [0.2]]], axis=1)               # finite, outside int32
    assert np.isfinite(orc.project(orc.SEQ_K, huge, orc.CUBE)).all() and _case(pose=huge)[1] == orc.LOST_BOX


def test_stale_marks_everything_downstream():
    poses = orc.sequence_poses(5)
    state = orc.box_set(fl.project_bbox(orc.SEQ_K, poses[0], orc.CUBE), orc.SEQ_K, S)
    flags, boxes = [], []
    for t in range(4):
        state = orc.box_from_pose(orc.SEQ_K, poses[t], 4 if t == 1 else 150, 0, orc.CUBE, state[0], state[1], 20, S)
        flags.append(state[1]); boxes.append(state[0])
    assert flags == [0, orc.LOST_POSE, orc.STALE, orc.STALE]
    assert np.array_equal(boxes[1], boxes[0]) and np.array_equal(boxes[3], boxes[0])         # the last good box is carried
    with pytest.raises(ValueError):
        orc.box_set([5, 5, 5, 9], orc.SEQ_K, S)


def test_binding_reads_the_header_and_refuses_the_cpu():
    assert track_device.ABI_VERSION == 1
    assert (track_device.LOST_POSE, track_device.LOST_BOX, track_device.STALE, track_device.NEEDS_HOST) == (orc.LOST_POSE, orc.LOST_BOX, orc.STALE,
                                                                                                              orc.NEEDS_HOST)
    assert (orc.STATUS_NO_POSE, orc.STATUS_NEEDS_MORE) == (pnp_device.STATUS_NO_POSE, pnp_device.STATUS_NEEDS_MORE)
    assert track_device.STATE_BYTES == 168
    with pytest.raises(TypeError, match="takes 11 arguments"):
        track_device.check_arity("optrk_box_set", (1, 2, 3))
    with pytest.raises(hip.HipLibraryError):
        track_device.set_box([0, 0, 4, 4], torch.eye(3, dtype=torch.float64), 64)
    with pytest.raises(hip.HipLibraryError):
        track_device.set_box([0, 0, 4, 4], np.eye(3), 64, device="cpu")
    with pytest.raises(hip.HipLibraryError):
        track_device.crop(torch.zeros(8, 8, dtype=torch.uint8), None, 8)
    cpu_poses = pnp_device.DevicePoses(torch.zeros(1, 3, 4, dtype=torch.float64), torch.zeros(1, dtype=torch.int32), torch.zeros(1, dtype=torch.int32),
                                       torch.zeros(1, dtype=torch.uint8), torch.zeros(1, 2, dtype=torch.int32))
    with pytest.raises(hip.HipLibraryError):
        track_device.next_box(cpu_poses, None, np.eye(3), torch.zeros(8, 3, dtype=torch.float64))


def test_sequence_runner_refuses_device_tracking_without_device_pnp():
    block = {"keypoints3d": torch.zeros(1, 4, 3)}
    with pytest.raises(ValueError, match="track='device' needs pnp='device'"):
        fl.SequenceRunner(None, block, np.eye(3), orc.CUBE, None, track="device")
    with pytest.raises(ValueError, match="track="):
        fl.SequenceRunner(None, block, np.eye(3), orc.CUBE, None, track="gpu")
    with pytest.raises(ValueError, match="lookahead"):
        fl.SequenceRunner(None, block, np.eye(3), orc.CUBE, None, pnp="device", track="device", lookahead=0)
