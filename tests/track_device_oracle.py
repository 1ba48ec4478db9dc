"""Oracle of the device tracking's two box entries (``include/onepose_track.h``) in Python float64, every sum
written out in the one order the kernels use:

* ``cam_r = ((R_r0 X + R_r1 Y) + R_r2 Z) + t_r``
* ``uvw_r = (K_r0 cam_0 + K_r1 cam_1) + K_r2 cam_2``, then ``u = uvw_0 / uvw_2``, ``v = uvw_1 / uvw_2``
* ``s = S / wb``, ``trans`` as in ``frameloop.crop_geometry``, ``K_crop_ij = ((t_i0 K_0j) + (t_i1 K_1j)) + (t_i2 K_2j)``

Python floats are IEEE doubles and nothing here is contracted, so the GPU test asks the kernels for these bits.  ``tests/test_track_device_cpu.py``
checks this file against ``frameloop.project_bbox`` / ``crop_geometry`` without a GPU.
"""
import math

import numpy as np

LOST_POSE, LOST_BOX, STALE, NEEDS_HOST = 1, 2, 4, 8
STATUS_NO_POSE, STATUS_NEEDS_MORE = 1, 4                     # include/onepose_pnp_device.h
CUBE = 0.1 * np.array([[i, j, k] for i in (-1, 1) for j in (-1, 1) for k in (-1, 1)], dtype=np.float64)


def project(K, pose, bbox3d):
    """-> uv [8, 2] float64 (division by zero gives inf / nan like numpy's, without the warning)"""
    K = [[float(v) for v in row] for row in np.asarray(K, np.float64).reshape(3, 3)]
    P = [[float(v) for v in row] for row in np.asarray(pose, np.float64).reshape(3, 4)]
    out = np.empty((8, 2), dtype=np.float64)
    for c, (X, Y, Z) in enumerate(np.asarray(bbox3d, np.float64).reshape(8, 3).tolist()):
        cam = [((P[r][0] * X + P[r][1] * Y) + P[r][2] * Z) + P[r][3] for r in range(3)]
        w = [(K[r][0] * cam[0] + K[r][1] * cam[1]) + K[r][2] * cam[2] for r in range(3)]
        with np.errstate(all="ignore"):
            out[c, 0], out[c, 1] = np.float64(w[0]) / np.float64(w[2]), np.float64(w[1]) / np.float64(w[2])
    return out


def fits_int32(v) -> bool:
    """v truncates toward zero to an int32 (False for nan and the infinities)"""
    return bool(v > -2147483649.0 and v < 2147483648.0)


def projected_box(K, pose, bbox3d):
    """-> ([x0, y0, x1, y1] int32, the float64 minima and maxima), or (None, None) when the projection is unusable (``LOST_BOX``)"""
    uv = project(K, pose, bbox3d)
    if not all(fits_int32(v) for v in uv.reshape(-1)):
        return None, None
    ext = [min(uv[:, 0].tolist()), min(uv[:, 1].tolist()), max(uv[:, 0].tolist()), max(uv[:, 1].tolist())]
    box = [math.trunc(v) for v in ext]
    if box[2] <= box[0] or box[3] <= box[1]:
        return None, None
    return np.array(box, dtype=np.int32), np.array(ext)


def geometry(box, K, S):
    """-> (K_crop [3, 3], trans [3, 3]) of an int32 box"""
    K = [[float(v) for v in row] for row in np.asarray(K, np.float64).reshape(3, 3)]
    x0, y0, x1, y1 = [float(int(v)) for v in box]
    wb, hb = x1 - x0, y1 - y0
    s = float(S) / wb
    t = [[s, 0.0, -s * x0], [0.0, s, 0.5 * float(S) - s * (y0 + 0.5 * hb)], [0.0, 0.0, 1.0]]
    Kc = [[((t[i][0] * K[0][j]) + (t[i][1] * K[1][j])) + (t[i][2] * K[2][j]) for j in range(3)] for i in range(3)]
    return np.array(Kc, dtype=np.float64), np.array(t, dtype=np.float64)


def box_set(box, K, S):
    """-> (box int32[4], flag, K_crop, trans)"""
    box = np.asarray(box).astype(np.int32)
    if box[2] <= box[0] or box[3] <= box[1]:
        raise ValueError("empty box")
    return (box, 0, *geometry(box, K, S))


def box_from_pose(K, pose, n_inliers, status, bbox3d, prev_box, prev_flag, min_inliers, S):
    """-> (box int32[4], flag, K_crop, trans)"""
    flag = 0
    if int(prev_flag) != 0:
        flag |= STALE
    if (int(status) & STATUS_NO_POSE) or int(n_inliers) < int(min_inliers):
        flag |= LOST_POSE
    if int(status) & STATUS_NEEDS_MORE:
        flag |= NEEDS_HOST
    box = np.asarray(prev_box).astype(np.int32)
    if flag == 0:
        got, _ = projected_box(K, pose, bbox3d)
        if got is None:
            flag |= LOST_BOX
        else:
            box = got
    return (box, flag, *geometry(box, K, S))


# ---- the inputs of the parity tests --------------------------------------------------------------------------------------------------------
SEQ_K = np.array([[900.0, 0, 320.0], [0, 900.0, 240.0], [0, 0, 1]])
RND_K = np.array([[600.0, 0.5, 320.0], [0, 610.0, 240.0], [0, 0, 1]])
# a box that collapses: the cube a kilometre away projects into the one pixel of a principal point at a half-pixel position
HALF_K = np.array([[900.0, 0, 320.5], [0, 900.0, 240.5], [0, 0, 1]])
FAR_POSE = np.concatenate([np.eye(3), [[0.0], [0.0], [1000.0]]], axis=1)


def sequence_poses(n=12):
    """the sequence recipe of tests/test_gpu_pnp_device.py: a = 0.05 t about z, t = (0.01 t, 0, 0.8)"""
    poses = []
    for t in range(n):
        a = 0.05 * t
        R = np.array([[np.cos(a), -np.sin(a), 0], [np.sin(a), np.cos(a), 0], [0, 0, 1]])
        poses.append(np.concatenate([R, [[0.01 * t], [0.0], [0.8]]], axis=1))
    return poses


def rodrigues(w):
    th = math.sqrt(w[0] * w[0] + w[1] * w[1] + w[2] * w[2])
    Kx = np.array([[0, -w[2], w[1]], [w[2], 0, -w[0]], [-w[1], w[0], 0]], dtype=np.float64)
    return np.eye(3) + math.sin(th) / th * Kx + (1.0 - math.cos(th)) / (th * th) * (Kx @ Kx)


def random_poses(n=200, seed=7):
    """axis-angle of 0.1 - 0.7 rad about a random axis, t = (0, 0, 0.6) + 0.03 N"""
    g = np.random.default_rng(seed)
    poses = []
    for _ in range(n):
        ax = g.normal(size=3)
        R = rodrigues(ax / np.linalg.norm(ax) * g.uniform(0.1, 0.7))
        t = np.array([0.0, 0.0, 0.6]) + 0.03 * g.normal(size=3)
        poses.append(np.concatenate([R, t[:, None]], axis=1))
    return poses
