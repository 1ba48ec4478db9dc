"""The specification of the pose evaluation (include/onepose_pose_eval.h) restated in numpy float64, one function per stage,
every expression in the written order.  The device kernels are compared with these bit for bit; nothing here calls a library routine whose
evaluation order is not pinned (no ``np.dot``, ``np.linalg.norm``, ``np.mean`` or pairwise ``np.sum``)."""
import numpy as np

BLOCK = 256
NO_POSE, BAD_INPUT = 1, 2
UNIT_SCALE = {"m": 100.0, "cm": 1.0, "mm": 0.1}


def _poses(p):
    p = np.asarray(p, dtype=np.float64)
    return p[:, :3, :]                                      # [F, 3, 4] of a [F, 3, 4] or [F, 4, 4] table


def flags(pose_pred, pose_gt, no_pose=None):
    """int32 [F]: ``NO_POSE`` where the caller says so, ``BAD_INPUT`` where either pose has a non-finite entry"""
    P, G = _poses(pose_pred), _poses(pose_gt)
    out = np.zeros(len(P), np.int32)
    if no_pose is not None:
        out[np.asarray(no_pose, bool)] |= NO_POSE
    bad = ~(np.isfinite(P).all(axis=(1, 2)) & np.isfinite(G).all(axis=(1, 2)))
    out[bad] |= BAD_INPUT
    return out


def errors(pose_pred, pose_gt, no_pose=None, unit="m"):
    """-> (rot_cos [F], t_err [F] in cm, flags [F]); a flagged frame: NaN and +inf"""
    P, G = _poses(pose_pred), _poses(pose_gt)
    fl = flags(P, G, no_pose)
    with np.errstate(all="ignore"):
        trace = np.zeros(len(P))
        for i in range(3):
            for j in range(3):
                trace = trace + P[:, i, j] * G[:, i, j]
        rot_cos = (np.where(trace <= 3.0, trace, 3.0) - 1.0) / 2.0
        dx, dy, dz = (P[:, k, 3] - G[:, k, 3] for k in range(3))
        t_err = UNIT_SCALE[unit] * np.sqrt((dx * dx + dy * dy) + dz * dz)
    return np.where(fl != 0, np.nan, rot_cos), np.where(fl != 0, np.inf, t_err), fl


def angles(rot_cos):
    """what the host does with the read-back: degrees; NaN below -1 as in the reference"""
    with np.errstate(invalid="ignore"):
        return np.rad2deg(np.arccos(np.asarray(rot_cos, dtype=np.float64)))


def transform(pose, verts):
    """[3, 4] pose, float32 [V, 3] vertices -> float64 [V, 3]"""
    x = np.asarray(verts, dtype=np.float32).astype(np.float64)
    R, t = pose[:, :3], pose[:, 3]
    return np.stack([((R[k, 0] * x[:, 0] + R[k, 1] * x[:, 1]) + R[k, 2] * x[:, 2]) + t[k] for k in range(3)], axis=1)


def block_mean(terms):
    """The one summation order of every mean: blocks of 256, the stride-128 .. 1 tree, the partials in ascending order, / V"""
    terms = np.asarray(terms, dtype=np.float64)
    V = len(terms)
    nblk = (V + BLOCK - 1) // BLOCK
    s = np.zeros((nblk, BLOCK))
    s.reshape(-1)[:V] = terms
    stride = BLOCK // 2
    while stride >= 1:
        s[:, :stride] = s[:, :stride] + s[:, stride:2 * stride]
        stride //= 2
    total = 0.0
    for b in range(nblk):
        total = total + s[b, 0]
    return total / float(V)


def _per_frame(fn, pose_pred, pose_gt, fl):
    P, G = _poses(pose_pred), _poses(pose_gt)
    fl = np.zeros(len(P), np.int32) if fl is None else fl
    with np.errstate(all="ignore"):
        return np.array([np.inf if fl[f] else fn(f, P[f], G[f]) for f in range(len(P))], dtype=np.float64)


def add(verts, pose_pred, pose_gt, fl=None):
    def one(f, p, g):
        d = transform(p, verts) - transform(g, verts)
        return block_mean(np.sqrt((d[:, 0] * d[:, 0] + d[:, 1] * d[:, 1]) + d[:, 2] * d[:, 2]))
    return _per_frame(one, pose_pred, pose_gt, fl)


def adds(verts, pose_pred, pose_gt, fl=None):
    """exact: per target vertex (ground-truth pose) the minimum squared distance over all predicted vertices, then its square root"""
    def one(f, p, g):
        a, b = transform(p, verts), transform(g, verts)
        m = np.full(len(b), np.inf)
        for lo in range(0, len(b), 512):                    # targets in slabs: [512, V] at a time
            t = b[lo:lo + 512]
            dx, dy, dz = (a[None, :, k] - t[:, None, k] for k in range(3))
            d2 = (dx * dx + dy * dy) + dz * dz
            m[lo:lo + 512] = np.fmin.reduce(d2, axis=1, initial=np.inf)       # if (d2 < m) m = d2: a NaN is never taken
        return block_mean(np.sqrt(m))
    return _per_frame(one, pose_pred, pose_gt, fl)


def project(K, pose, verts):
    X = transform(pose, verts)
    u = [(K[k, 0] * X[:, 0] + K[k, 1] * X[:, 1]) + K[k, 2] * X[:, 2] for k in range(3)]
    return np.stack([u[0] / u[2], u[1] / u[2]], axis=1)


def proj2d(verts, pose_pred, pose_gt, K, fl=None):
    K = np.asarray(K, dtype=np.float64)

    def one(f, p, g):
        k = K if K.ndim == 2 else K[f]
        d = project(k, p, verts) - project(k, g, verts)
        return block_mean(np.sqrt(d[:, 0] * d[:, 0] + d[:, 1] * d[:, 1]))
    return _per_frame(one, pose_pred, pose_gt, fl)


EPS = 2.0 ** -52


def coordinate_scale(verts, *pose_tables):
    """``S = max_k(sum_j |R[k][j] x_j| + |t_k|)`` over a case: the size a transformed coordinate's rounding is relative to"""
    x = np.abs(np.asarray(verts).astype(np.float64))
    return max(float((np.abs(p[:, :3]) @ x.T + np.abs(p[:, 3:4])).max()) for table in pose_tables for p in table)


def pixel_scale(verts, K, *pose_tables):
    """the same in pixels: ``max_k(sum_j |K[k][j] X'_j|) / |u_2|``"""
    worst = 0.0
    for table in pose_tables:
        for p in table:
            X = transform(p, verts)
            worst = max(worst, float((np.abs(K) @ np.abs(X).T / np.abs(K[2] @ X.T)).max()))
    return worst


def mean_bound(S, V, ref):
    """what two evaluation orders of the same exact mean may differ by: a few roundings of size ``S`` per coordinate, ``V`` roundings of
    the sum relative to itself"""
    return EPS * (32 * S + V * np.abs(ref))


def rotation(axis, angle_deg):
    """Rodrigues' formula: a test helper, not part of the specification"""
    a = np.asarray(axis, dtype=np.float64)
    a = a / np.linalg.norm(a)
    th = np.deg2rad(angle_deg)
    Kx = np.array([[0, -a[2], a[1]], [a[2], 0, -a[0]], [-a[1], a[0], 0]])
    return np.eye(3) + np.sin(th) * Kx + (1 - np.cos(th)) * (Kx @ Kx)


def scene(seed, F, V, max_angle=4.0, max_shift=0.01, extent=0.08, depth=0.6):
    """Seeded ground-truth poses in front of a camera, predictions a small rotation and shift away, a float32 model and one K"""
    g = np.random.default_rng(seed)
    verts = g.uniform(-extent, extent, size=(V, 3)).astype(np.float32)
    gt, pred = np.zeros((F, 3, 4)), np.zeros((F, 3, 4))
    for f in range(F):
        R = rotation(g.normal(size=3), g.uniform(0, 180))
        t = np.array([g.uniform(-0.05, 0.05), g.uniform(-0.05, 0.05), depth + g.uniform(-0.1, 0.1)])
        dR = rotation(g.normal(size=3), g.uniform(0.2, max_angle))
        gt[f, :, :3], gt[f, :, 3] = R, t
        pred[f, :, :3], pred[f, :, 3] = dR @ R, t + g.uniform(-max_shift, max_shift, size=3)
    K = np.array([[572.4, 0.0, 325.3], [0.0, 573.6, 242.0], [0.0, 0.0, 1.0]])
    return {"verts": verts, "pose_gt": gt, "pose_pred": pred, "K": K}
