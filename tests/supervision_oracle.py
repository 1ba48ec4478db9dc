"""The specification of the supervised signals (include/ext/onepose_supervision.h) restated in numpy, one function per
entry: float32 steps with numpy float32 scalars and arrays, float64 sums one element after another in the device's order (lane ``k`` of 256
takes the elements ``k, k + 256, ...`` ascending from 0.0, then the tree ``s[k] + s[k + stride]``, stride 128 .. 1).  Every function also
returns ``min_margin``: the smallest distance of any decision it took from that decision's threshold, so a test can tell an input whose
result could flip under another rounding from one that cannot.

``faults``: a set of names of seeded faults (tests/test_supervision_cpu.py plants each and checks that an output changes):
``depth_test``, ``half_away``, ``last_wins``, ``j_gt_M``, ``coarse_scale_8``, ``no_clamp``, ``per_frame_means``, ``w_not_normalised``.
``reverse``: every sum in the reversed order (lanes descending, the tree's operands swapped stride for stride): the spread of the result
under a change of order, which a tolerance against another math library's log is built from."""
import numpy as np

BLOCK = 256
NO_GT_XY = np.float32(-50.0)
OK, NONE, FORCED, EMPTY = 0, 1, 2, 3
LO, HI = 1e-6, 1 - 1e-6
f32 = np.float32


# ---- the fixed-order sum ------------------------------------------------------------------------------------------------------------------
def block_sum(terms, reverse=False):
    """``terms [..., n]`` float64 -> ``[...]``: the sum of the last axis in the order of OPSUP_BLOCK (``reverse``: in the opposite order)"""
    terms = np.asarray(terms, dtype=np.float64)
    n = terms.shape[-1]
    if reverse:
        terms = terms[..., ::-1]
    chunks = -(-max(n, 1) // BLOCK)
    padded = np.zeros(terms.shape[:-1] + (chunks * BLOCK,), dtype=np.float64)
    padded[..., :n] = terms
    padded = padded.reshape(terms.shape[:-1] + (chunks, BLOCK))
    acc = np.zeros(terms.shape[:-1] + (BLOCK,), dtype=np.float64)
    for c in range(chunks):                                  # a lane's elements one after another; + 0.0 changes no non-negative sum
        acc = acc + padded[..., c, :]
    s = BLOCK // 2
    while s > 0:
        acc = acc[..., :s] + acc[..., s:2 * s]
        s //= 2
    return acc[..., 0]


# ---- 1. the ground truth ------------------------------------------------------------------------------------------------------------------
def project(X, pose, K):
    """float32 in the written order: ``X [n, 3]`` -> ``p [n, 2]``, and the depth ``q_2``"""
    X, P, K = np.asarray(X, f32), np.asarray(pose, f32), np.asarray(K, f32)
    c = [((P[k, 0] * X[:, 0] + P[k, 1] * X[:, 1]) + P[k, 2] * X[:, 2]) + P[k, 3] for k in range(3)]
    q = [(K[k, 0] * c[0] + K[k, 1] * c[1]) + K[k, 2] * c[2] for k in range(3)]
    d = q[2] + f32(1e-6)
    with np.errstate(all="ignore"):
        return np.stack([q[0] / d, q[1] / d], axis=1).astype(f32), q[2]


def ground_truth(keypoints3d, point_ids, counts, pose_gt, K, image_hw, stride=8, faults=()):
    """``keypoints3d [B or 1, N, 3]``, ``point_ids [B, A]``, ``counts [B]`` or ``None``, ``pose_gt [B, 4, 4]``, ``K [3, 3]`` or ``[B, 3, 3]``
    -> dict ``gt_j [B, N]`` int64, ``gt_xy [B, N, 2]`` float32, ``gt_i [B, M]`` int64, ``n_gt [B]`` int32, ``min_margin`` (pixels: the distance of any
    projection from a half-way point of the rounding, which is also where an image bound can flip)"""
    kp = np.asarray(keypoints3d, f32)
    point_ids = np.asarray(point_ids, np.int64)
    B, A = point_ids.shape
    N, (H, W) = kp.shape[1], image_hw
    s = f32(stride)
    w_c = W // stride
    M = (H // stride) * w_c
    gt_j = np.full((B, N), -1, np.int64)
    gt_xy = np.full((B, N, 2), NO_GT_XY, f32)
    gt_i = np.full((B, M), -1, np.int64)
    n_gt = np.zeros(B, np.int32)
    margin = np.inf
    K = np.asarray(K)
    for b in range(B):
        n = A if counts is None else int(min(max(int(counts[b]), 0), A))
        rows = np.arange(n)
        ids = point_ids[b, :n]
        ok = (ids >= 0) & (ids < N)
        rows, ids = rows[ok], ids[ok]
        p, depth = project(kp[b if kp.shape[0] > 1 else 0][ids], np.asarray(pose_gt)[b], K if K.ndim == 2 else K[b])
        with np.errstate(all="ignore"):
            u = p / s
            if "half_away" in faults:
                rounded = np.where(u >= 0, np.floor(u + f32(0.5)), np.ceil(u - f32(0.5))).astype(f32)
            else:
                rounded = np.rint(u)
            pr = rounded * s
            inside = (pr[:, 0] >= 0) & (pr[:, 0] <= f32(W - 1)) & (pr[:, 1] >= 0) & (pr[:, 1] <= f32(H - 1))
            if "depth_test" in faults:
                inside &= depth > 0
            fin = np.isfinite(u).all(axis=1)
            if fin.any():
                frac = np.abs(u[fin].astype(np.float64) - np.floor(u[fin].astype(np.float64)) - 0.5)
                margin = min(margin, float(frac.min()) * stride)         # the four image bounds are tested on pr, a whole multiple of
                #                                                          the stride: they flip where the rounding flips, nowhere else
            j = np.where(inside, (pr[:, 1] / s) * f32(w_c) + pr[:, 0] / s, f32(-1)).astype(np.int64)
        keep = inside & ((j <= M) if "j_gt_M" in faults else (j < M))
        rows, ids, p, j = rows[keep], ids[keep], p[keep], j[keep]
        order = range(len(rows))
        taken = {}
        for k in (reversed(order) if "last_wins" in faults else order):          # annotation order: the first row of a cell stays
            if int(j[k]) not in taken:
                taken[int(j[k])] = k
        for cell, k in taken.items():
            if cell >= M:                                    # only with the j_gt_M fault: where the reference would fault
                n_gt[b] += 1
                continue
            gt_j[b, ids[k]] = cell
            gt_xy[b, ids[k]] = p[k]
            gt_i[b, cell] = ids[k]
            n_gt[b] += 1
    return {"gt_j": gt_j, "gt_xy": gt_xy, "gt_i": gt_i, "n_gt": n_gt, "min_margin": margin}


def to_dense(gt_j, gt_xy, M):
    """The reference's ``conf_matrix_gt [B, N, M]`` int16 and ``fine_location_matrix_gt [B, N, M, 2]`` float32 of the sparse form"""
    B, N = gt_j.shape
    conf = np.zeros((B, N, M), np.int16)
    loc = np.full((B, N, M, 2), NO_GT_XY, f32)
    b, i = np.nonzero(gt_j >= 0)
    conf[b, i, gt_j[b, i]] = 1
    loc[b, i, gt_j[b, i]] = gt_xy[b, i]
    return conf, loc


def _rotation(axis, angle):
    axis = np.asarray(axis, np.float64) / np.linalg.norm(axis)
    Kx = np.array([[0, -axis[2], axis[1]], [axis[2], 0, -axis[0]], [-axis[1], axis[0], 0]])
    return np.eye(3) + np.sin(angle) * Kx + (1 - np.cos(angle)) * (Kx @ Kx)


def _lift(pose, K, uv, z):
    """The 3D point that projects to pixel ``uv`` at depth ``z`` (float64; the float32 projection lands within ~1e-4 px of ``uv``)"""
    ray = np.linalg.inv(K) @ np.array([uv[0], uv[1], 1.0]) * z
    return pose[:3, :3].T @ (ray - pose[:3, 3])


def scene(seed, B=2, N=64, A=48, image_hw=(280, 296), stride=8, shared=False, out_of_range=True, exact_frame=False):
    """A seeded labelled batch with the planted rows of DESIGN.md section 6s in every frame: rows 0, 1 two points into one cell (row 0
    wins); rows 2, 3 the same point twice; rows 4 .. 7 a point out of each image side, row 8 a point inside the image that rounds out
    of it, row 9 one outside that rounds into it; row 10 a point BEHIND the camera that lands inside; rows 11, 12 ids out of range
    (``out_of_range``); the rest random, every one at least 0.01 px from a half-way point in EVERY frame (so ``shared`` -- one object for
    all frames -- keeps the margin).  ``exact_frame``: the last frame has the identity pose, focal length 64 and whole-number points at
    z = 64, where ``z + 1e-6f == z``: every projection is exact, rows 13 .. 16 lie exactly on halves (two round down, two up: to even).
    -> dict ``keypoints3d [B or 1, N, 3]`` float32, ``point_ids [B, A]`` int64, ``counts [B]`` int32, ``pose_gt [B, 4, 4]``, ``K [B, 3, 3]``
    float64, ``image_hw``"""
    rng = np.random.default_rng(seed)
    H, W = image_hw
    poses, Ks = np.zeros((B, 4, 4)), np.zeros((B, 3, 3))
    for b in range(B):
        poses[b] = np.eye(4)
        poses[b, :3, :3] = _rotation(rng.standard_normal(3), rng.uniform(0.05, 0.5))
        poses[b, :3, 3] = [rng.uniform(-0.05, 0.05), rng.uniform(-0.05, 0.05), rng.uniform(0.9, 1.3)]
        Ks[b] = [[rng.uniform(280, 340), 0, W / 2 + rng.uniform(-5, 5)], [0, rng.uniform(280, 340), H / 2 + rng.uniform(-5, 5)], [0, 0, 1]]
    if exact_frame:
        poses[-1] = np.eye(4)
        Ks[-1] = [[64, 0, W // 2], [0, 64, H // 2], [0, 0, 1]]
    frames = 1 if shared else B
    kp = np.zeros((frames, N, 3), f32)
    for f in range(frames):
        got = 0
        while got < N:                                      # random points, kept when far from a half-way point under every pose
            cand = rng.uniform(-0.45, 0.45, (4 * N, 3)).astype(f32)
            far = np.ones(len(cand), bool)
            for b in (range(B) if shared else [f]):
                if exact_frame and b == B - 1:
                    continue
                u = project(cand, poses[b], Ks[b])[0].astype(np.float64) / stride
                far &= (np.abs(u - np.floor(u) - 0.5) * stride >= 0.01).all(axis=1)
            take = cand[far][:N - got]
            kp[f, got:got + len(take)] = take
            got += len(take)
    targets = [(41.3, 46.3), (37.9, 48.9), (100.7, 61.2), None, (-6.2, 100.3), (W + 4.6, 100.3), (100.3, -6.2), (100.3, H + 4.6),
               (W - 1.9, 130.2), (-3.1, 50.3), (150.3, 90.7)]
    ids = np.zeros((B, A), np.int64)
    for b in range(B):
        ids[b] = rng.permutation(N)[:A] if A <= N else rng.integers(0, N, A)
        if shared:
            continue                                        # a shared object cannot be planted for every pose at once
        free = [i for i in range(N) if i not in set(ids[b, 13:].tolist())]
        for r, uv in enumerate(targets):
            ids[b, r] = free[r]
            if uv is None:
                ids[b, r] = ids[b, r - 1]
            elif not (exact_frame and b == B - 1):
                kp[b, free[r]] = _lift(poses[b], Ks[b], uv, -1.5 if r == 10 else rng.uniform(0.8, 1.4)).astype(f32)
        ids[b, 11:13] = (-1, N + 5) if out_of_range else (free[11], free[12])
    if exact_frame:
        b = B - 1
        cx, cy = W // 2, H // 2
        pix = np.stack([rng.integers(0, W, N), rng.integers(0, H, N)], axis=1)
        pix[ids[b, 13:17]] = [(4 + 8 * 5, 64), (4 + 8 * 6, 72), (120, 12 + 8 * 3), (128, 12 + 8 * 4)]         # .5 after 5, 6 | 4, 5
        kp[b] = np.concatenate([pix - [cx, cy], np.full((N, 1), 64)], axis=1).astype(f32)
    counts = np.full(B, A, np.int32)
    return {"keypoints3d": kp, "point_ids": ids, "counts": counts, "pose_gt": poses, "K": Ks, "image_hw": (H, W)}


# ---- 2. the fine targets ------------------------------------------------------------------------------------------------------------------
def fine_targets(b_ids, i_ids, j_ids, count, gt_j, gt_xy, w_c, resolution=(8, 2), radius=2, scale=None, faults=()):
    """-> ``expec_f_gt [n, 2]`` float32 of the first ``n = clamp(count)`` matches (``count=None``: all)"""
    b_ids, i_ids, j_ids = (np.asarray(a, np.int64) for a in (b_ids, i_ids, j_ids))
    cap = len(b_ids)
    n = cap if count is None else int(min(max(int(count), 0), cap))
    B, N = gt_j.shape
    coarse_res, fine_res = int(resolution[0]), int(resolution[1])
    out = np.zeros((n, 2), f32)
    for k in range(n):
        b, i, j = int(b_ids[k]), int(i_ids[k]), int(j_ids[k])
        b_ok = 0 <= b < B
        loc = gt_xy[b, i] if b_ok and 0 <= i < N and gt_j[b, i] == j else np.array([NO_GT_XY, NO_GT_XY], f32)
        cell = (j % w_c, j // w_c)                          # Python's floor division, as torch's
        for a in range(2):
            if scale is None:
                res = coarse_res if "coarse_scale_8" in faults else fine_res        # the reference's `else fine_scale`
                fs, g = f32(fine_res), f32(cell[a] * res)
            else:
                sc = f32(scale[b][1 - a]) if b_ok else f32(1.0)
                cs, fs = f32(coarse_res) * sc, f32(fine_res) * sc
                g = f32(cell[a]) * cs
            out[k, a] = ((f32(loc[a]) - g) / fs) / f32(radius)
    return out


# ---- 3. the focal loss --------------------------------------------------------------------------------------------------------------------
def focal_terms(conf, gt_j, alpha, gamma, faults=()):
    """-> ``(neg [B, N, M]`` float64 with 0.0 at the positives, ``pos [B, N]`` float64 with 0.0 where a row has none, ``is_pos [B, N]``,
    ``min_margin``: the distance of any element from the two clamps)"""
    x = np.asarray(conf, np.float32).astype(np.float64)
    B, N, M = x.shape
    with np.errstate(all="ignore"):
        c = x if "no_clamp" in faults else np.where(x < LO, LO, np.where(x > HI, HI, x))
        power = (lambda v: v * v) if gamma == 2.0 else (lambda v: np.power(v, gamma))
        neg = ((-(1.0 - alpha)) * power(c)) * np.log(1.0 - c)
        is_pos = (gt_j >= 0) & (gt_j < M)
        b, i = np.nonzero(is_pos)
        cp = c[b, i, gt_j[b, i]]
        pos = np.zeros((B, N), np.float64)
        pos[b, i] = ((-alpha) * power(1.0 - cp)) * np.log(cp)
    neg[b, i, gt_j[b, i]] = 0.0
    fin = np.isfinite(x)
    margin = float(min(np.abs(x[fin] - LO).min(), np.abs(x[fin] - HI).min())) if fin.any() else np.inf
    return neg, pos, is_pos, margin


def coarse_loss(conf, gt_j, alpha=0.25, gamma=2.0, pos_weight=1.0, neg_weight=1.0, faults=(), reverse=False):
    """-> dict ``pos_sum``, ``neg_sum``, ``loss_c`` (float64), ``n_pos``, ``n_neg``, ``min_margin``"""
    neg, pos, is_pos, margin = focal_terms(conf, gt_j, alpha, gamma, faults)
    B, N, M = neg.shape
    rows = np.stack([pos.reshape(-1), block_sum(neg, reverse).reshape(-1)], axis=0)        # the rows' pairs, over b * N + i
    with np.errstate(all="ignore"):
        if "per_frame_means" in faults:
            per = rows.reshape(2, B, N)
            n_p = is_pos.sum(axis=1)
            frames = [_focal_mean(block_sum(per[0, b], reverse), block_sum(per[1, b], reverse), int(n_p[b]), N * M - int(n_p[b]),
                                  pos_weight, neg_weight) for b in range(B)]
            loss = float(np.mean(frames))
            pos_sum, neg_sum = block_sum(rows, reverse)
        else:
            pos_sum, neg_sum = block_sum(rows, reverse)
            loss = None
        n_pos = int(is_pos.sum())
        n_neg = B * N * M - n_pos
        if loss is None:
            loss = _focal_mean(pos_sum, neg_sum, n_pos, n_neg, pos_weight, neg_weight)
    return {"pos_sum": float(pos_sum), "neg_sum": float(neg_sum), "loss_c": float(loss), "n_pos": n_pos, "n_neg": n_neg, "min_margin": margin}


def _focal_mean(pos_sum, neg_sum, n_pos, n_neg, pos_weight, neg_weight):
    if n_pos == 0:
        return neg_weight * (neg_sum / np.float64(n_neg))
    if n_neg == 0:
        return pos_weight * (pos_sum / np.float64(n_pos))
    return pos_weight * (pos_sum / np.float64(n_pos)) + neg_weight * (neg_sum / np.float64(n_neg))


# ---- 4. the fine loss ---------------------------------------------------------------------------------------------------------------------
def fine_loss(expec_f, expec_f_gt, count=None, correct_thr=1.0, training=False, faults=(), reverse=False):
    """-> dict ``loss_f`` (float64; NaN with NONE / EMPTY), ``n_correct``, ``status``, ``min_margin`` (of ``correct_thr``)"""
    e, g = np.asarray(expec_f, f32).astype(np.float64), np.asarray(expec_f_gt, f32).astype(np.float64)
    cap = len(e)
    n = cap if count is None else int(min(max(int(count), 0), cap))
    e, g = e[:n], g[:n]
    with np.errstate(all="ignore"):
        inv = 1.0 / np.where(e[:, 2] < 1e-10, 1e-10, e[:, 2])
        mean_inv = block_sum(inv, reverse) / np.float64(n)
        w = inv if "w_not_normalised" in faults else inv / mean_inv
        norm = np.maximum(np.abs(g[:, 0]), np.abs(g[:, 1]))
        correct = norm < correct_thr                        # False for NaN
        dx, dy = g[:, 0] - e[:, 0], g[:, 1] - e[:, 1]
        sq = dx * dx + dy * dy
        terms = np.where(correct, sq * w, 0.0)
        fin = np.isfinite(norm)
        margin = float(np.abs(norm[fin] - correct_thr).min()) if fin.any() else np.inf
        n_correct = int(correct.sum())
        if n_correct > 0:
            return {"loss_f": float(block_sum(terms, reverse) / np.float64(n_correct)), "n_correct": n_correct, "status": OK, "min_margin": margin}
    if not training:
        return {"loss_f": float("nan"), "n_correct": 0, "status": NONE, "min_margin": margin}
    if n > 0:
        return {"loss_f": float(sq[0] * 1e-6), "n_correct": 1, "status": FORCED, "min_margin": margin}
    return {"loss_f": float("nan"), "n_correct": 0, "status": EMPTY, "min_margin": margin}


def total_loss(loss_c, fine, coarse_weight=1.0, fine_weight=1.0):
    """``Loss.forward``'s scalars from :func:`coarse_loss`'s ``loss_c`` and :func:`fine_loss`'s dict (``None``: no ``expec_f``)"""
    loss = loss_c * coarse_weight
    out = {"loss_c": loss_c}
    if fine is not None:
        if fine["status"] == NONE:
            out["loss_f"] = 1.0
        else:
            loss = loss + fine["loss_f"] * fine_weight
            out["loss_f"] = fine["loss_f"]
    out["loss"] = loss
    return out
