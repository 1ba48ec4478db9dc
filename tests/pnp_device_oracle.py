"""The device PnP's specification (``onepose_st_amd/pnp_device.py``) restated in numpy float64, one function per
stage.  Row sums are sequential in row order (``np.cumsum``, never ``np.sum``).  The package does not import this file.

Also here: the frames the CPU and GPU tests share (``planted_frame``, ``hard_frame``: the matches an ideal matcher returns for the
synthetic c1 frames) and the seeded P3P samples.
"""
import math

import numpy as np

G = 0x9E3779B97F4A7C15
M64 = (1 << 64) - 1
MIN_INLIERS = 4
MAX_NEEDED = 1000000
STATUS_NO_POSE, STATUS_NEEDS_MORE = 1, 4
# the largest relative pose difference between p3p_one and the host library's p3p_poses over p3p_samples(), measured on the CPU
# (tests/test_pnp_device_cpu.py); the GPU test bounds the kernel's distance to p3p_one by ten times this
E_P3P = 2.62e-8
# object seed of the two c1 frames of the end-to-end tests: the three host runs agree on the inlier set and no match lies at the threshold
FRAME_SEED = 1
IDENTITY = np.array([[1.0, 0, 0, 0], [0, 1.0, 0, 0], [0, 0, 1.0, 0]])


# ---- stage 1 ---------------------------------------------------------------------------------------------------------------------------------
def ranges(b_ids, count, cap, F):
    n = min(max(int(count), 0), cap)
    if b_ids is None:
        return np.array([[0, n]], dtype=np.int32)
    b = np.asarray(b_ids[:n], dtype=np.int64)
    out = np.zeros((F, 2), dtype=np.int32)
    for f in range(F):
        lo, hi = int(np.searchsorted(b, f, side="left")), int(np.searchsorted(b, f + 1, side="left"))
        out[f] = (lo, max(hi, lo))
    return out


def inv3(m):
    m = [float(v) for v in np.asarray(m, dtype=np.float64).reshape(9)]
    d = m[0] * (m[4] * m[8] - m[5] * m[7]) - m[1] * (m[3] * m[8] - m[5] * m[6]) + m[2] * (m[3] * m[7] - m[4] * m[6])
    i = 1.0 / d
    return [(m[4] * m[8] - m[5] * m[7]) * i, (m[2] * m[7] - m[1] * m[8]) * i, (m[1] * m[5] - m[2] * m[4]) * i,
            (m[5] * m[6] - m[3] * m[8]) * i, (m[0] * m[8] - m[2] * m[6]) * i, (m[2] * m[3] - m[0] * m[5]) * i,
            (m[3] * m[7] - m[4] * m[6]) * i, (m[1] * m[6] - m[0] * m[7]) * i, (m[0] * m[4] - m[1] * m[3]) * i]


def prep(K, pts2d, pts3d, count, b_ids, F, scale=1.0):
    """-> rows [cap, 8]: X (3), pixel (2), ray (2), pad; rows at or beyond the count stay 0, rows of no frame are 0"""
    cap = pts2d.shape[0]
    n = min(max(int(count), 0), cap)
    K = np.asarray(K, dtype=np.float64).reshape(-1, 9)
    rows = np.zeros((cap, 8))
    for i in range(n):
        f = 0 if b_ids is None else int(b_ids[i])
        if f < 0 or f >= F:
            continue
        k = inv3(K[0] if K.shape[0] == 1 else K[f])
        u, v = float(pts2d[i, 0]), float(pts2d[i, 1])
        w = k[6] * u + k[7] * v + k[8]
        rows[i, :3] = [float(scale) * float(pts3d[i, d]) for d in range(3)]
        rows[i, 3:5] = (u, v)
        rows[i, 5] = (k[0] * u + k[1] * v + k[2]) / w
        rows[i, 6] = (k[3] * u + k[4] * v + k[5]) / w
    return rows


# ---- stage 2 ---------------------------------------------------------------------------------------------------------------------------------
def mix(z):
    z &= M64
    z ^= z >> 30; z = (z * 0xBF58476D1CE4E5B9) & M64
    z ^= z >> 27; z = (z * 0x94D049BB133111EB) & M64
    z ^= z >> 31
    return z


def draw3(seed, g, t, n):
    """three distinct group-local rows of trial t of group g (a frame here, a view in the detection), n >= 3"""
    base = (((g << 32) | t) * 4) & M64
    picks = []
    for k in range(3):
        r = mix((seed + G * ((base + k + 1) & M64)) & M64) % (n - k)
        for p in sorted(picks):
            if r >= p:
                r += 1
        picks.append(r)
    return tuple(picks)


def sample_one(seed, f, t, n):
    """:func:`draw3` of trial t of frame f, or (-1, -1, -1) when n < 4"""
    return draw3(seed, f, t, n) if n >= MIN_INLIERS else (-1, -1, -1)


def sample(rng, trials, seed):
    F = rng.shape[0]
    out = np.zeros((F, trials, 3), dtype=np.int32)
    for f in range(F):
        n = int(rng[f, 1] - rng[f, 0])
        for t in range(trials):
            out[f, t] = sample_one(seed, f, t, n)
    return out


# ---- stage 3: p3p_poses of the host solver, scalar float64 -----------------------------------------------------------------------------------
def _cbrt(x):
    return float(np.cbrt(x))                                          # the C library's cbrt, like the host solver's std::cbrt


def cubic_largest_root(A, B, C):
    a3 = A / 3.0
    P, Q = B - A * a3, 2.0 * a3 * a3 * a3 - a3 * B + C
    disc = 0.25 * Q * Q + P * P * P / 27.0
    if disc > 0.0:
        sq = math.sqrt(disc)
        w = _cbrt(-0.5 * Q + sq) + _cbrt(-0.5 * Q - sq)
    else:
        m = 2.0 * math.sqrt(-P / 3.0)
        arg = 3.0 * Q / (P * m) if m > 0.0 else 0.0
        arg = -1.0 if arg < -1.0 else (1.0 if arg > 1.0 else arg)
        w = m * math.cos(math.acos(arg) / 3.0)
    z = w - a3
    for _ in range(3):
        f, df = ((z + A) * z + B) * z + C, (3.0 * z + 2.0 * A) * z + B
        if abs(df) < 1e-300:
            break
        z -= f / df
    return z


def quartic_real_roots(c):
    if not (abs(c[4]) > 1e-14 * (abs(c[3]) + abs(c[2]) + abs(c[1]) + abs(c[0]) + 1e-300)):
        return []
    a, b, cc, d = c[3] / c[4], c[2] / c[4], c[1] / c[4], c[0] / c[4]
    a2 = a * a
    p, q = b - 0.375 * a2, cc - 0.5 * a * b + 0.125 * a2 * a
    r = d - 0.25 * a * cc + 0.0625 * a2 * b - (3.0 / 256.0) * a2 * a2
    y = []
    scale = abs(p) + math.sqrt(abs(r)) + 1e-300
    if abs(q) < 1e-12 * scale * math.sqrt(scale):
        disc = p * p - 4.0 * r
        if disc < 0.0:
            if disc > -1e-12 * scale * scale:
                disc = 0.0
            else:
                return []
        sq = math.sqrt(disc)
        for w in (0.5 * (-p + sq), 0.5 * (-p - sq)):
            if w < 0.0:
                continue
            s = math.sqrt(w)
            y += [s, -s]
    else:
        z = cubic_largest_root(2.0 * p, p * p - 4.0 * r, -q * q)
        if not z > 0.0:
            return []
        s = math.sqrt(z)
        t1, t2 = 0.5 * (p + z - q / s), 0.5 * (p + z + q / s)
        tol = 1e-10 * (z + abs(t1) + abs(t2))
        d1, d2 = z - 4.0 * t1, z - 4.0 * t2
        if d1 > -tol:
            d1 = math.sqrt(d1 if d1 > 0.0 else 0.0)
            y += [0.5 * (-s + d1), 0.5 * (-s - d1)]
        if d2 > -tol:
            d2 = math.sqrt(d2 if d2 > 0.0 else 0.0)
            y += [0.5 * (s + d2), 0.5 * (s - d2)]
    roots = []
    for y0 in y:
        x, live = y0 - 0.25 * a, True
        for _ in range(3):
            f = (((c[4] * x + c[3]) * x + c[2]) * x + c[1]) * x + c[0]
            df = ((4.0 * c[4] * x + 3.0 * c[3]) * x + 2.0 * c[2]) * x + c[1]
            live = live and abs(df) >= 1e-300
            if live:
                x -= f / df
        roots.append(x)
    return roots


def _cross(a, b):
    return [a[1] * b[2] - a[2] * b[1], a[2] * b[0] - a[0] * b[2], a[0] * b[1] - a[1] * b[0]]


def _norm(a):
    return math.sqrt(a[0] * a[0] + a[1] * a[1] + a[2] * a[2])


def p3p_one(ray, X):
    """ray [3][2], X [3][3] -> list of [3, 4] poses in the solver's root order"""
    ray = [[float(v) for v in r] for r in ray]
    X = [[float(v) for v in x] for x in X]
    fb = []
    for rx, ry in ray:
        inv = 1.0 / math.sqrt(rx * rx + ry * ry + 1.0)
        fb.append([rx * inv, ry * inv, inv])

    def dot(a, b):
        return a[0] * b[0] + a[1] * b[1] + a[2] * b[2]

    def d2(a, b):
        return (a[0] - b[0]) * (a[0] - b[0]) + (a[1] - b[1]) * (a[1] - b[1]) + (a[2] - b[2]) * (a[2] - b[2])
    ca, cb, cg = dot(fb[1], fb[2]), dot(fb[0], fb[2]), dot(fb[0], fb[1])
    a2, b2, c2 = d2(X[1], X[2]), d2(X[0], X[2]), d2(X[0], X[1])
    if not (a2 > 0.0 and b2 > 0.0 and c2 > 0.0):
        return []
    e1, w = [X[1][i] - X[0][i] for i in range(3)], [X[2][i] - X[0][i] for i in range(3)]
    n1 = _norm(e1)
    if not n1 > 1e-300:
        return []
    e1 = [v / n1 for v in e1]
    e3 = _cross(e1, w)
    n3, nw = _norm(e3), _norm(w)
    if not (n3 > 1e-9 * nw) or not nw > 0.0:
        return []
    e3 = [v / n3 for v in e3]
    e2 = _cross(e3, e1)
    EP = [[e1[i], e2[i], e3[i]] for i in range(3)]                    # EP[i][k]: component i of axis k
    p, k = (a2 - c2) / b2, c2 / b2
    N, D, E = [p + 1.0, -2.0 * p * cb, p - 1.0], [2.0 * cg, -2.0 * ca], [1.0, -2.0 * cb, 1.0]
    D2 = [D[0] * D[0], 2.0 * D[0] * D[1], D[1] * D[1]]
    c = [D2[0], D2[1], D2[2], 0.0, 0.0]
    for i in range(3):
        for j in range(3):
            c[i + j] += N[i] * N[j] - k * E[i] * D2[j]
    for i in range(3):
        for j in range(2):
            c[i + j] -= 2.0 * cg * N[i] * D[j]
    vs = quartic_real_roots(c)
    poses = []
    for ri, v in enumerate(vs):
        good = v > 0.0 and math.isfinite(v)
        for rj in range(ri):
            good = good and not (abs(vs[rj] - v) < 1e-9 * (1.0 + abs(v)))
        den = D[0] + D[1] * v
        good = good and abs(den) >= 1e-12
        if not good:
            continue
        u = (N[0] + (N[1] + N[2] * v) * v) / den
        if not u > 0.0:
            continue
        q = 1.0 + u * u - (2.0 * cg) * u
        if not q > 1e-300:
            continue
        s1 = math.sqrt(c2 / q)
        sd = [s1, u * s1, v * s1]
        Cc = [[sd[i] * fb[i][d] for d in range(3)] for i in range(3)]
        f1, w = [Cc[1][i] - Cc[0][i] for i in range(3)], [Cc[2][i] - Cc[0][i] for i in range(3)]
        n1 = _norm(f1)
        if not n1 > 1e-300:
            continue
        in1 = 1.0 / n1
        f1 = [t * in1 for t in f1]
        f3 = _cross(f1, w)
        n3, nw = _norm(f3), _norm(w)
        if not (n3 > 1e-9 * nw and nw > 0.0):
            continue
        in3 = 1.0 / n3
        f3 = [t * in3 for t in f3]
        f2 = _cross(f3, f1)
        ps = np.zeros((3, 4))
        for i in range(3):
            for j in range(3):
                ps[i, j] = f1[i] * EP[j][0] + f2[i] * EP[j][1] + f3[i] * EP[j][2]
            ps[i, 3] = Cc[0][i] - (ps[i, 0] * X[0][0] + ps[i, 1] * X[0][1] + ps[i, 2] * X[0][2])
        if not np.abs(ps).sum() < 1e300:
            continue
        poses.append(ps)
    return poses[:4]


def p3p(rows, rng, samples):
    F, trials = samples.shape[:2]
    hyps = np.full((F, 4 * trials, 3, 4), np.nan)
    nsol = np.zeros((F, trials), dtype=np.int32)
    for f in range(F):
        b, n = int(rng[f, 0]), int(rng[f, 1] - rng[f, 0])
        for t in range(trials):
            idx = [int(v) for v in samples[f, t]]
            if n < MIN_INLIERS or any(i < 0 or i >= n for i in idx):
                continue
            poses = p3p_one([rows[b + i, 5:7] for i in idx], [rows[b + i, :3] for i in idx])
            nsol[f, t] = len(poses)
            for k, ps in enumerate(poses):
                hyps[f, 4 * t + k] = ps
    return hyps, nsol


# ---- stage 4 ---------------------------------------------------------------------------------------------------------------------------------
def _intr(K, f):
    K = np.asarray(K, dtype=np.float64).reshape(-1, 9)
    k = K[0] if K.shape[0] == 1 else K[f]
    return k[0], k[1], k[2], k[4], k[5]                               # fx, sk, cx, fy, cy


def residuals(ps, rows, intr):
    """count_inliers' expression for hypotheses ps [H, 3, 4] on rows [n, 8] -> (front [H, n] bool, e2 [H, n])"""
    fx, sk, cx, fy, cy = intr
    ps = ps.reshape(-1, 12)
    x0, x1, x2 = rows[:, 0][None], rows[:, 1][None], rows[:, 2][None]
    with np.errstate(all="ignore"):
        xc = ps[:, 0:1] * x0 + ps[:, 1:2] * x1 + ps[:, 2:3] * x2 + ps[:, 3:4]
        yc = ps[:, 4:5] * x0 + ps[:, 5:6] * x1 + ps[:, 6:7] * x2 + ps[:, 7:8]
        zc = ps[:, 8:9] * x0 + ps[:, 9:10] * x1 + ps[:, 10:11] * x2 + ps[:, 11:12]
        front = zc > 1e-12
        zs = np.where(front, zc, 1.0)
        xn, yn = xc / zs, yc / zs
        du, dv = fx * xn + sk * yn + cx - rows[:, 3][None], fy * yn + cy - rows[:, 4][None]
        e2 = du * du + dv * dv
    return front, e2


def score(rows, rng, K, hyps, reproj):
    """-> cnt [F, H] int32, cost [F, H]; also usable with hand-made hypotheses"""
    F, H = hyps.shape[:2]
    thr2 = float(reproj) * float(reproj)
    cnt, cost = np.zeros((F, H), dtype=np.int32), np.zeros((F, H))
    for f in range(F):
        b, e = int(rng[f, 0]), int(rng[f, 1])
        ps = hyps[f].reshape(H, 12)
        finite = np.isfinite(ps).all(axis=1)
        if e > b:
            front, e2 = residuals(np.where(finite[:, None], ps, 0.0), rows[b:e], _intr(K, f))
            with np.errstate(invalid="ignore"):
                inl = front & (e2 < thr2)
            add = np.where(inl, e2, thr2)
            cnt[f] = inl.sum(axis=1)
            cost[f] = np.cumsum(add, axis=1)[:, -1]                   # sequential in row order
        cnt[f][~finite] = 0
        cost[f][~finite] = np.inf
    return cnt, cost


# ---- stage 5 ---------------------------------------------------------------------------------------------------------------------------------
def needed_for(cnt, n, confidence):
    w = float(cnt) / float(n)
    pw = w * w * w
    if pw > 1.0 - 1e-12:
        return 1.0
    if pw > 1e-12:
        nd = math.ceil(math.log(1.0 - confidence) / math.log(1.0 - pw))
        return float(nd) if nd < MAX_NEEDED else float(MAX_NEEDED)
    return float(MAX_NEEDED)


def select(cnt, cost, rows, rng, K, hyps, reproj, confidence, trials):
    F, H = cnt.shape
    thr2 = float(reproj) * float(reproj)
    best, n_in, status = np.full(F, -1, dtype=np.int32), np.zeros(F, dtype=np.int32), np.zeros(F, dtype=np.int32)
    mask = np.zeros(rows.shape[0], dtype=np.uint8)
    for f in range(F):
        b, e = int(rng[f, 0]), int(rng[f, 1])
        cand = [h for h in range(H) if cnt[f, h] > 0]
        if cand:
            best[f] = min(cand, key=lambda h: (-int(cnt[f, h]), float(cost[f, h]), h))
            n_in[f] = cnt[f, best[f]]
        st = STATUS_NO_POSE if n_in[f] < MIN_INLIERS else 0
        if e - b >= MIN_INLIERS and needed_for(n_in[f], e - b, confidence) > trials:
            st |= STATUS_NEEDS_MORE
        status[f] = st
        if best[f] >= 0 and e > b:
            front, e2 = residuals(hyps[f, best[f]][None], rows[b:e], _intr(K, f))
            with np.errstate(invalid="ignore"):
                mask[b:e] = (front & (e2 < thr2))[0]
    return best, n_in, status, mask


# ---- stage 6 ---------------------------------------------------------------------------------------------------------------------------------
def _seq(v):
    """sequential sum in row order"""
    return float(np.cumsum(v)[-1]) if len(v) else 0.0


def rodrigues(w):
    th = math.sqrt(w[0] * w[0] + w[1] * w[1] + w[2] * w[2])
    a = 1.0 - th * th / 6.0 if th < 1e-12 else math.sin(th) / th
    b = 0.5 - th * th / 24.0 if th < 1e-12 else (1.0 - math.cos(th)) / (th * th)
    Kx = np.array([[0, -w[2], w[1]], [w[2], 0, -w[0]], [-w[1], w[0], 0]], dtype=np.float64)
    return np.eye(3) + a * Kx + b * (Kx @ Kx)


def solve6(H, g):
    M = np.concatenate([H, g[:, None]], axis=1).astype(np.float64)
    for c in range(6):
        piv = c
        for r in range(c + 1, 6):
            if abs(M[r, c]) > abs(M[piv, c]):
                piv = r
        if abs(M[piv, c]) < 1e-300:
            return None
        if piv != c:
            M[[c, piv]] = M[[piv, c]]
        for r in range(c + 1, 6):
            M[r, c:] -= (M[r, c] / M[c, c]) * M[c, c:]
    dx = np.zeros(6)
    for i in range(5, -1, -1):
        s = M[i, 6]
        for j in range(i + 1, 6):
            s -= M[i, j] * dx[j]
        dx[i] = s / M[i, i]
    return dx


def lm_cost(ps, R, intr):
    front, e2 = residuals(ps[None], R, intr)
    return _seq(np.where(front[0], e2[0], 1e12))


def refine_lm(R, pose, intr, iters=20):
    """refine_lm of the host solver on the rows R [m, 8] (the masked ones); returns the refined [3, 4] pose"""
    fx, sk, cx, fy, cy = intr
    pose = pose.copy()
    lam = 1e-3
    cur = lm_cost(pose, R, intr)
    for _ in range(iters):
        p = pose.reshape(12)
        x, y, z = R[:, 0], R[:, 1], R[:, 2]
        pc0 = p[0] * x + p[1] * y + p[2] * z + p[3]
        pc1 = p[4] * x + p[5] * y + p[6] * z + p[7]
        pc2 = p[8] * x + p[9] * y + p[10] * z + p[11]
        fr = pc2 > 1e-12
        x, y, z, pc0, pc1, pc2, pu, pv = (a[fr] for a in (x, y, z, pc0, pc1, pc2, R[:, 3], R[:, 4]))
        iz = 1.0 / pc2
        xn, yn = pc0 * iz, pc1 * iz
        ru, rv = fx * xn + sk * yn + cx - pu, fy * yn + cy - pv
        Ju = [fx * iz, sk * iz, -(fx * xn + sk * yn) * iz]
        Jv = [np.zeros_like(iz), fy * iz, -fy * yn * iz]
        q = [pc0 - p[3], pc1 - p[7], pc2 - p[11]]
        ju = [-Ju[1] * q[2] + Ju[2] * q[1], Ju[0] * q[2] - Ju[2] * q[0], -Ju[0] * q[1] + Ju[1] * q[0], Ju[0], Ju[1], Ju[2]]
        jv = [-Jv[1] * q[2] + Jv[2] * q[1], Jv[0] * q[2] - Jv[2] * q[0], -Jv[0] * q[1] + Jv[1] * q[0], Jv[0], Jv[1], Jv[2]]
        H, g = np.zeros((6, 6)), np.zeros(6)
        for a in range(6):
            g[a] = -_seq(ju[a] * ru + jv[a] * rv)
            for b in range(a, 6):
                H[a, b] = H[b, a] = _seq(ju[a] * ju[b] + jv[a] * jv[b])
        improved = False
        for _tries in range(8):
            Hd = H.copy()
            for a in range(6):
                Hd[a, a] *= 1.0 + lam
            dx = solve6(Hd, g)
            if dx is None:
                lam *= 10.0
                continue
            dR = rodrigues(dx)
            npose = np.zeros((3, 4))
            for r in range(3):
                for c in range(3):
                    npose[r, c] = dR[r, 0] * pose[0, c] + dR[r, 1] * pose[1, c] + dR[r, 2] * pose[2, c]
                npose[r, 3] = pose[r, 3] + dx[3 + r]
            nc = lm_cost(npose, R, intr)
            if nc < cur:
                pose = npose
                rel = (cur - nc) / (cur + 1e-300)
                cur = nc
                lam = lam * 0.3 if lam > 1e-9 else lam
                improved = True
                if rel < 1e-12:
                    return pose
                break
            lam *= 10.0
        if not improved:
            return pose
    return pose


def refine(rows, rng, K, hyps, best, n_in, status, mask, reproj, scale=1.0):
    """the host's finish per frame -> pose [F, 3, 4], n_inliers, status, mask (new arrays)"""
    F = hyps.shape[0]
    thr2 = float(reproj) * float(reproj)
    pose_out = np.tile(IDENTITY, (F, 1, 1))
    n_in, status, mask = n_in.copy(), status.copy(), mask.copy()
    for f in range(F):
        b, e = int(rng[f, 0]), int(rng[f, 1])
        keep = int(status[f]) & STATUS_NEEDS_MORE
        have = best[f] >= 0 and e - b >= MIN_INLIERS and n_in[f] >= MIN_INLIERS
        cnt = 0
        if have:
            intr = _intr(K, f)
            pose = hyps[f, best[f]].copy()
            R = rows[b:e]
            for _round in range(2):
                pose = refine_lm(R[mask[b:e] != 0], pose, intr)
                front, e2 = residuals(pose[None], R, intr)
                with np.errstate(invalid="ignore"):
                    new = (front & (e2 < thr2))[0].astype(np.uint8)
                changed = not np.array_equal(new, mask[b:e])
                mask[b:e] = new
                cnt = int(new.sum())
                if cnt < MIN_INLIERS or not changed:
                    break
            have = cnt >= MIN_INLIERS
        if not have:
            mask[b:e] = 0
            n_in[f], status[f] = 0, keep | STATUS_NO_POSE
            continue
        pose[:, 3] = pose[:, 3] / float(scale)
        pose_out[f] = pose
        n_in[f], status[f] = cnt, keep
    return pose_out, n_in, status, mask


def solve(K, pts2d, pts3d, count=None, b_ids=None, F=1, scale=1.0, reproj=5.0, confidence=0.99, trials=1024, seed=1):
    """all stages -> dict(pose [F, 3, 4], n_inliers, status, mask [cap], ranges)"""
    cap = pts2d.shape[0]
    count = cap if count is None else count
    rng = ranges(b_ids, count, cap, F)
    rows = prep(K, pts2d, pts3d, count, b_ids, F, scale)
    smp = sample(rng, trials, seed)
    hyps, _ = p3p(rows, rng, smp)
    cnt, cost = score(rows, rng, K, hyps, reproj)
    best, n_in, status, mask = select(cnt, cost, rows, rng, K, hyps, reproj, confidence, trials)
    pose, n_in, status, mask = refine(rows, rng, K, hyps, best, n_in, status, mask, reproj, scale)
    return {"pose": pose, "n_inliers": n_in, "status": status, "mask": mask, "ranges": rng}


# ---- shared test data ------------------------------------------------------------------------------------------------------------------------
def frame_matches(inp):
    """The matches an ideal matcher returns for a ``synthetic.make_synthetic_inputs`` frame, in ascending 3D point order like the
    matcher's: the planted pairs at their fine pixel (the projection rounded to even pixels), the wrong pairs at their cell's centre.
    -> (K [3, 3] float64, pts2d [n, 2] float32, pts3d [n, 3] float32, wrong [n] bool)"""
    H, W = inp["image_hw"]
    wc = W // 8
    kp = inp["keypoints3d"][0].numpy()
    K = inp["K"].numpy().astype(np.float64)
    pose = inp["pose_gt"].numpy()
    pi, wi, wj = inp["planted_i"].numpy(), inp["wrong_i"].numpy(), inp["wrong_j"].numpy()
    cam = kp[pi].astype(np.float64) @ pose[:, :3].T + pose[:, 3]
    uv = cam[:, :2] / cam[:, 2:3] * K[0, 0] + K[:2, 2]
    good2d = 2.0 * np.round(uv / 2.0)
    wrong2d = np.stack([8.0 * (wj % wc), 8.0 * (wj // wc)], axis=1)
    idx = np.concatenate([pi, wi])
    p2 = np.concatenate([good2d, wrong2d.reshape(-1, 2)])
    wrong = np.concatenate([np.zeros(len(pi), bool), np.ones(len(wi), bool)])
    order = np.argsort(idx, kind="stable")
    return K, p2[order].astype(np.float32), kp[idx[order]].astype(np.float32), wrong[order]


def c1_frame(hard: bool, seed: int):
    """the planted (``hard=False``) or ``synthetic.HARD_PROFILE`` frame at c1 size with the object seed ``seed``"""
    from onepose_st_amd.config import default_config
    from onepose_st_amd.synthetic import CONFIG_SIZES, HARD_PROFILE, make_synthetic_inputs, make_synthetic_state_dict
    cfg = default_config()
    sd = make_synthetic_state_dict(0, cfg)
    n, hw, plant = CONFIG_SIZES["c1"]
    inp = make_synthetic_inputs(sd, n_points=n, image_hw=hw, n_plant=plant, seed=seed, config=cfg, **(HARD_PROFILE if hard else {}))
    return frame_matches(inp)


def p3p_samples(count=200, seed=7):
    """``count`` seeded well-conditioned P3P samples (rays [3, 2], X [3, 3]) with the host library's poses: a sample whose triangle is
    near-collinear (its smallest height below 5 % of its longest side, in the world or in the image) or whose host roots lie closer
    than 1e-6 (relative pose distance) to each other is drawn again"""
    from onepose_st_amd import pnp
    g = np.random.default_rng(seed)
    out = []
    while len(out) < count:
        X = g.uniform(-0.1, 0.1, size=(3, 3))
        ax = g.normal(size=3)
        ax /= np.linalg.norm(ax)
        R = rodrigues(ax * g.uniform(0, 0.8))
        t = np.array([0.0, 0.0, 0.5]) + 0.02 * g.normal(size=3)
        cam = X @ R.T + t
        ray = cam[:, :2] / cam[:, 2:3]

        def slim(P):
            a, b, c = np.linalg.norm(P[1] - P[0]), np.linalg.norm(P[2] - P[0]), np.linalg.norm(P[2] - P[1])
            s = 0.5 * (a + b + c)
            area = math.sqrt(max(s * (s - a) * (s - b) * (s - c), 0.0))
            return 2.0 * area / max(a, b, c) < 0.05 * max(a, b, c)
        if slim(X) or slim(np.concatenate([ray, np.ones((3, 1))], axis=1)):
            continue
        host = pnp.p3p(ray, X)
        if not host or any(pose_distance(host[i], host[j]) < 1e-6 for i in range(len(host)) for j in range(i)):
            continue
        out.append((ray, X, host))
    return out


def pose_distance(a, b):
    """the relative pose difference: max(|dR|_max, |dt| / |t|)"""
    a, b = np.asarray(a), np.asarray(b)
    return max(float(np.abs(a[:, :3] - b[:, :3]).max()), float(np.linalg.norm(a[:, 3] - b[:, 3]) / np.linalg.norm(b[:, 3])))
