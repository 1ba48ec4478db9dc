"""numpy restatement of include/onepose_temporal.h, one function per entry: the float32 pyramid, the float64
pyramidal Lucas-Kanade tracker with the device's summation order, collect and inject.  Plain loops over points, vectors over the window;
every expression in the header's order, so the device equals this bit for bit.  Also the analytic test scene of the temporal tests."""
import numpy as np

DEGENERATE, OUT_OF_IMAGE, FB_FAIL, BAD_INPUT, FLAG_MAX_ITERS, LOST = 1, 2, 4, 8, 16, 15
DEFAULTS = dict(window=21, max_iters=30, eps=0.01, min_eig=1.0, fb_threshold=1.0)
_LANES = np.arange(64)


# ---- 1. pyramid -------------------------------------------------------------------------------------------------------------------------
def level_shapes(H, W, levels):
    shapes = [(H, W)]
    for _ in range(levels - 1):
        h, w = shapes[-1]
        shapes.append(((h + 1) // 2, (w + 1) // 2))
    return shapes


def pyramid_bytes(H, W, levels):
    if not (1 <= levels <= 6 and 2 <= H <= 16384 and 2 <= W <= 16384) or min(level_shapes(H, W, levels)[-1]) < 2:
        return 0
    return sum((h * w + 63) // 64 * 256 for h, w in level_shapes(H, W, levels))


def _tap5(a, axis):
    n = a.shape[axis]
    idx = lambda k: np.clip(np.arange(n) + k, 0, n - 1)
    t = lambda k: np.take(a, idx(k), axis=axis)
    f4, f6, f16 = np.float32(4), np.float32(6), np.float32(0.0625)
    return (((t(-2) + t(2)) + f4 * (t(-1) + t(1))) + f6 * t(0)) * f16


def pyramid(frame_u8, levels):
    out = [np.asarray(frame_u8).astype(np.float32)]
    for _ in range(levels - 1):
        out.append(np.ascontiguousarray(_tap5(_tap5(out[-1], 0), 1)[::2, ::2]))
    assert all(a.dtype == np.float32 for a in out)
    return out


# ---- 2. sampling ------------------------------------------------------------------------------------------------------------------------
def _clamp_index(v, hi):
    v = np.asarray(v, np.float64)
    with np.errstate(invalid="ignore"):
        safe = np.where(v >= 0.0, np.minimum(v, float(hi)), 0.0)      # NaN -> 0
    return safe.astype(np.int64)


def sample(I, x, y):
    h, w = I.shape
    x, y = np.asarray(x, np.float64), np.asarray(y, np.float64)
    x0, y0 = np.floor(x), np.floor(y)
    fx, fy = x - x0, y - y0
    xa, xb, ya, yb = _clamp_index(x0, w - 1), _clamp_index(x0 + 1.0, w - 1), _clamp_index(y0, h - 1), _clamp_index(y0 + 1.0, h - 1)
    a, b, c, d = (I[ya, xa].astype(np.float64), I[ya, xb].astype(np.float64), I[yb, xa].astype(np.float64), I[yb, xb].astype(np.float64))
    top, bot = a + fx * (b - a), c + fx * (d - c)
    return top + fy * (bot - top)


# ---- 4. sums ----------------------------------------------------------------------------------------------------------------------------
def wave_sum(v):
    """element k on lane k % 64, ascending k per lane from 0.0, then the xor butterfly (offsets 32 .. 1)"""
    n = len(v)
    pad = np.zeros((n + 63) // 64 * 64)
    pad[:n] = v
    part = np.zeros(64)
    for row in pad.reshape(-1, 64):
        part = part + row          # a padding 0.0 changes no partial: a partial that started at +0.0 is never -0.0
    for off in (32, 16, 8, 4, 2, 1):
        part = part + part[_LANES ^ off]
    assert (part == part[0]).all() or np.isnan(part).all()
    return part[0]


# ---- 3. one point -----------------------------------------------------------------------------------------------------------------------
def _inside(x, y, W, H):
    return bool(x >= 0.0 and x <= W - 1 and y >= 0.0 and y <= H - 1)


def track_point(S, D, p, g, window, max_iters, eps, min_eig):
    """-> (q or (nan, nan), flags, iterations); S, D: pyramids (lists of float32 arrays)"""
    H, W = S[0].shape
    L = len(S)
    nan2 = (np.nan, np.nan)
    px, py, gx0, gy0 = float(p[0]), float(p[1]), float(g[0]), float(g[1])
    if not all(np.isfinite(v) for v in (px, py, gx0, gy0)) or not _inside(px, py, W, H):
        return nan2, BAD_INPUT, 0
    half = window // 2
    k = np.arange(window * window)
    ox, oy = (k % window - half).astype(np.float64), (k // window - half).astype(np.float64)
    top = float(1 << (L - 1))
    dx, dy = (gx0 - px) / top, (gy0 - py) / top
    flags, iters, eps2 = 0, 0, eps * eps
    for l in range(L - 1, -1, -1):
        s = float(1 << l)
        plx, ply = px / s, py / s
        x, y = plx + ox, ply + oy
        T = sample(S[l], x, y)
        Gx = 0.5 * (sample(S[l], x + 1.0, y) - sample(S[l], x - 1.0, y))
        Gy = 0.5 * (sample(S[l], x, y + 1.0) - sample(S[l], x, y - 1.0))
        Gxx, Gxy, Gyy = wave_sum(Gx * Gx), wave_sum(Gx * Gy), wave_sum(Gy * Gy)
        det = Gxx * Gyy - Gxy * Gxy
        m = ((Gxx + Gyy) - np.sqrt((Gxx - Gyy) * (Gxx - Gyy) + 4.0 * (Gxy * Gxy))) / (2.0 * float(window * window))
        if not det > 0.0 or not m >= min_eig:
            return nan2, flags | DEGENERATE, iters
        converged = False
        for _ in range(max_iters):
            cx, cy = plx + dx, ply + dy
            e = T - sample(D[l], cx + ox, cy + oy)
            bx, by = wave_sum(e * Gx), wave_sum(e * Gy)
            ddx, ddy = (Gyy * bx - Gxy * by) / det, (Gxx * by - Gxy * bx) / det
            dx, dy = dx + ddx, dy + ddy
            iters += 1
            if ddx * ddx + ddy * ddy < eps2:
                converged = True
                break
        if l == 0 and not converged:
            flags |= FLAG_MAX_ITERS
        if not _inside(px + s * dx, py + s * dy, W, H):
            return nan2, flags | OUT_OF_IMAGE, iters
        if l > 0:
            dx, dy = 2.0 * dx, 2.0 * dy
    return (px + dx, py + dy), flags, iters


# ---- 6. guess ---------------------------------------------------------------------------------------------------------------------------
def guess_of(p, row_guess, X, pose, K, scale, W, H):
    g = p if row_guess is None else row_guess
    if X is None:
        return g
    X = [scale * float(v) for v in X]
    with np.errstate(all="ignore"):
        cam = [((pose[i, 0] * X[0] + pose[i, 1] * X[1]) + pose[i, 2] * X[2]) + scale * pose[i, 3] for i in range(3)]
        u = [(K[i, 0] * cam[0] + K[i, 1] * cam[1]) + K[i, 2] * cam[2] for i in range(3)]
        ux, uy = np.float64(u[0]) / np.float64(u[2]), np.float64(u[1]) / np.float64(u[2])
    if cam[2] > 1e-12 and np.isfinite(ux) and np.isfinite(uy) and _inside(ux, uy, W, H):
        return (ux, uy)
    return g


# ---- 3 + 5 + 6: optmp_track -------------------------------------------------------------------------------------------------------------
def track(S, D, pts, count=None, guess=None, pts_3d=None, pose=None, K=None, scale=1.0, window=21, max_iters=30, eps=0.01, min_eig=1.0,
          fb_threshold=1.0, fill=None):
    """-> dict(pts [cap, 2], flags, iterations, fb_error); rows at or past the count keep ``fill`` = (pts, flags, iterations, fb_error)
    values (default NaN / 0)"""
    pts = np.asarray(pts, np.float64)
    cap = len(pts)
    n = cap if count is None else max(0, min(int(count), cap))
    H, W = S[0].shape
    fill = fill or (np.nan, 0, 0, np.nan)
    out = dict(pts=np.full((cap, 2), fill[0]), flags=np.full(cap, fill[1], np.int32), iterations=np.full(cap, fill[2], np.int32),
               fb_error=np.full(cap, fill[3]))
    for r in range(n):
        p = pts[r]
        g = guess_of(p, None if guess is None else guess[r], None if pts_3d is None else pts_3d[r], pose, K, float(scale), W, H)
        q, flags, iters = track_point(S, D, p, g, window, max_iters, eps, min_eig)
        fbe = np.nan
        if not flags & LOST and fb_threshold is not None and fb_threshold >= 0:
            back, bflags, _ = track_point(D, S, q, (q[0] - (g[0] - p[0]), q[1] - (g[1] - p[1])), window, max_iters, eps, min_eig)
            if bflags & LOST:
                flags |= FB_FAIL
            else:
                ex, ey = back[0] - p[0], back[1] - p[1]
                fbe = np.sqrt(ex * ex + ey * ey)
                if not fbe <= fb_threshold:
                    flags |= FB_FAIL
        out["pts"][r], out["flags"][r], out["iterations"][r], out["fb_error"][r] = q, flags, iters, fbe
    return out


# ---- 7. collect -------------------------------------------------------------------------------------------------------------------------
def inverse3(m):
    m = np.asarray(m, np.float64)
    c0 = m[1, 1] * m[2, 2] - m[1, 2] * m[2, 1]
    c1 = m[1, 2] * m[2, 0] - m[1, 0] * m[2, 2]
    c2 = m[1, 0] * m[2, 1] - m[1, 1] * m[2, 0]
    det = (m[0, 0] * c0 + m[0, 1] * c1) + m[0, 2] * c2
    return np.array([[c0 / det, (m[0, 2] * m[2, 1] - m[0, 1] * m[2, 2]) / det, (m[0, 1] * m[1, 2] - m[0, 2] * m[1, 1]) / det],
                     [c1 / det, (m[0, 0] * m[2, 2] - m[0, 2] * m[2, 0]) / det, (m[0, 2] * m[1, 0] - m[0, 0] * m[1, 2]) / det],
                     [c2 / det, (m[0, 1] * m[2, 0] - m[0, 0] * m[2, 1]) / det, (m[0, 0] * m[1, 1] - m[0, 1] * m[1, 0]) / det]])


def _homography(m, xy):
    xy = np.asarray(xy, np.float64).reshape(-1, 2)
    x, y = xy[:, 0], xy[:, 1]
    h = [(m[i, 0] * x + m[i, 1] * y) + m[i, 2] for i in range(3)]
    return np.stack([h[0] / h[2], h[1] / h[2]], axis=1)


def map_to_original(trans, pts_crop):
    return _homography(inverse3(trans), pts_crop)


def map_to_crop(trans, pts_orig):
    return _homography(np.asarray(trans, np.float64), pts_orig)


def collect(pts_2d, pts_3d, trans, count=None, mask=None):
    """-> (pts_orig [k, 2] float64, pts_3d [k, 3] float32, k)"""
    pts_2d, pts_3d = np.asarray(pts_2d, np.float32), np.asarray(pts_3d, np.float32)
    cap = len(pts_2d)
    n = cap if count is None else max(0, min(int(count), cap))
    rows = np.arange(n) if mask is None else np.nonzero(np.asarray(mask)[:n])[0]
    return map_to_original(trans, pts_2d[rows]), pts_3d[rows].copy(), len(rows)


# ---- 8. inject --------------------------------------------------------------------------------------------------------------------------
def inject(own_2d, own_3d, own_count, sources, trans, cap_total=None):
    """sources: [(pts_3d [cap_s, 3], tracked pts [cap_s, 2] float64, flags [cap_s], count or None), ...] oldest first
    -> (pts_2d [k, 2] float32, pts_3d [k, 3] float32, k)"""
    own_2d, own_3d = np.asarray(own_2d, np.float32), np.asarray(own_3d, np.float32)
    n = len(own_2d) if own_count is None else max(0, min(int(own_count), len(own_2d)))
    out2, out3 = [own_2d[:n]], [own_3d[:n]]
    for p3, q, flags, count in sources:
        m = len(q) if count is None else max(0, min(int(count), len(q)))
        rows = np.nonzero((np.asarray(flags)[:m] & LOST) == 0)[0]
        out2.append(map_to_crop(trans, np.asarray(q, np.float64)[rows]).astype(np.float32))
        out3.append(np.asarray(p3, np.float32)[rows])
    out2, out3 = np.concatenate(out2), np.concatenate(out3)
    if cap_total is not None:
        out2, out3 = out2[:cap_total], out3[:cap_total]
    return out2, out3, len(out2)


# ---- the analytic scene of the tests ----------------------------------------------------------------------------------------------------
class Texture:
    """tex(x, y): a seeded sum of 40 sinusoids with wavelengths 6-40 px, scaled into [0, 255] before quantisation"""

    def __init__(self, seed=0, terms=40):
        rng = np.random.default_rng(seed)
        lam, ang = rng.uniform(6.0, 40.0, terms), rng.uniform(0.0, 2 * np.pi, terms)
        self.kx, self.ky = 2 * np.pi / lam * np.cos(ang), 2 * np.pi / lam * np.sin(ang)
        self.ph, self.amp = rng.uniform(0.0, 2 * np.pi, terms), rng.uniform(0.5, 1.0, terms)
        self.norm = 3.0 * np.sqrt(np.sum(self.amp ** 2) / 2)

    def __call__(self, x, y):
        x, y = np.asarray(x, np.float64), np.asarray(y, np.float64)
        v = sum(a * np.sin(kx * x + ky * y + ph) for a, kx, ky, ph in zip(self.amp, self.kx, self.ky, self.ph))
        return np.clip(np.rint(127.5 + 127.5 * v / self.norm), 0, 255).astype(np.uint8)

    def image(self, H, W, inverse_map=None):
        """the image whose pixel (x, y) shows tex(inverse_map(x, y)): a point at u in the texture appears at map(u)"""
        yy, xx = np.mgrid[0:H, 0:W].astype(np.float64)
        if inverse_map is not None:
            xx, yy = inverse_map(xx, yy)
        return self(xx, yy)


def similarity(angle_deg=0.0, scale=1.0, shift=(0.0, 0.0), centre=(0.0, 0.0)):
    """-> (forward(x, y), inverse(x, y)) of u -> centre + scale R (u - centre) + shift"""
    c, s = np.cos(np.deg2rad(angle_deg)) * scale, np.sin(np.deg2rad(angle_deg)) * scale
    A = np.array([[c, -s], [s, c]])
    Ai = np.linalg.inv(A)
    cx, cy = centre

    def fwd(x, y):
        x, y = np.asarray(x, np.float64) - cx, np.asarray(y, np.float64) - cy
        return cx + A[0, 0] * x + A[0, 1] * y + shift[0], cy + A[1, 0] * x + A[1, 1] * y + shift[1]

    def inv(x, y):
        x, y = np.asarray(x, np.float64) - cx - shift[0], np.asarray(y, np.float64) - cy - shift[1]
        return cx + Ai[0, 0] * x + Ai[0, 1] * y, cy + Ai[1, 0] * x + Ai[1, 1] * y

    return fwd, inv


SHIFT = (6.3, -4.6)


def scene(kind="shift", H=120, W=160, seed=0, n_points=60, margin=25.0):
    """-> (source u8, target u8, points [n, 2], truth [n, 2]); kind: 'shift' or 'similarity' (3 deg, 3 %, the same shift)"""
    tex = Texture(seed)
    fwd, inv = similarity(0.0, 1.0, SHIFT) if kind == "shift" else similarity(3.0, 1.03, SHIFT, centre=(W / 2, H / 2))
    rng = np.random.default_rng(seed + 1000)
    pts = np.stack([rng.uniform(margin, W - 1 - margin, n_points), rng.uniform(margin, H - 1 - margin, n_points)], axis=1)
    return tex.image(H, W), tex.image(H, W, inv), pts, np.stack(fwd(pts[:, 0], pts[:, 1]), axis=1)


def planted_scene(kind="shift", H=120, W=160, seed=0):
    """The scene with one planted case per flag -> (source, target, points [64, 2]): the 60 scene points, then
    60: the centre of a constant 40 x 40 patch of the source (DEGENERATE: at level 1 at the latest a window of up to 15 and its gradient
        samples, +-16 px, plus the blur's +-2 px lie inside the patch, so every gradient is exactly 0);
    61: a point 3 px from the right border, which the shift carries off the image (OUT_OF_IMAGE);
    62: NaN (BAD_INPUT);
    63: a point whose true location is the centre of a 33 x 33 patch of the target replaced by an unrelated texture (FB_FAIL)."""
    src, dst, pts, _ = scene(kind, H, W, seed)
    src, dst = src.copy(), dst.copy()
    src[30:70, 30:70] = 128
    fwd, _ = similarity(0.0, 1.0, SHIFT) if kind == "shift" else similarity(3.0, 1.03, SHIFT, centre=(W / 2, H / 2))
    p_fb = np.array([110.0, 70.0])
    cx, cy = (int(round(float(v))) for v in fwd(p_fb[0], p_fb[1]))
    other = Texture(seed + 77).image(H, W)
    dst[cy - 16:cy + 17, cx - 16:cx + 17] = other[cy - 16:cy + 17, cx - 16:cx + 17]
    extra = np.array([[50.0, 50.0], [W - 4.0, 60.0], [np.nan, 5.0], p_fb])
    return src, dst, np.concatenate([pts, extra])


# ---- the plane sequence of the chain tests ---------------------------------------------------------------------------------------------
PLANE_K = np.array([[400.0, 0.0, 64.0], [0.0, 400.0, 48.0], [0.0, 0.0, 1.0]])
PLANE_PX_PER_M = 800.0           # texture pixels per metre of the plane z = 0: one texture pixel is about one image pixel at 0.5 m


def plane_poses(n=6):
    """[R | t] of a camera about 0.5 m in front of the plane, moving a few pixels per frame"""
    poses = []
    for t in range(n):
        a, b = 0.012 * t, -0.008 * t
        Rz = np.array([[np.cos(a), -np.sin(a), 0], [np.sin(a), np.cos(a), 0], [0, 0, 1]])
        Rx = np.array([[1, 0, 0], [0, np.cos(b), -np.sin(b)], [0, np.sin(b), np.cos(b)]])
        poses.append(np.concatenate([Rx @ Rz, [[0.003 * t], [-0.002 * t], [0.5 + 0.004 * t]]], axis=1))
    return poses


def plane_frame(pose, H=96, W=128, seed=5, K=PLANE_K):
    """the textured plane z = 0 seen under ``pose``: every pixel through the inverse of the homography K [r1 r2 t]"""
    Hi = np.linalg.inv(K @ pose[:, [0, 1, 3]])

    def inverse_map(x, y):
        w = Hi[2, 0] * x + Hi[2, 1] * y + Hi[2, 2]
        return ((Hi[0, 0] * x + Hi[0, 1] * y + Hi[0, 2]) / w * PLANE_PX_PER_M + 300.0,
                (Hi[1, 0] * x + Hi[1, 1] * y + Hi[1, 2]) / w * PLANE_PX_PER_M + 300.0)

    return Texture(seed).image(H, W, inverse_map)


def project(K, pose, X):
    cam = pose[:, :3] @ np.asarray(X, np.float64).T + pose[:, 3:4]
    uv = K @ cam
    return (uv[:2] / uv[2:]).T
