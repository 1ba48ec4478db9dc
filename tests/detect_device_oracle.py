"""The device detection's specification (include/onepose_detect.h, DESIGN.md section 6n, ``onepose_st_amd/detect_device.py``) restated
in numpy float64, one function per stage.  Elementwise numpy arithmetic only where rows or trials are independent (each element is the
scalar expression in the written order); every sum of the fit is a Python loop in the header's order.  The package does not import
this file.

Also here: the scenes the CPU and GPU tests share (``planted_scene``: V views of planted matches with outliers; the rule cases).
"""
import math
import os
import sys

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import pnp_device_oracle as pnp_orc  # noqa: E402
import track_device_oracle as trk_orc  # noqa: E402

M64 = pnp_orc.M64
STATUS_NO_MODEL, STATUS_DEGENERATE, STATUS_NEEDS_MORE = 1, 2, 4
THREADS = 256
IDENTITY = np.array([1.0, 0, 0, 0, 1.0, 0])
# corners of the two estimators' affinities on the planted scenes: the bar (derived in DESIGN.md section 6n: float64 normal equations at
# these coordinates err by about 1e-16 x a condition near 1e7 x 1e3 px = 1e-6 px; the box has a grain of 1 px)
CORNER_BAR = 1e-3


def ranges(b_ids, count, cap, V):
    return pnp_orc.ranges(np.asarray(b_ids), cap if count is None else count, cap, V)


def trial_floor(min_matches):
    return max(int(min_matches), 3)


# ---- sample ----------------------------------------------------------------------------------------------------------------------------------
def sample(rng, trials, seed, min_matches=6):
    V = rng.shape[0]
    out = np.full((V, trials, 3), -1, dtype=np.int32)
    for v in range(V):
        n = int(rng[v, 1] - rng[v, 0])
        if n < trial_floor(min_matches):
            continue
        for t in range(trials):
            out[v, t] = pnp_orc.draw3(seed & M64, v, t, n)          # the one sampler: the view in place of the frame
    return out


# ---- hypothesis, score -----------------------------------------------------------------------------------------------------------------------
def affine_from3(s, d):
    """``affine_from3`` of the host estimator on arrays of samples: s, d [T, 3, 2] float64 -> (A [T, 6], ok [T])"""
    x0, y0, x1, y1, x2, y2 = s[:, 0, 0], s[:, 0, 1], s[:, 1, 0], s[:, 1, 1], s[:, 2, 0], s[:, 2, 1]
    det = (x1 - x0) * (y2 - y0) - (x2 - x0) * (y1 - y0)
    scale = np.abs(x1 - x0) + np.abs(y1 - y0) + np.abs(x2 - x0) + np.abs(y2 - y0)
    ok = (np.abs(det) > 1e-9 * scale * scale) & (scale > 0.0)
    A = np.zeros((s.shape[0], 6))
    safe = np.where(ok, det, 1.0)
    for r in range(2):
        u0, u1, u2 = d[:, 0, r], d[:, 1, r], d[:, 2, r]
        a = ((u1 - u0) * (y2 - y0) - (u2 - u0) * (y1 - y0)) / safe
        b = ((x1 - x0) * (u2 - u0) - (x2 - x0) * (u1 - u0)) / safe
        A[:, 3 * r], A[:, 3 * r + 1], A[:, 3 * r + 2] = a, b, u0 - a * x0 - b * y0
    return A, ok


def inliers_of(A, s, d, thr):
    """A [T, 6]; s, d [n, 2] float64 -> bool [T, n]: ``affine_inliers``' expression"""
    x, y, u, w = s[None, :, 0], s[None, :, 1], d[None, :, 0], d[None, :, 1]
    ex = A[:, 0:1] * x + A[:, 1:2] * y + A[:, 2:3] - u
    ey = A[:, 3:4] * x + A[:, 4:5] * y + A[:, 5:6] - w
    return ex * ex + ey * ey < thr * thr


def score(mk0, mk1, rng, samples, thr=6.0):
    """-> cnt [V, trials] int32"""
    V, trials = samples.shape[:2]
    s64, d64 = np.asarray(mk0, np.float32).astype(np.float64), np.asarray(mk1, np.float32).astype(np.float64)
    cnt = np.zeros((V, trials), dtype=np.int32)
    for v in range(V):
        b, e = int(rng[v, 0]), int(rng[v, 1])
        if samples[v, 0, 0] < 0:
            continue
        idx = samples[v].astype(np.int64) + b
        A, ok = affine_from3(s64[idx], d64[idx])
        cnt[v] = np.where(ok, inliers_of(A, s64[b:e], d64[b:e], thr).sum(axis=1), 0)
    return cnt


# ---- select ----------------------------------------------------------------------------------------------------------------------------------
def needs_more(won, n, confidence, trials):
    w = float(won) / float(n)
    pw = w * w * w
    if pw > 1.0 - 1e-12:
        return trials < 1
    if pw > 1e-12:
        return math.ceil(math.log(1.0 - confidence) / math.log(1.0 - pw)) > trials
    return True


def select(mk0, mk1, rng, count, samples, cnt, min_matches=6, thr=6.0, confidence=0.99):
    """-> best [V], n_inliers [V], status [V] int32, mask [cap] uint8"""
    V, trials = cnt.shape
    cap = len(mk0)
    s64, d64 = np.asarray(mk0, np.float32).astype(np.float64), np.asarray(mk1, np.float32).astype(np.float64)
    best, n_in, status = np.full(V, -1, np.int32), np.zeros(V, np.int32), np.zeros(V, np.int32)
    mask = np.zeros(cap, dtype=np.uint8)
    for v in range(V):
        b, e = int(rng[v, 0]), int(rng[v, 1])
        n = e - b
        ran = n >= trial_floor(min_matches)
        won = 0
        if ran and cnt[v].max() > 0:
            best[v] = int(np.argmax(cnt[v]))                          # the first among equals
            won = int(cnt[v, best[v]])
        st = STATUS_NO_MODEL if (n < min_matches or won < 3) else 0
        if ran and needs_more(won, n, confidence, trials):
            st |= STATUS_NEEDS_MORE
        n_in[v], status[v] = won, st
        if best[v] >= 0:
            idx = samples[v, best[v]].astype(np.int64)[None] + b
            A, ok = affine_from3(s64[idx], d64[idx])
            if ok[0]:
                mask[b:e] = inliers_of(A, s64[b:e], d64[b:e], thr)[0]
    return best, n_in, status, mask


# ---- fit, box --------------------------------------------------------------------------------------------------------------------------------
def fit(s, d, m):
    """The normal equations on the masked rows of one view (s, d [n, 2] float64, m [n]) with every sum in the header's order: thread l of
    256 takes rows l, l + 256, ...; the partials are added in thread order.  -> affine [6] or None (singular)"""
    sums = [0.0] * 12
    part = [[0.0] * 12 for _ in range(THREADS)]
    for l in range(min(THREADS, len(s))):
        acc = part[l]
        for i in range(l, len(s), THREADS):
            if not m[i]:
                continue
            x, y, u, w = float(s[i, 0]), float(s[i, 1]), float(d[i, 0]), float(d[i, 1])
            for e, val in enumerate((x * x, x * y, x, y * y, y, 1.0, x * u, y * u, u, x * w, y * w, w)):
                acc[e] += val
    for l in range(THREADS):
        for e in range(12):
            sums[e] += part[l][e]
    S = [sums[0], sums[1], sums[2], sums[1], sums[3], sums[4], sums[2], sums[4], sums[5]]
    det = S[0] * (S[4] * S[8] - S[5] * S[7]) - S[1] * (S[3] * S[8] - S[5] * S[6]) + S[2] * (S[3] * S[7] - S[4] * S[6])
    if abs(det) < 1e-12:
        return None
    Si = pnp_orc.inv3(S)
    bu, bv = sums[6:9], sums[9:12]
    return np.array([Si[a * 3] * bu[0] + Si[a * 3 + 1] * bu[1] + Si[a * 3 + 2] * bu[2] for a in range(3)] +
                    [Si[a * 3] * bv[0] + Si[a * 3 + 1] * bv[1] + Si[a * 3 + 2] * bv[2] for a in range(3)])


def corners_through(A, hw):
    """-> [(x', y')] of (0, 0), (W, 0), (0, H), (W, H) in float64"""
    H, W = float(hw[0]), float(hw[1])
    A = [float(a) for a in A]
    return [(A[0] * X + A[1] * Y + A[2], A[3] * X + A[4] * Y + A[5]) for X, Y in ((0.0, 0.0), (W, 0.0), (0.0, H), (W, H))]


def centre_box(query_hw):
    H, W = int(query_hw[0]), int(query_hw[1])
    return np.array([W // 2 - 500, H // 2 - 500, W // 2 + 500, H // 2 + 500], dtype=np.int32)


def box_of(A, hw):
    """-> int32 [x0, y0, x1, y1], or None when a corner is not finite or truncates outside int32"""
    c = corners_through(A, hw)
    if not all(trk_orc.fits_int32(v) for p in c for v in p):
        return None
    xs, ys = [int(p[0]) for p in c], [int(p[1]) for p in c]              # int(): truncation toward zero
    return np.array([min(xs), min(ys), max(xs), max(ys)], dtype=np.int32)


def fit_box(mk0, mk1, rng, view_hw, query_hw, n_in, status, mask):
    """-> affine [V, 6], boxes [V, 4], and the updated copies of n_inliers, status, mask"""
    V = rng.shape[0]
    s64, d64 = np.asarray(mk0, np.float32).astype(np.float64), np.asarray(mk1, np.float32).astype(np.float64)
    n_in, status, mask = n_in.copy(), status.copy(), mask.copy()
    affine, boxes = np.zeros((V, 6)), np.zeros((V, 4), dtype=np.int32)
    for v in range(V):
        b, e = int(rng[v, 0]), int(rng[v, 1])
        A = box = None
        if not (status[v] & STATUS_NO_MODEL) and n_in[v] >= 3:
            A = fit(s64[b:e], d64[b:e], mask[b:e])
            box = box_of(A, view_hw[v]) if A is not None else None
        if box is None:
            A, box = IDENTITY, centre_box(query_hw)
            n_in[v], mask[b:e] = 0, 0
            status[v] |= STATUS_NO_MODEL
        affine[v], boxes[v] = A, box
    return affine, boxes, n_in, status, mask


# ---- vote ------------------------------------------------------------------------------------------------------------------------------------
def vote(boxes, n_in, status, query_hw, K, S):
    """-> winner, (box, flag, K_crop, trans), status"""
    status = status.copy()
    winner = int(np.argmax(n_in))                                         # the first among equals
    box = boxes[winner]
    if box[2] <= box[0] or box[3] <= box[1]:
        box = centre_box(query_hw)
        status[winner] |= STATUS_DEGENERATE
    return winner, trk_orc.box_set(box, K, S), status


def detect(mk0, mk1, b_ids, view_hw, query_hw, K, S=512, count=None, trials=2048, seed=1, min_matches=6, thr=6.0, confidence=0.99):
    """every stage -> dict of the outputs of ``detect_device.vote``"""
    cap, V = len(mk0), len(view_hw)
    rng = ranges(b_ids, count, cap, V)
    smp = sample(rng, trials, seed, min_matches)
    cnt = score(mk0, mk1, rng, smp, thr)
    best, n_in, status, mask = select(mk0, mk1, rng, count, smp, cnt, min_matches, thr, confidence)
    sel = dict(best=best, n_inliers=n_in.copy(), mask=mask.copy())
    affine, boxes, n_in, status, mask = fit_box(mk0, mk1, rng, view_hw, query_hw, n_in, status, mask)
    winner, state, status = vote(boxes, n_in, status, query_hw, K, S)
    return dict(ranges=rng, samples=smp, cnt=cnt, select=sel, affine=affine, boxes=boxes, n_inliers=n_in, status=status, mask=mask, winner=winner,
                state=state)


# ---- scenes ----------------------------------------------------------------------------------------------------------------------------------
QUERY_HW = (480, 640)
SCENE_K = np.array([[600.0, 0, 320.0], [0, 600.0, 240.0], [0, 0, 1]])


def planted_view(g, n, hw=QUERY_HW, noise=0.5, outliers=0.3):
    """n matches of one view: src uniform in the view, dst = A src + noise (each coordinate within +-noise / sqrt(2), so at most `noise`
    px off the model), a share of outliers at least 20 px off the model.  -> (mk0, mk1 float32 [n, 2], A_true [6])"""
    H, W = hw
    a, s = g.uniform(-0.5, 0.5), g.uniform(0.6, 1.2)
    A = np.array([s * math.cos(a), -s * math.sin(a), g.uniform(20, 120), s * math.sin(a), s * math.cos(a), g.uniform(20, 120)])
    src = np.stack([g.uniform(0, W, n), g.uniform(0, H, n)], axis=1)
    dst = np.stack([A[0] * src[:, 0] + A[1] * src[:, 1] + A[2], A[3] * src[:, 0] + A[4] * src[:, 1] + A[5]], axis=1)
    dst += g.uniform(-noise / math.sqrt(2), noise / math.sqrt(2), size=(n, 2))
    bad = g.permutation(n)[:int(round(outliers * n))]
    ang, mag = g.uniform(0, 2 * math.pi, len(bad)), g.uniform(22.0, 200.0, len(bad))
    dst[bad] += np.stack([mag * np.cos(ang), mag * np.sin(ang)], axis=1)
    return src.astype(np.float32), dst.astype(np.float32), A


def planted_scene(rows, seed, hw=QUERY_HW, noise=0.5):
    """one view per entry of ``rows`` -> dict(mk0, mk1 [cap, 2] float32, b_ids [cap] int64, view_hw [V, 2] int32, truth [V, 6])"""
    g = np.random.default_rng(seed)
    views = [planted_view(g, n, hw, noise) for n in rows]
    return dict(mk0=np.concatenate([v[0] for v in views]), mk1=np.concatenate([v[1] for v in views]),
                b_ids=np.concatenate([np.full(n, k, dtype=np.int64) for k, n in enumerate(rows)]),
                view_hw=np.array([hw] * len(rows), dtype=np.int32), truth=np.stack([v[2] for v in views]), rows=list(rows))


def residuals(A, mk0, mk1):
    s, d = np.asarray(mk0, np.float64), np.asarray(mk1, np.float64)
    return np.hypot(A[0] * s[:, 0] + A[1] * s[:, 1] + A[2] - d[:, 0], A[3] * s[:, 0] + A[4] * s[:, 1] + A[5] - d[:, 1])


def assert_scene_condition(scene, affine):
    """no row's residual under its view's fitted model lies in [5, 7] px: no estimator's inlier set depends on a rounding"""
    for v in range(len(scene["rows"])):
        sel = scene["b_ids"] == v
        r = residuals(affine[v], scene["mk0"][sel], scene["mk1"][sel])
        assert not ((r >= 5.0) & (r <= 7.0)).any(), (v, np.sort(r[(r >= 5.0) & (r <= 7.0)]))


# the planted scenes of the comparison against the host estimator: 3 views each, 40 to 300 rows
HOST_SCENES = [((40, 150, 300), 11), ((64, 257, 90), 12), ((300, 41, 200), 13)]
# V = 15, 40 to 300 rows per view
BIG_ROWS = (40, 300, 64, 65, 255, 256, 257, 100, 41, 180, 299, 77, 128, 210, 50)


# ---- the rule cases --------------------------------------------------------------------------------------------------------------------------
NEGATIVE_CORNER_A = np.array([0.5, 0.0, 10.7, 0.0, 0.5, -3.2])          # the affinity of tests/test_loftr_cpu.py's box [10, -3, 330, 236]


def exact_view(g, n, A, lo=(0.0, 0.0), hi=(QUERY_HW[1], QUERY_HW[0])):
    """n noise-free matches of the affinity A with src uniform in [lo, hi)"""
    src = np.stack([g.uniform(lo[0], hi[0], n), g.uniform(lo[1], hi[1], n)], axis=1)
    dst = np.stack([A[0] * src[:, 0] + A[1] * src[:, 1] + A[2], A[3] * src[:, 0] + A[4] * src[:, 1] + A[5]], axis=1)
    return src.astype(np.float32), dst.astype(np.float32), np.asarray(A, np.float64)


def rule_scene(name, hw=QUERY_HW):
    """The scenes of the rules (-> ``planted_scene``'s dict):
    ``too_small``: view 1 has 5 rows; ``collinear``: view 1's 30 reference points lie on one line; ``tie``: views 0 and 1 hold the same 80
    noise-free rows, view 2 fewer; ``negative_corner``: one view under NEGATIVE_CORNER_A; ``overflow``: view 0's affinity sends the view's
    corners beyond int32 (its points lie in the unit square, so that float32 holds their images to half a pixel); ``degenerate``: one view
    whose affinity shrinks the view into one pixel column and row."""
    g = np.random.default_rng(5)
    if name == "too_small":
        views = [planted_view(g, 60, hw), exact_view(g, 5, NEGATIVE_CORNER_A), planted_view(g, 50, hw)]
    elif name == "collinear":
        t = g.uniform(0, 200, 30)
        line = np.stack([t, 2.0 * t + 5.0], axis=1).astype(np.float32)
        views = [planted_view(g, 60, hw), (line, line + np.float32(10.0), IDENTITY), planted_view(g, 50, hw)]
    elif name == "tie":
        twin = exact_view(g, 80, [0.9, -0.1, 30.0, 0.1, 0.9, 12.0])
        views = [twin, twin, exact_view(g, 40, [1.0, 0.0, 5.0, 0.0, 1.0, 7.0])]
    elif name == "negative_corner":
        views = [exact_view(g, 50, NEGATIVE_CORNER_A)]
    elif name == "overflow":
        views = [exact_view(g, 40, [5e6, 0.0, 3.0, 0.0, 5e6, 4.0], hi=(1.0, 1.0)), planted_view(g, 40, hw)]
    elif name == "degenerate":
        views = [exact_view(g, 40, [0.001, 0.0, 100.2, 0.0, 0.001, 50.3])]
    else:
        raise KeyError(name)
    rows = [len(v[0]) for v in views]
    return dict(mk0=np.concatenate([v[0] for v in views]), mk1=np.concatenate([v[1] for v in views]),
                b_ids=np.concatenate([np.full(n, k, dtype=np.int64) for k, n in enumerate(rows)]),
                view_hw=np.array([hw] * len(rows), dtype=np.int32), truth=np.stack([v[2] for v in views]), rows=rows)


RULES = ("too_small", "collinear", "tie", "negative_corner", "overflow", "degenerate")


def check_rule(name, out, hw=QUERY_HW):
    """what the rule demands of the outputs of ``detect`` (or of the device's, in the same dict form) on ``rule_scene(name)``"""
    centre = centre_box(hw).tolist()
    boxes, n_in, status, winner = np.asarray(out["boxes"]), np.asarray(out["n_inliers"]), np.asarray(out["status"]), int(out["winner"])
    state_box = np.asarray(out["state"][0]).tolist()
    if name in ("too_small", "collinear"):
        assert boxes[1].tolist() == centre and n_in[1] == 0 and status[1] & STATUS_NO_MODEL
        assert winner == 0 and n_in[0] > n_in[2] >= 30 and state_box == boxes[0].tolist() and not (status[0] | status[2]) & STATUS_NO_MODEL
    elif name == "tie":
        assert n_in.tolist() == [80, 80, 40] and winner == 0 and boxes[0].tolist() == boxes[1].tolist() == state_box
    elif name == "negative_corner":
        assert boxes[0].tolist() == [10, -3, 330, 236] == state_box and n_in[0] == 50 and status[0] == 0
    elif name == "overflow":
        assert boxes[0].tolist() == centre and n_in[0] == 0 and status[0] & STATUS_NO_MODEL and winner == 1 and state_box == boxes[1].tolist()
    elif name == "degenerate":
        assert boxes[0].tolist() == [100, 50, 100, 50] and n_in[0] == 40 and winner == 0
        assert status[0] == STATUS_DEGENERATE and state_box == centre
    assert int(out["state"][1]) == 0                                        # the flag: the loop never re-detects on a detection
