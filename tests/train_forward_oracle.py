"""The specification of the training-mode forward's own step (include/ext/onepose_train_forward.h) restated in
numpy, one function per entry, sampler included.  Integers are exact; the two float32 products of a padded row are numpy float32.  The
draws are Python integers modulo 2^64, so nothing here depends on numpy's overflow rules."""
import numpy as np

OK, NO_GT = 0, 1
MAX_STEP = 2 ** 30
GOLDEN = 0x9E3779B97F4A7C15
MASK = 2 ** 64 - 1
f32 = np.float32


def mix64(z):
    """the splitmix64 finaliser (onepose_pnp_device.h, onepose_detect.h)"""
    z &= MASK
    z = ((z ^ (z >> 30)) * 0xBF58476D1CE4E5B9) & MASK
    z = ((z ^ (z >> 27)) * 0x94D049BB133111EB) & MASK
    return z ^ (z >> 31)


def h(seed, step, c, s):
    """draw ``s`` of kind ``c`` (0: predicted picks, 1: ground-truth picks) of call ``step``"""
    counter = (((step * 2 + c) << 32) | s) & MASK
    return mix64(seed + GOLDEN * (counter + 1))


def picks(seed, step, c, n, size):
    """``size`` picks in ``[0, n)``, with replacement: ``h(c, s) % n`` for ``s`` in ``range(size)``"""
    return np.array([h(seed, step, c, s) % n for s in range(size)], np.int64)


def train_rows(B, N, M, percent):
    """the reference's ``int(num_candidates_max * train_coarse_percent)`` on a Python float"""
    return int(B * min(N, M) * percent)


def gt_list(gt_j, M):
    """``gt_j [B, N]`` -> ``(gt_rows int32 [n], n)``: the rows ``r = b * N + i`` with ``0 <= gt_j < M``, ascending"""
    gt_j = np.asarray(gt_j, np.int64)
    rows = np.nonzero(((gt_j >= 0) & (gt_j < M)).reshape(-1))[0].astype(np.int32)
    return rows, len(rows)


def pad_matches(pred, count, gt_j, keypoints3d, M, w_c, T, G, seed, step, scale, query_scale=None):
    """``pred``: dict ``b_ids, i_ids, j_ids`` int64 ``[cap]``, ``mconf [cap]``, ``mkpts_3d [cap, 3]``, ``mkpts_c [cap, 2]`` float32;
    ``count``: its row count or ``None`` (``cap``); ``keypoints3d [B or 1, N, 3]``.  -> dict of the ``T`` rows (``b_ids, i_ids, j_ids, mconf,
    mkpts_3d, mkpts_c, gt_mask``; with ``NO_GT``: no row), ``count``, ``n_keep``, ``status``, and the draws' ``sources`` (predicted
    rows) and ``gt_picks`` (ground-truth rows ``r``)."""
    gt_j = np.asarray(gt_j, np.int64)
    B, N = gt_j.shape
    kp = np.asarray(keypoints3d, f32)
    cap = len(pred["b_ids"])
    assert 0 < G < T <= B * N and 0 <= step < MAX_STEP
    P = cap if count is None else min(max(int(count), 0), cap)
    n_keep = min(P, T - G)
    rows, n_gt = gt_list(gt_j, M)
    if n_gt == 0:
        return {"count": 0, "n_keep": n_keep, "status": NO_GT}
    src = np.arange(n_keep, dtype=np.int64) if P <= T - G else picks(seed, step, 0, P, n_keep)
    r = rows[picks(seed, step, 1, n_gt, T - n_keep)].astype(np.int64)
    b, i = r // N, r % N
    j = gt_j[b, i]
    sx = sy = f32(scale)
    if query_scale is not None:
        qs = np.asarray(query_scale, f32)
        sx, sy = f32(scale) * qs[b, 1], f32(scale) * qs[b, 0]
    xc = np.stack([(j % w_c).astype(f32) * sx, (j // w_c).astype(f32) * sy], axis=1).astype(f32)
    out = {"b_ids": np.concatenate([np.asarray(pred["b_ids"], np.int64)[src], b]),
           "i_ids": np.concatenate([np.asarray(pred["i_ids"], np.int64)[src], i]),
           "j_ids": np.concatenate([np.asarray(pred["j_ids"], np.int64)[src], j]),
           "mconf": np.concatenate([np.asarray(pred["mconf"], f32)[src], np.zeros(len(r), f32)]),
           "mkpts_3d": np.concatenate([np.asarray(pred["mkpts_3d"], f32).reshape(-1, 3)[src], kp[b if kp.shape[0] > 1 else 0 * b, i]]),
           "mkpts_c": np.concatenate([np.asarray(pred["mkpts_c"], f32).reshape(-1, 2)[src], xc])}
    out["gt_mask"] = out["mconf"] == 0
    out.update(count=T, n_keep=n_keep, status=OK, sources=src, gt_picks=r)
    return out


def reference_keys(out):
    """the keys the reference's ``get_coarse_match`` returns, cut as it cuts them (``coarse_matching.py:231-239``)"""
    n = out["n_keep"]
    return {"b_ids": out["b_ids"], "i_ids": out["i_ids"], "j_ids": out["j_ids"], "gt_mask": out["gt_mask"], "m_bids": out["b_ids"][:n],
            "mkpts_3d_db": out["mkpts_3d"][:n], "mkpts_query_c": out["mkpts_c"][:n], "mconf": out["mconf"][:n]}
