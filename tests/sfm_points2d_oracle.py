"""CPU restatement of the keypoint-free SfM's coarse-match merge (src/KeypointFreeSfM/coarse_match/, non-Ray branch of
coarse_match.py:141-186), written afresh in numpy and dicts: the yardstick of ``onepose_st_amd.sfm_coarse.merge_pair_matches``.

* ``match_to_points`` -- Match2Pts2D (utils.py:20-61): per image, ``[x, y, mconf]`` rows of every pair that holds it, pairs in dict order,
  rows in order;
* ``merge_points`` -- points2D_worker with agg_groupby_2d "sum" (coarse_match_worker.py:87-111, utils.py:5-18): keys ``astype(int)``,
  ``np.unique(axis=0)``, ``np.bincount`` float64 sums, ``sorted(..., reverse=True)`` by score -> ``{key: (rank, score)}``;
* ``index_matches`` -- update_matches (coarse_match_worker.py:119-155);
* ``to_arrays`` -- transform_points2D (:163-183).

``oracle_merge`` runs the four on the flat arrays of ``merge_pair_matches`` and returns the same flat result (numpy)."""
from __future__ import annotations

import numpy as np


def match_to_points(matches: dict, names: list) -> dict:
    """``{"a b": [N, 5] float32}`` -> ``{name: [n, 3] float32}`` (x, y, mconf of that side), the order of Match2Pts2D"""
    per = {name: [] for name in names}
    for key, m in matches.items():
        a, b = key.split(" ")
        per[a].append(m[:, [0, 1, 4]])
        per[b].append(m[:, [2, 3, 4]])
    return {name: (np.concatenate(v, 0) if v else np.empty((0, 3), np.float32)) for name, v in per.items()}


def merge_points(pts: np.ndarray) -> dict:
    """[n, 3] -> {(x, y): (rank, score)}; score = float64 sum in row order, rank = position in the stable descending sort"""
    keys = pts[:, :2].astype(int)
    if len(keys) == 0:
        return {}
    uniq, group = np.unique(keys, axis=0, return_inverse=True)
    sums = np.bincount(group.reshape(-1), weights=pts[:, 2], minlength=len(uniq))
    items = sorted(zip(map(tuple, uniq.tolist()), sums.tolist()), key=lambda kv: kv[1], reverse=True)
    return {k: (i, v) for i, (k, v) in enumerate(items)}


def index_matches(matches: dict, keypoints: dict) -> dict:
    out = {}
    for key, m in matches.items():
        a, b = key.split(" ")
        k0, k1 = keypoints[a], keypoints[b]
        ids = [[k0[tuple(p0)][0], k1[tuple(p1)][0]] for p0, p1 in zip(m[:, :2].astype(int).tolist(), m[:, 2:4].astype(int).tolist())]
        out[key] = np.array(ids, dtype=np.int64).reshape(-1, 2)
    return out


def to_arrays(keypoints: dict):
    kpts, scores = {}, {}
    for name, d in keypoints.items():
        assert len(d) != 0, "corner-case n_kpts=0 not handled."
        kpts[name] = np.array([list(k) for k in d.keys()], dtype=np.float32)
        scores[name] = np.array([v[1] for v in d.values()], dtype=np.float32)
    return kpts, scores


def reference_dicts(mkpts0, mkpts1, mconf, pair_offsets, pair_images, n_images):
    """flat arrays -> (matches dict, names, pair names) with names ``"0" .. str(I - 1)``"""
    mkpts0, mkpts1, mconf = (np.asarray(a, np.float32) for a in (mkpts0, mkpts1, mconf))
    off = np.asarray(pair_offsets, np.int64)
    pim = np.asarray(pair_images, np.int64).reshape(-1, 2)
    names = [str(i) for i in range(n_images)]
    pair_names = [f"{a} {b}" for a, b in pim.tolist()]
    rows = np.concatenate([mkpts0.reshape(-1, 2), mkpts1.reshape(-1, 2), mconf.reshape(-1, 1)], 1)
    matches = {pair_names[p]: rows[off[p]:off[p + 1]] for p in range(len(pim))}
    return matches, names, pair_names


def oracle_merge(mkpts0, mkpts1, mconf, pair_offsets, pair_images, n_images) -> dict:
    """-> {"keypoints" [U, 2] float32, "scores" [U] float32, "kpt_offsets" [I + 1] int64, "match_ids" [T, 2] int64}"""
    matches, names, pair_names = reference_dicts(mkpts0, mkpts1, mconf, pair_offsets, pair_images, n_images)
    if len(set(pair_names)) != len(pair_names):
        raise ValueError("the oracle keys pairs by name: every pair once")
    points = match_to_points(matches, names)
    keypoints = {name: merge_points(points[name]) for name in names}
    ids = index_matches(matches, keypoints)
    kpts, scores = to_arrays(keypoints)
    counts = [len(kpts[n]) for n in names]
    return {"keypoints": np.concatenate([kpts[n] for n in names], 0).reshape(-1, 2),
            "scores": np.concatenate([scores[n] for n in names], 0),
            "kpt_offsets": np.concatenate([[0], np.cumsum(counts)]).astype(np.int64),
            "match_ids": np.concatenate([ids[p] for p in pair_names], 0).reshape(-1, 2) if pair_names else np.empty((0, 2), np.int64)}


def oracle_merge_vectorised(mkpts0, mkpts1, mconf, pair_offsets, pair_images, n_images) -> dict:
    """``oracle_merge`` without dicts, for the cases of millions of rows: observations in (row, side) order, keys grouped by one
    ``np.unique`` of image / x / y packed into an int64 (signed order kept by a 2^20 bias), ``np.bincount`` sums in that order, then a
    stable sort by (image, score descending, key).  tests/test_sfm_points2d_cpu.py checks it against ``oracle_merge``."""
    mkpts0, mkpts1 = (np.asarray(a, np.float32).reshape(-1, 2) for a in (mkpts0, mkpts1))
    mconf = np.asarray(mconf, np.float32).reshape(-1)
    off = np.asarray(pair_offsets, np.int64)
    pim = np.asarray(pair_images, np.int64).reshape(-1, 2)
    T = len(mconf)
    pair_of_row = np.repeat(np.arange(len(pim)), np.diff(off))
    img = np.stack([pim[pair_of_row, 0], pim[pair_of_row, 1]], 1).reshape(-1)
    xy = np.stack([mkpts0, mkpts1], 1).reshape(-1, 2).astype(np.int64)
    assert np.abs(xy).max(initial=0) < (1 << 20)
    packed = (img << 42) | ((xy[:, 0] + (1 << 20)) << 21) | (xy[:, 1] + (1 << 20))
    uniq, inv = np.unique(packed, return_inverse=True)
    sums = np.bincount(inv.reshape(-1), weights=np.repeat(mconf, 2).astype(np.float64), minlength=len(uniq))
    uimg = uniq >> 42
    order = np.lexsort((np.arange(len(uniq)), -sums, uimg))
    counts = np.bincount(uimg, minlength=n_images)
    assert (counts > 0).all(), "corner-case n_kpts=0 not handled."
    kpt_offsets = np.concatenate([[0], np.cumsum(counts)]).astype(np.int64)
    rank = np.empty(len(uniq), np.int64)
    rank[order] = np.arange(len(uniq)) - kpt_offsets[uimg[order]]
    u = uniq[order]
    kp = np.stack([((u >> 21) & ((1 << 21) - 1)) - (1 << 20), (u & ((1 << 21) - 1)) - (1 << 20)], 1).astype(np.float32)
    return {"keypoints": kp, "scores": sums[order].astype(np.float32), "kpt_offsets": kpt_offsets,
            "match_ids": rank[inv.reshape(-1)].reshape(T, 2)}
