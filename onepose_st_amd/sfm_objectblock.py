"""Keypoint-free SfM post-processing: triangulated points + fine-match features -> the object block the matcher reads, on the device.

The reference's last two SfM steps, ``feature_aggregation_and_update`` (src/KeypointFreeSfM/post_optimization/feature_aggregation.py:
10-180) and ``postprocess`` (run.py:295-390: ``filter_bbox``, ``get_tkl``, ``filter_track_length``, ``merge``, ``get_kpt_ann`` twice),
are numpy / scipy arithmetic, so every bit is fixed; the float arithmetic is HIP (``csrc/sfm_objectblock.hip`` in
``libonepose_sfm.so``, include/onepose_sfm.h), the integer tables between the launches are sorted, scanned and
compacted with torch on the device.  File I/O (COLMAP models, h5 features, the box file, the npz, the random padding) stays with the
caller.  Images are ``0 .. I - 1`` in the caller's ``img_lists`` order; the 2D keypoints of all images form one table of ``U`` slots with
``kpt_offsets [I + 1]`` int64, the layout ``sfm_coarse.merge_pair_matches`` returns.

Stage A, ``aggregate_track_features`` (``aggregation_method="avg"``, ``keypoints_update_method="colmap_updated_keypoints"``):

* Inputs: ``P`` tracks in ``point_cloud_assigned_imgID_kptID`` order, track ``p`` with its query ``(assigned_image[p], assigned_kpt[p])``
  owning rows ``row_offsets[p] : row_offsets[p + 1]`` (at least one); per row the reference keypoint ``(ref_image, ref_kpt)`` and the
  fine matcher's ``feature_c0`` / ``feature_c1 [R, 256]``, ``feature0`` / ``feature1 [R, 128]`` float32.  The caller has resolved
  ``mkpts0_idx == query_kpt_idx`` to the row (and checked that exactly one row matches).
* Outputs, keypoint-major: ``desc_coarse [U, 256]``, ``desc_fine [U, 128]`` float32, ``written [U]`` and ``scores_cleared [U]`` bool.
  A slot nothing writes is 0 (the reference's ``np.zeros`` tables).  A reference slot receives ``feature_c1`` / ``feature1`` of its row;
  the query slot receives the float32 mean of the track's ``feature_c0`` / ``feature0`` rows: a float32 running sum in row order, then
  one float32 division by the count (what ``np.mean(np.stack(...), axis=0)`` computes).  When several writers hit one slot the last
  one in the reference's loop order wins: tracks in order; in a track the rows in order, then the query.  The query keypoint's score is
  set to 0 by the reference: ``scores_cleared`` is that mask.  Keypoint coordinates are not touched.
* The reference's tables are float64 ``np.zeros`` that receive float32 values, so every entry is exactly a float32: float32 storage
  here loses nothing, and stage C widens on load.

Stage B, ``select_points``: ``Q`` points (``point_ids`` int64 unique in any order, ``xyz [Q, 3]`` float64, ``track_len`` int64).

1. ``filter_bbox``: with ``v45, v40, v47`` from corner 4 keep ``0 < (p - c4).v < v.v`` for all three, strictly (``bbox_corners=None``:
   ``skip_bbox_filter``).
2. ``get_tkl``: ``thres = min(Q', max_num_kp3d)``; walking the distinct track lengths upwards and subtracting each one's count, the first
   length at which the rest is ``<= thres`` is ``track_length``; ``filter_by_track_length`` keeps ``len >= track_length``, so the points
   of exactly that length stay although they were just subtracted, and the kept count may exceed ``max_num_kp3d`` (the reference's quirk).
3. The kept points are ordered by ascending id.
4. ``merge``: ``close[j] = {i : sqrt((dx^2 + dy^2) + dz^2) < dist_threshold}`` in float64 (scipy's ``pdist``, bit for bit).  Walking ``j``
   upwards: if a member of ``close[j]`` was recorded, ``j`` is skipped; otherwise the new point is the float64 mean of ``xyz[close[j]]``
   (running sum in ascending member order, one division), all members are recorded, and the group's old ids are ``point_ids[close[j]]``.
   A skipped ``j`` that no group holds is dropped (the reference's quirk).  The N x N matrix is never formed.

Stage C, ``average_point_features``: ``point3D_ids [U]`` int64 per 2D keypoint (-1: none), a stage A table, stage B's groups ->
``descriptors3d [N, dim]`` float64 and ``scores3d [N, 1]`` ones (the reference's "fake score").  Point ``n``'s observations are ordered by
the member's position in the group, then image, then keypoint index (``count_features`` / ``gather_3d_ann``); the value is the float64
running sum in that order over the widened float32 entries, then one division by the count.  Observations of ids in no group are
ignored; a new point with no observation raises ``ValueError`` (the reference would average an empty span).

Errors, raised before any launch of the stage: shapes, dtypes, malformed offsets, non-finite coordinates, repeated or negative ids -> ``ValueError``;
an image or keypoint index outside its table -> ``IndexError``; other ``aggregation_method`` / ``keypoints_update_method`` ->
``NotImplementedError``; a box that rejects every point -> ``ValueError``; CPU tensors -> :class:`hip.HipLibraryError` (no CPU fallback).
Host reads: one flag tensor per stage's checks and the counts that size outputs.
"""
from __future__ import annotations

import torch

from . import cabi, hip

_BINDING = cabi.Binding.of(__name__)                # the header is the one place a signature or a constant is written
library_path, load, check_arity, call = _BINDING.library_path, _BINDING.load, _BINDING.check_arity, _BINDING.call
launch = hip.launcher(_BINDING, globals())          # every stream-taking entry is called through it, by the header's parameter names
EXPORTED_SYMBOLS = _BINDING.exported_symbols
ABI_VERSION = _BINDING.abi_version
MAX_ITEMS, PAIR_TILE, PAIR_MAX_CHUNKS = map(_BINDING.constant, ("MAX_ITEMS", "PAIR_TILE", "PAIR_MAX_CHUNKS"))
DIM_COARSE, DIM_FINE = 256, 128


def _check_offsets(name: str, off: torch.Tensor, total: int, min_len: int = 0):
    if off.dtype != torch.int64 or off.dim() != 1 or off.numel() < 2:
        raise ValueError(f"{name}: expected int64 [n + 1], n >= 1")
    d = off[1:] - off[:-1]
    ok = torch.stack([off[0] == 0, off[-1] == total, (d >= min_len).all()]).tolist()
    if not all(ok):
        raise ValueError(f"{name}: expected offsets from 0 to {total} in steps of at least {min_len}")


def _workspace(n_slots: int, n_points: int, dev) -> tuple:
    nbytes = load().opsfm_workspace_bytes(n_slots, n_points)
    if nbytes == 0:
        raise ValueError(f"at most {MAX_ITEMS} slots / points")
    return torch.empty(nbytes, dtype=torch.uint8, device=dev), nbytes


# ---- stage A ---------------------------------------------------------------------------------------------------------------------------
def check_track_inputs(assigned_image, assigned_kpt, row_offsets, ref_image, ref_kpt, feature_c0, feature_c1, feature0, feature1,
                       kpt_offsets, keypoints_update_method="colmap_updated_keypoints", aggregation_method="avg"):
    """Stage A's input checks, on tensors of any device -> (P, R, I, U)"""
    if aggregation_method != "avg":
        raise NotImplementedError(f"aggregation_method {aggregation_method!r}: the reference implements 'avg' only")
    if keypoints_update_method != "colmap_updated_keypoints":
        raise NotImplementedError(f"keypoints_update_method {keypoints_update_method!r}: only 'colmap_updated_keypoints' (coordinates untouched)")
    hip.need_tensors((("assigned_image", assigned_image), ("assigned_kpt", assigned_kpt), ("row_offsets", row_offsets), ("ref_image", ref_image),
                      ("ref_kpt", ref_kpt), ("feature_c0", feature_c0), ("feature_c1", feature_c1), ("feature0", feature0), ("feature1", feature1),
                      ("kpt_offsets", kpt_offsets)))
    R = ref_image.shape[0] if ref_image.dim() == 1 else -1
    P = assigned_image.shape[0] if assigned_image.dim() == 1 else -1
    for name, t, shape in (("assigned_image", assigned_image, (P,)), ("assigned_kpt", assigned_kpt, (P,)), ("ref_image", ref_image, (R,)),
                           ("ref_kpt", ref_kpt, (R,))):
        if t.dtype != torch.int64 or tuple(t.shape) != shape:
            raise ValueError(f"{name}: expected int64 {list(shape)}, got {t.dtype} {list(t.shape)}")
    for name, t, dim in (("feature_c0", feature_c0, DIM_COARSE), ("feature_c1", feature_c1, DIM_COARSE), ("feature0", feature0, DIM_FINE),
                         ("feature1", feature1, DIM_FINE)):
        if t.dtype != torch.float32 or tuple(t.shape) != (R, dim):
            raise ValueError(f"{name}: expected float32 [{R}, {dim}], got {t.dtype} {list(t.shape)}")
    if P < 1:
        raise ValueError("no tracks")
    if row_offsets.numel() != P + 1:
        raise ValueError(f"row_offsets: expected int64 [{P + 1}]")
    _check_offsets("row_offsets", row_offsets, R, 1)
    if kpt_offsets.dtype != torch.int64 or kpt_offsets.dim() != 1 or kpt_offsets.numel() < 2:
        raise ValueError("kpt_offsets: expected int64 [I + 1]")
    I = kpt_offsets.numel() - 1
    U = int(kpt_offsets[-1])
    _check_offsets("kpt_offsets", kpt_offsets, U, 0)
    if U < 1 or U > MAX_ITEMS or R + P > MAX_ITEMS:
        raise ValueError(f"{U} keypoints, {R} rows: between 1 and {MAX_ITEMS}")
    img = torch.cat([assigned_image, ref_image])
    kpt = torch.cat([assigned_kpt, ref_kpt])
    bad_img = ((img < 0) | (img >= I)).any()
    n_kpt = (kpt_offsets[1:] - kpt_offsets[:-1])[img.clamp(0, I - 1)]
    bad = torch.stack([bad_img, ((kpt < 0) | (kpt >= n_kpt)).any()]).tolist()
    if bad[0]:
        raise IndexError(f"an image index lies outside [0, {I})")
    if bad[1]:
        raise IndexError("a keypoint index lies outside its image's keypoints (kpt_offsets)")
    return P, R, I, U


def aggregate_track_features(assigned_image, assigned_kpt, row_offsets, ref_image, ref_kpt, feature_c0, feature_c1, feature0, feature1,
                             kpt_offsets, keypoints_update_method="colmap_updated_keypoints", aggregation_method="avg") -> dict:
    """Stage A of the module docstring -> ``{"desc_coarse" [U, 256], "desc_fine" [U, 128]`` float32, ``"written" [U]``,
    ``"scores_cleared" [U]`` bool, ``"kpt_offsets"`` as given``}``"""
    args = (assigned_image, assigned_kpt, row_offsets, ref_image, ref_kpt, feature_c0, feature_c1, feature0, feature1, kpt_offsets)
    names = ("assigned_image", "assigned_kpt", "row_offsets", "ref_image", "ref_kpt", "feature_c0", "feature_c1", "feature0", "feature1",
             "kpt_offsets")
    if aggregation_method == "avg" and keypoints_update_method == "colmap_updated_keypoints":
        hip.need_device(tuple(zip(names, args)))
    P, R, I, U = check_track_inputs(*args, keypoints_update_method=keypoints_update_method, aggregation_method=aggregation_method)
    dev = feature_c0.device
    ws, nbytes = _workspace(U, 0, dev)
    desc_c = torch.empty(U, DIM_COARSE, dtype=torch.float32, device=dev)
    desc_f = torch.empty(U, DIM_FINE, dtype=torch.float32, device=dev)
    written = torch.empty(U, dtype=torch.uint8, device=dev)
    cleared = torch.empty(U, dtype=torch.uint8, device=dev)
    launch("opsfm_aggregate", dict(zip(names, (t.contiguous() for t in args)), P=P, R=R, I=I, U=U, dim_c=DIM_COARSE, dim_f=DIM_FINE, workspace=ws,
                                   workspace_bytes=nbytes, desc_coarse=desc_c, desc_fine=desc_f, written=written, scores_cleared=cleared))
    return {"desc_coarse": desc_c, "desc_fine": desc_f, "written": written.bool(), "scores_cleared": cleared.bool(), "kpt_offsets": kpt_offsets}


# ---- stage B ---------------------------------------------------------------------------------------------------------------------------
def check_point_inputs(point_ids, xyz, track_len, bbox_corners, max_num_kp3d, dist_threshold):
    """Stage B's input checks, on tensors of any device -> Q"""
    named = [("point_ids", point_ids), ("xyz", xyz), ("track_len", track_len)] + ([] if bbox_corners is None else [("bbox_corners", bbox_corners)])
    hip.need_tensors(named)
    Q = point_ids.shape[0] if point_ids.dim() == 1 else -1
    if point_ids.dtype != torch.int64 or Q < 1:
        raise ValueError("point_ids: expected int64 [Q], Q >= 1")
    if track_len.dtype != torch.int64 or tuple(track_len.shape) != (Q,):
        raise ValueError(f"track_len: expected int64 [{Q}]")
    if xyz.dtype != torch.float64 or tuple(xyz.shape) != (Q, 3):
        raise ValueError(f"xyz: expected float64 [{Q}, 3], got {xyz.dtype} {list(xyz.shape)}")
    if bbox_corners is not None and (bbox_corners.dtype != torch.float64 or tuple(bbox_corners.shape) != (8, 3)):
        raise ValueError("bbox_corners: expected float64 [8, 3] (or None: no box filter)")
    if Q > MAX_ITEMS:
        raise ValueError(f"{Q} points: at most {MAX_ITEMS}")
    if int(max_num_kp3d) < 1:
        raise ValueError("max_num_kp3d >= 1")
    if not float(dist_threshold) > 0.0:
        raise ValueError("dist_threshold > 0")
    finite = torch.isfinite(xyz).all() if bbox_corners is None else torch.isfinite(xyz).all() & torch.isfinite(bbox_corners).all()
    s = torch.sort(point_ids).values
    bad = torch.stack([~finite, (s[1:] == s[:-1]).any(), (track_len < 0).any(), s[0] < 0]).tolist()
    if bad[0]:
        raise ValueError("non-finite coordinate")
    if bad[1]:
        raise ValueError("point_ids: an id occurs twice")
    if bad[2]:
        raise ValueError("track_len: negative")
    if bad[3]:
        raise ValueError("point_ids: negative id (-1 marks a keypoint of no point)")
    return Q


def pair_chunks(n: int) -> tuple:
    """The partner range of the pair test in at most PAIR_MAX_CHUNKS chunks of a multiple of two tiles -> (chunk_len, n_chunks)"""
    unit = 2 * PAIR_TILE
    chunk_len = unit * max(1, -(-n // (unit * PAIR_MAX_CHUNKS)))
    return chunk_len, -(-n // chunk_len)


def select_points(point_ids, xyz, track_len, bbox_corners=None, max_num_kp3d: int = 15000, dist_threshold: float = 1e-3) -> dict:
    """Stage B of the module docstring -> ``{"keypoints3d" [N, 3] float64, "group_offsets" [N + 1], "group_members" [sum] int64 (old ids),
    "track_length" int, "counts" {"input", "after_bbox", "after_track_length", "after_merge", "close_entries"}}``"""
    named = [("point_ids", point_ids), ("xyz", xyz), ("track_len", track_len)] + ([] if bbox_corners is None else [("bbox_corners", bbox_corners)])
    hip.need_device(named)
    Q = check_point_inputs(point_ids, xyz, track_len, bbox_corners, max_num_kp3d, dist_threshold)
    dev = xyz.device
    i64, u8 = torch.int64, torch.uint8
    xyz = xyz.contiguous()
    # 1. the box
    if bbox_corners is None:
        idx = torch.arange(Q, device=dev)
    else:
        keep = torch.empty(Q, dtype=u8, device=dev)
        launch("opsfm_box_test", dict(xyz=xyz, Q=Q, corners=bbox_corners.contiguous(), keep=keep))
        idx = torch.nonzero(keep).squeeze(1)
    Q1 = idx.numel()
    if Q1 == 0:
        raise ValueError("the box rejects every point")
    # 2. the track length that brings the count to max_num_kp3d (integers)
    lens = track_len[idx]
    uniq, cnt = torch.unique(lens, return_counts=True)                     # ascending
    rest = Q1 - torch.cumsum(cnt, 0)
    track_length = int(uniq[torch.nonzero(rest <= min(Q1, int(max_num_kp3d)))[0, 0]])
    # 3. ascending id
    sel = idx[lens >= track_length]
    ids, order = torch.sort(point_ids[sel])
    pts = xyz[sel[order]].contiguous()
    N0 = ids.numel()
    # 4. the merge
    chunk_len, C = pair_chunks(N0)
    counts = torch.empty(N0 * C, dtype=i64, device=dev)
    launch("opsfm_pair_count", dict(xyz=pts, N=N0, dist_threshold=dist_threshold, chunk_len=chunk_len, n_chunks=C, counts=counts))
    positions = torch.cat([torch.zeros(1, dtype=i64, device=dev), torch.cumsum(counts, 0)])
    E = int(positions[-1])                                                 # read-back: sizes the sparse lists
    if E > MAX_ITEMS:
        raise ValueError(f"{E} close pairs: at most {MAX_ITEMS}")
    nbr = torch.empty(E, dtype=torch.int32, device=dev)
    launch("opsfm_pair_emit", dict(xyz=pts, N=N0, dist_threshold=dist_threshold, chunk_len=chunk_len, n_chunks=C, positions=positions,
                                   neighbours=nbr, E=E))
    rows = positions[::C]                                                  # [N0 + 1]: point j owns nbr[rows[j] : rows[j + 1]]
    deg = rows[1:] - rows[:-1]
    accepted = (deg == 1).to(u8)                                           # alone: by symmetry nobody can have recorded it
    multi = torch.nonzero(deg > 1).squeeze(1)
    ws, nbytes = _workspace(0, N0, dev)
    launch("opsfm_merge_resolve", dict(positions=positions, n_chunks=C, neighbours=nbr, multi=multi, M=multi.numel(), N=N0, workspace=ws,
                                       workspace_bytes=nbytes, accepted=accepted))
    acc = torch.nonzero(accepted).squeeze(1)
    N = acc.numel()
    goff = torch.cat([torch.zeros(1, dtype=i64, device=dev), torch.cumsum(deg[acc], 0)])
    total = int(goff[-1])
    kp3d = torch.empty(N, 3, dtype=torch.float64, device=dev)
    members = torch.empty(total, dtype=i64, device=dev)
    launch("opsfm_group_emit", dict(xyz=pts, ids=ids, accepted_idx=acc, positions=positions, n_chunks=C, neighbours=nbr, group_offsets=goff, G=N,
                                    N=N0, keypoints3d=kp3d, group_members=members, members_total=total))
    return {"keypoints3d": kp3d, "group_offsets": goff, "group_members": members, "track_length": track_length,
            "counts": {"input": Q, "after_bbox": Q1, "after_track_length": N0, "after_merge": N, "close_entries": E}}


# ---- stage C ---------------------------------------------------------------------------------------------------------------------------
def observation_runs(point3D_ids, group_offsets, group_members) -> tuple:
    """Stage C's integer half: which 2D keypoints each new point averages, in the summation order.
    -> (obs [sum] int64 slots, runs [N + 1] int64): point n owns ``obs[runs[n] : runs[n + 1]]``"""
    hip.need_device((("point3D_ids", point3D_ids), ("group_offsets", group_offsets), ("group_members", group_members)))
    if point3D_ids.dtype != torch.int64 or point3D_ids.dim() != 1 or point3D_ids.numel() < 1:
        raise ValueError("point3D_ids: expected int64 [U], U >= 1")
    if group_members.dtype != torch.int64 or group_members.dim() != 1:
        raise ValueError("group_members: expected int64 [sum]")
    _check_offsets("group_offsets", group_offsets, group_members.numel(), 1)
    dev, i64 = point3D_ids.device, torch.int64
    N = group_offsets.numel() - 1
    # old id -> position m in group_members (ascending m = new point, then the member's position in its group)
    sorted_ids, perm = torch.sort(group_members)
    bad = torch.stack([(sorted_ids[1:] == sorted_ids[:-1]).any(), sorted_ids[0] < 0]).tolist()
    if bad[0]:
        raise ValueError("group_members: an id occurs twice")
    if bad[1]:
        raise ValueError("group_members: negative id (-1 marks a keypoint of no point)")
    where = torch.searchsorted(sorted_ids, point3D_ids).clamp(max=group_members.numel() - 1)
    hit = (sorted_ids[where] == point3D_ids) & (point3D_ids >= 0)
    obs = torch.nonzero(hit).squeeze(1)                                    # ascending slot = image, then keypoint index
    m_sorted, order = torch.sort(perm[where[obs]], stable=True)
    point_of = torch.searchsorted(group_offsets, m_sorted, right=True) - 1
    per_point = torch.bincount(point_of, minlength=N)
    if bool((per_point == 0).any()):
        raise ValueError(f"new point {int(torch.nonzero(per_point == 0)[0, 0])} has no observation")
    runs = torch.cat([torch.zeros(1, dtype=i64, device=dev), torch.cumsum(per_point, 0)])
    return obs[order].contiguous(), runs


def point_means(table, obs, runs) -> torch.Tensor:
    """Stage C's float half: ``table [U, dim]`` float32 -> ``[N, dim]`` float64 means over ``observation_runs``' rows, in their order"""
    hip.need_device((("table", table),))
    if table.dtype != torch.float32 or table.dim() != 2 or table.shape[0] < 1 or table.shape[1] < 1:
        raise ValueError(f"table: expected float32 [U, dim], got {table.dtype} {list(table.shape)}")
    N, (U, dim) = runs.numel() - 1, table.shape
    out = torch.empty(N, dim, dtype=torch.float64, device=table.device)
    launch("opsfm_point_mean", dict(table=table.contiguous(), U=U, dim=dim, obs=obs, run_offsets=runs, G=N, out=out))
    return out


def average_point_features(point3D_ids, table, group_offsets, group_members) -> tuple:
    """Stage C of the module docstring -> ``(descriptors3d [N, dim] float64, scores3d [N, 1] float64 ones)``"""
    hip.need_device((("point3D_ids", point3D_ids), ("table", table), ("group_offsets", group_offsets), ("group_members", group_members)))
    if table.dim() != 2 or point3D_ids.dim() != 1 or table.shape[0] != point3D_ids.shape[0]:
        raise ValueError("table: expected float32 [U, dim] with one row per entry of point3D_ids")
    obs, runs = observation_runs(point3D_ids, group_offsets, group_members)
    out = point_means(table, obs, runs)
    return out, torch.ones(out.shape[0], 1, dtype=torch.float64, device=out.device)


# ---- composite and adapters ---------------------------------------------------------------------------------------------------------------
def build_object_block(tracks: dict, points: dict, point3D_ids, kpt_offsets, bbox_corners=None, max_num_kp3d: int = 15000,
                       dist_threshold: float = 1e-3, keypoints_update_method="colmap_updated_keypoints", aggregation_method="avg") -> dict:
    """A, B, then C twice.  ``tracks``: stage A's per-track and per-row tensors by name (``assigned_image, assigned_kpt, row_offsets,
    ref_image, ref_kpt, feature_c0, feature_c1, feature0, feature1``); ``points``: ``point_ids, xyz, track_len``; ``point3D_ids [U]`` of
    the model the box filter has gone over or not (ids outside the groups are ignored either way).
    -> stage B's dict plus ``descriptors3d_coarse [N, 256]``, ``descriptors3d_fine [N, 128]`` float64, ``scores3d [N, 1]`` and stage A's
    dict under ``"features"``."""
    feats = aggregate_track_features(*(tracks[k] for k in ("assigned_image", "assigned_kpt", "row_offsets", "ref_image", "ref_kpt",
                                                           "feature_c0", "feature_c1", "feature0", "feature1")), kpt_offsets,
                                     keypoints_update_method=keypoints_update_method, aggregation_method=aggregation_method)
    res = select_points(points["point_ids"], points["xyz"], points["track_len"], bbox_corners, max_num_kp3d, dist_threshold)
    if point3D_ids.dim() != 1 or point3D_ids.shape[0] != feats["desc_coarse"].shape[0]:
        raise ValueError("point3D_ids: expected one entry per 2D keypoint (kpt_offsets)")
    obs, runs = observation_runs(point3D_ids, res["group_offsets"], res["group_members"])      # once: only the table differs
    dc, df = point_means(feats["desc_coarse"], obs, runs), point_means(feats["desc_fine"], obs, runs)
    scores = torch.ones(dc.shape[0], 1, dtype=torch.float64, device=dc.device)
    res.update(descriptors3d_coarse=dc, descriptors3d_fine=df, scores3d=scores, features=feats)
    return res


def to_reference_outputs(result: dict) -> tuple:
    """-> the two npz-shaped dicts of ``save_3d_anno`` (coarse, fine): ``keypoints3d [N, 3]``, ``descriptors3d [dim, N]`` float64 and
    ``scores3d [N, 1]``, numpy"""
    kp = result["keypoints3d"].cpu().numpy()
    sc = result["scores3d"].cpu().numpy()
    return tuple({"keypoints3d": kp, "descriptors3d": result[k].cpu().numpy().transpose(1, 0), "scores3d": sc}
                 for k in ("descriptors3d_coarse", "descriptors3d_fine"))


def to_model_inputs(result: dict) -> dict:
    """-> what ``read_anno3d`` makes of the two files, minus its random padding, on the device: float32 ``keypoints3d [1, N, 3]``,
    ``descriptors3d_db [1, 128, N]``, ``descriptors3d_coarse_db [1, 256, N]``"""
    return {"keypoints3d": result["keypoints3d"].float()[None].contiguous(),
            "descriptors3d_db": result["descriptors3d_fine"].float().t()[None].contiguous(),
            "descriptors3d_coarse_db": result["descriptors3d_coarse"].float().t()[None].contiguous()}
