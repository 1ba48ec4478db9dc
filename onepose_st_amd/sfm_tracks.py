"""Keypoint-free SfM post-optimisation: from the triangulated model to the fine matcher's work list and the optimiser's rows, on the device.

The reference turns a COLMAP model into keyframes with a feature-track assignment (``CoarseReconDataset.get_keyframes_greedy``,
``build_initial_depth_pose``, ``extract_corresponding_frames``: src/KeypointFreeSfM/dataset/coarse_colmap_dataset.py), the pair list with
coarse matches the fine matcher runs on (``MatchingPairData``, post_optimization/data_construct/construct_matching_data.py) and the
per-track rows the optimiser and the feature aggregation read (``ConstructOptimizationData``, construct_optimization_data.py, and the
aggregation loop at the top of ``optimizer.py:start_optimize``), all in Python loops over every track element.  Here the sequential
part is HIP (``csrc/sfm_tracks.hip`` in ``libonepose_sfm_tracks.so``, include/onepose_sfm_tracks.h); the integer
tables between the launches are sorted, scanned and compacted with torch on the device.  File I/O (``read_write_model``, images,
pickles), the matcher itself and the rotation-matrix / quaternion round trip stay with the caller; the model comes from
``sfm_triangulate.triangulate``.

The model, a dict of flat device tensors:

* images ``0 .. I - 1`` in the order of the reference's ``colmap_images`` dict: ``image_ids [I]`` int64 (COLMAP ids), ``kpt_offsets
  [I + 1]`` int64 over one table of ``U`` keypoint slots (the layout of ``sfm_coarse`` and ``sfm_objectblock``), per slot ``xys [U, 2]``
  float64 and ``point3D_ids [U]`` int64 (-1: none), per image ``K``, ``R [I, 3, 3]``, ``t [I, 3]`` float64;
* points ``0 .. Q - 1`` in ``colmap_3ds`` dict order: ``point_ids [Q]`` int64, ``xyz [Q, 3]`` float64, ``track_offsets [Q + 1]`` int64,
  ``track_image [E]`` / ``track_kpt [E]`` int64 as indices (image index, keypoint index in that image), not ids.

1. ``assign_tracks(model) -> plan``: the greedy keyframe selection, restated exactly.

   * Slot states: -1 unregistered, -2 unoccupied, -3 robbed, >= 0 the id of the point the slot owns.
   * A round takes the first of the remaining images ordered by unoccupied count, descending.  Python's ``sorted(..., reverse=True)`` is
     stable and the sorted dict is carried into the next round, so ties at round r fall in the order of round r - 1, not in the initial
     order; the popped image leaves the order.  All -2 slots of the keyframe take their point; every track element of those points in
     another image becomes -3; a slot of the keyframe that was robbed earlier stays -3.
   * A point with two keypoints in the keyframe: both slots take its id, its assigned keypoint is the later one (the last write wins).
   * The loop ends when every point is assigned, which for a consistent model is when the largest count reaches 0: every keyframe owns
     at least one track and there are at most I rounds.
   * ``initial_depth [U]``: -1, except on occupied slots (they all lie in keyframes): ``z`` of ``K (R X + t)`` in float64
     (``project_point_cloud_to_image``), computed as ``((r0 x + r1 y) + r2 z) + t`` per row and ``(k0 cx + k1 cy) + k2 cz``.
   * The plan: ``keyframes [Kf]`` in selection order, ``state [U]`` int64, ``is_keyframe [I]`` bool, ``assigned_image [Q]``,
     ``assigned_kpt [Q]`` int64, ``initial_depth [U]`` float64 (keys with an underscore are the module's own tables).
   * At most ``MAX_IMAGES`` images (the per-round ordering lives in one workgroup).

2. ``matching_pairs(plan, model) -> pairs``: ``pair_left [Np]``, ``pair_right [Np]`` (image indices), ``pair_offsets [Np + 1]``, per row
   ``mkpts0_c``, ``mkpts1_c [M, 2]`` float64 (exact copies of ``xys``), ``mkpts0_idx [M]``, ``row_left`` / ``row_right [M]``.  Left
   images follow the image order, keyframes only; right images ascend by COLMAP id (``np.unique``), the left image removed; rows ascend
   by left keypoint index over the slots with state >= 0 whose track contains the right image; when the right image occurs twice in a
   track the first occurrence supplies ``mkpts1_c``.

3. ``optimisation_rows(plan, model, pairs) -> rows``: for point p in order the distinct images of its track other than the assigned one,
   in first-occurrence order (``pairs_dict``: a repeated image keeps its first position and the keypoint of its last occurrence):
   ``ref_image``, ``ref_kpt``, ``row_point [R]``, ``fine_row [R]`` (the one pair row with that (left, right) and ``mkpts0_idx ==
   assigned_kpt[p]``; verified on the device, ``ValueError`` otherwise), ``n_query [Q]``, ``row_offsets [Q + 1]``.  A point seen in its
   assigned image only has no row: ``ValueError`` (the reference stacks an empty list).  ``to_optimizer_inputs`` gives the ``aggregated``
   dict and ``frame_poses`` of ``postopt.Optimizer.start_optimize``; ``to_aggregation_inputs`` the stage A track dict of
   ``sfm_objectblock.build_object_block``.  The aggregation loop of the reference visits every track element, so a track that holds an
   image twice feeds that pair's row twice into the query mean there; the rows here are the optimiser's (one per distinct image).

4. ``update_model(plan, model, depth, R, t)``: new ``xyz`` from ``postopt.points_from_depth`` at each point's assigned slot, new ``xys``
   of every registered slot from ``postopt.project_points``.

Errors, raised before any launch: shapes, dtypes, malformed offsets, a point without element, non-finite coordinates, repeated or
negative ids, ids of 2^53 or more (the reference keeps states in float64), a slot table and a track table that disagree (every slot with
``point3D_ids == p`` is an element of p's track and the other way round: the reference's assert and its KeyError paths) -> ``ValueError``;
an image or keypoint index outside its table -> ``IndexError``; another ``feature_track_assignment_strategy`` -> ``NotImplementedError``;
CPU tensors -> :class:`hip.HipLibraryError` (no CPU fallback).  Host reads: one flag tensor for the checks, the keyframe count after the
rounds (nothing is read inside the loop), the row counts that size outputs, one error flag.
"""
from __future__ import annotations

import torch

from . import cabi, hip, postopt

_BINDING = cabi.Binding.of(__name__)                # the header is the one place a signature or a constant is written
library_path, load, check_arity, call = _BINDING.library_path, _BINDING.load, _BINDING.check_arity, _BINDING.call
launch = hip.launcher(_BINDING, globals())          # every stream-taking entry is called through it, by the header's parameter names
EXPORTED_SYMBOLS = _BINDING.exported_symbols
ABI_VERSION = _BINDING.abi_version
MAX_IMAGES, MAX_ITEMS, CTRL_INTS = map(_BINDING.constant, ("MAX_IMAGES", "MAX_ITEMS", "CTRL_INTS"))
MAX_ID = 2 ** 53
MODEL_KEYS = ("image_ids", "kpt_offsets", "xys", "point3D_ids", "K", "R", "t", "point_ids", "xyz", "track_offsets", "track_image", "track_kpt")
PLAN_KEYS = ("keyframes", "state", "is_keyframe", "assigned_image", "assigned_kpt", "initial_depth")
PAIR_KEYS = ("pair_left", "pair_right", "pair_offsets", "mkpts0_c", "mkpts1_c", "mkpts0_idx", "row_left", "row_right")
ROW_KEYS = ("fine_row", "ref_image", "ref_kpt", "row_point", "n_query", "row_offsets")
TRACK_KEYS = ("assigned_image", "assigned_kpt", "row_offsets", "ref_image", "ref_kpt", "feature_c0", "feature_c1", "feature0", "feature1")


# ---- the model's checks ---------------------------------------------------------------------------------------------------------------
def check_model(model: dict, feature_track_assignment_strategy: str = "greedy") -> dict:
    """Every check of the module docstring, on tensors of any device -> the derived tables: ``I, U, Q, E, max_slots`` and
    ``slot_image [U]``, ``slot_point [U]`` (point index or -1), ``elem_point [E]``, ``elem_slot [E]``"""
    if feature_track_assignment_strategy != "greedy":
        raise NotImplementedError(f"feature_track_assignment_strategy {feature_track_assignment_strategy!r}: the reference implements 'greedy' only")
    missing = [k for k in MODEL_KEYS if k not in model]
    if missing:
        raise ValueError(f"model lacks {missing}")
    m = {k: model[k] for k in MODEL_KEYS}
    hip.need_tensors(m.items())
    i64, f64 = torch.int64, torch.float64
    I = m["image_ids"].shape[0] if m["image_ids"].dim() == 1 else -1
    Q = m["point_ids"].shape[0] if m["point_ids"].dim() == 1 else -1
    U = m["point3D_ids"].shape[0] if m["point3D_ids"].dim() == 1 else -1
    E = m["track_image"].shape[0] if m["track_image"].dim() == 1 else -1
    if I < 1 or Q < 1 or U < 1 or E < 1:
        raise ValueError("image_ids [I], point_ids [Q], point3D_ids [U], track_image [E]: one-dimensional and not empty")
    if I > MAX_IMAGES:
        raise ValueError(f"{I} images: at most {MAX_IMAGES}")
    if max(U, Q, E) > MAX_ITEMS:
        raise ValueError(f"at most {MAX_ITEMS} slots, points or track elements")
    for k, dtype, shape in (("image_ids", i64, (I,)), ("kpt_offsets", i64, (I + 1,)), ("xys", f64, (U, 2)), ("point3D_ids", i64, (U,)),
                            ("K", f64, (I, 3, 3)), ("R", f64, (I, 3, 3)), ("t", f64, (I, 3)), ("point_ids", i64, (Q,)), ("xyz", f64, (Q, 3)),
                            ("track_offsets", i64, (Q + 1,)), ("track_image", i64, (E,)), ("track_kpt", i64, (E,))):
        if m[k].dtype != dtype or tuple(m[k].shape) != shape:
            raise ValueError(f"{k}: expected {dtype} {list(shape)}, got {m[k].dtype} {list(m[k].shape)}")
    dev = m["image_ids"].device
    if any(v.device != dev for v in m.values()):
        raise ValueError("the model's tensors lie on different devices")
    ko, to = m["kpt_offsets"], m["track_offsets"]
    n_kpt, n_elem = ko[1:] - ko[:-1], to[1:] - to[:-1]
    sorted_pid, pid_perm = torch.sort(m["point_ids"])
    sorted_iid = torch.sort(m["image_ids"]).values
    p3d = m["point3D_ids"]
    flags = [ko[0] != 0, ko[-1] != U, (n_kpt < 0).any(),                                               # 0-2: kpt_offsets
             to[0] != 0, to[-1] != E, (n_elem < 1).any(),                                              # 3-5: track_offsets
             ~(torch.isfinite(m["xys"]).all() & torch.isfinite(m["xyz"]).all() & torch.isfinite(m["K"]).all()
               & torch.isfinite(m["R"]).all() & torch.isfinite(m["t"]).all()),                        # 6
             (sorted_pid[1:] == sorted_pid[:-1]).any(), (sorted_iid[1:] == sorted_iid[:-1]).any(),     # 7, 8
             (sorted_pid[0] < 0) | (sorted_iid[0] < 0) | (p3d < -1).any(),                             # 9
             (sorted_pid[-1] >= MAX_ID) | (sorted_iid[-1] >= MAX_ID) | (p3d >= MAX_ID).any(),          # 10
             ((m["track_image"] < 0) | (m["track_image"] >= I)).any()]                                 # 11
    bad = torch.stack([f.to(torch.bool) for f in flags]).tolist()
    if bad[0] or bad[1] or bad[2]:
        raise ValueError(f"kpt_offsets: expected non-decreasing offsets from 0 to {U}")
    if bad[3] or bad[4] or bad[5]:
        raise ValueError(f"track_offsets: expected offsets from 0 to {E} in steps of at least 1 (every point has at least one element)")
    if bad[6]:
        raise ValueError("non-finite coordinate")
    if bad[7] or bad[8]:
        raise ValueError("point_ids / image_ids: an id occurs twice")
    if bad[9]:
        raise ValueError("negative id (-1 marks a keypoint of no point)")
    if bad[10]:
        raise ValueError("an id of 2^53 or more (the reference keeps the states in float64)")
    if bad[11]:
        raise IndexError(f"track_image: an image index lies outside [0, {I})")
    # second read: what needs the tables above to be sound
    slot_image = torch.repeat_interleave(torch.arange(I, device=dev), n_kpt, output_size=U)
    elem_point = torch.repeat_interleave(torch.arange(Q, device=dev), n_elem, output_size=E)
    bad_kpt = ((m["track_kpt"] < 0) | (m["track_kpt"] >= n_kpt[m["track_image"]])).any()
    elem_slot = (ko[m["track_image"]] + m["track_kpt"]).clamp(0, U - 1)
    where = torch.searchsorted(sorted_pid, p3d).clamp(max=Q - 1)
    known = sorted_pid[where] == p3d
    slot_point = torch.where(known, pid_perm[where], torch.full_like(p3d, -1))
    unknown_id = ((p3d >= 0) & ~known).any()
    covered = torch.zeros(U, dtype=torch.bool, device=dev)
    covered[elem_slot] = True
    bad = torch.stack([bad_kpt, unknown_id, (slot_point[elem_slot] != elem_point).any(), (covered != (p3d >= 0)).any()]).tolist()
    if bad[0]:
        raise IndexError("track_kpt: a keypoint index lies outside its image's keypoints (kpt_offsets)")
    if bad[1]:
        raise ValueError("point3D_ids: an id that point_ids does not hold")
    if bad[2]:
        raise ValueError("a track element's slot does not carry the track's point id (point3D_ids)")
    if bad[3]:
        raise ValueError("a slot carries a point id but is an element of no track")
    return {"I": I, "U": U, "Q": Q, "E": E, "max_slots": int(n_kpt.max()), "slot_image": slot_image, "slot_point": slot_point,
            "elem_point": elem_point, "elem_slot": elem_slot}


# ---- 1. the greedy assignment ---------------------------------------------------------------------------------------------------------
def assign_tracks(model: dict, feature_track_assignment_strategy: str = "greedy") -> dict:
    """Section 1 of the module docstring -> the plan"""
    if feature_track_assignment_strategy == "greedy" and all(k in model for k in MODEL_KEYS):
        hip.need_device([(k, model[k]) for k in MODEL_KEYS])
    d = check_model(model, feature_track_assignment_strategy)
    I, U, Q, E = d["I"], d["U"], d["Q"], d["E"]
    dev = model["xys"].device
    i32, i64, f64 = torch.int32, torch.int64, torch.float64
    c = {k: model[k].contiguous() for k in MODEL_KEYS}
    registered = d["slot_point"] >= 0
    state = torch.where(registered, -2, -1).to(i32)
    count = torch.zeros(I, dtype=i64, device=dev).index_add_(0, d["slot_image"], registered.to(i64)).to(i32)
    order = torch.arange(I, dtype=i32, device=dev)
    assigned_image = torch.full((Q,), -1, dtype=i32, device=dev)
    assigned_kpt = torch.full((Q,), -1, dtype=i32, device=dev)
    keyframes = torch.full((I,), -1, dtype=i32, device=dev)
    ctrl = torch.tensor([0, I, 0, -1], dtype=i32, device=dev)
    launch("opsft_assign", dict(kpt_offsets=c["kpt_offsets"], slot_point=d["slot_point"], track_offsets=c["track_offsets"],
                                elem_image=c["track_image"], elem_slot=d["elem_slot"], I=I, U=U, Q=Q, E=E, max_slots=d["max_slots"], state=state,
                                count=count, order=order, assigned_image=assigned_image, assigned_kpt=assigned_kpt, keyframes=keyframes, ctrl=ctrl))
    state_ids = torch.empty(U, dtype=i64, device=dev)
    depth = torch.empty(U, dtype=f64, device=dev)
    launch("opsft_finish", dict(state=state, slot_image=d["slot_image"], point_ids=c["point_ids"], xyz=c["xyz"], K=c["K"], R=c["R"], t=c["t"], I=I,
                                U=U, Q=Q, state_ids=state_ids, initial_depth=depth))
    done, _, n_kf, _ = ctrl.tolist()                                       # the read-back after the rounds
    if not done or bool((assigned_image < 0).any()):
        raise RuntimeError("the greedy rounds ended with unassigned points")
    kf = keyframes[:n_kf].to(i64)
    is_kf = torch.zeros(I, dtype=torch.bool, device=dev)
    is_kf[kf] = True
    plan = {"keyframes": kf, "state": state_ids, "is_keyframe": is_kf, "assigned_image": assigned_image.to(i64),
            "assigned_kpt": assigned_kpt.to(i64), "initial_depth": depth}
    plan.update(_state=state, _assigned_image=assigned_image, _assigned_kpt=assigned_kpt, _tables=d)
    return plan


def _track_rows(plan: dict, model: dict) -> dict:
    """The optimiser's rows as track elements (computed once per plan): ``rows_e [R]`` element indices in order, ``n_query [Q]``,
    ``row_offsets [Q + 1]``, ``match_kpt`` / ``ref_kpt [E]``"""
    if "_rows" in plan:
        return plan["_rows"]
    hip.need_device([(k, model[k]) for k in MODEL_KEYS] + [("plan state", plan["_state"])])
    d = plan["_tables"]
    Q, E = d["Q"], d["E"]
    dev = model["xys"].device
    i64 = torch.int64
    other = torch.empty(E, dtype=torch.uint8, device=dev)
    match_kpt = torch.empty(E, dtype=i64, device=dev)
    ref_kpt = torch.empty(E, dtype=i64, device=dev)
    launch("opsft_track_rows", dict(track_offsets=model["track_offsets"].contiguous(), elem_point=d["elem_point"],
                                    elem_image=model["track_image"].contiguous(), track_kpt=model["track_kpt"].contiguous(),
                                    assigned_image=plan["_assigned_image"], Q=Q, E=E, other=other, match_kpt=match_kpt, ref_kpt=ref_kpt))
    rows_e = torch.nonzero(other).squeeze(1)
    n_query = torch.bincount(d["elem_point"][rows_e], minlength=Q)
    plan["_rows"] = {"rows_e": rows_e, "n_query": n_query, "row_offsets": hip.exclusive(n_query), "match_kpt": match_kpt, "ref_kpt": ref_kpt}
    return plan["_rows"]


# ---- 2. the fine matcher's work list ----------------------------------------------------------------------------------------------------
def matching_pairs(plan: dict, model: dict) -> dict:
    """Section 2 of the module docstring -> the pairs"""
    tr = _track_rows(plan, model)
    d = plan["_tables"]
    I, U, E = d["I"], d["U"], d["E"]
    dev = model["xys"].device
    i64, f64 = torch.int64, torch.float64
    owned = torch.nonzero(plan["_state"] >= 0).squeeze(1)                  # ascending slot = image, then keypoint index
    point_of = plan["_state"][owned].to(i64)
    per_slot = tr["n_query"][point_of]
    first = hip.exclusive(per_slot)
    M = int(first[-1])                                                     # read-back: sizes the rows
    if M == 0:
        raise ValueError("no point is seen in a second image: there is no pair to match")
    if M > MAX_ITEMS:
        raise ValueError(f"{M} pair rows: at most {MAX_ITEMS}")
    which = torch.repeat_interleave(torch.arange(owned.numel(), device=dev), per_slot, output_size=M)
    owner_slot = owned[which].contiguous()
    row_elem = tr["rows_e"][tr["row_offsets"][point_of[which]] + (torch.arange(M, device=dev) - first[which])].contiguous()
    id_rank = torch.empty(I, dtype=i64, device=dev)
    id_rank[torch.argsort(model["image_ids"])] = torch.arange(I, device=dev)
    ko, ti = model["kpt_offsets"].contiguous(), model["track_image"].contiguous()
    keys = torch.empty(M, dtype=i64, device=dev)
    launch("opsft_pair_keys", dict(owner_slot=owner_slot, row_elem=row_elem, slot_image=d["slot_image"], kpt_offsets=ko, elem_image=ti,
                                   id_rank=id_rank, I=I, U=U, E=E, M=M, key_stride=d["max_slots"], keys=keys))
    sorted_keys, perm = torch.sort(keys)                                   # the keys are distinct: (left, right, left keypoint)
    out = {"mkpts0_c": torch.empty(M, 2, dtype=f64, device=dev), "mkpts1_c": torch.empty(M, 2, dtype=f64, device=dev),
           "mkpts0_idx": torch.empty(M, dtype=i64, device=dev), "row_left": torch.empty(M, dtype=i64, device=dev),
           "row_right": torch.empty(M, dtype=i64, device=dev)}
    launch("opsft_pair_emit", dict(perm=perm, owner_slot=owner_slot, row_elem=row_elem, slot_image=d["slot_image"], kpt_offsets=ko, elem_image=ti,
                                   match_kpt=tr["match_kpt"], xys=model["xys"].contiguous(), I=I, U=U, E=E, M=M, **out))
    _, per_pair = torch.unique_consecutive(torch.div(sorted_keys, d["max_slots"], rounding_mode="floor"), return_counts=True)
    offsets = hip.exclusive(per_pair)
    out.update(pair_offsets=offsets, pair_left=out["row_left"][offsets[:-1]], pair_right=out["row_right"][offsets[:-1]])
    return out


def to_reference_outputs(pairs: dict, model: dict) -> dict:
    """-> ``{"{id0}-{id1}": {"mkpts0_c", "mkpts1_c" [n, 2], "mkpts0_idx" [n], "frame0_colmap_id", "frame1_colmap_id"}}`` in the order of
    ``MatchingPairData.all_pairs``, numpy: what its ``__getitem__`` adds to the two image dicts"""
    ids = model["image_ids"].cpu().numpy()
    off = pairs["pair_offsets"].cpu().numpy()
    left, right = pairs["pair_left"].cpu().numpy(), pairs["pair_right"].cpu().numpy()
    mk0, mk1, idx = (pairs[k].cpu().numpy() for k in ("mkpts0_c", "mkpts1_c", "mkpts0_idx"))
    out = {}
    for n in range(len(left)):
        a, b = int(ids[left[n]]), int(ids[right[n]])
        out[f"{a}-{b}"] = {"mkpts0_c": mk0[off[n]:off[n + 1]], "mkpts1_c": mk1[off[n]:off[n + 1]], "mkpts0_idx": idx[off[n]:off[n + 1]],
                           "frame0_colmap_id": a, "frame1_colmap_id": b}
    return out


# ---- 3. the optimiser's rows -------------------------------------------------------------------------------------------------------------
def optimisation_rows(plan: dict, model: dict, pairs: dict) -> dict:
    """Section 3 of the module docstring -> the rows"""
    hip.need_device([(k, pairs[k]) for k in ("pair_left", "pair_right", "pair_offsets", "mkpts0_idx")])
    tr = _track_rows(plan, model)
    d = plan["_tables"]
    I, Q = d["I"], d["Q"]
    dev = model["xys"].device
    i64, i32 = torch.int64, torch.int32
    rows_e = tr["rows_e"]
    R = rows_e.numel()
    if bool((tr["n_query"] == 0).any()):
        raise ValueError(f"point {int(torch.nonzero(tr['n_query'] == 0)[0, 0])} is seen in its assigned image only: it has no row")
    Np, M = pairs["pair_left"].numel(), pairs["mkpts0_idx"].numel()
    for k, n in (("pair_left", Np), ("pair_right", Np), ("pair_offsets", Np + 1), ("mkpts0_idx", M)):
        if pairs[k].dtype != i64 or tuple(pairs[k].shape) != (n,):
            raise ValueError(f"pairs[{k!r}]: expected int64 [{n}]")
    if Np < 1 or M < 1:
        raise ValueError("pairs: empty")
    row_point = d["elem_point"][rows_e].contiguous()
    ref_image = model["track_image"][rows_e].contiguous()
    ref_kpt = tr["ref_kpt"][rows_e].contiguous()
    fine_row = torch.empty(R, dtype=i64, device=dev)
    err = torch.zeros(1, dtype=i32, device=dev)
    launch("opsft_fine_rows", dict(row_point=row_point, ref_image=ref_image, assigned_image=plan["_assigned_image"],
                                   assigned_kpt=plan["_assigned_kpt"], image_ids=model["image_ids"].contiguous(),
                                   pair_left=pairs["pair_left"].contiguous(), pair_right=pairs["pair_right"].contiguous(),
                                   pair_offsets=pairs["pair_offsets"].contiguous(), mkpts0_idx=pairs["mkpts0_idx"].contiguous(), I=I, Q=Q, R=R,
                                   Np=Np, M=M, fine_row=fine_row, error_flag=err))
    if int(err.item()):
        j = int(torch.nonzero(fine_row < 0)[0, 0])
        raise ValueError(f"row {j} (point {int(row_point[j])}, image {int(ref_image[j])}): the pair list does not hold exactly one row "
                         f"with its (left, right) and mkpts0_idx == the assigned keypoint")
    return {"fine_row": fine_row, "ref_image": ref_image, "ref_kpt": ref_kpt, "row_point": row_point, "n_query": tr["n_query"],
            "row_offsets": tr["row_offsets"]}


def assigned_slots(plan: dict, model: dict) -> torch.Tensor:
    """[Q]: the slot of each point's assigned keypoint"""
    return model["kpt_offsets"][plan["assigned_image"]] + plan["assigned_kpt"]


def to_optimizer_inputs(plan: dict, model: dict, pairs: dict, rows: dict, mkpts1_f: torch.Tensor) -> tuple:
    """``mkpts1_f [M, 2]``: the fine matcher's refined right keypoints, one per pair row -> ``(aggregated, frame_poses)`` as
    ``postopt.Optimizer.start_optimize`` documents them (``ConstructOptimizationData`` reduced as ``start_optimize`` reduces it)"""
    hip.need_device([("mkpts1_f", mkpts1_f)])
    M = pairs["mkpts0_idx"].numel()
    if mkpts1_f.dim() != 2 or tuple(mkpts1_f.shape) != (M, 2):
        raise ValueError(f"mkpts1_f: expected [{M}, 2], got {list(mkpts1_f.shape)}")
    fr = rows["fine_row"]
    left, right = pairs["row_left"][fr], pairs["row_right"][fr]
    aggregated = {"depth": plan["initial_depth"][assigned_slots(plan, model)].reshape(-1, 1), "n_query": rows["n_query"],
                  "intrinsic0": model["K"][left], "intrinsic1": model["K"][right], "mkpts0_c": pairs["mkpts0_c"][fr],
                  "mkpts1_c": pairs["mkpts1_c"][fr], "mkpts1_f": mkpts1_f.to(torch.float64)[fr], "left_colmap_ids": model["image_ids"][left],
                  "right_colmap_ids": model["image_ids"][right], "point_cloud_id": model["point_ids"]}
    ids, R, t = model["image_ids"].tolist(), model["R"].cpu().numpy(), model["t"].cpu().numpy()
    return aggregated, {int(i): [R[n], t[n]] for n, i in enumerate(ids)}


def to_aggregation_inputs(plan: dict, rows: dict, feature_c0, feature_c1, feature0, feature1) -> dict:
    """The fine matcher's four feature tables, one row per pair row -> stage A's track dict of ``sfm_objectblock.build_object_block``"""
    feats = (("feature_c0", feature_c0), ("feature_c1", feature_c1), ("feature0", feature0), ("feature1", feature1))
    hip.need_device(feats)
    fr = rows["fine_row"]
    out = {"assigned_image": plan["assigned_image"], "assigned_kpt": plan["assigned_kpt"], "row_offsets": rows["row_offsets"],
           "ref_image": rows["ref_image"], "ref_kpt": rows["ref_kpt"]}
    for name, f in feats:
        if f.dim() != 2 or (fr.numel() and int(fr.max()) >= f.shape[0]):
            raise ValueError(f"{name}: expected one row per pair row")
        out[name] = f[fr]
    return out


# ---- 4. the model after the refinement ---------------------------------------------------------------------------------------------------
def update_model(plan: dict, model: dict, depth: torch.Tensor, R: torch.Tensor, t: torch.Tensor) -> dict:
    """``depth [Q]`` (or ``[Q, 1]``) and the refined poses ``R [I, 3, 3]``, ``t [I, 3]`` -> ``{"xyz" [Q, 3], "xys" [U, 2]}``: every point
    unprojected from its assigned keypoint, then every registered slot reprojected (update_optimize_results_to_colmap)"""
    hip.need_device([("depth", depth), ("R", R), ("t", t)] + [(k, model[k]) for k in MODEL_KEYS])
    d = plan["_tables"]
    xyz = postopt.points_from_depth(model["xys"][assigned_slots(plan, model)], depth, plan["assigned_image"], model["K"], R, t)
    reg = torch.nonzero(d["slot_point"] >= 0).squeeze(1)
    xys = model["xys"].clone()
    xys[reg] = postopt.project_points(xyz[d["slot_point"][reg]], d["slot_image"][reg], model["K"], R, t)
    return {"xyz": xyz, "xys": xys}
