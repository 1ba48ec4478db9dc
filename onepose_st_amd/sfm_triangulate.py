"""Keypoint-free SfM triangulation: from the merged coarse matches and the camera poses to the track model, on the device.

The reference writes the keypoints and matches into an sqlite database and shells out to the COLMAP binary (``point_triangulator``,
src/sfm_utils/triangulation.py:195-250, ``import_features`` :80-110).  COLMAP is not a dependency of this project, so this module does
not restate COLMAP: it implements a specification of its own, chosen so that every decision is deterministic and
independent of thread order.  The float64 work is HIP (``csrc/sfm_triangulate.hip`` in ``libonepose_sfm_triangulate.so``,
include/onepose_sfm_triangulate.h); sorting and segmenting the candidates by component between the launches is torch on the device.
What is *not* restated: COLMAP's incremental triangulator, its track merging and completion, its bundle adjustment.

``triangulate(merged, cameras, **options) -> model``

* ``merged``: what ``sfm_coarse.merge_pair_matches`` returns plus ``pair_images [P, 2]`` int64 -- ``keypoints [U, 2]`` float32,
  ``kpt_offsets [I + 1]``, ``match_ids [T, 2]`` (per-image keypoint ranks), ``pair_offsets [P + 1]`` int64.
* ``cameras``: ``image_ids [I]`` int64, ``K [I, 3, 3]``, ``R [I, 3, 3]``, ``t [I, 3]`` float64, world to camera;
  ``K = [[fx, s, cx], [0, fy, cy], [0, 0, 1]]``.
* ``model``: the dict ``sfm_tracks.check_model`` accepts (``sfm_tracks.MODEL_KEYS``), plus ``point_error [Q]`` float64 (the mean
  reprojection error of the track's elements, px), ``labels [U]`` int64 (the component of every slot) and ``n_rounds`` (int: the rounds
  that ran).  ``xys = float64(keypoints) + 0.5`` (``import_features``).

The specification (``tests/sfm_triangulate_oracle.py`` restates it in loop form):

1. Components.  Nodes are the ``U`` slots; match row ``(id0, id1)`` of pair ``(img0, img1)`` joins slot ``kpt_offsets[img0] + id0`` and
   ``kpt_offsets[img1] + id1``.  A component's label is its smallest slot.  A component may hold two slots of one image.
2. Candidates of a round: the slots of a component not yet assigned to a point, ascending, ``L`` of them.
3. Hypotheses.  ``L (L - 1) / 2 <= max_hypotheses``: every pair ``(a, b)``, ``a < b``, lexicographic.  Otherwise ``max_hypotheses`` pairs
   from splitmix64 with the state ``label * 256 + round`` (round = 0, 1, ...): hypothesis ``h`` takes outputs ``2 h`` and ``2 h + 1``,
   ``a = out mod L``, ``r = out mod (L - 1)``, ``b = r + (r >= a)``.  A pair from one image is skipped.  With unit rays ``d`` from the
   centres ``c``: ``n = da x db``, skipped when ``|n| < 1e-12``; ``w = ca - cb``, ``ta = ((da.db)(db.w) - da.w) / |n|^2``,
   ``tb = (db.w - (da.db)(da.w)) / |n|^2``, ``X = ((ca + ta da) + (cb + tb db)) / 2``.
4. Scoring.  With ``q = P (X, 1)``, ``P = K [R | t]``: an element is an inlier when ``q_2 > 0`` and ``(q_0 / q_2 - x)^2 + (q_1 / q_2 -
   y)^2 <= max_reproj_error^2``.  Most inliers win, among equals the earliest hypothesis; fewer than 2 inliers or one image only: no point.
5. Refit over the winner's inliers, ``X = (sum (I - d d^T))^-1 sum (I - d d^T) c``, by cofactors; then ``refine_steps`` Gauss-Newton steps
   on the squared reprojection error of those inliers (3 x 3 normal equations, cofactors).  A cost below ``n * 1e-18 px^2`` counts as 0;
   the refined point is kept only if its cost is lower than the refit's.
6. Filter.  The inliers of the final point: at least 2 from at least 2 images, and a pair of them whose rays centre -> X have
   ``cos <= cos(min_tri_angle)``.  The inliers of a kept point take it; all else stays a candidate.
7. Rounds: steps 2 to 6 on the leftovers, at most ``max_rounds`` times, stopping when a round adds no point.
8. Order: points ascend by their smallest slot, ``point_ids = 1 .. Q``; a track's elements ascend by slot; ``point3D_ids`` is -1 on
   unassigned slots.

Errors, raised before any launch: shapes, dtypes, malformed offsets, non-finite inputs, ``det R`` not within 1e-6 of 1, a ``K`` of another
form, repeated image ids, a self-pair, options out of range -> ``ValueError``; an image index outside ``[0, I)`` or a match id outside
its image's keypoints -> ``IndexError``; CPU tensors -> :class:`hip.HipLibraryError` (no CPU fallback).  Host reads: one flag tensor for
the checks (the match ids included: their gathers are clamped, so they are computed whatever the other tables hold); per round the sizes of
the compacted tables (the candidates, the components of at least two candidates, those above one wavefront), which size the launches and
their outputs, and the number of points the round added; at the end the number of track elements.
"""
from __future__ import annotations

import math

import torch

from . import cabi, hip

_BINDING = cabi.Binding.of(__name__)                # the header is the one place a signature or a constant is written
library_path, load, check_arity, call = _BINDING.library_path, _BINDING.load, _BINDING.check_arity, _BINDING.call
launch = hip.launcher(_BINDING, globals())          # every stream-taking entry is called through it, by the header's parameter names
EXPORTED_SYMBOLS = _BINDING.exported_symbols
ABI_VERSION = _BINDING.abi_version
MAX_ITEMS, SHORT_TRACK, MAX_HYPOTHESES, MAX_REFINE_STEPS, MAX_ROUNDS, CAMERA_DOUBLES = map(_BINDING.constant, (
    "MAX_ITEMS", "SHORT_TRACK", "MAX_HYPOTHESES", "MAX_REFINE_STEPS", "MAX_ROUNDS", "CAMERA_DOUBLES"))
MERGED_KEYS = ("keypoints", "kpt_offsets", "match_ids", "pair_offsets", "pair_images")
CAMERA_KEYS = ("image_ids", "K", "R", "t")
DEFAULTS = {"max_reproj_error": 4.0, "min_tri_angle": 1.5, "max_hypotheses": 256, "refine_steps": 5, "max_rounds": 3}


def check_options(options: dict) -> dict:
    unknown = sorted(set(options) - set(DEFAULTS))
    if unknown:
        raise TypeError(f"unknown options {unknown}: {sorted(DEFAULTS)}")
    o = dict(DEFAULTS, **options)
    if not (math.isfinite(o["max_reproj_error"]) and o["max_reproj_error"] >= 0):
        raise ValueError("max_reproj_error: a finite number >= 0")
    if not (0 <= o["min_tri_angle"] <= 180):
        raise ValueError("min_tri_angle: degrees in [0, 180]")
    for k, hi in (("max_hypotheses", MAX_HYPOTHESES), ("max_rounds", MAX_ROUNDS)):
        if int(o[k]) != o[k] or not 1 <= o[k] <= hi:
            raise ValueError(f"{k}: an integer in [1, {hi}]")
    if int(o["refine_steps"]) != o["refine_steps"] or not 0 <= o["refine_steps"] <= MAX_REFINE_STEPS:
        raise ValueError(f"refine_steps: an integer in [0, {MAX_REFINE_STEPS}]")
    return o


# ---- the input checks -------------------------------------------------------------------------------------------------------------------
def check_inputs(merged: dict, cameras: dict) -> dict:
    """Every check of the module docstring, on tensors of any device -> the derived tables: ``I, U, T, P`` and ``slot_image [U]``,
    ``slot0``, ``slot1 [T]`` (the two slots every match row joins)"""
    missing = [k for k in MERGED_KEYS if k not in merged] + [k for k in CAMERA_KEYS if k not in cameras]
    if missing:
        raise ValueError(f"merged / cameras lack {missing}")
    m = {k: merged[k] for k in MERGED_KEYS}
    m.update({k: cameras[k] for k in CAMERA_KEYS})
    hip.need_tensors(m.items())
    i64, f64 = torch.int64, torch.float64
    I = m["image_ids"].shape[0] if m["image_ids"].dim() == 1 else -1
    U = m["keypoints"].shape[0] if m["keypoints"].dim() == 2 else -1
    T = m["match_ids"].shape[0] if m["match_ids"].dim() == 2 else -1
    P = m["pair_offsets"].shape[0] - 1 if m["pair_offsets"].dim() == 1 else -1
    if I < 1 or U < 1 or T < 0 or P < 0:
        raise ValueError("image_ids [I], keypoints [U, 2], match_ids [T, 2], pair_offsets [P + 1]: I >= 1, U >= 1")
    if max(U, T) > MAX_ITEMS:
        raise ValueError(f"at most {MAX_ITEMS} slots or match rows")
    for k, dtype, shape in (("keypoints", torch.float32, (U, 2)), ("kpt_offsets", i64, (I + 1,)), ("match_ids", i64, (T, 2)),
                            ("pair_offsets", i64, (P + 1,)), ("pair_images", i64, (P, 2)), ("image_ids", i64, (I,)), ("K", f64, (I, 3, 3)),
                            ("R", f64, (I, 3, 3)), ("t", f64, (I, 3))):
        if m[k].dtype != dtype or tuple(m[k].shape) != shape:
            raise ValueError(f"{k}: expected {dtype} {list(shape)}, got {m[k].dtype} {list(m[k].shape)}")
    dev = m["keypoints"].device
    if any(v.device != dev for v in m.values()):
        raise ValueError("the tensors lie on different devices")
    ko, po, pim, K, R = m["kpt_offsets"], m["pair_offsets"], m["pair_images"], m["K"], m["R"]
    n_kpt, n_row = ko[1:] - ko[:-1], po[1:] - po[:-1]
    sorted_iid = torch.sort(m["image_ids"]).values
    det = (R[:, 0, 0] * (R[:, 1, 1] * R[:, 2, 2] - R[:, 1, 2] * R[:, 2, 1]) - R[:, 0, 1] * (R[:, 1, 0] * R[:, 2, 2] - R[:, 1, 2] * R[:, 2, 0])
           + R[:, 0, 2] * (R[:, 1, 0] * R[:, 2, 1] - R[:, 1, 1] * R[:, 2, 0]))
    false = torch.zeros((), dtype=torch.bool, device=dev)
    # the match ids against their image's keypoints, computed whatever the tables hold: every index is clamped into its table first
    ids = m["match_ids"]
    if T and P:
        row_pair = torch.searchsorted(po[1:].contiguous(), torch.arange(T, device=dev), right=True).clamp(max=P - 1)     # po[p] <= row < po[p + 1]
        img = pim.clamp(0, I - 1)[row_pair]                                                            # [T, 2]
        bad_id = ((ids < 0) | (ids >= n_kpt[img])).any()
    else:
        img, bad_id = torch.zeros(0, 2, dtype=i64, device=dev), false
    flags = [ko[0] != 0, ko[-1] != U, (n_kpt < 0).any(),                                               # 0-2: kpt_offsets
             po[0] != 0, po[-1] != T, (n_row < 0).any(),                                               # 3-5: pair_offsets
             ~(torch.isfinite(m["keypoints"]).all() & torch.isfinite(K).all() & torch.isfinite(R).all() & torch.isfinite(m["t"]).all()),   # 6
             ~((det - 1).abs() <= 1e-6).all(),                                                         # 7
             ~((K[:, 1, 0] == 0) & (K[:, 2, 0] == 0) & (K[:, 2, 1] == 0) & (K[:, 2, 2] == 1) & (K[:, 0, 0] > 0) & (K[:, 1, 1] > 0)).all(),   # 8
             (sorted_iid[1:] == sorted_iid[:-1]).any(),                                                # 9
             ((pim < 0) | (pim >= I)).any() if P else false,                                           # 10
             (pim[:, 0] == pim[:, 1]).any() if P else false,                                           # 11
             bad_id]                                                                                   # 12: after all the others
    bad = torch.stack([f.to(torch.bool) for f in flags]).tolist()
    if bad[0] or bad[1] or bad[2]:
        raise ValueError(f"kpt_offsets: expected non-decreasing offsets from 0 to {U}")
    if bad[3] or bad[4] or bad[5]:
        raise ValueError(f"pair_offsets: expected non-decreasing offsets from 0 to {T}")
    if bad[6]:
        raise ValueError("non-finite keypoint, K, R or t")
    if bad[7]:
        raise ValueError("R: det R is not within 1e-6 of 1")
    if bad[8]:
        raise ValueError("K: expected [[fx, s, cx], [0, fy, cy], [0, 0, 1]] with fx, fy > 0")
    if bad[9]:
        raise ValueError("image_ids: an id occurs twice")
    if bad[10]:
        raise IndexError(f"pair_images: an image index lies outside [0, {I})")
    if bad[11]:
        raise ValueError("pair_images: a pair holds one image on both sides")
    if bad[12]:
        raise IndexError("match_ids: a keypoint id lies outside its image's keypoints (kpt_offsets)")
    slot_image = torch.repeat_interleave(torch.arange(I, device=dev), n_kpt, output_size=U)           # the offsets are sound by now
    slots = ko[img] + ids
    return {"I": I, "U": U, "T": T, "P": P, "slot_image": slot_image, "slot0": slots[:, 0].contiguous(), "slot1": slots[:, 1].contiguous()}


# ---- the stages ------------------------------------------------------------------------------------------------------------------------------
def components(slot0: torch.Tensor, slot1: torch.Tensor, U: int) -> torch.Tensor:
    """Step 1: ``labels [U]`` int64, the smallest slot of every slot's component"""
    dev = slot0.device
    parent = torch.arange(U, dtype=torch.int32, device=dev)
    labels = torch.empty(U, dtype=torch.int64, device=dev)
    launch("opstr_components", dict(slot0=slot0, slot1=slot1, T=slot0.numel(), U=U, parent=parent, labels=labels))
    return labels


def triangulate(merged: dict, cameras: dict, **options) -> dict:
    """The module docstring's ``triangulate``"""
    o = check_options(options)
    named = [(k, merged.get(k)) for k in MERGED_KEYS] + [(k, cameras.get(k)) for k in CAMERA_KEYS]
    if all(isinstance(t, torch.Tensor) for _, t in named):      # anything else is check_inputs' to report
        hip.on_device(t for _, t in named)
    d = check_inputs(merged, cameras)
    I, U = d["I"], d["U"]
    dev = merged["keypoints"].device
    i32, i64, f64 = torch.int32, torch.int64, torch.float64
    K, R, t = (cameras[k].contiguous() for k in ("K", "R", "t"))
    ko = merged["kpt_offsets"].contiguous()
    slot_image = d["slot_image"]
    xys = (merged["keypoints"].to(f64) + 0.5).contiguous()
    labels = components(d["slot0"], d["slot1"], U)
    cams = torch.empty(I, CAMERA_DOUBLES, dtype=f64, device=dev)
    dirs = torch.empty(U, 3, dtype=f64, device=dev)
    launch("opstr_prepare", dict(K=K, R=R, t=t, xys=xys, slot_image=slot_image, I=I, U=U, cameras=cams, dirs=dirs))
    assigned = torch.full((U,), -1, dtype=i64, device=dev)            # the round-local point number of every slot
    cos_min = math.cos(math.radians(o["min_tri_angle"]))
    kept_xyz, kept_err, kept_min, kept_num = [], [], [], []
    base, n_rounds = 0, 0
    for rnd in range(o["max_rounds"]):
        cand = torch.nonzero(assigned < 0).squeeze(1)                    # ascending slots
        lab, order = torch.sort(labels[cand], stable=True)
        elem_slot = cand[order].contiguous()
        comp_label, comp_of, counts = torch.unique_consecutive(lab, return_inverse=True, return_counts=True)
        several = counts >= 2                                            # a component of one candidate has no hypothesis: no workgroup for it
        elem_slot = elem_slot[several[comp_of]].contiguous()
        comp_label, counts = comp_label[several], counts[several]
        offsets = hip.exclusive(counts)
        long_comps = torch.nonzero(counts > SHORT_TRACK).squeeze(1).contiguous()
        C, n_elems, n_long = comp_label.numel(), elem_slot.numel(), long_comps.numel()     # read-back: sizes the launch and its outputs
        if C == 0:
            break
        n_rounds += 1
        ok = torch.zeros(C, dtype=i32, device=dev)
        xyz = torch.zeros(C, 3, dtype=f64, device=dev)
        err = torch.zeros(C, dtype=f64, device=dev)
        min_slot = torch.full((C,), -1, dtype=i64, device=dev)
        nbytes = load().opstr_workspace_bytes(n_elems) if n_long else 0
        ws = torch.empty(max(nbytes, 8), dtype=torch.uint8, device=dev)
        launch("opstr_round", dict(comp_offsets=offsets, comp_label=comp_label.contiguous(), elem_slot=elem_slot,
                                   long_comps=long_comps if n_long else None, C=C, n_long=n_long, n_elems=n_elems, slot_image=slot_image, xys=xys,
                                   cameras=cams, dirs=dirs, I=I, U=U, round=rnd, max_reproj_error=o["max_reproj_error"], cos_min_tri_angle=cos_min,
                                   max_hypotheses=o["max_hypotheses"], refine_steps=o["refine_steps"], point_base=base, workspace=ws,
                                   workspace_bytes=nbytes, ok=ok, xyz=xyz, point_error=err, min_slot=min_slot, assigned=assigned))
        keep = torch.nonzero(ok).squeeze(1)
        if keep.numel() == 0:                                            # read-back: the points this round added
            break
        kept_xyz.append(xyz[keep])
        kept_err.append(err[keep])
        kept_min.append(min_slot[keep])
        kept_num.append(keep + base)
        base += C
    model = {"image_ids": cameras["image_ids"], "kpt_offsets": ko, "xys": xys, "K": K, "R": R, "t": t, "labels": labels, "n_rounds": n_rounds}
    if kept_xyz:
        first, order = torch.sort(torch.cat(kept_min))                   # the smallest slots are distinct: points share no slot
        Q = first.numel()
        rank = torch.full((base,), -1, dtype=i64, device=dev)
        rank[torch.cat(kept_num)[order]] = torch.arange(Q, device=dev)
        slot_point = torch.where(assigned >= 0, rank[assigned.clamp(min=0)], torch.full_like(assigned, -1))
        elems = torch.nonzero(slot_point >= 0).squeeze(1)
        point_of, by_point = torch.sort(slot_point[elems], stable=True)  # a track's elements ascend by slot
        elems = elems[by_point]
        track_image = slot_image[elems]
        model.update(point_ids=torch.arange(1, Q + 1, dtype=i64, device=dev), xyz=torch.cat(kept_xyz)[order].contiguous(),
                     point_error=torch.cat(kept_err)[order].contiguous(), point3D_ids=slot_point + (slot_point >= 0).to(i64),
                     track_offsets=hip.exclusive(torch.bincount(point_of, minlength=Q)), track_image=track_image,
                     track_kpt=elems - ko[track_image])
    else:
        model.update(point_ids=torch.zeros(0, dtype=i64, device=dev), xyz=torch.zeros(0, 3, dtype=f64, device=dev),
                     point_error=torch.zeros(0, dtype=f64, device=dev), point3D_ids=torch.full((U,), -1, dtype=i64, device=dev),
                     track_offsets=torch.zeros(1, dtype=i64, device=dev), track_image=torch.zeros(0, dtype=i64, device=dev),
                     track_kpt=torch.zeros(0, dtype=i64, device=dev))
    return model
