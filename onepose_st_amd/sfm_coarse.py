"""Keypoint-free SfM coarse matching: pair matches -> 2D keypoints per image and match indices, on the device.

The reference's ``detector_free_coarse_matching`` (src/KeypointFreeSfM/coarse_match/coarse_match.py:35-215, non-Ray branch :141-186)
runs the coarse-only LoFTR matcher on every covisible pair, then merges all pair matches in Python dicts keyed by coordinate tuples.
Here the merge is HIP (``csrc/sfm_points2d.hip``) and the matcher calls are batched.

The merge's contract (``merge_pair_matches``), bit-exact against the reference's four steps:

* Inputs: the reference's ``matches`` dict in its iteration order, flat -- ``P`` pairs ``(img0[p], img1[p])`` over ``I`` images, pair
  ``p`` owning rows ``pair_offsets[p] : pair_offsets[p + 1]``, per row ``mkpts0 [T, 2]``, ``mkpts1 [T, 2]``, ``mconf [T]`` float32 (the
  columns of the reference's ``(N, 5)`` arrays).
* Observations: row ``t`` of pair ``p`` gives ``(img0[p], mkpts0[t], mconf[t])`` and ``(img1[p], mkpts1[t], mconf[t])``.  Within one
  image they come in Match2Pts2D's order (utils.py:20-61): pairs in order, rows in order -- ascending global row, as no pair holds one
  image twice.
* Keys and scores (points2D_worker / agg_groupby_2d "sum", coarse_match_worker.py:87-111, utils.py:5-18): the key of an observation is
  ``(int(x), int(y))``, truncated toward zero like numpy's ``astype(int)`` (-0.5 -> 0, 7.9999995 -> 7); its score is the float64 sum of
  its observations' ``mconf`` added one after another in occurrence order (``np.bincount``).  The order matters for arbitrary float32
  inputs: 1.0 + 2^-30 + 2^-60 depends on it.
* Ranking: per image, score descending; equal scores keep ``np.unique(axis=0)``'s order, signed (x, y) lexicographic ascending (Python's
  ``sorted(..., reverse=True)`` is stable).  The rank is the keypoint id.
* Outputs (transform_points2D / update_matches, coarse_match_worker.py:119-183): per image ``keypoints [n_g, 2]`` float32 (x, y) in rank
  order and ``scores [n_g]`` = float32(sum), concatenated image after image with ``kpt_offsets [I + 1]``; per row ``match_ids [T, 2]``
  int64 = the rank of the row's key in ``img0[p]`` and in ``img1[p]``.  A pair with no rows has no ids.
* Errors, raised before any launch: an image with no observation raises ``AssertionError("corner-case n_kpts=0 not handled.")`` (the
  reference's transform_points2D assert); a self-pair, non-finite coordinates or scores, a truncated coordinate with
  ``|int(.)| >= 2^20`` (``COORD_LIMIT``: far beyond any image this project matches), malformed offsets or shapes raise ``ValueError``;
  an image index outside ``[0, I)`` raises ``IndexError``; CPU tensors raise :class:`hip.HipLibraryError`.

The pair order the caller passes IS the reference's dict order: it decides the float64 summation order.  The reference's
``random.shuffle`` of the pair list and its h5 files stay with the caller (h5py is not a dependency).  The merge's result, with
``pair_images`` added, is what ``sfm_triangulate.triangulate`` takes.
"""
from __future__ import annotations

import copy
from collections import OrderedDict

import numpy as np
import torch

from . import hip

COORD_LIMIT = 1 << 20                   # |int(x)|, |int(y)| < 2^20 (csrc/sfm_points2d.hip packs x + 2^20 into 21 bits)
MAX_ROWS = (1 << 30) - 1                # OPHIP_SFM_POINTS2D_MAX_ROWS
MAX_IMAGES = 1 << 22                    # OPHIP_SFM_POINTS2D_MAX_IMAGES


def check_inputs(mkpts0: torch.Tensor, mkpts1: torch.Tensor, mconf: torch.Tensor, pair_offsets: torch.Tensor, pair_images: torch.Tensor,
                 n_images: int):
    """``merge_pair_matches``' input checks, on tensors of any device (the errors of the module docstring) -> (T, P, I)"""
    hip.need_tensors((("mkpts0", mkpts0), ("mkpts1", mkpts1), ("mconf", mconf), ("pair_offsets", pair_offsets), ("pair_images", pair_images)))
    I = int(n_images)
    T = mconf.shape[0] if mconf.dim() == 1 else -1
    for name, t, shape in (("mkpts0", mkpts0, (T, 2)), ("mkpts1", mkpts1, (T, 2)), ("mconf", mconf, (T,))):
        if t.dtype != torch.float32 or tuple(t.shape) != shape:
            raise ValueError(f"{name}: expected float32 {list(shape)}, got {t.dtype} {list(t.shape)}")
    if pair_offsets.dtype != torch.int64 or pair_offsets.dim() != 1 or pair_offsets.numel() < 1:
        raise ValueError("pair_offsets: expected int64 [P + 1]")
    P = pair_offsets.numel() - 1
    if pair_images.dtype != torch.int64 or tuple(pair_images.shape) != (P, 2):
        raise ValueError(f"pair_images: expected int64 [{P}, 2]")
    if I < 1 or I > MAX_IMAGES:
        raise ValueError(f"n_images: {I} outside [1, {MAX_IMAGES}]")
    if T > MAX_ROWS:
        raise ValueError(f"{T} rows: at most {MAX_ROWS}")
    off = pair_offsets.cpu().numpy()
    pim = pair_images.cpu().numpy()
    if off[0] != 0 or off[-1] != T or (np.diff(off) < 0).any():
        raise ValueError(f"pair_offsets: expected non-decreasing offsets from 0 to {T}")
    if P and (pim.min() < 0 or pim.max() >= I):
        raise IndexError(f"pair_images: image index outside [0, {I})")
    if (pim[:, 0] == pim[:, 1]).any():
        raise ValueError(f"pair {int(np.argmax(pim[:, 0] == pim[:, 1]))} holds one image on both sides")
    seen = np.zeros(I, bool)
    seen[pim[np.diff(off) > 0].reshape(-1)] = True
    if not seen.all():
        raise AssertionError("corner-case n_kpts=0 not handled.")
    with torch.no_grad():
        bad = torch.stack([~torch.isfinite(mkpts0).all() | ~torch.isfinite(mkpts1).all(), ~torch.isfinite(mconf).all(),
                           (mkpts0.trunc().abs() >= COORD_LIMIT).any() | (mkpts1.trunc().abs() >= COORD_LIMIT).any()]).tolist()
    if bad[0] or bad[1]:
        raise ValueError("non-finite keypoint coordinate or score")
    if bad[2]:
        raise ValueError(f"a keypoint coordinate truncates outside (-{COORD_LIMIT}, {COORD_LIMIT})")
    return T, P, I


def merge_pair_matches(mkpts0: torch.Tensor, mkpts1: torch.Tensor, mconf: torch.Tensor, pair_offsets: torch.Tensor,
                       pair_images: torch.Tensor, n_images: int) -> dict:
    """The merge of the module docstring.  Device tensors in, device tensors out:
    ``{"keypoints" [U, 2] float32, "scores" [U] float32, "kpt_offsets" [I + 1] int64, "match_ids" [T, 2] int64,
    "pair_offsets" [P + 1] int64}`` (the last one as given).  Host reads: the small pair tables, one flag tensor of the input checks and
    the unique-key total."""
    for name, t in (("mkpts0", mkpts0), ("mkpts1", mkpts1), ("mconf", mconf), ("pair_offsets", pair_offsets), ("pair_images", pair_images)):
        hip.need_device([(name, t)])                # one at a time: the first input that is wrong in either way is the one reported
    T, P, I = check_inputs(mkpts0, mkpts1, mconf, pair_offsets, pair_images, n_images)

    lib = hip.load()
    dev = mconf.device
    nbytes = lib.ophip_sfm_points2d_workspace_bytes(T, I)
    ws = torch.empty(nbytes, dtype=torch.uint8, device=dev)
    ucount = torch.zeros(1, dtype=torch.int32, device=dev)
    mk0, mk1, mc = mkpts0.contiguous(), mkpts1.contiguous(), mconf.contiguous()
    po, pi = pair_offsets.contiguous(), pair_images.contiguous()
    hip.launch("ophip_sfm_points2d_group", dict(mkpts0=mk0, mkpts1=mk1, pair_offsets=po, pair_images=pi, P=P, T=T, I=I, workspace=ws,
                                                workspace_bytes=nbytes, unique_count=ucount))
    U = int(ucount.item())                                     # the one read-back: it sizes the outputs
    keypoints = torch.empty(U, 2, dtype=torch.float32, device=dev)
    scores = torch.empty(U, dtype=torch.float32, device=dev)
    kpt_offsets = torch.empty(I + 1, dtype=torch.int64, device=dev)
    match_ids = torch.empty(T, 2, dtype=torch.int64, device=dev)
    hip.launch("ophip_sfm_points2d_rank", dict(mconf=mc, T=T, I=I, U=U, workspace=ws, workspace_bytes=nbytes, keypoints=keypoints, scores=scores,
                                               kpt_offsets=kpt_offsets, match_ids=match_ids))
    return {"keypoints": keypoints, "scores": scores, "kpt_offsets": kpt_offsets, "match_ids": match_ids, "pair_offsets": pair_offsets}


def _pair_key(pair) -> str:
    return pair if isinstance(pair, str) else " ".join(pair)


def to_reference_outputs(result: dict, names, pair_names):
    """``merge_pair_matches``' result -> the reference's ``final_keypoints`` / ``final_scores`` ``{name: ndarray}`` and
    ``updated_matches`` ``{"name0 name1": [m, 2] int64}`` (``pair_names``: ``(name0, name1)`` tuples or ``"name0 name1"`` strings, in
    pair order)."""
    kp = result["keypoints"].cpu().numpy()
    sc = result["scores"].cpu().numpy()
    ko = result["kpt_offsets"].cpu().numpy()
    ids = result["match_ids"].cpu().numpy()
    po = result["pair_offsets"].cpu().numpy()
    if len(ko) != len(names) + 1 or len(po) != len(pair_names) + 1:
        raise ValueError("names / pair_names do not match the result")
    final_keypoints = {n: kp[ko[g]:ko[g + 1]] for g, n in enumerate(names)}
    final_scores = {n: sc[ko[g]:ko[g + 1]] for g, n in enumerate(names)}
    updated_matches = {_pair_key(p): ids[po[i]:po[i + 1]].reshape(-1, 2) for i, p in enumerate(pair_names)}
    return final_keypoints, final_scores, updated_matches


# ---- the matcher over a pair list -----------------------------------------------------------------------------------------------------
def build_model(state_dict: dict, config: dict | None = None):
    """the reference's ``build_model`` (coarse_match_worker.py:18-29): ``LoFTR_for_OnePose_Plus(config, enable_fine_matching=False)``,
    ``matcher.``-prefixed keys stripped, loaded with ``strict=True``, eval mode (move it to the device yourself)"""
    from .loftr import LoFTR_for_OnePose_Plus, default_cfg
    from .params import load_matcher_checkpoint

    return load_matcher_checkpoint(LoFTR_for_OnePose_Plus(copy.deepcopy(config or default_cfg), enable_fine_matching=False), state_dict)


@torch.no_grad()
def match_pairs(matcher, images, pairs, max_batch: int = 16) -> dict:
    """The coarse-only matcher over ``pairs`` (``(i0, i1)`` indices into ``images``; ``images[i]`` = ``(image [1, 1, H, W], scale [1, 2]
    float32)`` on the device, the caller's resized image and its [h, w] factors, as the reference's dataset hands them over).

    Pairs whose two image sizes agree are batched, at most ``max_batch`` per call: ``image0 [V] / image1 [V]``, ``scale0 / scale1 [V, 2]``.
    The matches of a call come out in ascending (pair, cell) order; they are split by ``b_ids`` and put back into the caller's pair order
    on the device.  The only host reads are each call's match count, which the matcher reads anyway.

    -> ``{"mkpts0" [T, 2], "mkpts1" [T, 2], "mconf" [T]`` (float32), ``"pair_offsets" [P + 1]``, ``"pair_images" [P, 2]`` (int64)``}``: the
    inputs of ``merge_pair_matches``."""
    if getattr(matcher, "enable_fine_matching", True):
        raise ValueError("match_pairs runs the coarse-only matcher: build it with enable_fine_matching=False (sfm_coarse.build_model)")
    if max_batch < 1:
        raise ValueError("max_batch >= 1")
    pairs = [(int(a), int(b)) for a, b in pairs]
    if not pairs:
        raise ValueError("no pairs")
    for a, b in pairs:
        if not (0 <= a < len(images) and 0 <= b < len(images)):
            raise IndexError(f"pair ({a}, {b}): image index outside [0, {len(images)})")
    for img, s in images:
        hip.on_device((img, s))
        if img.dim() != 4 or img.shape[:2] != (1, 1) or s.dtype != torch.float32 or tuple(s.shape) != (1, 2):
            raise ValueError("images: (tensor [1, 1, H, W], scale float32 [1, 2]) per image")
    dev = images[pairs[0][0]][0].device
    P = len(pairs)
    groups = OrderedDict()                                     # (size0, size1) -> pair indices, in first-appearance order
    for p, (a, b) in enumerate(pairs):
        groups.setdefault((tuple(images[a][0].shape[2:]), tuple(images[b][0].shape[2:])), []).append(p)
    # only the match lists leave this function: a dual-softmax matcher need not store conf_matrix (sinkhorn's entry point requires it)
    kw = {"conf_matrix": "lazy"} if not getattr(matcher, "sinkhorn", False) else {}
    calls = []
    pair_counts = torch.zeros(P, dtype=torch.int64, device=dev)
    T = 0
    for members in groups.values():
        for c in range(0, len(members), max_batch):
            ps = members[c:c + max_batch]
            V = len(ps)
            data = {"image0": torch.cat([images[pairs[p][0]][0] for p in ps], 0),
                    "image1": torch.cat([images[pairs[p][1]][0] for p in ps], 0),
                    "scale0": torch.cat([images[pairs[p][0]][1] for p in ps], 0).contiguous(),
                    "scale1": torch.cat([images[pairs[p][1]][1] for p in ps], 0).contiguous()}
            matcher(data, **kw)
            b_ids = data["b_ids"]
            K = b_ids.shape[0]                                 # the matcher read its count on the host
            counts = torch.zeros(V, dtype=torch.int64, device=dev).index_add_(0, b_ids, torch.ones_like(b_ids))
            pid = torch.tensor(ps, dtype=torch.int64, device=dev)
            pair_counts[pid] = counts
            calls.append((pid, b_ids, counts, data["mkpts0_f"], data["mkpts1_f"], data["mconf"], K))
            T += K
    pair_offsets = torch.cat([torch.zeros(1, dtype=torch.int64, device=dev), torch.cumsum(pair_counts, 0)])
    mk0 = torch.empty(T, 2, dtype=torch.float32, device=dev)
    mk1 = torch.empty(T, 2, dtype=torch.float32, device=dev)
    conf = torch.empty(T, dtype=torch.float32, device=dev)
    for pid, b_ids, counts, m0, m1, mc, K in calls:
        if K == 0:
            continue
        first = torch.cumsum(counts, 0) - counts               # the call's first row of every pair
        dst = pair_offsets[pid[b_ids]] + (torch.arange(K, device=dev) - first[b_ids])
        mk0[dst] = m0.float()
        mk1[dst] = m1.float()
        conf[dst] = mc.float()
    pair_images = torch.tensor(pairs, dtype=torch.int64, device=dev).reshape(P, 2)
    return {"mkpts0": mk0, "mkpts1": mk1, "mconf": conf, "pair_offsets": pair_offsets, "pair_images": pair_images}


def detector_free_coarse_matching(matcher, names, images, pairs, max_batch: int = 16):
    """``match_pairs`` then ``merge_pair_matches``: the reference's ``(final_keypoints, updated_matches)`` (coarse_match.py:141-186
    and :215) -- ``{name: [n, 2] float32}`` and ``{"name0 name1": [m, 2] int64}``.  ``images`` align with ``names``; ``pairs`` are
    ``(i0, i1)`` indices into them, in the order that is the reference's dict order."""
    if len(images) != len(names):
        raise ValueError("one image per name")
    m = match_pairs(matcher, images, pairs, max_batch=max_batch)
    res = merge_pair_matches(m["mkpts0"], m["mkpts1"], m["mconf"], m["pair_offsets"], m["pair_images"], len(names))
    final_keypoints, _, updated_matches = to_reference_outputs(res, names, [(names[a], names[b]) for a, b in pairs])
    return final_keypoints, updated_matches
