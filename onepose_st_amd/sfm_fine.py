"""Keypoint-free SfM fine matching: refine a whole pair list from one feature bank, on the device.

The reference refines the coarse matches of a model one pair at a time (``matchWorker``, post_optimization/matcher_model/
fine_match_worker.py): ``LoFTR_for_OnePose_Plus.forward`` with ``mkpts0_c`` / ``mkpts1_c``, ``scale0`` / ``scale1``,
``extract_coarse_feature=True`` and ``extract_fine_feature=True``, which runs the backbone on both images of every pair again, and a
copy of every result to the host.  Here the backbone runs once per image and every pair row reads the maps of its own two images:

1. ``build_feature_bank(matcher, images, scales=None, max_batch=16, max_bytes=None) -> bank``: the HIP backbone over all images, in
   batches of at most ``max_batch`` images of equal size.  Images of one size form a size group, in the order the sizes first occur;
   a group holds the fine maps ``fine [n, hf * wf, 128]`` and the coarse maps before the positional encoding ``coarse [n, hc * wc,
   256]`` of its images as two contiguous float32 tensors.  Per image: ``image_group``, ``image_index`` (within the group) ``[I]``
   int64, ``image_hw [I, 2]`` int32 (H, W), ``scales [I, 2]`` float32 (the reference's ``scale`` of each image, default ones), all on
   the device; ``n_images``, ``bytes`` (the maps' size; with ``max_bytes`` a larger bank raises ``ValueError`` before anything runs).
2. ``fine_match_pairs(matcher, bank, pairs, chunk_rows=8192) -> result``: ``pairs`` is the dict of ``sfm_tracks.matching_pairs`` or any
   dict with the device tensors ``mkpts0_c``, ``mkpts1_c [M, 2]`` (float32 or float64) and ``row_left``, ``row_right [M]`` (int64 image
   indices).  One ``opsff_row_ids`` launch clips all keypoints into copies and rounds them to cells; the rows are then processed in
   chunks of at most ``chunk_rows`` (a boundary may fall inside a pair), within a chunk in buckets of equal (size group of the left
   image, size group of the right image): ``ophip_fine2_gather_b`` on each side with the image's index within its group, the fine
   transformer as the matcher's config says, ``ophip_fine2_match_scaled`` with the right image's row of the scale table, and one
   ``opsff_sample_rows`` launch for the four feature tables.  Result, one row per pair row in the input order, on the device:
   ``mkpts0_c``, ``mkpts1_c`` (the clipped copies, input dtype), ``mkpts0_f`` (the same tensor as ``mkpts0_c``), ``mkpts1_f`` (the dtype
   of ``mkpts1_c``), ``expec_f [M, 3]``, ``i_ids``, ``j_ids``, ``feature_c0``, ``feature_c1 [M, 256]``, ``feature0``, ``feature1 [M, 128]``.

   The caller's ``mkpts0_c`` / ``mkpts1_c`` are NOT modified: the per-pair call clips the caller's tensors in place, this one returns
   clipped copies.

   Host reads per call: the control words of the ids kernel (bad-id count and first bad row), and, when the bank holds more than one
   size group, the rows' bucket keys in one copy; neither grows with the number of pairs.
3. ``to_reference_outputs(result, pairs, model, scales=None)``: the ``results_dict`` of the reference's ``matchWorker``, numpy.

Errors: a keypoint that rounds to a cell outside its image's coarse grid -> ``IndexError`` naming the count and the first such row,
before any fine work (the per-pair call's behaviour); an image index outside the bank -> ``IndexError``; wrong dtypes or shapes,
unequal lengths -> ``ValueError``; not a tensor -> ``TypeError``; a matcher with a ``feature_hook`` (its coarse rows carry the
positional encoding) or without fine matching -> ``NotImplementedError``; host tensors -> :class:`hip.HipLibraryError` (no CPU
fallback).  ``M == 0`` returns empty tensors of the right shapes and dtypes.
"""
from __future__ import annotations

import numpy as np
import torch

from . import cabi, hip
from .backbone_hip import HipBackbone

_BINDING = cabi.Binding.of(__name__)                # the header is the one place a signature or a constant is written
library_path, load, check_arity, call = _BINDING.library_path, _BINDING.load, _BINDING.check_arity, _BINDING.call
launch = hip.launcher(_BINDING, globals())          # every stream-taking entry is called through it, by the header's parameter names
EXPORTED_SYMBOLS = _BINDING.exported_symbols
ABI_VERSION = _BINDING.abi_version
MAX_ROWS, CTRL_INTS, NO_ROW = map(_BINDING.constant, ("MAX_ROWS", "CTRL_INTS", "NO_ROW"))
COARSE_SCALE = 8.0                                  # image rows per coarse row (ResNetFPN 8 -> 2)
PAIR_KEYS = ("mkpts0_c", "mkpts1_c", "row_left", "row_right")
RESULT_KEYS = ("mkpts0_c", "mkpts1_c", "mkpts0_f", "mkpts1_f", "expec_f", "i_ids", "j_ids", "feature_c0", "feature_c1", "feature0", "feature1")
REFERENCE_KEYS = ("mkpts0_c", "mkpts1_c", "mkpts0_f", "mkpts1_f", "mkpts0_idx", "scale0", "scale1", "feature_c0", "feature_c1", "feature0",
                  "feature1")


def _check_matcher(matcher):
    if getattr(matcher, "feature_hook", None) is not None:
        raise NotImplementedError("a matcher with a feature_hook: the hook's coarse rows carry the positional encoding, the feature "
                                  "bank keeps the map before it")
    if not matcher.enable_fine_matching:
        raise NotImplementedError("a matcher without fine matching has nothing to refine")
    if matcher.training:
        raise NotImplementedError("inference only")
    if getattr(matcher, "fine_context", False):
        from .loftr import FINE_ONLY_WITH_CONTEXT
        raise NotImplementedError(FINE_ONLY_WITH_CONTEXT)


# ---- 1. the feature bank ----------------------------------------------------------------------------------------------------------------
def bank_bytes(sizes) -> int:
    """float32 bytes of the fine and the coarse maps of images of the given ``(H, W)`` sizes"""
    return sum(4 * ((H // 2) * (W // 2) * 128 + (H // 8) * (W // 8) * 256) for H, W in sizes)


def _image_list(images) -> list:
    if isinstance(images, torch.Tensor):
        if images.dim() != 4 or images.shape[1] != 1:
            raise ValueError(f"images: a tensor [I, 1, H, W], got {list(images.shape)}")
        images = list(images)
    out = []
    for n, img in enumerate(images):
        hip.need_tensors([(f"images[{n}]", img)])
        if img.dim() not in (2, 3, 4) or any(s != 1 for s in img.shape[:-2]):
            raise ValueError(f"images[{n}]: one grey image [H, W], [1, H, W] or [1, 1, H, W], got {list(img.shape)}")
        H, W = img.shape[-2:]
        if H < 8 or W < 8 or H % 8 or W % 8:
            raise ValueError(f"images[{n}]: H and W must be multiples of 8, got {H} x {W}")
        out.append(img.reshape(1, 1, H, W))
    if not out:
        raise ValueError("images: empty")
    return out


@torch.no_grad()
def build_feature_bank(matcher, images, scales=None, max_batch: int = 16, max_bytes: int | None = None) -> dict:
    """Section 1 of the module docstring -> the bank"""
    _check_matcher(matcher)
    imgs = _image_list(images)
    I = len(imgs)
    if isinstance(max_batch, bool) or not isinstance(max_batch, int) or max_batch < 1:
        raise ValueError("max_batch: an int >= 1")
    if scales is not None:
        hip.need_tensors([("scales", scales)])
        if scales.dtype != torch.float32 or tuple(scales.shape) != (I, 2):
            raise ValueError(f"scales: expected float32 [{I}, 2], got {scales.dtype} {list(scales.shape)}")
    sizes = [tuple(int(s) for s in img.shape[-2:]) for img in imgs]
    total = bank_bytes(sizes)
    if max_bytes is not None and total > max_bytes:
        raise ValueError(f"the feature bank of {I} images takes {total} bytes, more than max_bytes = {max_bytes}")
    if not all(t.is_cuda for t in imgs) or (scales is not None and not scales.is_cuda):
        raise hip.HipLibraryError("the feature bank is built on the HIP device only (no CPU fallback)")
    hip.load()
    dev = imgs[0].device
    Wb = matcher._blocks(dev)
    bbk = HipBackbone("bf16x3")
    members = {}                                                           # size -> image indices, sizes in first-occurrence order
    for n, hw in enumerate(sizes):
        members.setdefault(hw, []).append(n)
    image_group, image_index, groups = [0] * I, [0] * I, []
    for g, ((H, W), idx) in enumerate(members.items()):
        fine = torch.empty(len(idx), (H // 2) * (W // 2), 128, device=dev)
        coarse = torch.empty(len(idx), (H // 8) * (W // 8), 256, device=dev)
        for a in range(0, len(idx), max_batch):
            part = idx[a:a + max_batch]
            batch = torch.cat([imgs[n] for n in part], 0)
            fm, ff = bbk.forward(Wb["backbone"], batch)                    # no table: the coarse map before the positional encoding
            coarse[a:a + len(part)].copy_(fm)
            fine[a:a + len(part)].copy_(ff)
        for k, n in enumerate(idx):
            image_group[n], image_index[n] = g, k
        groups.append({"hw": (H, W), "images": list(idx), "fine": fine, "coarse": coarse})
    return {"n_images": I, "groups": groups, "bytes": total,
            "image_group": torch.tensor(image_group, dtype=torch.int64, device=dev),
            "image_index": torch.tensor(image_index, dtype=torch.int64, device=dev),
            "image_hw": torch.tensor(sizes, dtype=torch.int32, device=dev),
            "scales": (torch.ones(I, 2, device=dev) if scales is None else scales.to(dev).contiguous())}


# ---- 2. the chunk / bucket planner --------------------------------------------------------------------------------------------------------
def plan_chunks(M: int, chunk_rows: int, keys=None) -> list:
    """Rows ``0 .. M - 1`` in chunks of at most ``chunk_rows`` consecutive rows (a boundary may fall inside a pair); within a chunk the
    rows of equal bucket key (``keys [M]`` ints; ``None``: one bucket) form a bucket, buckets in ascending key order, rows ascending.
    -> ``[(start, stop, [(key, rows), ...]), ...]`` with ``rows`` a numpy int64 array.  Pure host code."""
    if isinstance(chunk_rows, bool) or not isinstance(chunk_rows, (int, np.integer)) or chunk_rows < 1:
        raise ValueError("chunk_rows: an int >= 1")
    if M < 0:
        raise ValueError("M: a row count")
    if keys is not None:
        keys = np.asarray(keys, dtype=np.int64).reshape(-1)
        if keys.shape[0] != M:
            raise ValueError(f"keys: expected {M} entries, got {keys.shape[0]}")
    chunks = []
    for a in range(0, M, int(chunk_rows)):
        b = min(M, a + int(chunk_rows))
        if keys is None:
            buckets = [(0, np.arange(a, b, dtype=np.int64))]
        else:
            part = keys[a:b]
            buckets = [(int(k), a + np.nonzero(part == k)[0].astype(np.int64)) for k in np.unique(part)]
        chunks.append((a, b, buckets))
    return chunks


# ---- 3. the pair rows ---------------------------------------------------------------------------------------------------------------------
def check_pairs(pairs: dict, n_images: int, ranges: bool = True) -> int:
    """The input checks of the module docstring, on tensors of any device -> M.  ``ranges``: also that every image index lies in the
    bank (one host read; ``fine_match_pairs`` leaves it to the ids kernel, which counts such rows)."""
    missing = [k for k in PAIR_KEYS if k not in pairs]
    if missing:
        raise ValueError(f"pairs lacks {missing}")
    hip.need_tensors((f"pairs[{k!r}]", pairs[k]) for k in PAIR_KEYS)
    M = pairs["mkpts0_c"].shape[0] if pairs["mkpts0_c"].dim() == 2 else -1
    for k in ("mkpts0_c", "mkpts1_c"):
        t = pairs[k]
        if t.dtype not in (torch.float32, torch.float64) or t.dim() != 2 or t.shape[1] != 2:
            raise ValueError(f"pairs[{k!r}]: expected float32 or float64 [M, 2], got {t.dtype} {list(t.shape)}")
    for k in ("mkpts1_c", "row_left", "row_right"):
        if pairs[k].shape[0] != M:
            raise ValueError(f"pairs[{k!r}]: {pairs[k].shape[0]} rows, mkpts0_c has {M} (unequal lengths)")
    for k in ("row_left", "row_right"):
        t = pairs[k]
        if t.dtype != torch.int64 or t.dim() != 1:
            raise ValueError(f"pairs[{k!r}]: expected int64 [M], got {t.dtype} {list(t.shape)}")
    if M > MAX_ROWS:
        raise ValueError(f"{M} pair rows: at most {MAX_ROWS}")
    if any(pairs[k].device != pairs["mkpts0_c"].device for k in PAIR_KEYS):
        raise ValueError("the pairs' tensors lie on different devices")
    if ranges and M:
        _raise_for_image_index(pairs, n_images)
    return M


def _raise_for_image_index(pairs, n_images):
    for k in ("row_left", "row_right"):
        bad = torch.nonzero((pairs[k] < 0) | (pairs[k] >= n_images))
        if bad.numel():
            r = int(bad[0, 0])
            raise IndexError(f"pairs[{k!r}][{r}] = {int(pairs[k][r])}: the bank holds images 0 .. {n_images - 1}")


def row_ids(bank: dict, mkpts0_c, mkpts1_c, row_left, row_right) -> tuple:
    """``opsff_row_ids`` on contiguous device tensors -> ``(mkpts0_c clipped, mkpts1_c clipped, i_ids, j_ids, ctrl [2] int32)``;
    nothing is read back"""
    M, dev = mkpts0_c.shape[0], mkpts0_c.device
    out0, out1 = torch.empty_like(mkpts0_c), torch.empty_like(mkpts1_c)
    i_ids, j_ids = torch.empty(M, dtype=torch.int64, device=dev), torch.empty(M, dtype=torch.int64, device=dev)
    ctrl = torch.empty(CTRL_INTS, dtype=torch.int32, device=dev)
    launch("opsff_row_ids", dict(mkpts0=mkpts0_c, mk0_double=mkpts0_c.dtype == torch.float64, mkpts1=mkpts1_c,
                                 mk1_double=mkpts1_c.dtype == torch.float64, row_left=row_left, row_right=row_right, image_hw=bank["image_hw"],
                                 image_scale=bank["scales"], I=bank["n_images"], M=M, coarse_scale=COARSE_SCALE, mkpts0_out=out0, mkpts1_out=out1,
                                 i_ids=i_ids, j_ids=j_ids, ctrl=ctrl))
    return out0, out1, i_ids, j_ids, ctrl


def sample_rows(bank: dict, g0: int, g1: int, mkpts0, mkpts1, row_left, row_right, rows, row0: int, n: int, feature_c0, feature_c1,
                feature0, feature1) -> None:
    """``opsff_sample_rows``: the four feature tables of the rows ``rows`` (a device int64 tensor, or ``None``: ``row0 .. row0 + n``),
    whose left images lie in size group ``g0`` and right images in ``g1``, written at those rows of the ``[M, C]`` outputs"""
    G0, G1 = bank["groups"][g0], bank["groups"][g1]
    launch("opsff_sample_rows", dict(coarse0=G0["coarse"], coarse0_bstride=G0["coarse"].stride(0), fine0=G0["fine"],
                                     fine0_bstride=G0["fine"].stride(0), n_group0=G0["fine"].shape[0], H0=G0["hw"][0], W0=G0["hw"][1],
                                     coarse1=G1["coarse"], coarse1_bstride=G1["coarse"].stride(0), fine1=G1["fine"],
                                     fine1_bstride=G1["fine"].stride(0), n_group1=G1["fine"].shape[0], H1=G1["hw"][0], W1=G1["hw"][1],
                                     mkpts0=mkpts0, mk0_double=mkpts0.dtype == torch.float64, mkpts1=mkpts1,
                                     mk1_double=mkpts1.dtype == torch.float64, row_left=row_left, row_right=row_right,
                                     image_index=bank["image_index"], image_scale=bank["scales"], I=bank["n_images"], rows=rows, row0=row0, n=n,
                                     M=mkpts0.shape[0], feature_c0=feature_c0, feature_c1=feature_c1, feature0=feature0, feature1=feature1))


@torch.no_grad()
def fine_match_pairs(matcher, bank: dict, pairs: dict, chunk_rows: int = 8192) -> dict:
    """Section 2 of the module docstring -> the result"""
    _check_matcher(matcher)
    I = bank["n_images"]
    M = check_pairs(pairs, I, ranges=False)
    if isinstance(chunk_rows, bool) or not isinstance(chunk_rows, int) or chunk_rows < 1:
        raise ValueError("chunk_rows: an int >= 1")
    if not all(pairs[k].is_cuda for k in PAIR_KEYS):
        raise hip.HipLibraryError("fine_match_pairs runs on the HIP device only (no CPU fallback)")
    hip.load()
    dev = pairs["mkpts0_c"].device
    in0, in1 = pairs["mkpts0_c"].contiguous(), pairs["mkpts1_c"].contiguous()
    left, right = pairs["row_left"].contiguous(), pairs["row_right"].contiguous()
    mk0, mk1, i_ids, j_ids, ctrl = row_ids(bank, in0, in1, left, right)
    out = {"mkpts0_c": mk0, "mkpts1_c": mk1, "mkpts0_f": mk0, "mkpts1_f": torch.empty_like(mk1), "expec_f": torch.empty(M, 3, device=dev),
           "i_ids": i_ids, "j_ids": j_ids, "feature_c0": torch.empty(M, 256, device=dev), "feature_c1": torch.empty(M, 256, device=dev),
           "feature0": torch.empty(M, 128, device=dev), "feature1": torch.empty(M, 128, device=dev)}
    if M == 0:
        return out
    nbad, first = ctrl.tolist()                                            # the one read-back of every call
    if nbad:
        _raise_for_image_index(pairs, I)                                   # the error path may read more
        raise IndexError(f"{nbad} provided coarse keypoint(s) round to a cell outside the coarse grid of their image; the first is in "
                         f"row {first} (images {int(left[first])} and {int(right[first])})")
    groups = bank["groups"]
    G = len(groups)
    keys = None
    if G > 1:                                                              # one copy of the rows' bucket keys, however many pairs
        keys = (bank["image_group"][left] * G + bank["image_group"][right]).cpu().numpy()
    index_l, index_r = bank["image_index"][left], bank["image_index"][right]
    Wb = matcher._blocks(dev)
    for _, _, buckets in plan_chunks(M, chunk_rows, keys):
        for key, rows in buckets:
            g0, g1 = divmod(key, G)
            n, a = len(rows), int(rows[0])
            if int(rows[-1]) - a + 1 == n:                                 # consecutive rows: views, no index tensors
                rows_d, take = None, (lambda t: t[a:a + n])
            else:
                rows_d = torch.from_numpy(rows).to(dev)
                take = lambda t: t[rows_d]                                 # noqa: E731
            (H0, W0), (H1, W1) = groups[g0]["hw"], groups[g1]["hw"]
            d = {}
            matcher._fine(Wb, d, groups[g0]["fine"], groups[g1]["fine"], take(index_l), take(i_ids), take(j_ids), take(mk0), take(mk1), n,
                          (H0 // 8, W0 // 8), (H0 // 2, W0 // 2), (H1 // 8, W1 // 8), (H1 // 2, W1 // 2), H0, bank["scales"], scaled=True,
                          debug=False, b_ids1=take(index_r), scale_ids=take(right))
            if rows_d is None:
                out["mkpts1_f"][a:a + n].copy_(d["mkpts1_f"])
                out["expec_f"][a:a + n].copy_(d["expec_f"])
            else:
                out["mkpts1_f"].index_copy_(0, rows_d, d["mkpts1_f"])
                out["expec_f"].index_copy_(0, rows_d, d["expec_f"])
            sample_rows(bank, g0, g1, mk0, out["mkpts1_f"], left, right, rows_d, a if rows_d is None else 0, n, out["feature_c0"],
                        out["feature_c1"], out["feature0"], out["feature1"])
    return out


# ---- 4. the reference's form ------------------------------------------------------------------------------------------------------------
def to_reference_outputs(result: dict, pairs: dict, model: dict, scales=None) -> dict:
    """-> ``{"{id0}-{id1}": {"mkpts0_c", "mkpts1_c", "mkpts0_f", "mkpts1_f" [n, 2], "mkpts0_idx" [n], "scale0", "scale1" [1, 2],
    "feature_c0", "feature_c1" [n, 256], "feature0", "feature1" [n, 128]}}``, numpy, pairs in the order of
    ``sfm_tracks.to_reference_outputs``: the ``results_dict`` of the reference's ``matchWorker``.  ``scales [I, 2]``: what the bank was
    built with (``None``: ones)."""
    def host(t):
        return t.detach().cpu().numpy() if isinstance(t, torch.Tensor) else np.asarray(t)
    ids = host(model["image_ids"])
    off, left, right = host(pairs["pair_offsets"]), host(pairs["pair_left"]), host(pairs["pair_right"])
    sc = np.ones((len(ids), 2), dtype=np.float32) if scales is None else host(scales)
    if sc.shape != (len(ids), 2):
        raise ValueError(f"scales: expected [{len(ids)}, 2], got {list(sc.shape)}")
    rows = {k: host(result[k]) for k in RESULT_KEYS if k in REFERENCE_KEYS}
    rows["mkpts0_idx"] = host(pairs["mkpts0_idx"])
    M = rows["mkpts0_idx"].shape[0]
    for k, v in rows.items():
        if v.shape[0] != M:
            raise ValueError(f"{k}: {v.shape[0]} rows, the pair list has {M}")
    out = {}
    for n in range(len(left)):
        a, b = int(off[n]), int(off[n + 1])
        entry = {k: rows[k][a:b] for k in REFERENCE_KEYS if k in rows}
        entry["scale0"], entry["scale1"] = sc[left[n]][None], sc[right[n]][None]
        out[f"{int(ids[left[n]])}-{int(ids[right[n]])}"] = {k: entry[k] for k in REFERENCE_KEYS}
    return out
