"""CPU oracle of the SfM calls of the LoFTR matcher (``src/KeypointFreeSfM/loftr_for_sfm/loftr.py:34-167``): image scales, the fine-only
branch on provided coarse matches, and the backbone-feature sampler (``loftr_for_sfm/utils/sample_feature_from_featuremap.py``).

The wrapper logic and the sampler are restated from the reference tree statement by statement, in the dtypes the reference computes in
(the keypoints' own dtype, float32 scales); the LoFTR internals come from ``oracle/loftr_oracle.py`` (published zju3dv/LoFTR), which runs
in whatever dtype it is given (float64 where a test asks for it).  The sampler goes through ``torch.nn.functional.grid_sample``, the
reference's own arithmetic.  The oracle modules themselves are not edited.
"""
from __future__ import annotations

import torch
import torch.nn.functional as F

from oracle import loftr_oracle as lo
from oracle import onepose_oracle as orc


# ---- the sampler (sample_feature_from_featuremap.py:6-80, patch_feature_size None, norm_feature False) -------------------------------
def coord_normalization(keypoints, h, w, scale=1):
    keypoints = keypoints - scale / 2 + 0.5
    rescale_tensor = torch.tensor([(w - 1) * scale, (h - 1) * scale]).to(keypoints)
    if len(keypoints.shape) == 2:
        rescale_tensor = rescale_tensor[None]
    elif len(keypoints.shape) == 4:
        rescale_tensor = rescale_tensor[None, None, None]
    else:
        raise NotImplementedError
    keypoints /= rescale_tensor
    return keypoints * 2 - 1


def imghw(scale, hw_i):
    """loftr.py:137: ``scale.squeeze(0) * torch.tensor(hw_i).to(scale)``"""
    return scale.squeeze(0) * torch.tensor(tuple(hw_i)).to(scale)


def sample_grid(kpts, hw):
    """the float32 grid ``grid_sample`` receives: ``[1, K, 1, 2]``"""
    return coord_normalization(kpts[None, :, None, :], hw[0], hw[1]).float()


def sample_feature_from_featuremap(feature_map, kpts, hw, sample_mode="bilinear"):
    """``feature_map [1, C, h, w]`` (or ``[C, h, w]``), ``kpts [K, 2]``, ``hw`` = imghw -> ``[K, C]`` float32 rows"""
    fm = feature_map.unsqueeze(0) if feature_map.dim() == 3 else feature_map
    feat = F.grid_sample(fm, sample_grid(kpts, hw).to(fm.device), mode=sample_mode, align_corners=True)      # [1, C, K, 1]
    return feat[0, :, :, 0].t()


def unnormalised(grid, size):
    """where ``grid_sample`` (align_corners) reads: ``((g + 1) / 2) * (size - 1)``, in float64 (for the near-half-integer count)"""
    return (grid.double() + 1) / 2 * (size - 1)


def channels_first(rows, hw):
    """``[h * w, C]`` channels-last rows -> ``[1, C, h, w]``"""
    return rows.reshape(hw[0], hw[1], -1).permute(2, 0, 1)[None].contiguous()


# ---- image scales on the coarse path (LoFTR get_coarse_match step 4, FineMatching) ----------------------------------------------
def scaled_coarse_keypoints(i_ids, b_ids, hw_c, hw_i0, hw_c0, scale_t):
    """``stack([i % w, i // w]) * (scale * scale_t[b_ids])``, the scale applied as given (component 0 on x)"""
    scale = hw_i0[0] / hw_c0[0]
    s = scale * (scale_t[b_ids] if scale_t.shape[0] > 1 else scale_t.expand(len(b_ids), 2))
    return torch.stack([i_ids % hw_c[1], i_ids // hw_c[1]], dim=1) * s


def fine_keypoints1(mkpts1_c, coords, W, hw0_i, hw0_f, scale1, b_ids):
    """FineMatching ``get_fine_match``: ``mkpts1_c + (coords * (W // 2) * scale1)``, ``scale1 = scale * data['scale1'][b_ids]``
    (``scale`` when no scales are given)"""
    scale = hw0_i[0] / hw0_f[0]
    if scale1 is None:
        s = scale
    else:
        s = scale * (scale1[b_ids] if scale1.shape[0] > 1 else scale1.expand(len(b_ids), 2))
    return mkpts1_c + (coords * (W // 2) * s)


# ---- the fine-only branch (loftr.py:79-115) ----------------------------------------------------------------------------------------
def coarse_ids(data):
    """clips ``data['mkpts*_c']`` IN PLACE and returns ``(b_ids, i_ids, j_ids)`` (needs hw*_i / hw*_c in ``data``)"""
    b_ids = torch.zeros((data["mkpts0_c"].shape[0],), device=data["mkpts0_c"].device).long()
    data["mkpts0_c"][:, 0] = torch.clip(data["mkpts0_c"][:, 0], min=0, max=data["hw0_i"][1] - 2)
    data["mkpts0_c"][:, 1] = torch.clip(data["mkpts0_c"][:, 1], min=0, max=data["hw0_i"][0] - 2)
    data["mkpts1_c"][:, 0] = torch.clip(data["mkpts1_c"][:, 0], min=0, max=data["hw1_i"][1] - 2)
    data["mkpts1_c"][:, 1] = torch.clip(data["mkpts1_c"][:, 1], min=0, max=data["hw1_i"][0] - 2)
    scale = data["hw0_i"][0] / data["hw0_c"][0]
    scale0 = scale * data["scale0"][b_ids][:, [1, 0]] if "scale0" in data else scale
    scale1 = scale * data["scale1"][b_ids][:, [1, 0]] if "scale1" in data else scale
    m0 = torch.round(data["mkpts0_c"] / scale0)
    m1 = torch.round(data["mkpts1_c"] / scale1)
    i_ids = (m0[:, 1] * data["hw0_c"][1] + m0[:, 0]).long()
    j_ids = (m1[:, 1] * data["hw1_c"][1] + m1[:, 0]).long()
    return b_ids, i_ids, j_ids


def fine_only_forward(sd, cfg, data, ff0, ff1, enable_fine_matching=True):
    """``data``: image sizes (``hw*_i``), ``mkpts*_c`` (clipped in place), optional ``scale0`` / ``scale1``; ``ff0``, ``ff1``: the fine maps
    ``[1, 128, hf, wf]``.  -> the keys the reference adds (without extraction)"""
    hw0_i, hw1_i = data["hw0_i"], data["hw1_i"]
    out = dict(data)
    out.update({"hw0_c": (hw0_i[0] // 8, hw0_i[1] // 8), "hw1_c": (hw1_i[0] // 8, hw1_i[1] // 8),
                "hw0_f": tuple(ff0.shape[2:]), "hw1_f": tuple(ff1.shape[2:])})
    b_ids, i_ids, j_ids = coarse_ids(out)
    out.update({"m_bids": b_ids, "b_ids": b_ids, "i_ids": i_ids, "j_ids": j_ids, "mconf": torch.ones_like(b_ids)})
    if not enable_fine_matching:
        out.update({"mkpts0_f": out["mkpts0_c"], "mkpts1_f": out["mkpts1_c"]})
        return out
    W = cfg["fine_window_size"]
    w0 = lo.fine_windows(ff0, b_ids, i_ids, out["hw0_c"], W)
    w1 = lo.fine_windows(ff1, b_ids, j_ids, out["hw1_c"], W)
    if w0.size(0) != 0:
        w0, w1 = lo.transformer_two_images(sd, "loftr_fine", cfg["fine"]["layer_names"], cfg["fine"]["nhead"], w0, w1)
    out["fine_f0"], out["fine_f1"] = w0, w1
    fm = lo.fine_matching(w0, w1, out["mkpts0_c"], out["mkpts1_c"], hw0_i, out["hw0_f"])
    out["expec_f"], out["mkpts0_f"] = fm["expec_f"], out["mkpts0_c"]
    if w0.size(0) == 0:
        out["mkpts1_f"] = out["mkpts1_c"]
    else:
        out["mkpts1_f"] = fine_keypoints1(out["mkpts1_c"], fm["expec_f"][:, :2], W, hw0_i, out["hw0_f"], out.get("scale1"), b_ids)
    return out


def backbone_maps(sd, image):
    """the reference's ``feat_c*_backbone`` / ``feat_f*_backbone``: the backbone's maps before the positional encoding"""
    return orc.backbone_8_2(sd, image)


def pe_rows(hw_c, d_model=256):
    """the positional-encoding rows ``[hc * wc, 256]`` the coarse path adds to the map (the floor-division table)"""
    pe = orc.position_table(d_model)[0, :, : hw_c[0], : hw_c[1]]
    return pe.flatten(1).t()


def near_half(u, eps=1e-4):
    """coordinates within ``eps`` of a half-integer (where nearest sampling may round either way)"""
    return ((u - torch.floor(u)) - 0.5).abs() < eps

