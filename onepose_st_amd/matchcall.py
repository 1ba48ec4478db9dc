"""The one Python home of the coarse-matching and fine-refinement C calls (include/onepose_hip.h): ``ophip_coarse_match`` / ``_conf`` /
``_select`` / ``_masked``, ``ophip_coarse_match_2d`` / ``_masked`` / ``_sinkhorn`` / ``_sinkhorn_masked`` and ``ophip_fine_refine`` / ``_scaled`` /
``_bf16`` / ``_bf16_scaled``, every argument bound by its name in the header (``hip.call_named``).

Each call is two steps.  ``plan_*`` is pure: it chooses the entry point and returns ``(entry, {parameter name: tensor or scalar})`` without
``stream``; it checks nothing the C side checks, so what C refuses is still refused by C.  ``launch`` turns every value into what the
header's C type of that parameter asks for and calls the entry on ``stream`` (a ``torch.cuda.Stream``; ``None``: the current one)."""
from __future__ import annotations

import torch

from . import hip

_TAIL = ("b_ids", "i_ids", "j_ids", "mconf", "mk3d", "mkc", "m_bids", "gt_mask", "count")
launch = hip.launch          # the launch step, shared with layercall


class MatchLists:
    """The output lists of one coarse call at capacity ``cap`` (header: ``b_ids, i_ids, j_ids, mconf, mkpts3d | mkpts0, mkpts_c | mkpts1_c,
    m_bids, gt_mask, count``) and, with ``conf_shape``, its ``conf``.  ``m_bids`` / ``gt_mask`` may be ``None`` (C skips them); ``mkc`` may
    alias the caller's final 2D points when no fine stage follows."""
    __slots__ = (*_TAIL, "conf")

    def __init__(self, b_ids, i_ids, j_ids, mconf, mk3d, mkc, m_bids, gt_mask, count, conf=None):
        self.b_ids, self.i_ids, self.j_ids, self.mconf, self.mk3d, self.mkc = b_ids, i_ids, j_ids, mconf, mk3d, mkc
        self.m_bids, self.gt_mask, self.count, self.conf = m_bids, gt_mask, count, conf

    @classmethod
    def empty(cls, cap, device, conf_shape=None, count_ints=4):
        conf = None if conf_shape is None else torch.empty(*conf_shape, device=device)
        ids = [torch.empty(cap, dtype=torch.int64, device=device) for _ in range(4)]
        return cls(*ids[:3], torch.empty(cap, device=device), torch.empty(cap, 3, device=device), torch.empty(cap, 2, device=device), ids[3],
                   torch.empty(cap, dtype=torch.bool, device=device), torch.zeros(count_ints, dtype=torch.int32, device=device), conf)

    def trim(self, K):
        """``(b_ids, i_ids, j_ids, m_bids, gt_mask, mconf, mk3d, mkc)`` of the first ``K`` matches"""
        return tuple(getattr(self, k)[:K] for k in ("b_ids", "i_ids", "j_ids", "m_bids", "gt_mask", "mconf", "mk3d", "mkc"))

    def named(self, mk3d, mkc):
        """under the header's parameter names; ``mk3d`` and ``mkc``: those of the two keypoint lists"""
        return {{"mk3d": mk3d, "mkc": mkc}.get(k, k): getattr(self, k) for k in _TAIL}


def _floats(helper, x0, x1):
    return torch.empty(getattr(hip.load(), helper)(x0.shape[0], x0.shape[1], x1.shape[1]), device=x0.device, dtype=torch.float32)


def plan_coarse_match(feat3d, feat2d, keypoints3d, *, wc, temperature, thr, border_rm, scale, nsplit, lists, conf, workspace, parts=3,
                      query_mask=None, query_scale=None, planes_ready=False, kpts_bstride=None):
    named = dict(feat3d=feat3d, feat2d=feat2d, keypoints3d=keypoints3d,
                 kpts_bstride=hip.bstride(keypoints3d) if kpts_bstride is None else kpts_bstride,
                 B=feat3d.shape[0], N=feat3d.shape[1], M=feat2d.shape[1], wc=wc, temperature=temperature, thr=thr, border_rm=border_rm, scale=scale,
                 conf=conf, workspace=workspace, **lists.named("mkpts3d", "mkpts_c"),
                 nsplit=nsplit | (hip.COARSE_PLANES_READY if planes_ready else 0))
    if query_mask is None and query_scale is None and parts in (1, 2, 3):
        return ("ophip_coarse_match_conf", "ophip_coarse_match_select", "ophip_coarse_match")[parts - 1], named
    return "ophip_coarse_match_masked", dict(named, parts=parts, query_mask=query_mask, query_scale=query_scale)


def coarse_match(feat3d, feat2d, keypoints3d, *, workspace=None, stream=None, **kw):
    """3D-2D coarse matching (``conf=None``: the lazy form).  A mask or a scale, or ``parts`` other than 1, 2, 3 -> ``_masked`` with
    ``parts``; else 1 -> ``_conf``, 2 -> ``_select``, 3 -> the plain entry.  ``planes_ready`` ors ``hip.COARSE_PLANES_READY`` into ``nsplit``."""
    workspace = _floats("ophip_coarse_workspace_floats", feat3d, feat2d) if workspace is None else workspace
    launch(*plan_coarse_match(feat3d, feat2d, keypoints3d, workspace=workspace, **kw), stream)


def plan_coarse_match_2d(x0, x1, points0, *, w0c, w1c, thr, border_rm, scale, lists, conf, workspace, temperature=None, sinkhorn=None,
                         masks=None, nsplit=3):
    named = dict(feat0=x0, feat1=x1, points0=points0, points_bstride=hip.bstride(points0), B=x0.shape[0], L0=x0.shape[1], L1=x1.shape[1],
                 w0c=w0c, w1c=w1c, thr=thr, border_rm=border_rm, scale=scale, conf=conf, workspace=workspace, **lists.named("mkpts0", "mkpts1_c"))
    if sinkhorn is None:
        named.update(temperature=temperature, nsplit=nsplit)
    else:
        named.update(zip(("bin_score", "iters", "prefilter"), sinkhorn))
    if masks is not None:
        named.update(mask0=masks[0], mask1=masks[1])
    return "ophip_coarse_match_2d" + ("" if sinkhorn is None else "_sinkhorn") + ("" if masks is None else "_masked"), named


def coarse_match_2d(x0, x1, points0, *, workspace=None, stream=None, **kw):
    """2D-2D coarse matching of the LoFTR matcher: dual softmax with ``temperature`` and ``nsplit`` (``conf=None``: lazy), or
    ``sinkhorn=(bin_score, iters, prefilter)``; ``masks=(mask0, mask1)`` -> the ``_masked`` entries"""
    if workspace is None:
        workspace = _floats("ophip_coarse_workspace_floats" if kw.get("sinkhorn") is None else "ophip_coarse_sinkhorn_workspace_floats", x0, x1)
    launch(*plan_coarse_match_2d(x0, x1, points0, workspace=workspace, **kw), stream)


def plan_fine_refine(feat_f, strides, hf, wf, desc3d_f, *, max_matches, wpack, nlayers, cross_bits, encoder_enable, nsplit, wc, stride,
                     fine_scale, expec_f, mkpts_f, lists=None, b_ids=None, i_ids=None, j_ids=None, count=None, mkpts_c=None,
                     dbg_win=None, dbg_f3=None, query_scale=None):
    if lists is not None:
        b_ids, i_ids, j_ids, count, mkpts_c = lists.b_ids, lists.i_ids, lists.j_ids, lists.count, lists.mkc
    named = dict(zip(("fs_b", "fs_c", "fs_y", "fs_x"), strides), feat_f=feat_f, hf=hf, wf=wf, desc3d_f=desc3d_f, ds_b=hip.bstride(desc3d_f),
                 ds_c=desc3d_f.stride(1), b_ids=b_ids, i_ids=i_ids, j_ids=j_ids, count=count, max_matches=max_matches, mkpts_c=mkpts_c,
                 wpack=wpack, nlayers=nlayers, cross_bits=cross_bits, encoder_enable=encoder_enable, wc=wc, stride=stride,
                 fine_scale=fine_scale, expec_f=expec_f, mkpts_f=mkpts_f, dbg_win=dbg_win, dbg_f3=dbg_f3)
    if nsplit is not None:
        named["nsplit"] = nsplit
    if query_scale is not None:
        named["query_scale"] = query_scale
    return "ophip_fine_refine" + ("" if nsplit is None else "_bf16") + ("" if query_scale is None else "_scaled"), named


def fine_refine(feat_f, strides, hf, wf, desc3d_f, *, stream=None, **kw):
    """the fine stage on a coarse call's lists (``lists``, or ``b_ids, i_ids, j_ids, count, mkpts_c``).  ``nsplit=None``: the exact-f32
    entries (they have no ``nsplit``), else the bf16 pipe; ``query_scale`` -> ``_scaled``"""
    launch(*plan_fine_refine(feat_f, strides, hf, wf, desc3d_f, **kw), stream)
