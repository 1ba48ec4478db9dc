"""CPU float64 oracle of the keypoint-free SfM depth refinement (``src/KeypointFreeSfM/post_optimization``): the residual of
``optimizer/residual.py`` with ``AngleAxisRotatePoint`` (``residual_utils.py``), pytorch3d's published ``so3_exp_map`` / ``so3_log_map`` /
``acos_linear_extrapolation`` (pytorch3d is not installed; restated), and ``FirstOrderSolve``
(``first_order_solver.py``): autograd through the residual, ``torch.optim.Adam(foreach=False)``, the relative-decrease early stop.

``folded_rows`` / ``folded_residual`` evaluate the same residual on the device kernels' form ``h(d) = d * a + b``: running the solver on
both forms measures how far last-bit differences of the residual carry through Adam (the yardstick of the GPU full-run bars).
Test-only: nothing under ``onepose_st_amd`` imports this module.  The functions run on any device (tools/time_postopt.py times them on
the GPU as the reference's form).
"""
from __future__ import annotations

import math

import torch

F64 = torch.float64


def hat(v):
    o = torch.zeros(v.shape[0], 3, 3, dtype=v.dtype, device=v.device)
    o[:, 0, 1], o[:, 0, 2] = -v[:, 2], v[:, 1]
    o[:, 1, 0], o[:, 1, 2] = v[:, 2], -v[:, 0]
    o[:, 2, 0], o[:, 2, 1] = -v[:, 1], v[:, 0]
    return o


def so3_exp_map(w, eps=1e-4):
    th = torch.clamp((w * w).sum(1), eps).sqrt()
    a = (1.0 / th) * th.sin()
    b = (1.0 / th) * (1.0 / th) * (1.0 - th.cos())
    S = hat(w)
    return a[:, None, None] * S + b[:, None, None] * torch.bmm(S, S) + torch.eye(3, dtype=w.dtype, device=w.device)[None]


def acos_linear_extrapolation(x, lower, upper):
    out = torch.empty_like(x)
    hi, lo = x >= upper, x <= lower
    mid = ~hi & ~lo
    out[mid] = torch.acos(x[mid])
    out[hi] = (x[hi] - upper) * (-1.0 / math.sqrt(1.0 - upper * upper)) + math.acos(upper)
    out[lo] = (x[lo] - lower) * (-1.0 / math.sqrt(1.0 - lower * lower)) + math.acos(lower)
    return out


def so3_log_map(R, eps=1e-4, cos_bound=1e-4):
    c = (R[:, 0, 0] + R[:, 1, 1] + R[:, 2, 2] - 1.0) * 0.5
    phi = acos_linear_extrapolation(c, -(1.0 - cos_bound), 1.0 - cos_bound)
    s = phi.sin()
    f = torch.empty_like(phi)
    big = s.abs() > 0.5 * eps
    f[big] = phi[big] / (2.0 * s[big])
    f[~big] = 0.5 + (phi[~big] ** 2) * (1.0 / 12)
    A = f[:, None, None] * (R - R.transpose(1, 2))
    return torch.stack([A[:, 2, 1], A[:, 0, 2], A[:, 1, 0]], 1)


def angle_axis_rotate_point(aa, pt):
    """AngleAxisRotatePoint: Rodrigues where |aa|^2 > 0, ``pt + aa x pt`` where it is 0, blended by a 0/1 mask as the reference does."""
    t2 = (aa * aa).sum(1)
    mask = (t2 > 0).to(aa.dtype)
    th = torch.sqrt(t2 + (1 - mask))
    ct, st = torch.cos(th), torch.sin(th)
    w = aa * (1.0 / th)[:, None]
    wx = torch.stack([w[:, 1] * pt[:, 2] - w[:, 2] * pt[:, 1], w[:, 2] * pt[:, 0] - w[:, 0] * pt[:, 2],
                      w[:, 0] * pt[:, 1] - w[:, 1] * pt[:, 0]], 1)
    dot = (w[:, 0] * pt[:, 0] + w[:, 1] * pt[:, 1] + w[:, 2] * pt[:, 2]) * (1.0 - ct)
    rod = pt * ct[:, None] + wx * st[:, None] + w * dot[:, None]
    ax = torch.stack([aa[:, 1] * pt[:, 2] - aa[:, 2] * pt[:, 1], aa[:, 2] * pt[:, 0] - aa[:, 0] * pt[:, 2],
                      aa[:, 0] * pt[:, 1] - aa[:, 1] * pt[:, 0]], 1)
    first = pt + ax
    m = mask[:, None].expand(-1, 3)
    return rod * m + first * (1 - m)


def depth_residual(depth, pose0, pose1, K0, K1, mkpts0_c, mkpts1_f):
    """residual.py, mode "geometry_error": depth [L, 1] (expanded per row), poses [L, 6], K [L, 3, 3], keypoints [L, 2] -> [L, 2]."""
    ones = torch.ones(mkpts0_c.shape[0], 1, dtype=mkpts0_c.dtype, device=mkpts0_c.device)
    p_cam0 = (K0.inverse() @ (torch.cat([mkpts0_c, ones], -1) * depth).unsqueeze(-1)).squeeze(-1)
    Rinv = so3_exp_map(pose0[:, :3]).inverse()
    tinv = -1 * (Rinv @ pose0[:, 3:6].unsqueeze(-1)).squeeze(-1)
    aainv = so3_log_map(Rinv)
    p_world = angle_axis_rotate_point(aainv, p_cam0) + tinv
    p_cam1 = angle_axis_rotate_point(pose1[:, :3], p_world) + pose1[:, 3:6]
    h = (K1 @ p_cam1.unsqueeze(-1)).squeeze(-1)
    return h[:, :2] / (h[:, [2]] + 1e-4) - mkpts1_f


def folded_rows(pose0, pose1, K0, K1, mkpts0_c):
    """(a [L, 3], b [L, 3]) with the residual's homogeneous projection h(d) = d * a + b (b[:, 2] includes the + 1e-4)."""
    ones = torch.ones(mkpts0_c.shape[0], 1, dtype=mkpts0_c.dtype, device=mkpts0_c.device)
    ray = (K0.inverse() @ torch.cat([mkpts0_c, ones], -1).unsqueeze(-1)).squeeze(-1)
    Rinv = so3_exp_map(pose0[:, :3]).inverse()
    tinv = -1 * (Rinv @ pose0[:, 3:6].unsqueeze(-1)).squeeze(-1)
    aainv = so3_log_map(Rinv)
    a = angle_axis_rotate_point(pose1[:, :3], angle_axis_rotate_point(aainv, ray))
    b = angle_axis_rotate_point(pose1[:, :3], tinv) + pose1[:, 3:6]
    a = (K1 @ a.unsqueeze(-1)).squeeze(-1)
    b = (K1 @ b.unsqueeze(-1)).squeeze(-1)
    b[:, 2] += 1e-4
    return a, b


def folded_residual(depth, a, b, mkpts1_f):
    h = depth * a + b
    return h[:, :2] / h[:, [2]] - mkpts1_f


def first_order_solve(depth, indices, residual_fn, lr=3e-2, max_steps=1000, record=False):
    """FirstOrderSolve of one variable: -> (depth [P, 1], losses [steps] as floats, per-step depths when ``record``).  The reference's
    final residual (re-evaluated on the indexed copy taken before the last step) equals ``losses[-1]``."""
    var = torch.nn.Parameter(depth.clone())
    opt = torch.optim.Adam([var], lr=lr, foreach=False)
    losses, traj, last = [], [], None
    for i in range(max_steps):
        expanded = var[indices]
        opt.zero_grad()
        r = residual_fn(expanded)
        loss = torch.sum(0.5 * r * r)
        loss.backward()
        opt.step()
        cur = loss.detach().clone()
        losses.append(cur.item())
        if record:
            traj.append(var.detach().clone())
        if i > 0:
            ratio = (last - cur) / last
            last = cur
            if ratio < 0.0001 and i > max_steps * 0.2:
                break
        else:
            last = cur
    return var.detach(), losses, traj


def stop_ratios(losses):
    """the relative decrease the solver tests at every step i >= 1 (index i of the returned list; entry 0 is None)"""
    out = [None]
    for i in range(1, len(losses)):
        a, b = torch.tensor(losses[i - 1], dtype=F64), torch.tensor(losses[i], dtype=F64)
        out.append(float((a - b) / a))
    return out


def expand_inputs(data):
    """per-row poses and the depth index of the synthetic dict (onepose_st_amd.synthetic.make_synthetic_sfm_tracks)"""
    aa = data["angle_axis_to_world"]
    idx = torch.repeat_interleave(torch.arange(data["depth"].shape[0], device=aa.device), data["n_query"])
    return aa[data["left_pose_idx"]], aa[data["right_pose_idx"]], idx


def solve_literal(data, lr=3e-2, max_steps=1000, record=False):
    p0, p1, idx = expand_inputs(data)
    return first_order_solve(data["depth"], idx, lambda d: depth_residual(d, p0, p1, data["intrinsic0"], data["intrinsic1"],
                                                                           data["mkpts0_c"], data["mkpts1_f"]), lr, max_steps, record)


def solve_folded(data, lr=3e-2, max_steps=1000, record=False):
    p0, p1, idx = expand_inputs(data)
    a, b = folded_rows(p0, p1, data["intrinsic0"], data["intrinsic1"], data["mkpts0_c"])
    return first_order_solve(data["depth"], idx, lambda d: folded_residual(d, a, b, data["mkpts1_f"]), lr, max_steps, record)
