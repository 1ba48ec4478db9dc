"""Keypoint-free SfM post-optimisation: depth refinement on the device, first-order (the reference's) and second-order.

The reference (src/KeypointFreeSfM/post_optimization/optimizer/optimizer.py) refines the depth of every 3D point of a new object's
map with a Python loop of up to 1 000 float64 autograd + Adam steps (first_order_solver.py:6-172) over the residual of
residual.py:6-78.  Here the whole loop is HIP (``csrc/postopt.hip``): one prep kernel folds every residual row into
``h(d) = d * a + b``, then one step kernel per Adam step, enqueued with no synchronisation between steps, with the early stop decided
on the device.  ``refine_depths_lm`` is the second-order solver the reference's configs ask for and the reference cannot run: one
Levenberg-Marquardt solve per track, all in one launch (``csrc/postopt_lm.hip``, its own library).  Also here: the caller's
depth-to-world and reprojection updates (dataset/coarse_colmap_dataset.py:353-423), and float64 restatements of pytorch3d's
``so3_exp_map`` / ``so3_log_map`` (pytorch3d is not a dependency).

Device tensors only: CPU inputs raise :class:`hip.HipLibraryError`.  COLMAP I/O and feature aggregation stay with the
caller; the triangulation is ``sfm_triangulate``'s.
"""
from __future__ import annotations

import math
import warnings

import numpy as np
import torch

from . import hip

ADAM_BETAS = (0.9, 0.999)
ADAM_EPS = 1e-8
MAX_STEPS = 1000            # optimizer.py:224


# ---- pytorch3d's published so3 maps, restated in float64 (any device) ---------------------------------------------------------------
def _hat(v: torch.Tensor) -> torch.Tensor:
    z = torch.zeros_like(v[:, 0])
    return torch.stack([torch.stack([z, -v[:, 2], v[:, 1]], 1), torch.stack([v[:, 2], z, -v[:, 0]], 1),
                        torch.stack([-v[:, 1], v[:, 0], z], 1)], 1)


def so3_exp_map(log_rot: torch.Tensor, eps: float = 1e-4) -> torch.Tensor:
    """[N, 3] axis-angle -> [N, 3, 3]: theta^2 clamped at ``eps``, ``I + sin(t)/t hat + (1 - cos t)/t^2 hat^2``."""
    nrms = (log_rot * log_rot).sum(1)
    angles = torch.clamp(nrms, eps).sqrt()
    inv = 1.0 / angles
    fac1 = inv * angles.sin()
    fac2 = inv * inv * (1.0 - angles.cos())
    skews = _hat(log_rot)
    return fac1[:, None, None] * skews + fac2[:, None, None] * torch.bmm(skews, skews) + \
        torch.eye(3, dtype=log_rot.dtype, device=log_rot.device)[None]


def _acos_linear_extrapolation(x: torch.Tensor, lo: float, hi: float) -> torch.Tensor:
    out = torch.acos(x.clamp(lo, hi))
    up, down = x >= hi, x <= lo
    out = torch.where(up, (x - hi) * ((-1.0) / math.sqrt(1.0 - hi * hi)) + math.acos(hi), out)
    return torch.where(down, (x - lo) * ((-1.0) / math.sqrt(1.0 - lo * lo)) + math.acos(lo), out)


def so3_log_map(R: torch.Tensor, eps: float = 1e-4, cos_bound: float = 1e-4) -> torch.Tensor:
    """[N, 3, 3] -> [N, 3] axis-angle: the angle's cosine bounded at ``1 - cos_bound`` with linear extrapolation of acos,
    ``phi / (2 sin phi)``, or ``0.5 + phi^2 / 12`` where ``|sin phi| <= 0.5 * eps``."""
    if R.dim() != 3 or R.shape[1:] != (3, 3):
        raise ValueError("Input has to be a batch of 3x3 Tensors.")
    trace = R[:, 0, 0] + R[:, 1, 1] + R[:, 2, 2]
    if ((trace < -1.0 - eps) + (trace > 3.0 + eps)).any():
        raise ValueError("A matrix has trace outside valid range [-1-eps,3+eps].")
    bound = 1.0 - cos_bound
    phi = _acos_linear_extrapolation((trace - 1.0) * 0.5, -bound, bound)
    s = torch.sin(phi)
    ok = s.abs() > (0.5 * eps)
    fac = torch.where(ok, phi / (2.0 * torch.where(ok, s, torch.ones_like(s))), 0.5 + (phi ** 2) * (1.0 / 12))
    h = fac[:, None, None] * (R - R.permute(0, 2, 1))
    return torch.stack([h[:, 2, 1], h[:, 0, 2], h[:, 1, 0]], 1)


def convert_pose2angleAxis(pose) -> np.ndarray:
    """[R 3x3, t 3] (numpy) -> [1, 6] ``so3_log_map(R) | t`` (utils/geometry_utils.py:20-27)."""
    aa = so3_log_map(torch.from_numpy(np.copy(pose[0])).unsqueeze(0)).squeeze().numpy()
    return np.concatenate([aa[None], np.asarray(pose[1])[None]], axis=1)


# ---- device calls ----------------------------------------------------------------------------------------------------------------------
def _dev64(t: torch.Tensor, name: str, shape_tail: tuple) -> torch.Tensor:
    hip.need_device([(name, t)])
    if tuple(t.shape[1:]) != shape_tail:
        raise ValueError(f"{name}: expected shape [N, {', '.join(map(str, shape_tail))}], got {tuple(t.shape)}")
    return t.to(torch.float64).contiguous()


def _dev_index(t: torch.Tensor, name: str, n: int, hi: int) -> torch.Tensor:
    hip.on_device([t])
    t = t.reshape(-1).to(torch.int64).contiguous()
    if t.numel() != n:
        raise ValueError(f"{name}: expected {n} entries, got {t.numel()}")
    if n and (int(t.min()) < 0 or int(t.max()) >= hi):
        raise IndexError(f"{name}: frame index outside [0, {hi})")
    return t


def adam_step_table(lr: float, max_steps: int, betas=ADAM_BETAS) -> list:
    """[(step_size, bias_correction2 ** 0.5)] of steps 1..max_steps, computed as torch.optim.Adam's single-tensor path computes them."""
    b1, b2 = betas
    out = []
    for i in range(max_steps):
        step = float(np.float32(i + 1))         # the float32 step counter, read with .item()
        out.append((lr / (1 - b1 ** step), (1 - b2 ** step) ** 0.5))
    return out


def _flat_problem(depth, n_query, intrinsic0, intrinsic1, mkpts0_c, mkpts1_f, left_pose_idx, right_pose_idx, angle_axis_to_world):
    """The validation and flat layout both solvers share: -> (d [P] (a copy), offs [P + 1], K0, K1, mk0, mk1, li, ri, aa, P, L, F)."""
    if not isinstance(n_query, torch.Tensor):               # host numbers are refused like a CPU tensor
        raise hip.HipLibraryError(hip.NO_CPU_FALLBACK)
    hip.on_device([n_query, depth])
    d = _dev64(depth.reshape(-1, 1), "depth", (1,)).reshape(-1).clone()
    P = d.numel()
    K0 = _dev64(intrinsic0, "intrinsic0", (3, 3))
    K1 = _dev64(intrinsic1, "intrinsic1", (3, 3))
    mk0 = _dev64(mkpts0_c, "mkpts0_c", (2,))
    mk1 = _dev64(mkpts1_f, "mkpts1_f", (2,))
    aa = _dev64(angle_axis_to_world, "angle_axis_to_world", (6,))
    L, F = K0.shape[0], aa.shape[0]
    if P < 1 or F < 1:
        raise ValueError("no tracks or no frames")
    if not (K1.shape[0] == mk0.shape[0] == mk1.shape[0] == L):
        raise ValueError("per-row inputs disagree in length")
    nq = n_query.reshape(-1).to(torch.int64)
    if nq.numel() != P or int(nq.min()) < 1 or int(nq.sum()) != L:
        raise ValueError("n_query: one count >= 1 per track, summing to the number of rows")
    li = _dev_index(left_pose_idx, "left_pose_idx", L, F)
    ri = _dev_index(right_pose_idx, "right_pose_idx", L, F)
    offs = torch.zeros(P + 1, dtype=torch.int64, device=d.device)
    offs[1:] = torch.cumsum(nq.to(d.device), 0)
    return d, offs, K0, K1, mk0, mk1, li, ri, aa, P, L, F


def refine_depths(depth: torch.Tensor, n_query: torch.Tensor, intrinsic0: torch.Tensor, intrinsic1: torch.Tensor,
                  mkpts0_c: torch.Tensor, mkpts1_f: torch.Tensor, left_pose_idx: torch.Tensor, right_pose_idx: torch.Tensor,
                  angle_axis_to_world: torch.Tensor, lr: float = 3e-2, max_steps: int = MAX_STEPS, mode: str = "geometry_error",
                  return_residuals: bool = False) -> dict:
    """The reference's FirstOrderSolve of the depth procedure on flat arrays (the data loader's padding removed).

    depth [P, 1] (or [P]); n_query [P] rows per track, each >= 1, rows laid out track after track; intrinsic0 / intrinsic1 [L, 3, 3];
    mkpts0_c / mkpts1_f [L, 2]; left_pose_idx / right_pose_idx [L] into angle_axis_to_world [F, 6].  Everything is taken as float64.

    Returns ``{"depth": [P, 1] float64, "initial_residual": l_0, "final_residual": l of the last executed step (the reference's quirk),
    "steps": steps run, "loss": [steps] float64}`` plus ``"residuals"`` [L, 2] of the last evaluated depths when asked."""
    if mode != "geometry_error":
        raise NotImplementedError
    if int(max_steps) < 1:
        raise ValueError("max_steps must be >= 1")
    max_steps = int(max_steps)
    d, offs, K0, K1, mk0, mk1, li, ri, aa, P, L, F = _flat_problem(depth, n_query, intrinsic0, intrinsic1, mkpts0_c, mkpts1_f, left_pose_idx,
                                                                   right_pose_idx, angle_axis_to_world)
    table = torch.tensor(adam_step_table(float(lr), max_steps), dtype=torch.float64, device=d.device)
    loss = torch.empty(max_steps, dtype=torch.float64, device=d.device)
    steps = torch.zeros(1, dtype=torch.int32, device=d.device)
    resid = torch.empty(L, 2, dtype=torch.float64, device=d.device) if return_residuals else None
    ws_bytes = hip.load().ophip_postopt_workspace_bytes(L, P, max_steps)
    ws = torch.empty(ws_bytes, dtype=torch.uint8, device=d.device)
    hip.launch("ophip_postopt_refine", dict(depth=d, track_offsets=offs, P=P, L=L, intrinsic0=K0, intrinsic1=K1, mkpts0_c=mk0, mkpts1_f=mk1,
                                            left_idx=li, right_idx=ri, angle_axis=aa, F=F, step_table=table, max_steps=max_steps,
                                            beta1=ADAM_BETAS[0], beta2=ADAM_BETAS[1], eps=ADAM_EPS, loss=loss, steps_run=steps, residuals=resid,
                                            workspace=ws, workspace_bytes=ws_bytes))
    n = int(steps.item())                       # the one read-back: depths, loss[] and the step count follow the same stream
    hist = loss[:n]
    lh = hist.tolist()
    out = {"depth": d.reshape(P, 1), "initial_residual": lh[0], "final_residual": lh[-1], "steps": n, "loss": hist}
    if return_residuals:
        out["residuals"] = resid
    return out


LM_DEFAULTS = dict(lam0=1e-4, up=10.0, down=0.1, lam_min=1e-12, lam_max=1e12, step_tol=1e-8)


def refine_depths_lm(depth: torch.Tensor, n_query: torch.Tensor, intrinsic0: torch.Tensor, intrinsic1: torch.Tensor,
                     mkpts0_c: torch.Tensor, mkpts1_f: torch.Tensor, left_pose_idx: torch.Tensor, right_pose_idx: torch.Tensor,
                     angle_axis_to_world: torch.Tensor, max_iters: int = 50, lam0: float = LM_DEFAULTS["lam0"],
                     up: float = LM_DEFAULTS["up"], down: float = LM_DEFAULTS["down"], lam_min: float = LM_DEFAULTS["lam_min"],
                     lam_max: float = LM_DEFAULTS["lam_max"], step_tol: float = LM_DEFAULTS["step_tol"],
                     return_residuals: bool = False) -> dict:
    """The second-order solver of the same problem as :func:`refine_depths` (same arguments, validation and flat layout): one scalar
    Levenberg-Marquardt solve per track, all iterations of all tracks in one launch of ``csrc/postopt_lm.hip``.

    Returns ``{"depth": [P, 1] float64, "iterations" / "rejects" / "status": [P] int32 (``postopt_lm.CONVERGED`` ...), "lambda" /
    "initial_cost" / "final_cost": [P] float64, "initial_residual" / "final_residual": the per-track costs summed on the device in a
    fixed order, "steps": the largest iteration count}`` plus ``"residuals"`` [L, 2] at the returned depths when asked."""
    from . import postopt_lm

    max_iters = int(max_iters)
    if max_iters < 0:
        raise ValueError("max_iters must be >= 0")
    d, offs, K0, K1, mk0, mk1, li, ri, aa, P, L, F = _flat_problem(depth, n_query, intrinsic0, intrinsic1, mkpts0_c, mkpts1_f, left_pose_idx,
                                                                   right_pose_idx, angle_axis_to_world)
    dev = d.device
    ints = torch.empty(3, P, dtype=torch.int32, device=dev)              # iterations, rejects, status
    reals = torch.empty(3, P, dtype=torch.float64, device=dev)           # lambda, initial_cost, final_cost
    totals = torch.empty(2, dtype=torch.float64, device=dev)
    resid = torch.empty(L, 2, dtype=torch.float64, device=dev) if return_residuals else None
    ws_bytes = postopt_lm.load().oplm_workspace_bytes(L, P)
    ws = torch.empty(ws_bytes, dtype=torch.uint8, device=dev)
    postopt_lm.launch("oplm_refine", {
        "depth": d, "track_offsets": offs, "P": P, "L": L, "intrinsic0": K0, "intrinsic1": K1, "mkpts0_c": mk0, "mkpts1_f": mk1, "left_idx": li,
        "right_idx": ri, "angle_axis": aa, "F": F, "lam0": lam0, "up": up, "down": down, "lam_min": lam_min, "lam_max": lam_max,
        "step_tol": step_tol, "max_iters": max_iters, "iterations": ints[0], "rejects": ints[1], "status": ints[2], "lambda": reals[0],
        "initial_cost": reals[1], "final_cost": reals[2], "initial_residual": totals[0:1], "final_residual": totals[1:2], "residuals": resid,
        "workspace": ws, "workspace_bytes": ws_bytes})                    # a dict display: ``lambda`` is no keyword argument
    # the one read-back: both totals and the largest iteration count follow the solve on the same stream
    initial, final, steps = torch.cat([totals, ints[0].max().to(torch.float64)[None]]).tolist()
    out = {"depth": d.reshape(P, 1), "iterations": ints[0], "rejects": ints[1], "status": ints[2], "lambda": reals[0],
           "initial_cost": reals[1], "final_cost": reals[2], "initial_residual": initial, "final_residual": final, "steps": int(steps)}
    if return_residuals:
        out["residuals"] = resid
    return out


def _frames(K: torch.Tensor, R: torch.Tensor, t: torch.Tensor):
    K = _dev64(K, "K", (3, 3))
    R = _dev64(R, "R", (3, 3))
    t = _dev64(t, "t", (3,))
    if not (K.shape[0] == R.shape[0] == t.shape[0]) or K.shape[0] < 1:
        raise ValueError("K, R, t: one entry per frame")
    return K, R, t


def points_from_depth(keypoints: torch.Tensor, depth: torch.Tensor, frame_idx: torch.Tensor, K: torch.Tensor, R: torch.Tensor,
                      t: torch.Tensor) -> torch.Tensor:
    """World points [N, 3] of keypoints [N, 2] at depth [N] (or [N, 1]) in frames frame_idx [N] with intrinsics K [F, 3, 3] and
    world-to-camera poses R [F, 3, 3], t [F, 3]: ``inv(T) (K^-1 [x, y, 1] d)`` (coarse_colmap_dataset.py:353-380)."""
    kp = _dev64(keypoints, "keypoints", (2,))
    N = kp.shape[0]
    dd = _dev64(depth.reshape(-1, 1), "depth", (1,))
    if dd.shape[0] != N:
        raise ValueError("depth: one per keypoint")
    K, R, t = _frames(K, R, t)
    fi = _dev_index(frame_idx, "frame_idx", N, K.shape[0])
    out = torch.empty(N, 3, dtype=torch.float64, device=kp.device)
    hip.launch("ophip_postopt_points_from_depth", dict(keypoints=kp, depth=dd, frame_idx=fi, N=N, K=K, R=R, t=t, F=K.shape[0], points=out))
    return out


def project_points(points: torch.Tensor, frame_idx: torch.Tensor, K: torch.Tensor, R: torch.Tensor, t: torch.Tensor) -> torch.Tensor:
    """Keypoints [N, 2] of world points [N, 3] in frames frame_idx [N]: ``xy / (z + 1e-4)`` of ``K (R X + t)``
    (coarse_colmap_dataset.py:404-419)."""
    X = _dev64(points, "points", (3,))
    N = X.shape[0]
    K, R, t = _frames(K, R, t)
    fi = _dev_index(frame_idx, "frame_idx", N, K.shape[0])
    out = torch.empty(N, 2, dtype=torch.float64, device=X.device)
    hip.launch("ophip_postopt_project_points", dict(points=X, frame_idx=fi, N=N, K=K, R=R, t=t, F=K.shape[0], keypoints=out))
    return out


class Optimizer:
    """optimizer.py's ``Optimizer`` without its data loading: ``start_optimize`` takes the aggregated flat arrays.

    cfgs: ``solver_type``, ``residual_mode``, ``optimize_lr`` ({"depth": lr}), ``optim_procedure`` (a list of "depth"); other keys of the
    reference's cfg (num_workers, batch_size, image_i_f_scale, verbose) are accepted and unused.  DeepLM is not vendored in the reference,
    so every solver type runs the first-order solver, as there; anything but "FirstOrder" warns.  ``hip_second_order`` (this project's
    key, default ``False``): with ``True`` and ``solver_type == "SecondOrder"`` every "depth" procedure runs :func:`refine_depths_lm`
    instead, without that warning, and ``steps`` holds the largest iteration count of each."""

    def __init__(self, cfgs: dict):
        self.solver_type = cfgs["solver_type"]
        self.residual_mode = cfgs["residual_mode"]
        self.optimize_lr = cfgs["optimize_lr"]
        self.optim_procedure = cfgs["optim_procedure"]
        self.verbose = cfgs.get("verbose", False)
        self.hip_second_order = bool(cfgs.get("hip_second_order", False))
        self.initial_residual = None
        self.final_residual = None
        self.steps = []

    def start_optimize(self, aggregated: dict, frame_poses: dict) -> dict:
        """aggregated: device tensors ``depth`` [P, 1], ``n_query`` [P], ``intrinsic0`` / ``intrinsic1`` [L, 3, 3], ``mkpts0_c`` /
        ``mkpts1_c`` / ``mkpts1_f`` [L, 2], ``left_colmap_ids`` / ``right_colmap_ids`` [L], ``point_cloud_id`` [P].  frame_poses:
        {colmap frame id: [R 3x3, t 3]} (or {id: {"initial_pose": [R, t]}}), in the order the frames are indexed.

        Returns the reference's dict: ``pose`` [R [F, 3, 3], t [F, 3]], ``colmap_frame_ids`` [F], ``depth`` [P, 1],
        ``point_cloud_ids`` [P] (numpy)."""
        for procedure in self.optim_procedure:
            if procedure != "depth":
                raise NotImplementedError
        if self.residual_mode != "geometry_error":
            raise NotImplementedError
        second_order = self.hip_second_order and self.solver_type == "SecondOrder"
        if self.solver_type != "FirstOrder" and not second_order:
            warnings.warn("Failed to import DeepLM module. Use our first-order optimizer instead. "
                          "Please check whether installation is correct!")
            self.solver_type = "FirstOrder"
        depth = aggregated["depth"]
        hip.on_device([depth])
        dev = depth.device
        ids = list(frame_poses.keys())
        poses = [v["initial_pose"] if isinstance(v, dict) else v for v in frame_poses.values()]
        aa = torch.from_numpy(np.concatenate([convert_pose2angleAxis(p) for p in poses])).to(dev)
        id2index = {k: i for i, k in enumerate(ids)}
        left = torch.tensor([id2index[k] for k in aggregated["left_colmap_ids"].cpu().numpy().tolist()], dtype=torch.int64, device=dev)
        right = torch.tensor([id2index[k] for k in aggregated["right_colmap_ids"].cpu().numpy().tolist()], dtype=torch.int64, device=dev)
        depth = depth.to(torch.float64)
        self.steps = []
        for i, procedure in enumerate(self.optim_procedure):
            rows = (depth, aggregated["n_query"], aggregated["intrinsic0"], aggregated["intrinsic1"], aggregated["mkpts0_c"],
                    aggregated["mkpts1_f"], left, right, aa)
            r = refine_depths_lm(*rows) if second_order else refine_depths(*rows, lr=self.optimize_lr[procedure], mode=self.residual_mode)
            if i == 0:
                self.initial_residual = r["initial_residual"]
            self.final_residual = r["final_residual"]
            self.steps.append(r["steps"])
            depth = r["depth"]
        R = so3_exp_map(aa[:, :3])
        return {"pose": [R.cpu().numpy(), aa[:, 3:6].cpu().numpy()],
                "colmap_frame_ids": np.array(ids),
                "depth": depth.cpu().numpy(),
                "point_cloud_ids": aggregated["point_cloud_id"].long().cpu().numpy()}
