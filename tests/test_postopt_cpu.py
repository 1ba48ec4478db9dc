"""SfM depth refinement without a GPU: the oracle's residual and rotations against hand-computed values, the restated pytorch3d maps,
the kernel's Adam arithmetic fed from the host's step table against ``torch.optim.Adam(foreach=False)``, rejected options, CPU tensors,
the new C entries in the header / binding / library, and spills of the ``postopt_`` kernels."""
import ctypes
import math
import os

import numpy as np
import pytest
import torch

from onepose_st_amd import hip, postopt
from onepose_st_amd.synthetic import make_synthetic_sfm_tracks
from tests import postopt_oracle as po
from tests.test_disasm_guards import device_asm  # noqa: F401  (fixture)

F64 = torch.float64
NEW_ENTRIES = ("ophip_postopt_refine", "ophip_postopt_points_from_depth", "ophip_postopt_project_points")


def _rodrigues(aa):
    th = float(np.linalg.norm(aa))
    if th == 0.0:
        return np.eye(3)
    k = aa / th
    K = np.array([[0, -k[2], k[1]], [k[2], 0, -k[0]], [-k[1], k[0], 0]])
    return np.eye(3) + math.sin(th) * K + (1 - math.cos(th)) * K @ K


def test_residual_matches_a_hand_computed_projection():
    # identity pose0, pose1 a pure translation: X = d K0^-1 [u, v, 1], x1 = K1 (X + t1), r = x1[:2] / (x1[2] + 1e-4) - f
    K0 = torch.tensor([[500.0, 0, 320], [0, 510, 240], [0, 0, 1]], dtype=F64)
    K1 = torch.tensor([[450.0, 0, 300], [0, 455, 250], [0, 0, 1]], dtype=F64)
    u, v, d = 400.0, 180.0, 2.5
    t1 = np.array([0.1, -0.2, 0.3])
    X = d * np.array([(u - 320) / 500, (v - 240) / 510, 1.0])
    x1 = K1.numpy() @ (X + t1)
    want = np.array([x1[0] / (x1[2] + 1e-4), x1[1] / (x1[2] + 1e-4)]) - np.array([310.0, 200.0])
    pose0 = torch.zeros(1, 6, dtype=F64)
    pose1 = torch.tensor([[0, 0, 0, *t1]], dtype=F64)
    r = po.depth_residual(torch.tensor([[d]], dtype=F64), pose0, pose1, K0[None], K1[None], torch.tensor([[u, v]], dtype=F64),
                          torch.tensor([[310.0, 200.0]], dtype=F64))
    assert np.allclose(r.numpy()[0], want, rtol=0, atol=1e-10), (r, want)
    a, b = po.folded_rows(pose0, pose1, K0[None], K1[None], torch.tensor([[u, v]], dtype=F64))
    rf = po.folded_residual(torch.tensor([[d]], dtype=F64), a, b, torch.tensor([[310.0, 200.0]], dtype=F64))
    assert np.allclose(rf.numpy()[0], want, rtol=0, atol=1e-10)


def test_angle_axis_rotate_point_is_rodrigues_including_zero():
    g = torch.Generator().manual_seed(3)
    aa = torch.randn(64, 3, generator=g, dtype=F64) * 1.2
    aa[0] = 0.0
    pt = torch.randn(64, 3, generator=g, dtype=F64)
    got = po.angle_axis_rotate_point(aa, pt).numpy()
    want = np.stack([_rodrigues(a) @ p for a, p in zip(aa.numpy(), pt.numpy())])
    assert np.abs(got - want).max() < 1e-13
    assert np.array_equal(got[0], pt[0].numpy())                 # theta = 0: p + 0 x p


@pytest.mark.parametrize("mod", ["product", "oracle"])
def test_restated_so3_maps_round_trip_in_the_safe_range(mod):
    exp_map, log_map = (postopt.so3_exp_map, postopt.so3_log_map) if mod == "product" else (po.so3_exp_map, po.so3_log_map)
    g = torch.Generator().manual_seed(5)
    axis = torch.randn(200, 3, generator=g, dtype=F64)
    axis = axis / axis.norm(dim=1, keepdim=True)
    ang = 0.05 + torch.rand(200, generator=g, dtype=F64) * (math.pi - 0.1)
    w = axis * ang[:, None]
    R = torch.from_numpy(np.stack([_rodrigues(x) for x in w.numpy()]))
    assert (exp_map(w) - R).abs().max() < 1e-13
    assert (exp_map(log_map(R)) - R).abs().max() < 1e-12
    assert (log_map(R) - w).abs().max() < 1e-11


@pytest.mark.parametrize("mod", ["product", "oracle"])
def test_restated_small_angle_branches(mod):
    exp_map, log_map = (postopt.so3_exp_map, postopt.so3_log_map) if mod == "product" else (po.so3_exp_map, po.so3_log_map)
    # exp: theta^2 clamped at 1e-4 -> theta = 0.01 in the factors: R = I + (sin .01 / .01) hat(w) + ((1 - cos .01) / 1e-4) hat(w)^2
    w = torch.tensor([[1e-3, -2e-3, 0.5e-3]], dtype=F64)
    K = po.hat(w)[0].numpy()
    want = np.eye(3) + (math.sin(0.01) / 0.01) * K + ((1 - math.cos(0.01)) / 1e-4) * K @ K
    assert np.abs(exp_map(w)[0].numpy() - want).max() < 1e-15
    # log of the identity: cos phi = 1 >= 1 - 1e-4, phi = acos(0.9999) extrapolated linearly to (1 - 0.9999) * -1/sqrt(1 - 0.9999^2) +
    # acos(0.9999); the factor phi / (2 sin phi) times R - R^T = 0
    assert torch.equal(log_map(torch.eye(3, dtype=F64)[None]), torch.zeros(1, 3, dtype=F64))
    # a rotation of 1e-3 rad about z: the cosine 1 - 5e-7 is past the bound; phi = (c - 0.9999) * dacos(0.9999) + acos(0.9999)
    th = 1e-3
    R = torch.tensor([[[math.cos(th), -math.sin(th), 0], [math.sin(th), math.cos(th), 0], [0, 0, 1]]], dtype=F64)
    c = ((R[0, 0, 0] + R[0, 1, 1] + R[0, 2, 2]).item() - 1.0) * 0.5
    phi = (c - 0.9999) * (-1.0 / math.sqrt(1.0 - 0.9999 ** 2)) + math.acos(0.9999)
    want_z = phi / (2.0 * math.sin(phi)) * (R[0, 1, 0] - R[0, 0, 1]).item()
    got = log_map(R)[0]
    assert abs(got[2].item() - want_z) < 1e-18 and got[0].item() == 0.0 and got[1].item() == 0.0
    # a half turn: cos phi = -1 is past the lower bound, phi = (c + 0.9999) * dacos(-0.9999) + acos(-0.9999) = 3.1345..., and R - R^T = 0
    # loses the axis, as in pytorch3d.  (The 0.5 + phi^2 / 12 branch needs |sin phi| <= 0.5e-4, which the extrapolation never reaches for
    # a trace the map accepts: phi stays >= 0.0035 and <= pi - 0.0035.)
    Rpi = torch.diag(torch.tensor([1.0, -1.0, -1.0], dtype=F64))[None]
    phi = (-1.0 + 0.9999) * (-1.0 / math.sqrt(1.0 - 0.9999 ** 2)) + math.acos(-0.9999)
    assert abs(phi - 3.1345216) < 1e-6
    assert torch.equal(log_map(Rpi), torch.zeros(1, 3, dtype=F64))


def test_kernel_adam_order_matches_torch_adam():
    """the step kernel's arithmetic (fma(1 - b1, g - m, m); fma((1 - b2) g, g, b2 v); d + (-step_size m) / (sqrt(v) / bc2_sqrt + eps)),
    fed from the host's step table, against torch.optim.Adam(foreach=False) on one tensor over 50 steps"""
    from fractions import Fraction

    def fma(a, b, c):
        return float(Fraction(a) * Fraction(b) + Fraction(c))

    g = torch.Generator().manual_seed(7)
    x0 = torch.randn(24, generator=g, dtype=F64)
    target = torch.randn(24, generator=g, dtype=F64)
    lr = 3e-2
    var = torch.nn.Parameter(x0.clone())
    opt = torch.optim.Adam([var], lr=lr, foreach=False)
    table = postopt.adam_step_table(lr, 50)
    d, m, v = x0.tolist(), [0.0] * 24, [0.0] * 24
    b1, b2, eps = postopt.ADAM_BETAS[0], postopt.ADAM_BETAS[1], postopt.ADAM_EPS
    for i in range(50):
        opt.zero_grad()
        loss = ((var - target) ** 3).abs().sum()
        loss.backward()
        grad = var.grad.tolist()
        opt.step()
        step_size, bc2 = table[i]
        for k in range(24):
            m[k] = fma(1.0 - b1, grad[k] - m[k], m[k])
            v[k] = fma((1.0 - b2) * grad[k], grad[k], v[k] * b2)
            d[k] = d[k] + (-step_size * m[k]) / (math.sqrt(v[k]) / bc2 + eps)
        got = torch.tensor(d, dtype=F64)
        assert ((got - var.detach()).abs() <= 1e-15 * var.detach().abs()).all(), i
        with torch.no_grad():
            var.copy_(got)                          # both continue from the same state


def test_rejected_options_and_cpu_tensors():
    data = make_synthetic_sfm_tracks(0, n_frames=4, n_tracks=8, mean_len=3, long_len=0)
    args = (data["depth"], data["n_query"], data["intrinsic0"], data["intrinsic1"], data["mkpts0_c"], data["mkpts1_f"],
            data["left_pose_idx"], data["right_pose_idx"], data["angle_axis_to_world"])
    with pytest.raises(NotImplementedError):
        postopt.refine_depths(*args, mode="reprojection_error")
    with pytest.raises(hip.HipLibraryError):
        postopt.refine_depths(*args)
    with pytest.raises(hip.HipLibraryError):
        postopt.points_from_depth(data["mkpts0_c"][:8], data["depth"], data["left_pose_idx"][:8], data["K"], data["R"], data["t"])
    with pytest.raises(hip.HipLibraryError):
        postopt.project_points(data["points"], data["left_pose_idx"][:8], data["K"], data["R"], data["t"])
    agg = {k: data[k] for k in ("depth", "n_query", "intrinsic0", "intrinsic1", "mkpts0_c", "mkpts1_c", "mkpts1_f", "left_colmap_ids",
                                "right_colmap_ids", "point_cloud_id")}
    base = {"solver_type": "FirstOrder", "residual_mode": "geometry_error", "optimize_lr": {"depth": 3e-2}, "optim_procedure": ["depth"]}
    with pytest.raises(NotImplementedError):
        postopt.Optimizer(dict(base, optim_procedure=["depth", "pose"])).start_optimize(agg, data["frame_poses"])
    with pytest.raises(NotImplementedError):
        postopt.Optimizer(dict(base, residual_mode="feature_metric_error")).start_optimize(agg, data["frame_poses"])
    with pytest.raises(hip.HipLibraryError):
        postopt.Optimizer(base).start_optimize(agg, data["frame_poses"])
    with pytest.warns(UserWarning, match="DeepLM"), pytest.raises(hip.HipLibraryError):
        postopt.Optimizer(dict(base, solver_type="SecondOrder")).start_optimize(agg, data["frame_poses"])


def test_synthetic_tracks_have_single_and_long_tracks_and_safe_rotations():
    data = make_synthetic_sfm_tracks(0)
    nq = data["n_query"]
    assert (nq[:3] == 1).all() and nq[3] >= 1000 and int(nq.sum()) == data["mkpts0_c"].shape[0]
    ang = data["angle_axis_to_world"][:, :3].norm(dim=1)
    assert (ang >= 0.05 - 1e-12).all() and (ang <= math.pi - 0.05 + 1e-12).all()
    assert (data["depth"] > 0).all()


def test_new_entries_are_declared_registered_and_exported():
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    with open(os.path.join(root, "include", "onepose_hip.h")) as f:
        header = f.read()
    with open(os.path.join(root, "onepose_st_amd", "csrc", "Makefile")) as f:
        assert "postopt.hip" in f.read()
    lib = ctypes.CDLL(hip.library_path())
    for name in NEW_ENTRIES:
        assert f"int {name}(" in header, name
        assert name in hip.EXPORTED_SYMBOLS, name
        assert hasattr(lib, name), name
    assert "size_t ophip_postopt_workspace_bytes(" in header and hasattr(lib, "ophip_postopt_workspace_bytes")
    assert hip.ABI_VERSION == 4


def test_postopt_kernels_do_not_spill(device_asm):  # noqa: F811
    ks = {k: v for k, v in device_asm.items() if "postopt_" in k}
    for name in ("postopt_prep_kernel", "postopt_step_kernel", "postopt_points_kernel", "postopt_project_kernel"):
        assert len([k for k in ks if name in k]) == 1, sorted(ks)
    for sym, ins in ks.items():
        spills = [t for t in ins if t.startswith("scratch_")]
        assert not spills, (sym, spills[:4])
