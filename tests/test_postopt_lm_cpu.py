"""The second-order depth solver without a GPU: the numpy restatement (tests/postopt_lm_oracle.py) against the literal residual and
the first-order oracle, the header and binding of ``libonepose_postopt_lm.so`` (what tests/test_cabi_binding.py does not state for every
row of ``cabi.LIBRARIES``), its argument checks (which come before any HIP call, so they answer on a machine with no device), and the
``hip_second_order`` key of ``postopt.Optimizer`` on CPU tensors."""
import ctypes
import os
import re
import shutil
import subprocess
import tempfile
import warnings

import numpy as np
import pytest
import torch

from onepose_st_amd import cabi, hip, postopt, postopt_lm
from onepose_st_amd.synthetic import make_synthetic_sfm_tracks
from tests import postopt_lm_oracle as lm
from tests import postopt_oracle as po

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
OBJDUMP = "/opt/rocm/lib/llvm/bin/llvm-objdump"


def literal_cost(data, depth):
    p0, p1, idx = po.expand_inputs(data)
    r = po.depth_residual(depth[idx], p0, p1, data["intrinsic0"], data["intrinsic1"], data["mkpts0_c"], data["mkpts1_f"])
    return torch.sum(0.5 * r * r).item()


@pytest.mark.parametrize("seed", [0, 1])
def test_oracle_converges_below_the_first_order_cost(seed):
    data = make_synthetic_sfm_tracks(seed)
    out = lm.solve(data)
    assert (out["status"] == lm.CONVERGED).all() and out["iterations"].max() <= 5, (out["status"], out["iterations"].max())
    assert (out["final_cost"] <= out["initial_cost"]).all()
    d_lm = torch.from_numpy(out["depth"])
    d_adam, _, _ = po.solve_literal(data)
    c_lm, c_adam = literal_cost(data, d_lm), literal_cost(data, d_adam)
    assert c_lm <= c_adam, (c_lm, c_adam)
    assert abs(out["final_residual"] - c_lm) <= 1e-12 * c_lm              # the folded rows evaluate the literal residual
    again = lm.solve(data, depth=d_lm, max_iters=0)                         # max_iters = 0 asks whether a point is stationary
    assert (again["status"] == lm.CONVERGED).all() and (again["iterations"] == 0).all()
    assert np.array_equal(again["depth"], out["depth"])


@pytest.mark.parametrize("seed,factor,rejects,tracks", [(0, 0.4, 4, 1), (3, 1.6, 7, 2)])
def test_far_starts_reject_steps_and_their_decisions_do_not_hang_on_last_bits(seed, factor, rejects, tracks):
    """the two starts of the GPU trajectory test: steps are rejected there, every track still converges, and a 1e-12 relative
    perturbation of every sum changes no decision -- which is why that test may ask for equal counts"""
    data = make_synthetic_sfm_tracks(seed)
    data["depth"] = factor * data["depth_true"]
    out = lm.solve(data)
    assert (out["status"] == lm.CONVERGED).all() and out["iterations"].max() <= 8
    assert out["rejects"].sum() == rejects and (out["rejects"] > 0).sum() == tracks
    for k in (1, 2, 3, 4, 50):
        a, b = lm.solve(data, max_iters=k), lm.solve(data, max_iters=k, perturb=1e-12, seed=k)
        for key in ("iterations", "rejects", "status"):
            assert np.array_equal(a[key], b[key]), (k, key)


def test_oracle_reports_budget_and_degenerate_tracks():
    data = make_synthetic_sfm_tracks(1, depth_noise=0.15)
    out = lm.solve(data, max_iters=1)
    assert set(out["status"].tolist()) <= {lm.CONVERGED, lm.MAX_ITERS} and (out["status"] == lm.MAX_ITERS).any()
    assert out["iterations"].max() == 1
    data["mkpts1_f"][2, 0] = float("nan")                                    # track 2 has one row
    bad = lm.solve(data)
    assert bad["status"][2] == lm.DEGENERATE and bad["iterations"][2] == 0 and bad["depth"][2, 0] == data["depth"][2, 0].item()
    assert (np.delete(bad["status"], 2) == lm.CONVERGED).all()


def test_header_and_binding():
    assert postopt_lm.ABI_VERSION == 1
    # the problem's arguments are ophip_postopt_refine's, names and types in order
    first = cabi.parse(open(os.path.join(REPO, "include", "onepose_hip.h")).read()).prototypes["ophip_postopt_refine"].params
    mine = postopt_lm._BINDING.header.prototypes["oplm_refine"].params
    assert mine[:12] == first[:12] and mine[-3:] == first[-3:] and len(mine) == 31
    assert (postopt_lm.CONVERGED, postopt_lm.MAX_ITERS, postopt_lm.STALLED, postopt_lm.DEGENERATE) == \
        (lm.CONVERGED, lm.MAX_ITERS, lm.STALLED, lm.DEGENERATE)
    assert postopt_lm.load().oplm_workspace_bytes(100, 10) >= 100 * 64 and postopt_lm.load().oplm_workspace_bytes(5, 10) == 0
    mk = open(os.path.join(REPO, "onepose_st_amd", "csrc", "Makefile")).read()
    assert re.search(r"^HDRS :=.*\bpostopt_fold\.h\b", mk, re.M) and re.search(r"^PLM_HDRS :=.*\bpostopt_fold\.h\b", mk, re.M)
    assert re.search(r"^PLM_FLAGS := -ffp-contract=off$", mk, re.M)


def test_one_copy_of_the_fold():
    csrc = os.path.join(REPO, "onepose_st_amd", "csrc")
    for name in ("postopt.hip", "postopt_lm.hip"):
        text = open(os.path.join(csrc, name)).read()
        assert '#include "postopt_fold.h"' in text and "so3_log(" not in text and "aa_rotate(" not in text, name
    assert open(os.path.join(csrc, "postopt_fold.h")).read().count("void fold_row(") == 1


def test_solver_kernel_has_no_scratch_no_atomics_and_no_lds():
    """one wave per track and every lane holding the same sums: nothing to spill, to add atomically or to exchange through LDS"""
    assert os.path.exists(OBJDUMP), OBJDUMP
    with tempfile.TemporaryDirectory() as tmp:
        so = os.path.join(tmp, "lib.so")
        shutil.copy(postopt_lm.library_path(), so)
        subprocess.run([OBJDUMP, "--offloading", so], cwd=tmp, check=True, capture_output=True)
        code, = [n for n in os.listdir(tmp) if n.endswith("gfx950")]
        text = subprocess.run([OBJDUMP, "-d", os.path.join(tmp, code)], check=True, capture_output=True, text=True).stdout
    kernels, cur = {}, None
    for line in text.splitlines():
        hit = re.match(r"^[0-9a-f]+ <(\S+)>:$", line)
        if hit:
            cur = kernels.setdefault(hit.group(1), [])
        elif cur is not None and line.startswith("\t"):
            cur.append(line.strip().split("//")[0].strip())
    solver, = [k for k in kernels if "postopt_lm_kernel" in k]
    totals, = [k for k in kernels if "postopt_lm_totals_kernel" in k]
    for sym in (solver, totals):
        assert not [t for t in kernels[sym] if t.startswith("scratch_") or re.match(r"(global|flat)_atomic", t)], sym
    assert not [t for t in kernels[solver] if re.match(r"ds_(read|write|load|store)", t)]
    assert [t for t in kernels[solver] if t.startswith("ds_bpermute") or t.startswith("ds_swizzle") or "dpp" in t or t.startswith("v_permlane")]


def test_rejected_calls_answer_before_any_launch():
    _PTR = ctypes.c_void_p(256)          # not null and never followed: every call below returns from its argument checks
    params = postopt_lm._BINDING.header.prototypes["oplm_refine"].params

    def args(**given):
        return [given.get(n, None if c.endswith("*") else 0) for c, n in params]

    def last_error():
        return postopt_lm.load().oplm_last_error().decode()

    ptrs = {n: _PTR for c, n in params if c.endswith("*") and n not in ("residuals", "stream")}
    sizes = dict(P=2, L=5, F=3)
    consts = dict(lam0=1e-4, up=10.0, down=0.1, lam_min=1e-12, lam_max=1e12, step_tol=1e-8, max_iters=50)
    for change, text in ((dict(L=1), "bad sizes"), (dict(F=0), "bad sizes"), (dict(max_iters=-1), "max_iters outside [0, 2^20]"),
                         (dict(up=1.0), "LM constants"), (dict(lam0=float("nan")), "LM constants"), (dict(down=0.0), "LM constants"),
                         (dict(step_tol=float("inf")), "LM constants"), (dict(workspace_bytes=0), "workspace too small"),
                         (dict(workspace_bytes=4096, workspace=ctypes.c_void_p(8)), "workspace 256-byte")):
        with pytest.raises(ValueError, match=re.escape(text)):
            postopt_lm.call("oplm_refine", *args(**{**ptrs, **sizes, **consts, "workspace_bytes": 4096, **change}))
        assert text in last_error()


def test_cpu_tensors_are_refused_without_the_deeplm_warning():
    data = make_synthetic_sfm_tracks(0, n_frames=4, n_tracks=8, mean_len=3, long_len=0)
    rows = (data["depth"], data["n_query"], data["intrinsic0"], data["intrinsic1"], data["mkpts0_c"], data["mkpts1_f"],
            data["left_pose_idx"], data["right_pose_idx"], data["angle_axis_to_world"])
    with pytest.raises(hip.HipLibraryError):
        postopt.refine_depths_lm(*rows)
    with pytest.raises(ValueError):
        postopt.refine_depths_lm(*rows, max_iters=-1)
    agg = {k: data[k] for k in ("depth", "n_query", "intrinsic0", "intrinsic1", "mkpts0_c", "mkpts1_c", "mkpts1_f", "left_colmap_ids",
                                "right_colmap_ids", "point_cloud_id")}
    cfgs = {"solver_type": "SecondOrder", "residual_mode": "geometry_error", "optimize_lr": {"depth": 3e-2}, "optim_procedure": ["depth"],
            "hip_second_order": True}
    with warnings.catch_warnings(record=True) as caught:
        warnings.simplefilter("always")
        with pytest.raises(hip.HipLibraryError):
            postopt.Optimizer(cfgs).start_optimize(agg, data["frame_poses"])
    assert not [w for w in caught if "DeepLM" in str(w.message)]
    # the key alone changes nothing: any other solver type still warns and takes the first-order path
    with pytest.warns(UserWarning, match="DeepLM"), pytest.raises(hip.HipLibraryError):
        postopt.Optimizer(dict(cfgs, solver_type="DeepLM")).start_optimize(agg, data["frame_poses"])
    with pytest.warns(UserWarning, match="DeepLM"), pytest.raises(hip.HipLibraryError):
        postopt.Optimizer(dict(cfgs, hip_second_order=False)).start_optimize(agg, data["frame_poses"])
