"""The pose evaluation without a GPU: the numpy restatement of its specification (tests/pose_eval_oracle.py) against what the reference's
own functions returned (tests/golden/pose_eval_small.npz) and against independent forms, the PLY reader, ``aggregate_metrics``, the
header and binding of ``libonepose_pose_eval.so`` (what tests/test_cabi_binding.py does not state for every row of ``cabi.LIBRARIES``)
and its argument checks, which come before any HIP call and so answer on a machine with no device.

Bounds.  Two evaluation orders of the same exact mean differ by the rounding of the coordinates and of the sum: each coordinate of a
transformed vertex carries at most a few units of rounding of size ``S = max_k(sum_j |R[k][j] x_j| + |t_k|)``, and a sum of ``V`` terms
carries at most ``V`` roundings relative to itself: ``|got - ref| <= 2^-52 (32 S + V ref)``.  For the projection error the same holds in
pixels: ``S`` is then ``max_k(sum_j |K[k][j] X'_j|) / |u_2|``.  An angle moves by the rounding of the cosine's argument (9 products and
sums, a clamp, a division: below ``16 * 2^-53``) through the arc cosine's slope ``1 / sin(theta)``.  A translation error is a 3-term norm
and a scale: at most 4 roundings, ``4 * 2^-52`` relative."""
import ctypes
import os
import re
import struct

import numpy as np
import pytest
import torch

from onepose_st_amd import hip, pose_eval
from tests import pose_eval_oracle as po

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
EPS, coordinate_scale, pixel_scale, mean_bound = po.EPS, po.coordinate_scale, po.pixel_scale, po.mean_bound


@pytest.fixture(scope="module")
def golden():
    return dict(np.load(os.path.join(REPO, "tests", "golden", "pose_eval_small.npz")))


def test_golden_is_the_seeded_scene(golden):
    s = po.scene(seed=7, F=12, V=300, max_angle=6.0, max_shift=0.03)
    for k in ("verts", "pose_gt", "pose_pred", "K"):
        assert np.array_equal(s[k], golden[k]), k
    bbox = pose_eval.model_corners(golden["verts"].astype(np.float64))
    assert abs(pose_eval.model_diameter(bbox) - float(golden["diameter"])) <= 4 * EPS * float(golden["diameter"])
    assert golden["verts"].dtype == np.float32 and golden["verts"].shape == (300, 3) and golden["pose_gt"].shape == (12, 3, 4)
    assert (golden["R_errs_m"] >= 0.1).all()


@pytest.mark.parametrize("unit", ["m", "cm", "mm"])
def test_oracle_errors_against_the_reference(golden, unit):
    rot_cos, t_err, fl = po.errors(golden["pose_pred"], golden["pose_gt"], unit=unit)
    assert (fl == 0).all()
    ref_r, ref_t = golden[f"R_errs_{unit}"], golden[f"t_errs_{unit}"]
    bound_deg = np.rad2deg(16 * 2.0 ** -53 / np.sin(np.deg2rad(ref_r)))
    err_r, err_t = np.abs(po.angles(rot_cos) - ref_r), np.abs(t_err - ref_t)
    print("angle error / bound", (err_r / bound_deg).max(), "translation error / ulp", (err_t / (EPS * ref_t)).max())
    assert (err_r <= bound_deg).all()
    assert (err_t <= 4 * EPS * ref_t).all()


def test_oracle_means_against_the_reference_and_independent_forms(golden):
    scipy_spatial = pytest.importorskip("scipy.spatial")
    verts, pred, gt, K = golden["verts"], golden["pose_pred"], golden["pose_gt"], golden["K"]
    V, x = len(verts), golden["verts"].astype(np.float64)
    S = coordinate_scale(verts, pred, gt)
    add, adds, proj = po.add(verts, pred, gt), po.adds(verts, pred, gt), po.proj2d(verts, pred, gt, K)
    for f in range(len(gt)):
        a, b = x @ pred[f][:, :3].T + pred[f][:, 3], x @ gt[f][:, :3].T + gt[f][:, 3]
        ref_add = np.mean(np.linalg.norm(a - b, axis=-1))
        ref_adds = np.mean(scipy_spatial.cKDTree(a).query(b, k=1)[0])
        assert abs(add[f] - ref_add) <= mean_bound(S, V, ref_add), (f, add[f], ref_add)
        assert abs(adds[f] - ref_adds) <= mean_bound(S, V, ref_adds), (f, adds[f], ref_adds)
        assert ref_add == golden["add_mean"][f] and ref_adds == golden["adds_mean"][f]
    Spx = pixel_scale(verts, K, pred, gt)
    err = np.abs(proj - golden["proj2d"])
    print("proj2d error / bound", (err / mean_bound(Spx, V, golden["proj2d"])).max())
    assert (err <= mean_bound(Spx, V, golden["proj2d"])).all()
    # per-frame K: the shared one repeated gives the same bits
    assert np.array_equal(po.proj2d(verts, pred, gt, np.repeat(K[None], len(gt), axis=0)), proj)
    thr = float(golden["diameter"]) * float(golden["percentage"])
    assert np.array_equal(add < thr, golden["add"]) and np.array_equal(adds < thr, golden["adds"])
    assert (adds <= add + mean_bound(S, V, add)).all()                         # the nearest vertex is no further than the vertex's own image


def test_aggregate_equals_the_reference(golden):
    add = po.add(golden["verts"], golden["pose_pred"], golden["pose_gt"])
    rot_cos, t_err, _ = po.errors(golden["pose_pred"], golden["pose_gt"])
    metrics = {"R_errs": po.angles(rot_cos), "t_errs": t_err, "ADD_metric": add < float(golden["diameter"]) * float(golden["percentage"]),
               "proj2D_metric": po.proj2d(golden["verts"], golden["pose_pred"], golden["pose_gt"], golden["K"])}
    agg = pose_eval.aggregate_metrics(metrics)
    assert list(agg) == [str(k) for k in golden["aggregate_keys"]] == ["1cm@1degree", "3cm@3degree", "5cm@5degree", "ADD metric", "proj2D metric"]
    assert np.array_equal(np.array(list(agg.values())), golden["aggregate_values"])


def test_aggregate_metrics_hand_written():
    m = {"R_errs": [0.5, 2.0, 0.5, np.inf, np.nan, 4.9], "t_errs": [0.5, 0.5, 2.9, np.inf, 0.1, 5.0]}
    agg = pose_eval.aggregate_metrics(m)
    assert agg == {"1cm@1degree": 1 / 6, "3cm@3degree": 3 / 6, "5cm@5degree": 3 / 6}          # strict: 5.0 fails 5; inf and NaN fail all
    agg = pose_eval.aggregate_metrics({**m, "ADD_metric": [True, False, False, False, True, True], "proj2D_metric": [1.0, 5.0, 4.99, np.inf, np.nan, 7]},
                                      pose_thres=(3,), proj2d_thres=5)
    assert agg == {"3cm@3degree": 0.5, "ADD metric": 0.5, "proj2D metric": 2 / 6}
    empty = pose_eval.aggregate_metrics({"R_errs": [], "t_errs": [], "ADD_metric": [], "proj2D_metric": []})
    assert set(empty) == {"1cm@1degree", "3cm@3degree", "5cm@5degree", "ADD metric", "proj2D metric"} and all(np.isnan(v) for v in empty.values())


def test_oracle_flags_clamp_and_half_turn():
    I = np.concatenate([np.eye(3), np.zeros((3, 1))], axis=1)
    half = I.copy()
    half[:, :3] = np.diag([1.0, -1.0, -1.0])
    over = I.copy()
    over[:, :3] = np.eye(3) * (1 + 2.0 ** -30)              # trace of the pair with itself rounds above 3
    bad = I.copy()
    bad[1, 2] = np.nan
    pred, gt = np.stack([I, half, over, bad, I]), np.stack([I, I, over, I, I])
    rot_cos, t_err, fl = po.errors(pred, gt, no_pose=[0, 0, 0, 0, 1])
    assert list(fl) == [0, 0, 0, po.BAD_INPUT, po.NO_POSE]
    assert rot_cos[0] == 1.0 and rot_cos[1] == -1.0 and rot_cos[2] == 1.0 and np.isnan(rot_cos[3:]).all()
    assert list(t_err[:3]) == [0.0, 0.0, 0.0] and np.isinf(t_err[3:]).all()
    assert list(po.angles(rot_cos[:3])) == [0.0, 180.0, 0.0]
    verts = po.scene(1, 1, 5)["verts"]
    assert np.isinf(po.add(verts, pred, gt, fl)[3:]).all() and po.add(verts, pred, gt, fl)[0] == 0.0
    below = I.copy()
    below[:, :3] = np.diag([-1.0, -1.0, -1.0]) * (1 + 2.0 ** -30)             # not a rotation: the cosine's argument is below -1
    assert np.isnan(po.angles(po.errors(below[None], over[None])[0]))[0]       # NaN as in the reference, and NaN fails every threshold


def test_block_mean_is_the_written_order():
    g = np.random.default_rng(0)
    for V in (1, 255, 256, 257, 513):
        t = g.uniform(0, 1, size=V)
        s = np.zeros(((V + 255) // 256) * 256)
        s[:V] = t
        total = 0.0
        for b in range(len(s) // 256):
            blk = list(s[256 * b:256 * (b + 1)])
            stride = 128
            while stride:
                for l in range(stride):
                    blk[l] = blk[l] + blk[l + stride]
                stride //= 2
            total = total + blk[0]
        assert po.block_mean(t) == total / V
    assert po.block_mean(np.zeros(300)) == 0.0


def _write_ply(path, fmt, verts, props=("x", "y", "z"), coord="float", faces=0, truncate=0):
    """a PLY file of this test's own making: ``props`` in file order (others than x y z are uchar), ``coord`` float or double"""
    lines = ["ply", f"format {fmt} 1.0", "comment made by the test", f"element vertex {len(verts)}"]
    lines += [f"property {coord if p in 'xyz' else 'uchar'} {p}" for p in props]
    if faces:
        lines += [f"element face {faces}", "property list uchar int vertex_indices"]
    head = ("\n".join(lines) + "\nend_header\n").encode()
    body = b""
    for v in verts:
        vals = [float(v["xyz".index(p)]) if p in "xyz" else 200 for p in props]
        if fmt == "ascii":
            body += (" ".join(repr(x) for x in vals) + "\n").encode()
        else:
            body += b"".join(struct.pack("<d" if coord == "double" else "<f", x) if p in "xyz" else struct.pack("<B", x) for p, x in zip(props, vals))
    for _ in range(faces):
        body += b"3 0 1 2\n" if fmt == "ascii" else struct.pack("<Biii", 3, 0, 1, 2)
    data = head + body
    with open(path, "wb") as fh:
        fh.write(data[:len(data) - truncate] if truncate else data)


def test_ply_reader(tmp_path):
    g = np.random.default_rng(2)
    verts = g.uniform(-0.1, 0.1, size=(17, 3)).astype(np.float32)
    cases = [("ascii", dict()), ("binary_little_endian", dict()), ("ascii", dict(props=("x", "y", "z", "red", "green"), faces=3)),
             ("binary_little_endian", dict(props=("red", "x", "y", "nx", "z"), faces=2)), ("binary_little_endian", dict(coord="double")),
             ("ascii", dict(coord="double"))]
    for n, (fmt, kw) in enumerate(cases):
        path = str(tmp_path / f"model_{n}.ply")
        _write_ply(path, fmt, verts, **kw)
        got, bbox = pose_eval.load_model_points(path)
        assert got.dtype == np.float32 and bbox.dtype == np.float32 and np.array_equal(got, verts), (fmt, kw)
        lo, hi = verts.min(axis=0), verts.max(axis=0)
        assert np.array_equal(bbox[0], lo) and np.array_equal(bbox[7], hi) and bbox.shape == (9, 3)
        assert np.array_equal(bbox[1], [lo[0], lo[1], hi[2]]) and np.array_equal(bbox[4], [hi[0], lo[1], lo[2]])      # z fastest, x slowest
        assert np.array_equal(bbox[8], ((hi.astype(np.float64) + lo.astype(np.float64)) / 2).astype(np.float32))
        assert pose_eval.model_diameter(bbox) == float(np.linalg.norm(bbox[7] - bbox[0]))
        assert pose_eval.load_model_points(path, max_num=17)[0].shape == (17, 3)
        with pytest.raises(NotImplementedError, match="open3d"):
            pose_eval.load_model_points(path, max_num=16)
    for fmt, cut in (("binary_little_endian", 5), ("ascii", 30)):
        path = str(tmp_path / f"cut_{fmt}.ply")
        _write_ply(path, fmt, verts, truncate=cut)
        with pytest.raises(ValueError, match="truncated"):
            pose_eval.load_model_points(path)
    path = str(tmp_path / "big_endian.ply")
    _write_ply(path, "binary_big_endian", verts)
    with pytest.raises(ValueError, match="format"):
        pose_eval.load_model_points(path)
    (tmp_path / "not.ply").write_bytes(b"solid\n")
    with pytest.raises(ValueError, match="not a PLY"):
        pose_eval.load_model_points(str(tmp_path / "not.ply"))
    src = open(os.path.join(REPO, "onepose_st_amd", "pose_eval.py")).read()
    assert not re.search(r"^\s*(import|from)\s+(open3d|plyfile)", src, re.M)


def test_header_and_binding():
    assert pose_eval.ABI_VERSION == 1
    assert (pose_eval.NO_POSE, pose_eval.BAD_INPUT, pose_eval.BLOCK) == (po.NO_POSE, po.BAD_INPUT, po.BLOCK)
    assert pose_eval.MAX_VERTICES == 2 ** 18 and pose_eval.MAX_FRAMES >= 65536 and pose_eval.UNIT_SCALE == po.UNIT_SCALE
    assert pose_eval.MAX_VERTICES * pose_eval.BLOCK <= pose_eval.MAX_PAIRS_PER_LAUNCH        # one block of the largest model fits one launch
    mk = open(os.path.join(REPO, "onepose_st_amd", "csrc", "Makefile")).read()
    assert re.search(r"^EVL_FLAGS := -ffp-contract=off$", mk, re.M) and re.search(r"^EVL_HDRS := capi_error\.h ", mk, re.M)
    assert not re.search(r"^(SRCS|HDRS) :=.*pose_eval", mk, re.M)
    src = open(os.path.join(REPO, "onepose_st_amd", "csrc", "pose_eval.hip")).read()
    assert "#pragma clang fp contract(off)" in src and "__builtin_amdgcn_mfma" not in src


def test_rejected_calls_answer_before_any_launch():
    _PTR = ctypes.c_void_p(256)          # not null and never followed: every call below returns from its argument checks
    protos = pose_eval._BINDING.header.prototypes

    def args(name, **given):
        return [given.get(n, None if c.endswith("*") else 0) for c, n in protos[name].params]

    def last_error():
        return pose_eval.load().opevl_last_error().decode()

    entries = ("opevl_errors", "opevl_add", "opevl_adds", "opevl_proj2d")
    for name in entries:
        with pytest.raises(ValueError, match="null pointer"):
            pose_eval.call(name, *args(name))
        assert last_error() == f"{name}: null pointer"
    good = dict(V=300, frames=4, pred_stride=12, gt_stride=16, unit_scale=100.0, k_shared=1)
    for name in entries:
        optional = ("status", "stream") if name == "opevl_errors" else ("flags", "stream")       # flags: an output of errors, optional elsewhere
        ptrs = {n: _PTR for c, n in protos[name].params if c.endswith("*") and n not in optional}
        base = {**ptrs, **{k: v for k, v in good.items() if k in {n for _, n in protos[name].params}}}
        changes = [(dict(frames=0), "frames outside"), (dict(frames=pose_eval.MAX_FRAMES + 1), "frames outside"), (dict(pred_stride=9), "pose stride"),
                   (dict(gt_stride=0), "pose stride")]
        if name == "opevl_errors":
            changes += [(dict(unit_scale=0.0), "unit_scale"), (dict(unit_scale=float("nan")), "unit_scale")]
        else:
            changes += [(dict(V=0), "V outside"), (dict(V=pose_eval.MAX_VERTICES + 1), "V outside")]
        if name == "opevl_adds":
            changes += [(dict(pair_budget=300 * 256 - 1), "pair_budget outside"), (dict(pair_budget=pose_eval.MAX_PAIRS_PER_LAUNCH + 1), "pair_budget outside"),
                        (dict(pair_budget=-1), "pair_budget outside"), (dict(V=100, pair_budget=100 * 100 - 1), "pair_budget outside")]
        for change, text in changes:
            with pytest.raises(ValueError, match=re.escape(text)):
                pose_eval.call(name, *args(name, **{**base, **change}))
            assert text in last_error()


def test_python_api_refuses_cpu_tensors_and_bad_options():
    s = po.scene(3, 2, 7)
    pred, gt = torch.tensor(s["pose_pred"]), torch.tensor(s["pose_gt"])
    with pytest.raises(hip.HipLibraryError):
        pose_eval.pose_errors(pred, gt)
    with pytest.raises(hip.HipLibraryError):
        pose_eval.pose_errors(pred, s["pose_gt"], model_points=torch.tensor(s["verts"]), K=s["K"], symmetric=True)
    with pytest.raises(TypeError):
        pose_eval.pose_errors(s["pose_pred"], gt)
    with pytest.raises(NotImplementedError, match="unit"):
        pose_eval.pose_errors(pred, gt, unit="km")
    with pytest.raises(ValueError, match="K without model_points"):
        pose_eval.pose_errors(pred, gt, K=s["K"])
    with pytest.raises(ValueError, match="no records"):
        pose_eval.evaluate_records([], s["pose_gt"])
    with pytest.raises(ValueError, match="key"):
        pose_eval.evaluate_records([{"pose": s["pose_pred"][0], "inliers": np.arange(5)}], s["pose_gt"][:1], key="bbox")
    data = {"mkpts_query_f": torch.zeros(8, 2), "mkpts_3d_db": torch.zeros(8, 3), "m_bids": torch.zeros(8, dtype=torch.int64)}
    cfg = {"point_cloud_rescale": 1000, "pnp_reprojection_error": 7, "model_unit": "m", "use_pycolmap_ransac": False}
    with pytest.raises(NotImplementedError, match="adaptive policy"):
        pose_eval.compute_query_pose_errors(data, s["K"], gt, cfg)
    with pytest.raises(hip.HipLibraryError):
        pose_eval.compute_query_pose_errors(data, s["K"], gt, {**cfg, "use_pycolmap_ransac": True})
    errs = pose_eval.DevicePoseErrors(*(torch.tensor(v) for v in (np.array([0.5, np.nan]), np.array([1.0, np.inf]), np.array([0.01, np.inf]))), None,
                                      torch.tensor([0, pose_eval.NO_POSE], dtype=torch.int32))
    host = errs.to_host(diameter=0.2)                       # the packing itself needs no device
    assert host["R_errs"][0] == np.rad2deg(np.arccos(0.5)) and np.isinf(host["R_errs"][1]) and np.isinf(host["t_errs"][1])
    assert list(host["ADD_metric"]) == [True, False] and "proj2D_metric" not in host and list(host["flags"]) == [0, 1]
