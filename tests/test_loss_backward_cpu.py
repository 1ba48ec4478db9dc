"""The loss backward (``onepose_st_amd/loss_backward.py``, include/ext/onepose_loss_backward.h) without a GPU: the numpy
float64 oracle (``tests/loss_backward_oracle.py``) against what the reference itself computed under float64 autograd
(``tests/golden/loss_backward_small.npz``, recipe ``tests/golden/make_loss_backward_golden.py``) and against difference quotients of the
loss it differentiates; the header, the binding and the calls the built library refuses before any launch; the precision bar of the
coarse entry's device test, derived here from a float32 split-bf16 stand-in over that test's cases; and the seeded faults, each measured
against that bar."""
import ctypes
import os
import re

import numpy as np
import pytest
import torch

from onepose_st_amd import cabi, hip, loss_backward, supervision
from tests import loss_backward_cases as cases
from tests import loss_backward_oracle as oracle
from tests.golden import make_loss_backward_golden as recipe

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
FEATURES = ("feat0", "feat1", "feat_f0", "feat_f1")


@pytest.fixture(scope="module")
def golden():
    return dict(np.load(os.path.join(REPO, "tests", "golden", "loss_backward_small.npz")))


def oracle_grads(g):
    cfg = recipe.LOSS_CONFIG
    coarse = oracle.coarse_grads(g["feat0"], g["feat1"], g["gt_j"], recipe.TEMPERATURE, cfg["focal_alpha"], cfg["focal_gamma"], cfg["pos_weight"],
                                 cfg["neg_weight"], scale=cfg["coarse_weight"])
    fine = oracle.fine_grads(g["feat_f0"], g["feat_f1"], g["ref_expec_f"], g["expec_f_gt"], correct_thr=cfg["fine_correct_thr"],
                             scale=cfg["fine_weight"])
    return {"feat0": coarse["grad0"], "feat1": coarse["grad1"], "feat_f0": fine["grad_f0"], "feat_f1": fine["grad_f1"]}, coarse, fine


def test_golden_is_the_seeded_inputs(golden):
    inputs = recipe.make_inputs()
    for key, value in inputs.items():
        assert golden[key].dtype == value.dtype and np.array_equal(golden[key], value), key
    assert golden["feat0"].shape == (2, 19, 256) and golden["feat1"].shape == (2, 23, 256) and golden["feat_f1"].shape == (11, 25, 128)
    conf, pos = golden["ref_conf_matrix"], oracle.positives(golden["gt_j"], 23)
    # what the case plants: positives below 1e-6, one above 1 - 1e-6, confident positives and negatives, rows that are not correct
    assert (conf[pos] < 1e-6).sum() == 4 and (conf[pos] > 1 - 1e-6).sum() == 1 and (conf[pos] > 0.5).sum() > 8 and (conf[~pos] > 0.1).sum() == 3
    assert (np.abs(golden["expec_f_gt"]).max(axis=1) >= 1.0).sum() == 4
    assert np.array_equal(golden["expec_f"], golden["ref_expec_f"].astype(np.float32))


def test_oracle_equals_the_reference_at_float64_rounding(golden):
    """The bar: 1e-12 of the tensor's largest gradient (float64 rounding; the float32 level is 7e-8)"""
    got, coarse, fine = oracle_grads(golden)
    assert np.abs(coarse["conf"] - golden["ref_conf_matrix"]).max() <= 1e-14
    co, _ = oracle.fine_expectation(golden["feat_f0"], golden["feat_f1"])
    assert np.abs(co - golden["ref_expec_f"][:, :2]).max() <= 1e-14
    assert fine["status"] == oracle.OK and fine["n_correct"] == 7
    for key in FEATURES:
        want = golden[f"ref_grad_{key}"]
        err = np.abs(got[key] - want).max() / np.abs(want).max()
        assert got[key].shape == want.shape and err <= 1e-12, (key, err)
    loss = oracle.total_loss(golden["feat0"], golden["feat1"], golden["gt_j"], recipe.TEMPERATURE, golden["feat_f0"], golden["feat_f1"],
                             golden["ref_expec_f"], golden["expec_f_gt"], recipe.LOSS_CONFIG)
    assert abs(loss - float(golden["ref_loss"])) <= 1e-14 * abs(loss)
    assert not got["feat_f0"][[2, 5, 6, 9]].any() and not got["feat_f1"][[2, 5, 6, 9]].any()         # rows that are not correct: zeros


def test_oracle_is_the_gradient_of_the_loss_it_differentiates(golden):
    """Central differences of the float64 forward along 8 seeded directions per tensor against <grad, d>.  Step 1e-5 on features of size
    1: the truncation error is about h^2 = 1e-10 of the directional derivative, the rounding error 1e-16 / h = 1e-11 of the loss."""
    got, _, _ = oracle_grads(golden)
    rng = np.random.default_rng(5)
    h = 1e-5

    def loss_at(**changed):
        x = {k: golden[k].astype(np.float64) for k in FEATURES}
        x.update(changed)
        return oracle.total_loss(x["feat0"], x["feat1"], golden["gt_j"], recipe.TEMPERATURE, x["feat_f0"], x["feat_f1"], golden["ref_expec_f"],
                                 golden["expec_f_gt"], recipe.LOSS_CONFIG)
    for key in FEATURES:
        x = golden[key].astype(np.float64)
        for _ in range(8):
            d = rng.standard_normal(x.shape)
            d /= np.linalg.norm(d)
            quotient = (loss_at(**{key: x + h * d}) - loss_at(**{key: x - h * d})) / (2 * h)
            want = float((got[key] * d).sum())
            assert abs(quotient - want) <= 1e-6 * abs(want) + 1e-10, (key, quotient, want)


# ---- header and binding ----------------------------------------------------------------------------------------------------------------
SYMBOLS = ("opbwd_abi_version", "opbwd_last_error", "opbwd_coarse_workspace_bytes", "opbwd_coarse_grads", "opbwd_fine_grads")
PARAMS = {
    "opbwd_coarse_workspace_bytes": ("B", "N", "M"),
    "opbwd_coarse_grads": ("feat0", "feat1", "gt_j", "gt_i", "B", "N", "M", "temperature", "alpha", "gamma", "pos_weight", "neg_weight", "scale",
                           "workspace", "workspace_bytes", "grad0", "grad1", "stream"),
    "opbwd_fine_grads": ("feat_f0", "feat_f1", "expec_f", "expec_f_gt", "count", "cap", "W", "correct_thr", "training", "scale", "grad_f0", "grad_f1",
                         "n_correct", "status", "stream"),
}


def test_header_and_binding(tmp_path):
    entry, = cabi.BACKWARD
    assert tuple(entry) == ("opbwd", "ext/onepose_loss_backward.h", "libonepose_loss_backward.so", "OPBWD_LIB", "loss_backward")
    for table in (cabi.LIBRARIES, cabi.EXTENSIONS, cabi.ADDONS, cabi.TRAINING):   # disjoint, column by column
        assert entry not in table
        for column, taken in zip(entry, zip(*table)):
            assert column not in taken
    text = open(os.path.join(REPO, "include", "ext", "onepose_loss_backward.h")).read()
    header = cabi.parse(text, cabi.names_of("opbwd"))
    assert tuple(header.prototypes) == SYMBOLS == loss_backward.EXPORTED_SYMBOLS
    for name, params in PARAMS.items():
        assert tuple(n for _, n in header.prototypes[name].params) == params, name
    types = dict((n, c) for c, n in header.prototypes["opbwd_coarse_grads"].params)
    assert all(types[n] == "double" for n in ("temperature", "alpha", "gamma", "pos_weight", "neg_weight", "scale"))
    assert (types["gt_j"], types["gt_i"], types["workspace_bytes"], types["grad0"]) == ("const long long*", "const long long*", "size_t", "float*")
    assert header.prototypes["opbwd_coarse_workspace_bytes"].ret == "size_t"
    assert header.defines == {"OPBWD_ABI_VERSION": 1, "OPBWD_BLOCK": 256, "OPBWD_OWNED_ROWS": 128, "OPBWD_SWEPT_ROWS": 32, "OPBWD_CHANNELS": 256,
                              "OPBWD_FINE_CHANNELS": 128, "OPBWD_MAX_BATCH": 65535, "OPBWD_MAX_ROWS": 2 ** 20, "OPBWD_OK": 0, "OPBWD_NONE": 1,
                              "OPBWD_FORCED": 2, "OPBWD_EMPTY": 3}
    assert (loss_backward.OK, loss_backward.NONE, loss_backward.FORCED, loss_backward.EMPTY) == (oracle.OK, oracle.NONE, oracle.FORCED, oracle.EMPTY) \
        == (supervision.OK, supervision.NONE, supervision.FORCED, supervision.EMPTY)
    assert loss_backward.BLOCK == supervision.BLOCK == 256 and loss_backward.ABI_VERSION == 1
    assert (loss_backward.CHANNELS, loss_backward.FINE_CHANNELS) == (oracle.CHANNELS, oracle.FINE_CHANNELS)
    for words in ("2 * u_ij - Pr_ij * r_i - Pc_ij * c_j", "gets NO", "v_mfma_f32_32x32x16_bf16", "identical bytes", "frag_planes_kernel"):
        assert words in text, words                                               # the header states the formulas, the quirk and the passes
    assert cabi.parse(text).prototypes == {}                                      # the table's reader does not know the prefix
    assert cabi.Binding.of("onepose_st_amd.loss_backward").header_path == loss_backward._BINDING.header_path
    for folder in ("include", os.path.join("include", "ext")):                    # no other header is the place of these entry points
        for other in os.listdir(os.path.join(REPO, folder)):
            if other.endswith(".h") and other != "onepose_loss_backward.h":
                assert "opbwd_" not in open(os.path.join(REPO, folder, other)).read()
    mk = open(os.path.join(REPO, "onepose_st_amd", "csrc", "Makefile")).read()
    assert re.search(r"^BWD_SRCS := loss_backward.hip$", mk, re.M)
    hdrs = re.search(r"^BWD_HDRS := (.*)$", mk, re.M).group(1).split()
    assert {"capi_error.h", "device_loop.h", "reduce_f64.h", "tile_bf16.h"} <= set(hdrs)
    assert len(re.findall(r"^\$\(eval \$\(call satellite,BWD,bwd,loss_backward\)\)$", mk, re.M)) == 1
    src = open(os.path.join(REPO, "onepose_st_amd", "csrc", "loss_backward.hip")).read()
    for shared in ('#include "tile_bf16.h"', '#include "reduce_f64.h"', '#include "device_loop.h"', "red64::block_sums", "mma_bf16<3>"):
        assert shared in src, shared                                              # shared code is included, not copied
    assert "atomicAdd" not in src and "atomic_add" not in src                     # no float atomics (and no other)
    entry_py = open(os.path.join(REPO, "__graft_entry__.py")).read()
    assert "cabi.LIBRARIES + cabi.EXTENSIONS + cabi.ADDONS + cabi.TRAINING + cabi.BACKWARD" in entry_py       # build() checks and loads it
    py = open(os.path.join(REPO, "onepose_st_amd", "loss_backward.py")).read()
    assert not re.search(r"^\s*(from|import)\s+(oracle|tests)\b", py, re.M)       # the product does not import oracle or tests
    absent = cabi.Binding(entry.header, entry.so, entry.prefix, "OPBWD_NO_SUCH_VARIABLE", names=cabi.names_of("opbwd"))
    absent.path = str(tmp_path / "libonepose_absent.so")
    with pytest.raises(cabi.HipLibraryError, match="libonepose_absent.so not found"):
        absent.load()


P_ = ctypes.c_void_p(1 << 20)                                                    # never dereferenced: every call below is refused first
GOOD = {
    "opbwd_coarse_grads": dict(feat0=P_, feat1=P_, gt_j=P_, gt_i=P_, B=2, N=64, M=30, temperature=0.1, alpha=0.25, gamma=2.0, pos_weight=1.0,
                               neg_weight=1.0, scale=1.0, workspace=P_, workspace_bytes=1 << 30, grad0=P_, grad1=P_, stream=None),
    "opbwd_fine_grads": dict(feat_f0=P_, feat_f1=P_, expec_f=P_, expec_f_gt=P_, count=None, cap=16, W=5, correct_thr=1.0, training=1, scale=1.0,
                             grad_f0=P_, grad_f1=P_, n_correct=P_, status=P_, stream=None),
}


def test_names_and_arity_without_a_library(monkeypatch):
    monkeypatch.setattr(loss_backward._BINDING, "load", lambda: pytest.fail("the names are checked without the library"))
    for name, named in GOOD.items():
        args = loss_backward.order(name, **dict(reversed(list(named.items()))))
        assert args == tuple(named.values()) and len(args) == len(PARAMS[name])
        loss_backward.check_arity(name, args)
        with pytest.raises(TypeError, match=f"{name} takes {len(args)} arguments"):
            loss_backward.check_arity(name, args[:-1])
    with pytest.raises(TypeError, match="missing status; unknown flags"):
        loss_backward.order("opbwd_fine_grads", **{**{n: 0 for n in PARAMS["opbwd_fine_grads"] if n != "status"}, "flags": 0})
    with pytest.raises(TypeError, match="missing grad1; unknown grad"):
        loss_backward.launch("opbwd_coarse_grads", {**{n: None for n in PARAMS["opbwd_coarse_grads"][:-2]}, "grad": None})


def test_built_library_rejects_before_any_launch():
    assert os.path.exists(loss_backward.library_path()), "libonepose_loss_backward.so: run __graft_entry__.build()"
    lib = loss_backward.load()
    assert all(hasattr(lib, s) for s in SYMBOLS) and lib.opbwd_abi_version() == 1
    # per side two plane sets of 1 KiB per padded row and three statistics of 4 bytes per padded row + 32, each rounded up to 256; 256 of constants
    def want_bytes(B, N, M):
        total = 256
        for rows in (N, M):
            pad = -(-rows // 32) * 32
            total += 2 * B * pad * 1024 + 3 * (-(-(B * (pad + 32) * 4) // 256) * 256)
        return total
    for shape in ((1, 1, 1), (2, 300, 1295), (4, 7000, 4800), (3, 33, 31)):
        assert lib.opbwd_coarse_workspace_bytes(*shape) == want_bytes(*shape), shape
    assert lib.opbwd_coarse_workspace_bytes(4, 7000, 4800) < 4 * (7000 + 4800 + 64) * 2200       # O(B (N + M)): nothing N x M
    assert lib.opbwd_coarse_workspace_bytes(0, 5, 5) == 0 and lib.opbwd_coarse_workspace_bytes(1, 2 ** 20 + 1, 5) == 0

    def refused(name, message, **change):
        with pytest.raises(ValueError, match=message):
            loss_backward.call(name, *loss_backward.order(name, **{**GOOD[name], **change}))
    for name, args in GOOD.items():
        for key, value in args.items():
            if value is P_ and key != "gt_i":                                     # (gt_i is accepted and not read: the header says why)
                refused(name, f"^{name}: {name}: null pointer$", **{key: None})
    refused("opbwd_coarse_grads", "B outside", B=0)
    refused("opbwd_coarse_grads", "B outside", B=65536)
    refused("opbwd_coarse_grads", "N and M", N=0)
    refused("opbwd_coarse_grads", "N and M", M=2 ** 20 + 1)
    refused("opbwd_coarse_grads", "16-byte aligned", feat1=ctypes.c_void_p((1 << 20) + 4))
    refused("opbwd_coarse_grads", "256-byte aligned", workspace=ctypes.c_void_p((1 << 20) + 16))
    refused("opbwd_coarse_grads", "finite", gamma=float("nan"))
    refused("opbwd_coarse_grads", "finite", scale=float("inf"))
    refused("opbwd_coarse_grads", "positive", temperature=-0.5)
    refused("opbwd_coarse_grads", "workspace_bytes below", workspace_bytes=lib.opbwd_coarse_workspace_bytes(2, 64, 30) - 1)
    refused("opbwd_fine_grads", "cap outside", cap=0)
    refused("opbwd_fine_grads", "cap outside", cap=2 ** 20 + 1)
    for w in (1, 4, 13):
        refused("opbwd_fine_grads", "window: odd, from 3 to 11", W=w)
    refused("opbwd_fine_grads", "correct_thr", correct_thr=float("nan"))
    refused("opbwd_fine_grads", "scale: finite", scale=float("nan"))


def test_python_api_and_the_models_switch():
    from onepose_st_amd.config import default_config
    from onepose_st_amd.model import OnePosePlus_model
    gt = supervision.GroundTruth(torch.zeros(2, 4, dtype=torch.int64), torch.zeros(2, 4, 2), torch.zeros(2, 6, dtype=torch.int64),
                                 torch.zeros(2, dtype=torch.int32), (2, 3))
    f0, f1 = torch.zeros(2, 4, 256), torch.zeros(2, 6, 256)
    ff0, ff1, ef, eg = torch.zeros(3, 128), torch.zeros(3, 25, 128), torch.zeros(3, 3), torch.zeros(3, 2)
    for call in (lambda: loss_backward.coarse_grads(f0, f1, gt, temperature=0.1), lambda: loss_backward.fine_grads(ff0, ff1, ef, eg)):
        with pytest.raises(hip.HipLibraryError, match=re.escape(hip.NO_CPU_FALLBACK)):
            call()
    with pytest.raises(ValueError, match="feat_f1"):
        loss_backward.fine_grads(ff0, torch.zeros(3, 16, 128), ef, eg)
    with pytest.raises(ValueError, match="feat_f0"):
        loss_backward.fine_grads(ff0.double(), ff1, ef, eg)
    with pytest.raises(ValueError, match="at least one match"):
        loss_backward.fine_grads(ff0[:0], ff1[:0], ef[:0], eg[:0])
    with pytest.raises(TypeError, match="feat_f0: expected a tensor"):
        loss_backward.fine_grads(None, ff1, ef, eg)
    assert set(vars(loss_backward.stages)) >= {"coarse_grads", "fine_grads"}
    cfg = default_config()
    data = {"conf_matrix_gt": torch.zeros(2, 4, 6), "fine_location_matrix_gt": torch.zeros(2, 4, 6, 2), "expec_f": ef, "expec_f_gt": eg}
    with pytest.raises(KeyError, match="feat_c0.*hip_keep_features"):
        loss_backward.backward(dict(data), recipe.LOSS_CONFIG, {"OnePosePlus": cfg})
    with pytest.raises(KeyError, match="feat_f0.*hip_keep_features"):
        loss_backward.backward({**data, "feat_c0": f0, "feat_c1": f1}, recipe.LOSS_CONFIG, cfg)
    with pytest.raises(NotImplementedError, match="mask0"):
        loss_backward.backward({**data, "mask0": None}, recipe.LOSS_CONFIG, cfg)
    with pytest.raises(NotImplementedError, match="focal"):
        loss_backward.backward({**data, "feat_c0": f0, "feat_c1": f1, "feat_f0": ff0, "feat_f1": ff1}, {**recipe.LOSS_CONFIG, "coarse_type": "ce"}, cfg)
    assert "hip_keep_features" not in cfg                                         # an opt-in key
    assert not OnePosePlus_model(cfg).keep_features and OnePosePlus_model({**cfg, "hip_keep_features": True}).keep_features


# ---- the precision bar of the coarse entry, and the seeded faults ---------------------------------------------------------------------------
@pytest.fixture(scope="module")
def standin_errors():
    """name -> frame_error of the float32 split-bf16 stand-in against the float64 oracle, over the device test's cases"""
    out = {}
    for name, (args, kw) in cases.COARSE_CASES.items():
        case = cases.coarse_case(**args)
        want = oracle.coarse_grads(case["feat0"], case["feat1"], case["gt_j"], cases.TEMPERATURE, **kw)
        s0, s1 = oracle.coarse_standin(case["feat0"], case["feat1"], case["gt_j"], cases.TEMPERATURE, **kw)
        out[name] = (max(oracle.frame_error(s0, want["grad0"]), oracle.frame_error(s1, want["grad1"])), want)
    return out


def test_the_cases_meet_the_condition(standin_errors):
    """No positive's confidence within 1 % of 1e-6, no element within 1e-9 of 1 - 1e-6: across those bounds g jumps, so an element that
    straddles one would be a property of the input, not of the kernel.  No case is left out."""
    assert set(standin_errors) == set(cases.COARSE_CASES) and len(standin_errors) == 26
    shapes = {(a["N"], a["M"]) for a, _ in cases.COARSE_CASES.values()}
    assert {(n, m) for n in (1, cases.R - 1, cases.R, cases.R + 1, 2 * cases.R + 1) for m in (2, cases.S - 1, cases.S, cases.S + 1)} <= shapes
    assert (300, 35 * 37) in shapes
    for name, (_, want) in standin_errors.items():
        assert want["pos_margin"] >= 0.01 and want["hi_margin"] >= 1e-9, (name, want["pos_margin"], want["hi_margin"])
    below = sum(int((w["conf"][w["is_pos"]] < 1e-6).sum()) for _, w in standin_errors.values())
    assert below > 80                                                             # positives that must get no direct gradient


def test_the_precision_bar(standin_errors):
    """The project's method: the statistic is |y - y_ref| / max |y_ref over the frame's tensor|, worst element; the bar
    is twice the worst value of a float32 stand-in that splits at the kernel's operand points (feat / 16 for S; dS and the swept operand
    for the gradient products).  Measured here: 2.98e-5 (case no_positive: confident negatives alone, where 1 / (1 - c) amplifies the
    rounding of c); the median case 8.5e-6.  So the bar is 6.0e-5.  Nothing comes from a device;
    ``cases.STANDIN_WORST`` records the value and this test holds it to what it measures (float32 sums differ a little between BLAS builds)."""
    worst = max(e for e, _ in standin_errors.values())
    print({k: f"{e:.2e}" for k, (e, _) in standin_errors.items()})
    assert 0.75 * cases.STANDIN_WORST <= worst <= 1.15 * cases.STANDIN_WORST, worst
    assert cases.COARSE_BAR == 2 * cases.STANDIN_WORST and 2e-5 < cases.COARSE_BAR < 1e-4


FAULT_CASES = {"rc_exchanged": dict(seed=41, B=1, N=70, M=70), "no_factor_2": dict(seed=42, B=1, N=70, M=45),
               "no_clamp_mask": dict(seed=43, B=1, N=70, M=45, pushed=True), "per_frame_counts": dict(seed=44, B=2, N=70, M=45, empty_frames=(1,)),
               "pr_pc_exchanged": dict(seed=45, B=1, N=70, M=45)}


@pytest.mark.parametrize("fault", list(FAULT_CASES))
def test_seeded_faults_lie_far_outside_the_bar(fault):
    """Each fault's frame_error against the true gradient, in units of the bar (6.0e-5); each must be at least 10.  Measured:
    rc_exchanged 7.8e3, no_factor_2 8.5e3, no_clamp_mask 3.6e2, per_frame_counts 1.7e4, pr_pc_exchanged 3.1e3."""
    case = cases.coarse_case(**FAULT_CASES[fault])
    want = oracle.coarse_grads(case["feat0"], case["feat1"], case["gt_j"], cases.TEMPERATURE)
    got = oracle.coarse_grads(case["feat0"], case["feat1"], case["gt_j"], cases.TEMPERATURE, faults={fault})
    err = min(oracle.frame_error(got["grad0"], want["grad0"]), oracle.frame_error(got["grad1"], want["grad1"]))
    print(f"{fault}: {err / cases.COARSE_BAR:.3g} bars")
    assert err >= 10 * cases.COARSE_BAR, (fault, err)
