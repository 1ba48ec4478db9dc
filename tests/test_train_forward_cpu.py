"""The training-mode forward's own step (``onepose_st_amd/train_forward.py``, include/ext/onepose_train_forward.h)
without a GPU: the numpy oracle (``tests/train_forward_oracle.py``) against what the reference itself computed
(``tests/golden/train_forward_small.npz``, recipe ``tests/golden/make_train_forward_golden.py``) -- exactly, on every key of every case --
the sampler, the binding's header-driven parts, the calls the built library refuses before any launch, and the model's switch."""
import ctypes
import os
import re

import numpy as np
import pytest
import torch

from onepose_st_amd import cabi, hip, supervision, train_forward
from tests import train_forward_oracle as oracle
from tests.golden import make_train_forward_golden as recipe

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
T, G = 18, recipe.G


@pytest.fixture(scope="module")
def golden():
    return dict(np.load(os.path.join(REPO, "tests", "golden", "train_forward_small.npz")))


def case_of(golden, name):
    return {k[len(name) + 2:]: v for k, v in golden.items() if k.startswith(name + "__")}


def oracle_run(c):
    pred = {"b_ids": c["pred_b_ids"], "i_ids": c["pred_i_ids"], "j_ids": c["pred_j_ids"], "mconf": c["pred_mconf"],
            "mkpts_3d": c["pred_mkpts_3d_db"], "mkpts_c": c["pred_mkpts_query_c"]}
    return oracle.pad_matches(pred, None, c["gt_j"], c["keypoints3d"], recipe.M, recipe.HW_C[1], T, G, recipe.SEED, int(c["step"]),
                              recipe.HW_I[0] / recipe.HW_C[0], c.get("scale"))


def test_golden_is_the_seeded_inputs(golden):
    assert oracle.train_rows(recipe.B, recipe.N, recipe.M, recipe.PERCENT) == T and T - G == 13
    inputs = recipe.make_inputs()
    assert list(inputs) == list(recipe.CASES) and {k.split("__")[0] for k in golden} == set(inputs)
    for name, inp in inputs.items():
        c = case_of(golden, name)
        for key in ("conf_matrix", "gt_j", "keypoints3d"):
            assert np.array_equal(inp[key], c[key]), (name, key)
        assert int(c["step"]) == inp["step"] and (("scale" in c) == (inp["scale"] is not None))
        assert len(c["pred_b_ids"]) == recipe.CASES[name][0]                     # P
    assert sorted(len(case_of(golden, n)["pred_b_ids"]) for n in ("p0", "p5", "p13", "p14", "p40")) == [0, 5, 13, 14, 40]
    assert int((case_of(golden, "one_gt")["gt_j"] >= 0).sum()) == 1
    assert int((case_of(golden, "batch1_gt")["gt_j"][0] >= 0).sum()) == 0 < int((case_of(golden, "batch1_gt")["gt_j"][1] >= 0).sum())


@pytest.mark.parametrize("name", list(recipe.CASES))
def test_oracle_equals_the_reference_exactly(golden, name):
    c = case_of(golden, name)
    out = oracle_run(c)
    P = len(c["pred_b_ids"])
    assert out["status"] == oracle.OK and out["count"] == T and out["n_keep"] == min(P, T - G)
    got = oracle.reference_keys(out)
    assert set(got) == set(recipe.KEYS)
    for key in recipe.KEYS:
        want = c[f"ref_{key}"]
        assert got[key].dtype == want.dtype and got[key].shape == want.shape and got[key].tobytes() == want.tobytes(), (name, key)
    # what the case is there for
    n = out["n_keep"]
    assert not out["gt_mask"][:n].any() and out["gt_mask"][n:].all() and len(out["gt_picks"]) == T - n >= G
    if P <= T - G:
        assert np.array_equal(out["sources"], np.arange(P))                      # the keep-all branch: in order
    else:
        assert len(out["sources"]) == T - G and len(set(out["sources"].tolist())) > 1 and out["sources"].max() < P
    if name == "one_gt":
        assert len(set(out["gt_picks"].tolist())) == 1
    if name == "batch1_gt":
        assert (out["b_ids"][n:] == 1).all()
    if name == "scaled":
        b, j = out["b_ids"][n:], out["j_ids"][n:]
        assert np.array_equal(out["mkpts_c"][n:, 0], (j % 6).astype(np.float32) * (np.float32(8) * recipe.SCALE[b, 1]))
        assert len(set(b.tolist())) == 2 and not np.array_equal(out["mkpts_c"][n:, 0], (j % 6).astype(np.float32) * np.float32(8))


def test_the_oracle_pads_from_the_sparse_ground_truth_in_torch_where_order(golden):
    c = case_of(golden, "p14")
    gt_j = torch.from_numpy(c["gt_j"])
    gt_i = torch.full((recipe.B, recipe.M), -1, dtype=torch.int64)
    sparse = supervision.GroundTruth(gt_j, torch.zeros(recipe.B, recipe.N, 2), gt_i, torch.zeros(recipe.B, dtype=torch.int32), recipe.HW_C)
    b, i, j = torch.where(sparse.to_dense()[0])
    rows, n = oracle.gt_list(c["gt_j"], recipe.M)
    assert n == len(b) == 40 and rows.dtype == np.int32 and np.array_equal(rows, (b * recipe.N + i).numpy())
    assert np.array_equal(c["gt_j"].reshape(-1)[rows], j.numpy())
    far = c["gt_j"].copy()
    far[0, 0], far[1, 5] = recipe.M, -7                                          # a cell outside the grid is no ground truth
    assert not set(oracle.gt_list(far, recipe.M)[0].tolist()) & {0, recipe.N + 5}
    assert oracle.gt_list(np.full((2, 3), -1), 4)[1] == 0
    none = oracle.pad_matches({k: c[f"pred_{k}"] for k in ("b_ids", "i_ids", "j_ids", "mconf")} | {"mkpts_3d": c["pred_mkpts_3d_db"],
                              "mkpts_c": c["pred_mkpts_query_c"]}, None, np.full((2, 64), -1), c["keypoints3d"], 30, 6, T, G, 1, 0, 8.0)
    assert none == {"count": 0, "n_keep": 13, "status": oracle.NO_GT}


def test_the_sampler():
    assert oracle.mix64(0x9E3779B97F4A7C15) == 0xE220A8397B1DCDAF == oracle.h(0, 0, 0, 0)          # splitmix64's first output from state 0
    assert oracle.h(2 ** 64 - 1, 0, 0, 0) == oracle.mix64(0x9E3779B97F4A7C15 - 1)                   # modulo 2^64
    assert oracle.h(5, 3, 1, 9) == oracle.mix64((5 + 0x9E3779B97F4A7C15 * (((7 << 32) | 9) + 1)) % 2 ** 64)
    draws = {(step, c): tuple(oracle.picks(7, step, c, 1000, 16).tolist()) for step in (0, 1, oracle.MAX_STEP - 1) for c in (0, 1)}
    assert len(set(draws.values())) == 6 and all(0 <= v < 1000 for d in draws.values() for v in d)
    assert oracle.picks(7, 0, 1, 1, 5).tolist() == [0] * 5
    counts = np.bincount(oracle.picks(11, 2, 1, 8, 4000), minlength=8)           # with replacement, and even: 500 +- 4 sigma (sigma ~ 21)
    assert counts.min() > 400 and counts.max() < 600


def test_train_rows():
    for B, N, M, p in ((2, 64, 30, 0.3), (4, 7000, 4800, 0.3), (1, 3, 5, 0.9), (4, 500, 3072, 0.25), (3, 17, 11, 0.1)):
        want = int(B * min(N, M) * p)                                            # the reference's line 182 on a Python float
        assert train_forward.train_rows(B, N, M, p) == oracle.train_rows(B, N, M, p) == want
        assert type(train_forward.train_rows(np.int64(B), N, M, p)) is int
    assert train_forward.train_rows(2, 64, 30, 0.3) == 18 and train_forward.train_rows(4, 7000, 4800, 0.3) == 5760
    assert train_forward.train_rows(1, 10, 10, 0.29) == 2                        # 2.9: cut, not rounded


# ---- header and binding ----------------------------------------------------------------------------------------------------------------
SYMBOLS = ("optrn_abi_version", "optrn_last_error", "optrn_gt_list_bytes", "optrn_gt_list", "optrn_pad_matches")
PARAMS = {
    "optrn_gt_list_bytes": ("B", "N"),
    "optrn_gt_list": ("gt_j", "B", "N", "M", "workspace", "workspace_bytes", "gt_rows", "n_gt_total", "stream"),
    "optrn_pad_matches": ("b_ids", "i_ids", "j_ids", "mconf", "mkpts_3d", "mkpts_c", "count", "cap", "gt_rows", "n_gt_total", "gt_j", "keypoints3d",
                          "kp_bstride", "B", "N", "M", "w_c", "T", "G", "seed", "step", "scale", "query_scale", "out_b_ids", "out_i_ids",
                          "out_j_ids", "out_mconf", "out_mkpts_3d", "out_mkpts_c", "out_gt_mask", "out_count", "n_keep", "status", "stream"),
}


def test_header_and_binding(tmp_path):
    entry, = cabi.TRAINING
    assert tuple(entry) == ("optrn", "ext/onepose_train_forward.h", "libonepose_train_forward.so", "OPTRN_LIB", "train_forward")
    for table in (cabi.LIBRARIES, cabi.EXTENSIONS, cabi.ADDONS):                  # disjoint, column by column
        assert entry not in table
        for column, taken in zip(entry, zip(*table)):
            assert column not in taken
    text = open(os.path.join(REPO, "include", "ext", "onepose_train_forward.h")).read()
    header = cabi.parse(text, cabi.names_of("optrn"))
    assert tuple(header.prototypes) == SYMBOLS == train_forward.EXPORTED_SYMBOLS
    for name, params in PARAMS.items():
        assert tuple(n for _, n in header.prototypes[name].params) == params, name
    types = dict((n, c) for c, n in header.prototypes["optrn_pad_matches"].params)
    assert (types["seed"], types["step"], types["scale"], types["out_gt_mask"], types["gt_rows"]) == \
        ("unsigned long long", "int", "float", "unsigned char*", "const int*")
    assert header.prototypes["optrn_gt_list_bytes"].ret == "size_t"
    assert header.defines == {"OPTRN_ABI_VERSION": 1, "OPTRN_BLOCK": 256, "OPTRN_MAX_BATCH": 65535, "OPTRN_MAX_ROWS": 2 ** 24,
                              "OPTRN_MAX_STEP": 2 ** 30, "OPTRN_OK": 0, "OPTRN_NO_GT": 1}
    assert (train_forward.OK, train_forward.NO_GT, train_forward.MAX_STEP) == (oracle.OK, oracle.NO_GT, oracle.MAX_STEP)
    assert train_forward.BLOCK == 256 and train_forward.ABI_VERSION == 1
    assert cabi.parse(text).prototypes == {}                                      # the table's reader does not know the prefix
    assert cabi.Binding.of("onepose_st_amd.train_forward").header_path == train_forward._BINDING.header_path
    for other in os.listdir(os.path.join(REPO, "include")):                       # no other header is the place of these entry points
        if other.endswith(".h"):
            assert "optrn_" not in open(os.path.join(REPO, "include", other)).read()
    for other in os.listdir(os.path.join(REPO, "include", "ext")):
        if other != "onepose_train_forward.h":
            assert "optrn_" not in open(os.path.join(REPO, "include", "ext", other)).read()
    mk = open(os.path.join(REPO, "onepose_st_amd", "csrc", "Makefile")).read()
    assert re.search(r"^TRN_SRCS := train_forward.hip$", mk, re.M) and re.search(r"^TRN_FLAGS := -ffp-contract=off$", mk, re.M)
    assert "device_loop.h" in re.search(r"^TRN_HDRS := (.*)$", mk, re.M).group(1).split()
    assert len(re.findall(r"^\$\(eval \$\(call satellite,TRN,trn,train_forward\)\)$", mk, re.M)) == 1
    entry_py = open(os.path.join(REPO, "__graft_entry__.py")).read()
    assert "cabi.LIBRARIES + cabi.EXTENSIONS + cabi.ADDONS + cabi.TRAINING" in entry_py      # build() checks and loads it
    src = open(os.path.join(REPO, "onepose_st_amd", "train_forward.py")).read()
    assert not re.search(r"^\s*(from|import)\s+(oracle|tests)\b", src, re.M)     # the product does not import oracle or tests
    absent = cabi.Binding(entry.header, entry.so, entry.prefix, "OPTRN_NO_SUCH_VARIABLE", names=cabi.names_of("optrn"))
    absent.path = str(tmp_path / "libonepose_absent.so")
    with pytest.raises(cabi.HipLibraryError, match="libonepose_absent.so not found"):
        absent.load()
    no_header = cabi.Binding("ext/no_such_header.h", entry.so, entry.prefix, entry.env, names=cabi.names_of("optrn"))
    assert no_header.exported_symbols == () and no_header.abi_version is None
    with pytest.raises(cabi.HipLibraryError, match="no_such_header.h not found"):
        no_header.load()


P_ = ctypes.c_void_p(1 << 20)                                                    # never dereferenced: every call below is refused first
GOOD = {
    "optrn_gt_list": dict(gt_j=P_, B=2, N=64, M=30, workspace=P_, workspace_bytes=256, gt_rows=P_, n_gt_total=P_, stream=None),
    "optrn_pad_matches": dict(b_ids=P_, i_ids=P_, j_ids=P_, mconf=P_, mkpts_3d=P_, mkpts_c=P_, count=None, cap=128, gt_rows=P_, n_gt_total=P_,
                              gt_j=P_, keypoints3d=P_, kp_bstride=0, B=2, N=64, M=30, w_c=6, T=18, G=5, seed=ctypes.c_ulonglong(1), step=0,
                              scale=8.0, query_scale=None, out_b_ids=P_, out_i_ids=P_, out_j_ids=P_, out_mconf=P_, out_mkpts_3d=P_,
                              out_mkpts_c=P_, out_gt_mask=P_, out_count=P_, n_keep=P_, status=P_, stream=None),
}


def test_names_and_arity_without_a_library(monkeypatch):
    monkeypatch.setattr(train_forward._BINDING, "load", lambda: pytest.fail("the names are checked without the library"))
    for name, named in GOOD.items():
        args = train_forward.order(name, **dict(reversed(list(named.items()))))
        assert args == tuple(named.values()) and len(args) == len(PARAMS[name])
        train_forward.check_arity(name, args)
        with pytest.raises(TypeError, match=f"{name} takes {len(args)} arguments"):
            train_forward.check_arity(name, args[:-1])
    with pytest.raises(TypeError, match="missing status; unknown flags"):
        train_forward.order("optrn_pad_matches", **{**{n: 0 for n in PARAMS["optrn_pad_matches"] if n != "status"}, "flags": 0})
    with pytest.raises(TypeError, match="missing n_gt_total; unknown total"):
        train_forward.launch("optrn_gt_list", {**{n: None for n in PARAMS["optrn_gt_list"][:-2]}, "total": None})


def test_built_library_rejects_before_any_launch():
    assert os.path.exists(train_forward.library_path()), "libonepose_train_forward.so: run __graft_entry__.build()"
    lib = train_forward.load()
    assert all(hasattr(lib, s) for s in SYMBOLS) and lib.optrn_abi_version() == 1
    assert lib.optrn_gt_list_bytes(1, 1) == 256 and lib.optrn_gt_list_bytes(1, 65537) == 1280 and lib.optrn_gt_list_bytes(4, 7000) == 512
    assert lib.optrn_gt_list_bytes(0, 5) == 0 and lib.optrn_gt_list_bytes(2, 2 ** 23 + 1) == 0

    def refused(name, message, **change):
        with pytest.raises(ValueError, match=message):
            train_forward.call(name, *train_forward.order(name, **{**GOOD[name], **change}))
    for name, args in GOOD.items():
        for key, value in args.items():
            if value is P_:
                refused(name, f"^{name}: {name}: null pointer$", **{key: None})
    refused("optrn_gt_list", "B outside", B=0)
    refused("optrn_gt_list", "B outside", B=65536)
    refused("optrn_gt_list", "N and M", M=0)
    refused("optrn_gt_list", "N and M", N=2 ** 24 + 1, B=1)
    refused("optrn_gt_list", r"B \* N above", B=3, N=2 ** 23)
    refused("optrn_gt_list", "workspace smaller", workspace_bytes=255)
    refused("optrn_pad_matches", "0 < G < T", G=0)                                # the reference's assert
    refused("optrn_pad_matches", "0 < G < T", G=18)
    refused("optrn_pad_matches", "0 < G < T", G=5, T=5)
    refused("optrn_pad_matches", r"T above B \* N", T=129)
    refused("optrn_pad_matches", "B outside", B=0)
    refused("optrn_pad_matches", "N and M", N=0)
    refused("optrn_pad_matches", "N and M", M=2 ** 24 + 1)
    refused("optrn_pad_matches", "cap outside", cap=0)
    refused("optrn_pad_matches", "w_c", w_c=0)
    refused("optrn_pad_matches", "step outside", step=-1)
    refused("optrn_pad_matches", "step outside", step=2 ** 30)
    refused("optrn_pad_matches", "kp_bstride", kp_bstride=191)


def test_python_api_and_the_models_switch():
    from onepose_st_amd.config import default_config
    from onepose_st_amd.model import OnePosePlus_model
    ids, kp = torch.zeros(2, 4, dtype=torch.int64), torch.zeros(2, 4, 3)
    gt = supervision.GroundTruth(ids, torch.zeros(2, 4, 2), torch.zeros(2, 6, dtype=torch.int64), torch.zeros(2, dtype=torch.int32), (2, 3))
    from onepose_st_amd.matchcall import MatchLists
    lists = MatchLists(ids[0], ids[0], ids[0], torch.zeros(4), torch.zeros(4, 3), torch.zeros(4, 2), None, None, None)
    for call in (lambda: train_forward.gt_list(gt),
                 lambda: train_forward.pad_matches(lists, gt, kp, T=3, G=1, seed=0, step=0, w_c=3, scale=8.0)):
        with pytest.raises(hip.HipLibraryError, match=re.escape(hip.NO_CPU_FALLBACK)):
            call()
    assert set(vars(train_forward.stages)) >= {"gt_list", "pad_matches"}
    cfg = default_config()
    assert "hip_train_forward" not in cfg and "hip_train_seed" not in cfg         # opt-in keys
    m = OnePosePlus_model(cfg)
    assert m.training and not m.train_forward and (m.train_seed, m.train_calls) == (0, 0)
    with pytest.raises(NotImplementedError, match="call .eval()"):                # unset: a training-mode call raises exactly as before
        m({"query_image": torch.zeros(1, 1, 32, 32)})
    on = OnePosePlus_model({**cfg, "hip_train_forward": True, "hip_train_seed": 9})
    assert on.train_forward and (on.train_seed, on.train_calls) == (9, 0)
    on.reseed(4, calls=7)
    assert (on.train_seed, on.train_calls) == (4, 7)
    on.reseed(5)
    assert (on.train_seed, on.train_calls) == (5, 0)
    data = {"keypoints3d": torch.zeros(1, 40, 3), "descriptors3d_db": torch.zeros(1, 128, 40), "descriptors3d_coarse_db": torch.zeros(1, 256, 40)}
    with pytest.raises(hip.HipLibraryError):                                      # set: no CPU fallback either
        on.forward_features(data, torch.zeros(1, 256, 4, 4), torch.zeros(1, 128, 16, 16), (32, 32))
    assert on.train_calls == 0                                                    # a refused call is not counted
