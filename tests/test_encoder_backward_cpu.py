"""The encoder layer's backward (``onepose_st_amd/encoder_backward.py``, include/ext/onepose_encoder_backward.h) without a
GPU: the numpy float64 oracle (``tests/encoder_backward_oracle.py``) against what the reference's own layer computed under float64 autograd
(``tests/golden/encoder_backward_small.npz``, recipe ``tests/golden/make_encoder_backward_golden.py``), against difference quotients of its own
forward, and its chain against torch autograd of the project's oracle transformer; the header, the binding and the calls the built library
refuses before any launch; the precision bars of the device test, derived here from the float32 split-bf16 stand-in over that test's cases;
the seeded faults, each measured against the bar; the ReLU margin of every case; and ``coarse_backward``'s routing."""
import ctypes
import os
import re

import numpy as np
import pytest
import torch

from onepose_st_amd import cabi, encoder_backward as eb, hip, params as params_mod
from tests import encoder_backward_cases as cases
from tests import encoder_backward_oracle as oracle
from tests import train_forward_oracle
from tests.golden import make_encoder_backward_golden as recipe

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.fixture(scope="module")
def golden():
    return dict(np.load(os.path.join(REPO, "tests", "golden", "encoder_backward_small.npz")))


# ---- 1. the oracle against the reference ----------------------------------------------------------------------------------------------------
def test_the_generator_is_the_one_the_fixture_was_made_with(golden):
    k = np.arange(1, 6, dtype=np.uint64)
    with np.errstate(over="ignore"):
        got = cases.mix64(np.uint64(5) + np.uint64(cases.GOLDEN) * k)
    assert [int(v) for v in got] == [train_forward_oracle.mix64(5 + cases.GOLDEN * int(i)) for i in k]
    P = cases.weights(7)
    for name, sums in recipe.weight_sums(P).items():
        assert np.array_equal(sums, golden[f"weights/{name}"]), f"{name}: the weight generator has drifted from the fixture's"
        assert P[name].dtype == np.float32 and P[name].shape == oracle.PARAM_SHAPES[name]
    assert abs(float(P["norm1.weight"].mean()) - 1) < 0.05 and abs(float(P["norm2.bias"].mean())) < 0.05 and P["norm1.bias"].std() > 0.05
    for tag, args in recipe.GOLDEN_CASES.items():
        case = cases.layer_case(**args)
        for key in ("x", "dy") + (() if args.get("self_layer") else ("source",)):
            assert golden[f"{tag}/{key}"].dtype == np.float32 and np.array_equal(golden[f"{tag}/{key}"], case[key]), (tag, key)
    assert golden["cross/x"].shape == (2, 19, 256) and golden["cross/source"].shape == (2, 23, 256) and golden["self/x"].shape == (1, 13, 256)


@pytest.mark.parametrize("tag", list(recipe.GOLDEN_CASES))
def test_oracle_equals_the_reference_at_float64_rounding(golden, tag):
    """The bar: 1e-12 of each tensor's largest value"""
    case = cases.layer_case(**recipe.GOLDEN_CASES[tag])
    got = oracle.layer_grads(case["x"], case["source"], case["dy"], case["P"])

    def close(a, b, what):
        assert a.shape == b.shape and np.abs(a - b).max() <= 1e-12 * np.abs(b).max(), (tag, what, np.abs(a - b).max() / np.abs(b).max())
    close(got["y"], golden[f"{tag}/y"], "y")
    close(got["dx"], golden[f"{tag}/dx"], "dx")
    close(got["dsource"], golden[f"{tag}/dsource"], "dsource")
    assert ("self/source" in golden) is False and case["source"] is (case["x"] if tag == "self" else case["source"])
    for name, shape in oracle.PARAM_SHAPES.items():
        g = got["dparams"][name]
        assert g.shape == shape
        if name in oracle.MATRICES:
            U, V = recipe.sketches(shape)
            close(g @ V, golden[f"{tag}/{name}/right"], name + " right")
            close(U.T @ g, golden[f"{tag}/{name}/left"], name + " left")
        else:
            close(g, golden[f"{tag}/{name}"], name)


# ---- 2. difference quotients ----------------------------------------------------------------------------------------------------------------
def test_oracle_is_the_gradient_of_its_forward():
    """Central differences of the float64 forward's <y, dy> along 8 seeded directions for x, source and every parameter tensor.  Step 1e-5
    of unit directions: truncation h^2 = 1e-10 of the derivative, rounding 1e-16 / h = 1e-11 of the value, which is near 100 (1e-9); the
    case keeps every pre-activation 3e-4 from the ReLU's kink and a step moves one by 1e-5 at most, so no step crosses it."""
    case = cases.layer_case(seed=31, B=2, L=7, S=9)
    x, source, dy, P = case["x"].astype(np.float64), case["source"].astype(np.float64), case["dy"].astype(np.float64), case["P"]
    got = oracle.layer_grads(x, source, dy, P)
    draw, h = cases.Stream(32), 1e-5

    def value(x_, s_, P_):
        return float((oracle.layer_forward(x_, s_, P_)["y"] * dy).sum())
    targets = [("x", got["dx"]), ("source", got["dsource"])] + [(n, got["dparams"][n]) for n in oracle.PARAM_SHAPES]
    for name, grad in targets:
        for _ in range(8):
            d = draw.uniform(grad.shape)
            d /= np.linalg.norm(d)
            def at(step):
                if name == "x":
                    return value(x + step * d, source, P)
                if name == "source":
                    return value(x, source + step * d, P)
                return value(x, source, {**{k: v.astype(np.float64) for k, v in P.items()}, name: P[name].astype(np.float64) + step * d})
            quotient, want = (at(h) - at(-h)) / (2 * h), float((grad * d).sum())
            assert abs(quotient - want) <= 1e-6 * abs(want) + 1e-8, (name, quotient, want)


# ---- 3. the chain's wiring ------------------------------------------------------------------------------------------------------------------
def chain_params():
    return [cases.weights(100 + i) for i in range(len(cases.CHAIN_NAMES))]


def test_chain_oracle_against_autograd_of_the_oracle_transformer():
    from oracle import onepose_oracle as orc
    B, N, M = 2, 5, 4
    x3, x2, g3, g2 = cases.chain_inputs(41, B, N, M)
    Ps = chain_params()
    sd = {f"loftr_coarse.layers.{i}.{n}": torch.tensor(v, dtype=torch.float64, requires_grad=True) for i, P in enumerate(Ps) for n, v in P.items()}
    t3, t2 = (torch.tensor(v, dtype=torch.float64, requires_grad=True) for v in (x3, x2))
    d3, d2 = orc.feature_transformer(sd, "loftr_coarse", cases.CHAIN_NAMES, 8, t3.transpose(1, 2), t2)
    ((d3 * torch.tensor(g3, dtype=torch.float64)).sum() + (d2 * torch.tensor(g2, dtype=torch.float64)).sum()).backward()
    kept, (y3, y2) = oracle.chain_forward(cases.CHAIN_NAMES, Ps, x3, x2)
    assert np.abs(y3 - d3.detach().numpy()).max() <= 1e-12 and np.abs(y2 - d2.detach().numpy()).max() <= 1e-12
    a3, a2, dps = oracle.chain_grads(cases.CHAIN_NAMES, Ps, kept, g3, g2)
    for got, want in [(a3, t3.grad.numpy()), (a2, t2.grad.numpy())] + [(dps[i][n], sd[f"loftr_coarse.layers.{i}.{n}"].grad.numpy())
                                                                      for i in range(len(Ps)) for n in oracle.PARAM_SHAPES]:
        assert np.abs(got - want).max() <= 1e-11 * np.abs(want).max()


# ---- 4, 5. header and binding ---------------------------------------------------------------------------------------------------------------
SYMBOLS = ("openb_abi_version", "openb_last_error", "openb_layer_workspace_bytes", "openb_layer_grads")
PARAMS = {"openb_layer_workspace_bytes": ("B", "L", "S"),
          "openb_layer_grads": ("x", "source", "dy", "B", "L", "S", "params", "workspace", "workspace_bytes", "dx", "dsource", "dparams", "accumulate",
                                "stream")}


def test_header_and_binding(tmp_path):
    entry, = cabi.ENCODER_BACKWARD
    assert tuple(entry) == ("openb", "ext/onepose_encoder_backward.h", "libonepose_encoder_backward.so", "OPENB_LIB", "encoder_backward")
    for table in (cabi.LIBRARIES, cabi.EXTENSIONS, cabi.ADDONS, cabi.TRAINING, cabi.BACKWARD):   # disjoint, column by column
        assert entry not in table
        for column, taken in zip(entry, zip(*table)):
            assert column not in taken
    text = open(os.path.join(REPO, "include", "ext", "onepose_encoder_backward.h")).read()
    header = cabi.parse(text, cabi.names_of("openb"))
    assert tuple(header.prototypes) == SYMBOLS == eb.EXPORTED_SYMBOLS
    for name, names in PARAMS.items():
        assert tuple(n for _, n in header.prototypes[name].params) == names, name
    types = dict((n, c) for c, n in header.prototypes["openb_layer_grads"].params)
    assert (types["x"], types["params"], types["workspace"], types["workspace_bytes"], types["dparams"], types["accumulate"]) == \
        ("const float*", "const float*", "void*", "size_t", "float*", "int")
    assert header.prototypes["openb_layer_workspace_bytes"].ret == "size_t"
    d = header.defines
    assert (d["OPENB_ABI_VERSION"], d["OPENB_CHANNELS"], d["OPENB_HEADS"], d["OPENB_HEAD_DIM"], d["OPENB_HIDDEN"]) == (1, 256, 8, 32, 512)
    assert d["OPENB_PARAM_FLOATS"] == 4 * 65536 + 262144 + 131072 + 4 * 256 == 656384 == eb.PARAM_FLOATS
    # the parameter buffer against EncoderLayerParams: names, order, shapes, offsets
    holder = params_mod.EncoderLayerParams(256)
    assert tuple(n for n, _ in holder.named_parameters()) == ("q_proj.weight", "k_proj.weight", "v_proj.weight", "merge.weight", "mlp.0.weight",
                                                               "mlp.2.weight", "norm1.weight", "norm1.bias", "norm2.weight", "norm2.bias")
    assert tuple(eb.PARAM_LAYOUT) == eb.PARAM_NAMES == tuple(oracle.PARAM_SHAPES)
    at = 0
    for name, p in holder.named_parameters():
        assert eb.PARAM_LAYOUT[name] == (at, tuple(p.shape)) and oracle.PARAM_SHAPES[name] == tuple(p.shape), name
        at += p.numel()
    assert at == eb.PARAM_FLOATS
    flat = eb.pack_params(holder)
    assert flat.shape == (eb.PARAM_FLOATS,) and flat.dtype == torch.float32
    views = eb.unpack_grads(flat, "loftr_coarse.layers.3.")
    for name, p in holder.named_parameters():
        assert torch.equal(views["loftr_coarse.layers.3." + name], p.detach())
    sd = {"enc." + n: p.detach() for n, p in holder.named_parameters()}
    assert torch.equal(eb.pack_params(sd, "enc."), flat)
    with pytest.raises(KeyError, match="enc.q_proj.weight"):
        eb.pack_params({}, "enc.")
    assert np.array_equal(oracle.flat_params(cases.weights(7)), eb.pack_params({n: torch.from_numpy(v) for n, v in cases.weights(7).items()}).numpy())
    assert (eb.ROW_TILE, eb.SPLIT_ROWS, eb.MAX_SPLITS, eb.ROW_BLOCK) == (64, 128, 16, 32) and eb.ABI_VERSION == 1
    assert [eb.rows_per_split(t) for t in (1, 128, 129, 2048, 2049, 2100, 28000)] == [128, 128, 128, 128, 160, 160, 1760]
    for words in ("dden_lh = -Z_lh * (dm_lh . m_lh)", "v_mfma_f32_32x32x16_bf16", "identical bytes", "rows_per_split = max(OPENB_SPLIT_ROWS",
                  "vector ALU", "these are all the points at which a value is split"):
        assert words in text, words
    assert cabi.parse(text).prototypes == {}                                      # the table's reader does not know the prefix
    assert cabi.Binding.of("onepose_st_amd.encoder_backward").header_path == eb._BINDING.header_path
    for folder in ("include", os.path.join("include", "ext")):                    # no other header is the place of these entry points
        for other in os.listdir(os.path.join(REPO, folder)):
            if other.endswith(".h") and other != "onepose_encoder_backward.h":
                assert "openb_" not in open(os.path.join(REPO, folder, other)).read()
    mk = open(os.path.join(REPO, "onepose_st_amd", "csrc", "Makefile")).read()
    assert re.search(r"^ENB_SRCS := encoder_backward.hip$", mk, re.M) and re.search(r"^ENB_FLAGS :=$", mk, re.M)
    hdrs = re.search(r"^ENB_HDRS := (.*)$", mk, re.M).group(1).split()
    assert {"capi_error.h", "tile.h", "tile_bf16.h", "../../include/ext/onepose_encoder_backward.h"} == set(hdrs)
    assert len(re.findall(r"^\$\(eval \$\(call satellite,ENB,enb,encoder_backward\)\)$", mk, re.M)) == 1
    src = open(os.path.join(REPO, "onepose_st_amd", "csrc", "encoder_backward.hip")).read()
    for shared in ('#include "tile_bf16.h"', '#include "capi_error.h"', "mma_bf16<3>", "split_bf16"):
        assert shared in src, shared                                              # shared code is included, not copied
    assert "atomicAdd" not in src and "atomic_add" not in src and "hipDeviceGetAttribute" not in src      # no atomics; no split from the CU count
    entry_py = open(os.path.join(REPO, "__graft_entry__.py")).read()
    assert "cabi.LIBRARIES + cabi.EXTENSIONS + cabi.ADDONS + cabi.TRAINING + cabi.BACKWARD + cabi.ENCODER_BACKWARD" in entry_py
    py = open(os.path.join(REPO, "onepose_st_amd", "encoder_backward.py")).read()
    assert not re.search(r"^\s*(from|import)\s+(oracle|tests)\b", py, re.M)       # the product does not import oracle or tests
    absent = cabi.Binding(entry.header, entry.so, entry.prefix, "OPENB_NO_SUCH_VARIABLE", names=cabi.names_of("openb"))
    absent.path = str(tmp_path / "libonepose_absent.so")
    with pytest.raises(cabi.HipLibraryError, match="libonepose_absent.so not found"):
        absent.load()


A_, B_, C_, D_, E_, F_, G_, W_ = (ctypes.c_void_p((k + 1) << 32) for k in range(8))     # never dereferenced: every call below is refused first
GOOD = dict(x=A_, source=B_, dy=C_, B=2, L=64, S=30, params=D_, workspace=W_, workspace_bytes=1 << 30, dx=E_, dsource=F_, dparams=G_, accumulate=0,
            stream=None)


def test_names_and_arity_without_a_library(monkeypatch):
    monkeypatch.setattr(eb._BINDING, "load", lambda: pytest.fail("the names are checked without the library"))
    name = "openb_layer_grads"
    args = eb.order(name, **dict(reversed(list(GOOD.items()))))
    assert args == tuple(GOOD.values()) and len(args) == len(PARAMS[name])
    eb.check_arity(name, args)
    with pytest.raises(TypeError, match=f"{name} takes {len(args)} arguments"):
        eb.check_arity(name, args[:-1])
    with pytest.raises(TypeError, match="missing dparams; unknown grads"):
        eb.launch(name, {**{n: None for n in PARAMS[name][:-1] if n != "dparams"}, "grads": None})
    assert set(eb.launch.converters(name)) == set(PARAMS[name]) - {"stream"}


def test_built_library_rejects_before_any_launch():
    assert os.path.exists(eb.library_path()), "libonepose_encoder_backward.so: run __graft_entry__.build()"
    lib = eb.load()
    assert all(hasattr(lib, s) for s in SYMBOLS) and lib.openb_abi_version() == 1

    def want_bytes(B, L, S):
        up = lambda floats: -(-(floats * 4) // 256) * 256                        # noqa: E731
        rx, rs, blocks = B * L, B * S, -(-(B * L) // 32)
        splits = lambda t: -(-t // eb.rows_per_split(t))                          # noqa: E731
        total = 5 * up(rx * 256) + 2 * up(rx * 512) + up(rs * 512) + 2 * up(rx * 8) + 2 * up(blocks * 512)
        for t in (S, L):
            total += up(B * splits(t) * 8192) + up(B * splits(t) * 256) + up(B * 8192) + up(B * 256)
        return total + up(eb.MAX_SPLITS * 512 * 512)
    for shape in ((1, 1, 1), (2, 300, 1295), (4, 7000, 4800), (3, 33, 31), (1, 15000, 15000)):
        assert lib.openb_layer_workspace_bytes(*shape) == want_bytes(*shape) == eb.workspace_bytes(*shape), shape
    big = lib.openb_layer_workspace_bytes(4, 7000, 4800)
    assert big < 4 * (7000 * 2400 + 4800 * 520) * 4 + (17 << 20)                  # O(B (L + S)) rows plus the bounded weight-sized partials
    for shape in ((0, 5, 5), (1, 2 ** 20 + 1, 5), (1, 5, 0), (65536, 1, 1), (8, 2 ** 20, 1)):
        assert lib.openb_layer_workspace_bytes(*shape) == 0, shape
    with pytest.raises(ValueError, match="B \\* L and B \\* S"):
        eb.workspace_bytes(8, 2 ** 20, 1)

    name = "openb_layer_grads"

    def refused(message, **change):
        with pytest.raises(ValueError, match=message):
            eb.call(name, *eb.order(name, **{**GOOD, **change}))
    for key, value in GOOD.items():
        if isinstance(value, ctypes.c_void_p):
            refused(f"^{name}: {name}: null pointer$", **{key: None})
    refused("B outside", B=0)
    refused("B outside", B=65536)
    refused("L and S", L=0)
    refused("L and S", S=2 ** 20 + 1)
    refused("at most OPENB_MAX_TOTAL_ROWS", B=8, L=2 ** 20)
    refused("16-byte aligned", source=ctypes.c_void_p((2 << 32) + 4))
    refused("16-byte aligned", dparams=ctypes.c_void_p((7 << 32) + 8))
    refused("256-byte aligned", workspace=ctypes.c_void_p((8 << 32) + 16))
    refused("workspace_bytes below", workspace_bytes=lib.openb_layer_workspace_bytes(2, 64, 30) - 1)
    refused("an output overlaps an input", dx=A_)                                 # x
    refused("an output overlaps an input", dx=ctypes.c_void_p((1 << 32) + 2 * 64 * 1024 - 16))      # the last 16 bytes of x
    refused("an output overlaps an input", dsource=C_)                            # dy
    refused("an output overlaps an input", dparams=D_)                            # params
    refused("an output overlaps an input or the workspace", dx=ctypes.c_void_p((8 << 32) + 4096))
    refused("two outputs overlap", dsource=E_)
    refused("an input overlaps the workspace", dy=ctypes.c_void_p((8 << 32) + 256))
    eb.order(name, **{**GOOD, "source": A_})                                      # x == source is an allowed call (a self layer)


def test_python_api_and_the_models_switch():
    from onepose_st_amd.config import default_config
    from onepose_st_amd.model import OnePosePlus_model
    x, s, p = torch.zeros(2, 4, 256), torch.zeros(2, 6, 256), torch.zeros(eb.PARAM_FLOATS)
    with pytest.raises(hip.HipLibraryError, match=re.escape(hip.NO_CPU_FALLBACK)):
        eb.layer_backward(x, s, x, p)
    with pytest.raises(TypeError, match="source: expected a tensor"):
        eb.layer_backward(x, None, x, p)
    with pytest.raises(ValueError, match="flat"):
        eb.unpack_grads(torch.zeros(5))
    assert set(vars(eb.stages)) >= {"layer_backward"}
    cfg = default_config()
    assert "hip_keep_layer_inputs" not in cfg                                     # an opt-in key
    assert not OnePosePlus_model(cfg).keep_layer_inputs and OnePosePlus_model({**cfg, "hip_keep_layer_inputs": True}).keep_layer_inputs
    model = OnePosePlus_model(cfg)
    data = {"grad_feat_c0": x, "grad_feat_c1": s}
    with pytest.raises(KeyError, match="layer_inputs_c.*hip_keep_layer_inputs"):
        eb.coarse_backward(dict(data), model)
    with pytest.raises(KeyError, match="grad_feat_c1"):
        eb.coarse_backward({"grad_feat_c0": x, "layer_inputs_c": []}, model)
    with pytest.raises(NotImplementedError, match="masks"):
        eb.coarse_backward({**data, "layer_inputs_c": [], "query_image_mask": None}, model)


def test_the_new_table_is_built_and_loaded():
    import __graft_entry__ as entry
    text = open(entry.__file__).read()
    loop = re.search(r"for entry in (.*):", text).group(1)
    assert loop.split(" + ") == ["cabi.LIBRARIES", "cabi.EXTENSIONS", "cabi.ADDONS", "cabi.TRAINING", "cabi.BACKWARD", "cabi.ENCODER_BACKWARD"]
    assert eb.load().openb_abi_version() == eb.ABI_VERSION


# ---- 6. the precision bars ------------------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def standin_errors():
    """name -> (worst statistic of the float32 split-bf16 stand-in against the float64 oracle, where) over the device test's cases"""
    out = {}
    for name, args in cases.LAYER_CASES.items():
        c = cases.layer_case(**args)
        want = oracle.layer_grads(c["x"], c["source"], c["dy"], c["P"])
        out[name] = oracle.worst_error(oracle.layer_grads(c["x"], c["source"], c["dy"], c["P"], standin=True), want)
    return out


def chain_standin():
    """The stand-in through the six layers (forward and backward) against the float64 chain on the device chain test's own scene
    (cases.chain_scene) with seeded upstream gradients -> (the worst statistic over the two input gradients (per frame) and every
    parameter tensor of every layer, where, the hidden units whose sign differs between stand-in and oracle)"""
    scene = cases.chain_scene()
    Ps, x3, x2 = scene["params"], scene["x3"], scene["x2"]
    _, _, g3, g2 = cases.chain_inputs(43, 2, cases.CHAIN_POINTS, x2.shape[1])
    k64, k32 = (oracle.chain_forward(cases.CHAIN_NAMES, Ps, x3, x2, standin=s)[0] for s in (False, True))
    flips = 0
    for i, name in enumerate(cases.CHAIN_NAMES):
        (a3, a2), (b3, b2) = k64[i], k32[i]
        for (x, s), (xs, ss) in (((a2, a2 if name == "self" else a3), (b2, b2 if name == "self" else b3)),
                                 ((a3, a3 if name == "self" else a2), (b3, b3 if name == "self" else b2))):
            flips += int(((oracle.layer_forward(x, s, Ps[i])["pre"] > 0) != (oracle.layer_forward(xs, ss, Ps[i], standin=True)["pre"] > 0)).sum())
    want = oracle.chain_grads(cases.CHAIN_NAMES, Ps, k64, g3, g2)
    got = oracle.chain_grads(cases.CHAIN_NAMES, Ps, k32, g3, g2, standin=True)
    errs = {"x3": oracle.frame_error(got[0], want[0]), "x2": oracle.frame_error(got[1], want[1])}
    errs.update({f"{i}.{n}": oracle.tensor_error(got[2][i][n], want[2][i][n]) for i in range(len(Ps)) for n in oracle.PARAM_SHAPES})
    where = max(errs, key=errs.get)
    return errs[where], where, flips


def test_the_precision_bars(standin_errors):
    """The project's method: the statistic is max |y - y_ref| / max |y_ref| over a frame's dx / dsource and over each
    parameter tensor (oracle.call_errors says what S = 1 does to dWq and dWk); the bar is between two and four times the worst value of
    the float32 stand-in that splits at the header's operand points.  Measured here: 1.8e-5 over the 45 layer cases (dWv of
    cross_b1_l65_s1; the median case 1.3e-5), so LAYER_BAR = 5.0e-5.  Through the six layers of the device chain test's scene: 1.2e-2, at
    dW of layer 4's mlp.0 -- in that scene hidden units lie at the ReLU's kink (the smallest pre-activation of layer 4's 3D call is 0.07
    stand-in deviations from zero) and the stand-in takes one on the other side; every other tensor of the chain is within 6e-3.  A scene
    of a million pre-activations cannot avoid this, so CHAIN_BAR = 3.3e-2 is a bar for the chain's WIRING (a wrong route is an error of order
    one); the arithmetic is held by the layer cases at LAYER_BAR.  Nothing comes from a device."""
    assert set(standin_errors) == set(cases.LAYER_CASES) and len(standin_errors) == 45
    worst = max(e for e, _ in standin_errors.values())
    print({k: f"{e:.2e} {w}" for k, (e, w) in standin_errors.items()})
    assert 2 * worst <= cases.LAYER_BAR <= 4 * worst, worst
    chain, where, flips = chain_standin()
    print(f"chain stand-in worst {chain:.3e} at {where}, {flips} hidden units of another sign")
    assert 2 * chain <= cases.CHAIN_BAR <= 4 * chain, chain


def test_the_cases_cover_the_edges():
    R, K = cases.R, cases.K
    shapes = {(a["B"], a["L"], a["S"]) for a in cases.LAYER_CASES.values() if not a.get("self_layer")}
    assert {(b, l, s) for b in (1, 2) for l in (1, R - 1, R, R + 1, 2 * R + 1) for s in (1, K - 1, K, K + 1)} <= shapes
    assert {(a["B"], a["L"]) for a in cases.LAYER_CASES.values() if a.get("self_layer")} == {(b, l) for b in (1, 2) for l in (1, R + 1)}
    many = cases.LAYER_CASES["many_splits"]
    rows = many["B"] * many["L"]
    per = eb.rows_per_split(rows)
    assert per > K and -(-rows // per) > 1 and rows % per not in (0,) and rows % 16 != 0      # several splits, a ragged last one


# ---- 7. seeded faults -----------------------------------------------------------------------------------------------------------------------
FAULTS = ("residual_dropped", "dhc_x_dropped", "relu_mask_ignored", "ln_no_mean_terms", "dks_dropped", "dv_not_divided", "dk_wk_dropped")


@pytest.mark.parametrize("fault", FAULTS)
def test_seeded_faults_lie_far_outside_the_bar(fault):
    """Each fault's worst statistic against the true gradient, in units of LAYER_BAR; each must be at least 10"""
    c = cases.layer_case(**cases.LAYER_CASES["cross_b2_l65_s127"])
    want = oracle.layer_grads(c["x"], c["source"], c["dy"], c["P"])
    err, where = oracle.worst_error(oracle.layer_grads(c["x"], c["source"], c["dy"], c["P"], faults={fault}), want)
    print(f"{fault}: {err / cases.LAYER_BAR:.3g} bars at {where}")
    assert err >= 10 * cases.LAYER_BAR, (fault, err, where)


# ---- 8. the ReLU margin ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", list(cases.LAYER_CASES))
def test_the_relu_mask_is_unambiguous(name):
    c = cases.layer_case(**cases.LAYER_CASES[name])
    bad, want, dev = cases.relu_margin(c["x"], c["source"], c["P"])
    got = oracle.layer_forward(c["x"], c["source"], c["P"], standin=True)["pre"]
    assert not bad.any() and ((got > 0) == (want > 0)).all() and np.abs(want).min() > cases.MARGIN * dev > 0
    assert c["sweeps"] < cases.MAX_SWEEPS and (c["source"] is c["x"]) == bool(cases.LAYER_CASES[name].get("self_layer"))


# ---- 9. coarse_backward's routing -----------------------------------------------------------------------------------------------------------
def test_coarse_backward_routes_the_gradients(monkeypatch):
    """``layer_backward`` replaced by a recording stub whose outputs are tagged scalars: which gradients meet where, which calls accumulate"""
    from onepose_st_amd.config import default_config
    from onepose_st_amd.model import OnePosePlus_model
    model = OnePosePlus_model(default_config())
    names = list(model.loftr_coarse.layer_names)
    assert names == ["self", "cross"] * 3
    kept = [(torch.full((1, 3, 256), 10.0 * i + 3), torch.full((1, 2, 256), 10.0 * i + 2)) for i in range(6)]
    calls = []

    def stub(x, source, dy, params, *, dparams=None, accumulate=False, workspace=None, out=None, stream=None):
        k = len(calls)
        calls.append(dict(x=float(x[0, 0, 0]), source=float(source[0, 0, 0]), dy=float(dy[0, 0, 0]), accumulate=accumulate, same=dparams,
                          params=params))
        new = torch.full((eb.PARAM_FLOATS,), float(k)) if dparams is None else dparams.add_(float(k))
        return torch.full_like(x, 2.0 ** (2 * k)), torch.full_like(source, 2.0 ** (2 * k + 1)), new
    monkeypatch.setattr(eb, "layer_backward", stub)
    data = {"grad_feat_c0": torch.full((1, 3, 256), 0.5), "grad_feat_c1": torch.full((1, 2, 256), 0.25), "layer_inputs_c": kept}
    eb.coarse_backward(data, model)
    assert len(calls) == 12
    g3, g2 = 0.5, 0.25
    for n, i in enumerate(reversed(range(6))):
        first, second = calls[2 * n], calls[2 * n + 1]
        x3, x2 = 10.0 * i + 3, 10.0 * i + 2
        cross = names[i] == "cross"
        assert (first["x"], first["source"], first["dy"]) == (x2, x3 if cross else x2, g2)              # the 2D stream, from 3D in a cross layer
        assert (second["x"], second["source"], second["dy"]) == (x3, x2 if cross else x3, g3)
        assert not first["accumulate"] and first["same"] is None and second["accumulate"] and second["same"] is not None
        assert torch.equal(first["params"], eb.pack_params(model.loftr_coarse.layers[i])) and torch.equal(second["params"], first["params"])
        k = 2 * n
        dx2, ds_first, dx3, ds_second = 2.0 ** (2 * k), 2.0 ** (2 * k + 1), 2.0 ** (2 * k + 2), 2.0 ** (2 * k + 3)
        g2, g3 = (dx2 + ds_second, dx3 + ds_first) if cross else (dx2 + ds_first, dx3 + ds_second)
        grads = data["grad_params_c"]
        assert float(grads[f"loftr_coarse.layers.{i}.mlp.0.weight"][0, 0]) == float(k + k + 1)          # written by the first, added to once
    assert float(data["grad_x3d_c"][0, 0, 0]) == g3 and float(data["grad_x2d_c"][0, 0, 0]) == g2
    assert set(data["grad_params_c"]) == {f"loftr_coarse.layers.{i}.{n}" for i in range(6) for n in eb.PARAM_NAMES}
    assert data["grad_params_c"]["loftr_coarse.layers.5.norm2.bias"].shape == (256,)
    assert all(p.grad is None for p in model.parameters())                        # no .grad is set
