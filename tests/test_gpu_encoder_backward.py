"""The encoder layer's backward on the device (``onepose_st_amd/encoder_backward.py``, ``libonepose_encoder_backward.so``) against its numpy
float64 restatement (tests/encoder_backward_oracle.py): every gradient of a layer call within the bar that tests/test_encoder_backward_cpu.py
derives from the float32 split-bf16 stand-in over these very cases (tests/encoder_backward_cases.py), zeros for a zero gradient, the
accumulation, identical bytes run to run and batch to halves, the rejected calls, and the six-layer chain behind the training-mode forward
and the loss backward.  Every buffer of a call sits on a guarded arena (tests/guarded.py); outputs are NaN-filled with spare rows that must
stay NaN.  Everything is small: at most 2 100 rows."""
import numpy as np
import pytest
import torch

from tests import encoder_backward_cases as cases
from tests import encoder_backward_oracle as oracle
from tests import guarded

pytestmark = pytest.mark.gpu

DEV = "cuda:0"
SPARE = 3


@pytest.fixture(scope="module")
def eb():
    from onepose_st_amd import encoder_backward
    encoder_backward.load()
    assert (encoder_backward.ROW_TILE, encoder_backward.SPLIT_ROWS) == (cases.R, cases.K)
    return encoder_backward


def spare_out(arena, shape, name):
    """A NaN-filled output of ``shape`` with SPARE more rows behind it -> (the output, the spare rows)"""
    rows = int(np.prod(shape[:-1]))
    whole = arena.typed((rows + SPARE, shape[-1]), torch.float32, name=name)
    return whole[:rows].view(*shape), whole[rows:]


def run_layer(eb, case, accumulate_onto=None):
    """One call on a guarded arena -> dict ``dx``, ``dsource`` (numpy), ``dparams`` (name -> numpy) and ``flat`` (the whole buffer).  The
    arena is checked, the spare rows are still NaN, every written value is finite.  ``accumulate_onto``: a flat float32 numpy buffer the
    call adds to."""
    x, source, dy = case["x"], case["source"], case["dy"]
    B, L, _ = x.shape
    S = source.shape[1]
    need = eb.workspace_bytes(B, L, S) + 8 * 4 * B * (L + S + 2 * SPARE) * cases.C + 3 * 4 * eb.PARAM_FLOATS + 24 * guarded.GUARD
    arena = guarded.Arena(DEV, need)
    tx = arena.put(torch.from_numpy(x).to(DEV), name="x")
    ts = tx if source is x else arena.put(torch.from_numpy(source).to(DEV), name="source")
    tdy = arena.put(torch.from_numpy(dy).to(DEV), name="dy")
    params = arena.put(torch.from_numpy(oracle.flat_params(case["P"])).to(DEV), name="params")
    (dx, sx), (ds, ss) = spare_out(arena, (B, L, cases.C), "dx"), spare_out(arena, (B, S, cases.C), "dsource")
    whole = arena.typed((eb.PARAM_FLOATS + SPARE,), torch.float32, name="dparams")
    dparams, sp = whole[:eb.PARAM_FLOATS], whole[eb.PARAM_FLOATS:]
    if accumulate_onto is not None:
        dparams.copy_(torch.from_numpy(accumulate_onto).to(DEV))
    with guarded.guarded_empty(arena, 0xFF, [eb]):              # the workspace: poisoned, on the arena
        got = eb.layer_backward(tx, ts, tdy, params, dparams=dparams, accumulate=accumulate_onto is not None, out=(dx, ds))
    torch.cuda.synchronize()
    assert got[0] is dx and got[1] is ds and got[2] is dparams
    arena.check()
    assert all(bool(torch.isnan(t).all()) for t in (sx, ss, sp))
    out = {"dx": dx.cpu().numpy(), "dsource": ds.cpu().numpy(), "flat": dparams.cpu().numpy()}
    assert all(np.isfinite(v).all() for v in out.values())
    out["dparams"] = {n: v.numpy() for n, v in eb.unpack_grads(torch.from_numpy(out["flat"])).items()}
    return out


_WANT = {}


def want_of(name):
    """The case and its float64 oracle, computed once and shared"""
    if name not in _WANT:
        case = cases.layer_case(**cases.LAYER_CASES[name])
        _WANT[name] = (case, oracle.layer_grads(case["x"], case["source"], case["dy"], case["P"]))
    return _WANT[name]


# ---- 1. one layer call ----------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", list(cases.LAYER_CASES))
def test_layer_parity_within_the_bar(eb, name):
    case, want = want_of(name)
    got = run_layer(eb, case)
    errs = oracle.call_errors(got, want)
    print(f"{name}: " + " ".join(f"{k} {v:.2e}" for k, v in errs.items()) + f" (bar {cases.LAYER_BAR:.1e})")
    assert max(errs.values()) <= cases.LAYER_BAR, {k: v for k, v in errs.items() if v > cases.LAYER_BAR}


def test_zero_gradient_gives_zeros(eb):
    got = run_layer(eb, cases.layer_case(seed=61, B=2, L=cases.R + 1, S=cases.K + 1, zero_dy=True))
    assert not got["dx"].any() and not got["dsource"].any() and not got["flat"].any()


def test_accumulate_adds_once_per_element(eb):
    a, b = cases.layer_case(seed=62, B=1, L=cases.R + 1, S=40), cases.layer_case(seed=63, B=1, L=40, S=cases.R + 1)
    first, second = run_layer(eb, a), run_layer(eb, b)
    both = run_layer(eb, b, accumulate_onto=first["flat"])
    assert both["flat"].tobytes() == (first["flat"] + second["flat"]).tobytes()           # the elementwise float32 sum, bit for bit
    assert both["dx"].tobytes() == second["dx"].tobytes() and both["dsource"].tobytes() == second["dsource"].tobytes()


def test_identical_bytes_and_frames_alone(eb):
    for name in ("cross_b2_l129_s129", "self_b2_l65"):
        case, _ = want_of(name)
        first, again = run_layer(eb, case), run_layer(eb, case)
        for key in ("dx", "dsource", "flat"):
            assert first[key].tobytes() == again[key].tobytes(), (name, key)
        for b in range(2):                                                                  # a frame alone: the same bytes of dx and dsource
            xb = np.ascontiguousarray(case["x"][b:b + 1])
            half = {"x": xb, "source": xb if case["source"] is case["x"] else np.ascontiguousarray(case["source"][b:b + 1]),
                    "dy": np.ascontiguousarray(case["dy"][b:b + 1]), "P": case["P"]}
            alone = run_layer(eb, half)
            assert alone["dx"].tobytes() == first["dx"][b:b + 1].tobytes() and alone["dsource"].tobytes() == first["dsource"][b:b + 1].tobytes()


def test_rejected_calls_launch_nothing(eb):
    arena = guarded.Arena(DEV, eb.workspace_bytes(1, 8, 8) + 16 * 4 * 8 * cases.C + 2 * 4 * eb.PARAM_FLOATS + 24 * guarded.GUARD)
    x, dy = (arena.put(torch.ones(1, 8, cases.C, device=DEV), name=n) for n in ("x", "dy"))
    params = arena.put(torch.ones(eb.PARAM_FLOATS, device=DEV), name="params")
    dx, ds = (arena.typed((1, 8, cases.C), torch.float32, name=n) for n in ("dx", "dsource"))
    dparams = arena.typed((eb.PARAM_FLOATS,), torch.float32, name="dparams")
    small = arena.typed((eb.workspace_bytes(1, 8, 8) - 256,), torch.uint8, name="workspace")
    good = dict(x=x, source=x, dy=dy, B=1, L=8, S=8, params=params, workspace=small, workspace_bytes=eb.workspace_bytes(1, 8, 8), dx=dx, dsource=ds,
                dparams=dparams, accumulate=False)
    for change, message in ((dict(workspace_bytes=small.numel()), "workspace_bytes below"), (dict(dx=x), "an output overlaps an input"),
                            (dict(dsource=dx), "two outputs overlap"), (dict(L=0), "L and S"), (dict(dparams=None), "null pointer"),
                            (dict(dy=dy.view(-1)[1:]), "16-byte aligned")):
        with pytest.raises(ValueError, match=message):
            eb.launch("openb_layer_grads", {**good, **change})
    torch.cuda.synchronize()
    arena.check()
    assert all(bool(torch.isnan(t).all()) for t in (dx, ds, dparams)) and bool((small == 0xFF).all())      # nothing was launched


# ---- 2. the chain ---------------------------------------------------------------------------------------------------------------------------
LOSS_CONFIG = {"coarse_type": "focal", "coarse_weight": 1.0, "focal_alpha": 0.25, "focal_gamma": 2.0, "pos_weight": 1.0, "neg_weight": 1.0,
               "fine_type": "l2_with_std", "fine_weight": 0.5, "fine_correct_thr": 1.0}
HW, NP = cases.CHAIN_HW, cases.CHAIN_POINTS


def test_the_chain_behind_the_training_forward_and_the_loss_backward(eb):
    from onepose_st_amd import loss_backward, supervision
    from onepose_st_amd.config import default_config
    from onepose_st_amd.model import OnePosePlus_model
    scene = cases.chain_scene()                                                         # the scene the CPU test derived CHAIN_BAR on
    cfg, sd, frames = scene["cfg"], scene["sd"], scene["frames"]
    feat_c, feat_f = (torch.cat([f[k] for f in frames]).to(DEV) for k in ("feat_c", "feat_f"))
    pose = np.stack([np.eye(4)] * 2)
    for b, f in enumerate(frames):
        pose[b, :3] = f["pose_gt"].numpy()
    ids = torch.from_numpy(np.stack([np.arange(NP, dtype=np.int64)] * 2)).to(DEV)
    gt = supervision.ground_truth(frames[0]["keypoints3d"].to(DEV), ids, pose, frames[0]["K"].numpy(), HW)

    def run(keep):
        model = OnePosePlus_model({**cfg, "hip_keep_layer_inputs": keep})
        model.load_state_dict(sd, strict=True)
        model.to(DEV).train()
        data = {k: frames[0][k].to(DEV) for k in ("keypoints3d", "descriptors3d_db", "descriptors3d_coarse_db")}
        data["ground_truth"] = gt
        data["query_image_scale"] = torch.ones(2, 2, device=DEV)
        model.enqueue_features(data, feat_c, feat_f, HW).finish()
        supervision.fine_supervision(data, {"OnePosePlus": cfg})
        supervision.Loss(LOSS_CONFIG).train()(data)
        return model, data

    (_, plain), (model, kept) = run(False), run(True)
    assert set(kept) - set(plain) == {"layer_inputs_c"}                                # without the key, no new entry
    for key in plain:
        if isinstance(plain[key], torch.Tensor):
            assert torch.equal(plain[key], kept[key]), key                              # and the same bytes everywhere
    with pytest.raises(KeyError, match="hip_keep_layer_inputs"):
        loss_backward.backward(plain, LOSS_CONFIG, {"OnePosePlus": cfg})
        eb.coarse_backward(plain, model)
    names = list(model.loftr_coarse.layer_names)
    inputs = kept["layer_inputs_c"]
    assert len(inputs) == len(names) == 6 and all(a.shape == (2, NP, 256) and b.shape == (2, 20, 256) for a, b in inputs)
    assert len({t.data_ptr() for pair in inputs for t in pair} | {kept["feat_c0"].data_ptr(), kept["feat_c1"].data_ptr()}) == 14
    # each kept pair is, byte for byte, what the forward consumed there: a model cut to the first n layers leaves layer n's inputs as its
    # coarse features (the training forward's matching, padding and fine stage behind them do not write them)
    for n in range(1, 6):
        cut_cfg = {**cfg, "loftr_coarse": {**cfg["loftr_coarse"], "layer_names": names[:n], "layer_iter_n": 1}}
        cut = OnePosePlus_model(cut_cfg)
        cut.load_state_dict({k: v for k, v in sd.items() if not any(k.startswith(f"loftr_coarse.layers.{j}.") for j in range(n, 6))}, strict=True)
        cut.to(DEV).train()
        data = {k: frames[0][k].to(DEV) for k in ("keypoints3d", "descriptors3d_db", "descriptors3d_coarse_db")}
        data.update(ground_truth=gt, query_image_scale=torch.ones(2, 2, device=DEV))
        cut.enqueue_features(data, feat_c, feat_f, HW).finish()
        assert torch.equal(data["feat_c0"], inputs[n][0]) and torch.equal(data["feat_c1"], inputs[n][1]), n
    loss_backward.backward(kept, LOSS_CONFIG, {"OnePosePlus": cfg}, grad=2.0)
    eb.coarse_backward(kept, model)
    torch.cuda.synchronize()
    assert all(p.grad is None for p in model.parameters())

    # what the forward consumed: every layer's kept inputs give the next layer's (the last: feat_c0 / feat_c1) through the float64 layer
    Ps = scene["params"]
    x3, x2 = (t.cpu().numpy() for t in inputs[0])
    for got, want in ((x3, scene["x3"]), (x2, scene["x2"])):                            # layer_inputs_c[0]: the stage's inputs
        assert np.abs(got - want).max() <= 1e-4 * np.abs(want).max()
    chain_kept, (y3, y2) = oracle.chain_forward(names, Ps, x3, x2)
    for i in range(6):
        nxt = inputs[i + 1] if i < 5 else (kept["feat_c0"], kept["feat_c1"])
        for got, want in zip(nxt, chain_kept[i + 1] if i < 5 else (y3, y2)):
            err = np.abs(got.cpu().numpy() - want).max() / np.abs(want).max()
            assert err <= 1e-3, (i, err)                                                 # (the forward's own parity tests hold it tighter)
    margins = []
    for i, name in enumerate(names):                                                     # the ReLU mask of every layer call is unambiguous
        a3, a2 = chain_kept[i]
        for xx, ss in ((a2, a2 if name == "self" else a3), (a3, a3 if name == "self" else a2)):
            bad, pre, dev = cases.relu_margin(xx.astype(np.float32), ss.astype(np.float32), Ps[i])
            margins.append(float(np.abs(pre).min() / dev))
    print(f"chain: smallest |pre-activation| in stand-in deviations, per call: {' '.join(f'{m:.3g}' for m in margins)}")
    g3, g2 = kept["grad_feat_c0"].cpu().numpy(), kept["grad_feat_c1"].cpu().numpy()
    w3, w2, wp = oracle.chain_grads(names, Ps, chain_kept, g3, g2)
    errs = {"grad_x3d_c": oracle.frame_error(kept["grad_x3d_c"].cpu().numpy(), w3), "grad_x2d_c": oracle.frame_error(kept["grad_x2d_c"].cpu().numpy(), w2)}
    grads = kept["grad_params_c"]
    assert set(grads) == {f"loftr_coarse.layers.{i}.{n}" for i in range(6) for n in oracle.PARAM_SHAPES}
    for i in range(6):
        for n in oracle.PARAM_SHAPES:
            errs[f"{i}.{n}"] = oracle.tensor_error(grads[f"loftr_coarse.layers.{i}.{n}"].cpu().numpy(), wp[i][n])
    worst = max(errs, key=errs.get)
    print(f"chain: worst {worst} {errs[worst]:.3e} (bar {cases.CHAIN_BAR:.1e}); inputs {errs['grad_x3d_c']:.3e} {errs['grad_x2d_c']:.3e}")
    assert errs[worst] <= cases.CHAIN_BAR, {k: v for k, v in errs.items() if v > cases.CHAIN_BAR}
