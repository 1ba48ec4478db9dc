"""``fine_concat_coarse_feat`` on the MI355X (run with ``-m gpu``): ``opfcx_merge`` of csrc/fine_context.hip against
the un-rounded float64 reference of tests/loftr_fine_context_reference.py at every tile edge, and the whole matcher with the switch.

Every buffer of a kernel call is a region of one guarded arena (tests/guarded.py) filled with 0xFF (NaN); outputs hold capacity for two
matches more than K, which must stay NaN.  Statistic and bar: ``|y - y_ref| / max(1, max |y_ref row|)`` against ``ROWS_BAR`` = 2.22e-05,
twice the float32 stand-in's worst value measured on the CPU; nothing here sizes a bar.

Largest device errors (MI355X, this file's own print-out; row error against the bar 2.220e-05):
    merge against float64 (in place == out of place, bit for bit)      1.121e-05
    composed form (ophip_rows_linear_x3 + torch) against float64       1.121e-05
    merge against the composed form                                    1.510e-06
    matcher windows 5 and 9, merged windows (forced)                   1.297e-05
    matcher, three views, masks and scales, merged windows (forced)    1.191e-05
    matcher, fine_f0 / fine_f1 against the oracle                      0.38 / 0.24 (window 5), 0.34 / 0.26 (window 9) of the bar (1e-3, 5e-4)
    matcher, mkpts1_f against the oracle                               2.1e-04 px (window 5), 2.6e-04 px (window 9)
"""
import copy
import ctypes

import pytest
import torch

from oracle import loftr_oracle as lo
from onepose_st_amd import fine_context, hip, loftr, packing
from onepose_st_amd.synthetic import make_synthetic_loftr_state_dict
from tests import loftr_fine_context_reference as R
from tests import test_gpu_loftr as tgl
from tests.guarded import Arena, guarded_empty
from tests.loftr_helpers import device_hook, planted_pair

pytestmark = pytest.mark.gpu

FIGURES = {}          # family -> (largest error seen, unit)
P, I64 = hip.ptr, torch.int64
SPARE = 2             # matches of capacity behind K in every window buffer: never touched


@pytest.fixture(scope="module")
def dev():
    if not torch.cuda.is_available():
        pytest.skip("needs the MI355X")
    hip.load()
    fine_context.load()
    yield torch.device("cuda:0")
    for family, (value, unit) in sorted(FIGURES.items()):
        print(f"largest device error  {family:44s} {value:.3e} {unit}")


@pytest.fixture(scope="module")
def sd():
    return make_synthetic_loftr_state_dict(0, fine_concat_coarse_feat=True)


@pytest.fixture(scope="module")
def wpack(sd, dev):
    return packing.pack_fine_context(sd).to(dev)


def note(family, value, unit):
    FIGURES[family] = (max(value, FIGURES.get(family, (0.0, unit))[0]), unit)


def within_rows_bar(family, got, ref, msg=""):
    e = R.row_error(got, ref)
    note(family, e, f"row error, bar {R.ROWS_BAR:.3e}")
    print(f"{family} {msg}: {e:.3e}")
    assert e <= R.ROWS_BAR, (family, msg, e)


def merge_on_arena(dev, case, wpack, in_place):
    """one ``fine_context.merge`` with every buffer (the call's own scratch too) on a guarded arena, the window buffers with SPARE matches
    of capacity behind K -> (out0, out1) on the host"""
    K, WW = case["K"], case["W"] ** 2
    arena = Arena(dev, 16 * (1 << 20) + 8 * (K + SPARE) * WW * 128 * 4 + 4 * (case["x0"].numel() + case["x1"].numel()))
    full = [arena.typed((K + SPARE, WW, 128), torch.float32, name=f"win{s}") for s in (0, 1)]
    for t, w in zip(full, (case["win0"], case["win1"])):
        t[:K].copy_(w)
    x0, x1, wp = arena.put(case["x0"], name="x0"), arena.put(case["x1"], name="x1"), arena.put(wpack, name="wpack")
    ids = [arena.put(case[k], name=k) for k in ("b_ids", "i_ids", "j_ids")]
    outs = full if in_place else [arena.typed((K + SPARE, WW, 128), torch.float32, name=f"out{s}") for s in (0, 1)]
    with guarded_empty(arena, 0xFF, [fine_context]):
        got = fine_context.merge(full[0][:K], full[1][:K], x0, x1, *ids, case["W"], wp, out=None if in_place else (outs[0][:K], outs[1][:K]))
    torch.cuda.synchronize()
    arena.check()
    assert got[0].data_ptr() == outs[0].data_ptr() and got[1].data_ptr() == outs[1].data_ptr()
    for o in outs:
        assert not bool(torch.isnan(o[:K]).any()) and bool(torch.isnan(o[K:]).all())          # every row of a match < K, none behind
    if not in_place:
        assert torch.equal(full[0][:K].cpu(), case["win0"]) and torch.equal(full[1][:K].cpu(), case["win1"])
    assert torch.equal(x0.cpu(), case["x0"]) and torch.equal(ids[1].cpu(), case["i_ids"])
    return outs[0][:K].cpu(), outs[1][:K].cpu()


def linear_x3(dev, x, w):
    """``x [T, kin] @ w.T`` through ``ophip_rows_linear_x3``"""
    T, kin = x.shape
    wp = packing.pack_linear_x3(w).to(dev)
    y = torch.full((T, w.shape[0]), float("nan"), device=dev)
    hip.call("ophip_rows_linear_x3", P(x), kin, None, 0, T, P(wp, None), w.shape[0], 0, P(y), hip.stream_handle())
    return y


def composed(dev, sd, win, x, b_ids, ids):
    """the same step from ``ophip_rows_linear_x3`` and torch: gather, three products, repeat, add"""
    wd, bd, wm, bm = (t.to(dev) for t in R._w(sd, torch.float32))
    K, WW = win.shape[:2]
    rows = x.to(dev)[(b_ids if x.shape[0] > 1 else torch.zeros_like(b_ids)).to(dev), ids.to(dev)].contiguous()
    c = linear_x3(dev, rows, wd.cpu()) + bd
    u = linear_x3(dev, c, wm[:, 128:].cpu()) + bm
    y = linear_x3(dev, win.to(dev).reshape(K * WW, 128).contiguous(), wm[:, :128].cpu())
    return (y.view(K, WW, 128) + u[:, None, :]).cpu()


# ---- the kernel at every tile edge ----------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", sorted(R.CASES))
def test_merge_at_every_tile_edge(dev, sd, wpack, name):
    case = R.make_case(name)
    ref = R.both_images(R.reference, sd, case)
    out = merge_on_arena(dev, case, wpack, in_place=False)
    inp = merge_on_arena(dev, case, wpack, in_place=True)
    for s in (0, 1):
        assert torch.equal(out[s], inp[s]), (name, s)                           # in place and out of place: the same bits
        within_rows_bar("merge against float64", out[s], ref[s], f"{name} image {s}")
    comp = (composed(dev, sd, case["win0"], case["x0"], case["b_ids"], case["i_ids"]),
            composed(dev, sd, case["win1"], case["x1"], case["b_ids"], case["j_ids"]))
    for s in (0, 1):
        within_rows_bar("merge against the composed form", out[s], comp[s], f"{name} image {s}")
        within_rows_bar("composed form against float64", comp[s], ref[s], f"{name} image {s}")


def test_no_matches_and_refused_arguments(dev, sd, wpack):
    case = R.make_case("w5_k3")
    K, S = case["K"], hip.stream_handle()
    d = {k: (v.to(dev) if isinstance(v, torch.Tensor) else v) for k, v in case.items()}
    out0, out1 = torch.full((K, 25, 128), float("nan"), device=dev), torch.full((K, 25, 128), float("nan"), device=dev)
    ctx = torch.full((2 * K * 128,), float("nan"), device=dev)
    good = dict(win0=P(d["win0"]), win1=P(d["win1"]), coarse0=P(d["x0"]), coarse0_bstride=0, coarse1=P(d["x1"]), coarse1_bstride=0,
                b_ids=P(d["b_ids"], I64), i_ids=P(d["i_ids"], I64), j_ids=P(d["j_ids"], I64), K=K, B=1, L0=30, L1=40, W=5, wpack=P(wpack, None),
                context=P(ctx), out0=P(out0), out1=P(out1), stream=S)
    call = lambda **change: fine_context.call("opfcx_merge", *fine_context.order("opfcx_merge", **{**good, **change}))
    call(K=0)                                                                   # no launch, nothing written
    torch.cuda.synchronize()
    assert bool(torch.isnan(out0).all()) and bool(torch.isnan(out1).all()) and bool(torch.isnan(ctx).all())
    empty = torch.empty(0, 25, 128, device=dev)
    none = torch.empty(0, dtype=I64, device=dev)
    assert fine_context.merge(empty, empty, d["x0"], d["x1"], none, none, none, 5, wpack)[0] is empty
    for change in ([{n: None} for n in ("win0", "win1", "coarse0", "coarse1", "b_ids", "i_ids", "j_ids", "wpack", "context", "out0", "out1")] +
                   [dict(K=-1), dict(B=0), dict(L0=0), dict(L1=0), dict(W=2), dict(W=4), dict(W=1), dict(W=13), dict(coarse0_bstride=-4),
                    dict(B=2, coarse1_bstride=40 * 256 - 4), dict(out0=ctypes.c_void_p(out0.data_ptr() + 4))]):
        with pytest.raises(ValueError, match="^opfcx_merge: opfcx_merge: "):
            call(**change)
    with pytest.raises(TypeError, match="takes 19 arguments"):
        fine_context.call("opfcx_merge", *fine_context.order("opfcx_merge", **good), S)
    with pytest.raises(ValueError, match="win1: a contiguous tensor"):
        fine_context.merge(d["win0"], d["win1"][:, :9], d["x0"], d["x1"], d["b_ids"], d["i_ids"], d["j_ids"], 5, wpack)
    with pytest.raises(TypeError):
        fine_context.merge(d["win0"], d["win1"], d["x0"], d["x1"], d["b_ids"].int(), d["i_ids"], d["j_ids"], 5, wpack)
    torch.cuda.synchronize()
    assert bool(torch.isnan(out0).all()) and bool(torch.isnan(out1).all()) and bool(torch.isnan(ctx).all())
    call()                                                                      # and the unchanged arguments run
    torch.cuda.synchronize()
    within_rows_bar("merge against float64", out0, R.both_images(R.reference, sd, case)[0], "after the refusals")


def test_a_cell_outside_the_tables_reads_a_zero_row(dev, sd, wpack):
    """the header's promise: nothing outside ``coarse`` is read; such a match gets the context of a zero coarse row"""
    case = R.make_case("w3_k7")
    bad = dict(case, i_ids=case["i_ids"].clone(), b_ids=case["b_ids"].clone())
    bad["i_ids"][2], bad["i_ids"][5] = 30, -1
    zero = dict(case, x0=torch.cat([case["x0"], torch.zeros(1, 30, 256)], 0), b_ids=case["b_ids"].clone())
    zero["b_ids"][2], zero["b_ids"][5] = 1, 1                                   # the same two matches on an all-zero image
    d = {k: (v.to(dev) if isinstance(v, torch.Tensor) else v) for k, v in bad.items()}
    got = fine_context.merge(d["win0"].clone(), d["win1"].clone(), d["x0"], d["x1"], d["b_ids"], d["i_ids"], d["j_ids"], 3, wpack)
    ref = R.reference(sd, zero["win0"], zero["x0"], zero["b_ids"], case["i_ids"])
    within_rows_bar("merge against float64", got[0], ref, "ids 30 and -1 of 30 cells")


# ---- the whole matcher ------------------------------------------------------------------------------------------------------------------
def config(W=9, **sub):
    cfg = copy.deepcopy(loftr.default_cfg)
    cfg["fine_concat_coarse_feat"], cfg["fine_window_size"] = True, W
    for k, v in sub.items():
        cfg[k].update(v)
    return cfg


def matcher_of(dev, sd, cfg):
    m = loftr.LoFTR_for_OnePose_Plus(cfg).eval()
    m.load_state_dict(sd, strict=True)
    return m.to(dev)


@pytest.mark.parametrize("W", [5, 9])
def test_matcher_with_the_switch_against_the_oracle(dev, sd, W):
    """the bars of ``test_gpu_loftr.py::test_matcher_on_planted_features_against_the_oracle`` on the floats, the indices exactly, and the
    merged windows against the float64 reference fed the DEVICE's coarse rows (forced: a coarse error cannot hide in the new step)"""
    H, Wi = 96, 128
    pair = planted_pair((H, Wi))
    cfg = config(W)
    with torch.no_grad():
        ref = R.forward_from_features(sd, cfg, *pair, (H, Wi))
    m = matcher_of(dev, sd, cfg)
    img = torch.zeros(1, 1, H, Wi)
    data = tgl._run(m, dev, img, img, device_hook(pair, dev))
    K = len(ref["i_ids"])
    assert K >= 40 and float((ref["mconf"] - 0.2).abs().min()) > 0.05           # the precondition, on the reference alone
    assert data["i_ids"].tolist() == ref["i_ids"].tolist() and data["j_ids"].tolist() == ref["j_ids"].tolist()
    assert data["b_ids"].tolist() == ref["b_ids"].tolist()
    close = tgl.close
    close(data["_feat_c0"], ref["feat_c0"], 2e-3, 1e-3, "coarse rows of image 0")
    close(data["_feat_c1"], ref["feat_c1"], 2e-3, 1e-3, "coarse rows of image 1")
    close(data["mconf"], ref["mconf"], 2e-3, 1e-5)
    assert torch.equal(data["mkpts0_c"].cpu(), ref["mkpts0_c"]) and torch.equal(data["mkpts1_c"].cpu(), ref["mkpts1_c"])
    for s, ids in ((0, "i_ids"), (1, "j_ids")):
        forced = R.reference(sd, ref[f"windows{s}"], data[f"_feat_c{s}"].cpu(), ref["b_ids"], ref[ids])
        within_rows_bar(f"matcher window {W}, merged windows (forced)", data[f"_fine_in{s}"], forced, f"image {s}")
        assert tuple(data[f"_fine_in{s}"].shape) == (K, W * W, 128)
    close(data["_fine_f0"], ref["fine_f0"], 1e-3, 5e-4, "fine transformer, image 0 windows")
    close(data["_fine_f1"], ref["fine_f1"], 1e-3, 5e-4, "fine transformer, image 1 windows")
    close(data["expec_f"][:, :2], ref["expec_f"][:, :2], 1e-3, 2e-4)
    close(data["mkpts1_f"], ref["mkpts1_f"], 1e-4, 2e-3)
    assert torch.equal(data["mkpts0_f"], data["mkpts0_c"])
    for key, rtol, atol in (("fine_f0", 1e-3, 5e-4), ("fine_f1", 1e-3, 5e-4)):
        note(f"matcher window {W}, {key}", float(((data["_" + key].cpu() - ref[key]).abs() / (atol + rtol * ref[key].abs())).max()),
             f"of the bar ({rtol}, {atol})")
    note(f"matcher window {W}, mkpts1_f", float((data["mkpts1_f"].cpu() - ref["mkpts1_f"]).abs().max()), "px")
    # the switch is live: the same weights without it give other fine features
    plain = matcher_of(dev, {k: v for k, v in sd.items() if not k.startswith("fine_preprocess.")}, dict(cfg, fine_concat_coarse_feat=False))
    other = tgl._run(plain, dev, img, img, device_hook(pair, dev))
    assert other["i_ids"].tolist() == data["i_ids"].tolist() and not torch.equal(other["_fine_f0"], data["_fine_f0"])
    assert "_fine_in0" not in other


def test_batched_views_lazy_and_full_forms(dev, sd):
    """three views against ONE query in one call: every pair's outputs are bit-identical to that pair run alone (the context of image 1 is
    then read from rows ``[V, L1, 256]``); the lazy form gives the eager form's bits; full fine attention runs on the merged windows"""
    H, Wi = 96, 128
    x0, g0, xq, gq = planted_pair((H, Wi), seed=30)
    g = torch.Generator().manual_seed(31)
    views = [(x0, g0),
             (x0 + 0.05 * torch.randn(x0.shape, generator=g), g0 + 0.05 * torch.randn(g0.shape, generator=g)),
             (torch.randn(x0.shape, generator=g), torch.randn(g0.shape, generator=g))]
    cl = lambda t: t[0].permute(1, 2, 0).reshape(-1, 128).contiguous()

    def batched_hook(fc0, ff0, fc1, ff1):
        assert fc0.shape[0] == 3 and fc1.shape[0] == 1
        return (torch.cat([v[0] for v in views]).to(dev), torch.stack([cl(v[1]) for v in views]).to(dev), xq.to(dev), cl(gq)[None].to(dev))
    m = matcher_of(dev, sd, config(5))
    zeros = lambda n: torch.zeros(n, 1, H, Wi)
    batch = tgl._run(m, dev, zeros(3), zeros(1), batched_hook)
    singles = [tgl._run(m, dev, zeros(1), zeros(1), device_hook((v[0], v[1], xq, gq), dev)) for v in views]
    assert len(singles[0]["i_ids"]) >= 40 and len(singles[1]["i_ids"]) >= 40
    keys = ("i_ids", "j_ids", "mconf", "mkpts0_c", "mkpts1_c", "mkpts0_f", "mkpts1_f", "expec_f", "_fine_in0", "_fine_in1", "_fine_f0", "_fine_f1")
    for k, one in enumerate(singles):
        sel = batch["b_ids"] == k
        assert torch.equal(batch["b_ids"][sel], torch.full_like(one["b_ids"], k))
        for key in keys:
            assert torch.equal(batch[key][sel], one[key]), (k, key)
    # lazy conf_matrix: the same bits
    m.feature_hook = batched_hook
    try:
        lazy = {"image0": zeros(3).to(dev), "image1": zeros(1).to(dev)}
        m(lazy, _debug=True, conf_matrix="lazy")
    finally:
        m.feature_hook = None
    assert not isinstance(lazy["conf_matrix"], torch.Tensor)
    for key in ("b_ids",) + keys:
        assert torch.equal(lazy[key], batch[key]), key
    # masks (all cells real: the masked kernels) and scales in one call: the merged windows against the reference fed this call's rows
    ones = lambda n: torch.ones(n, H // 8, Wi // 8, dtype=torch.bool, device=dev)
    m.feature_hook = batched_hook
    try:
        extra = {"image0": zeros(3).to(dev), "image1": zeros(1).to(dev), "mask0": ones(3), "mask1": ones(1),
                 "scale0": torch.tensor([[1.25, 0.75], [1.0, 1.0], [0.5, 2.0]], device=dev), "scale1": torch.tensor([[2.0, 1.5]], device=dev)}
        m(extra, _debug=True)
    finally:
        m.feature_hook = None
    b_ids = extra["b_ids"].cpu()
    assert len(b_ids) >= 80 and extra["mkpts1_f"].shape == (len(b_ids), 2) and bool(torch.isfinite(extra["mkpts1_f"]).all())
    maps = (torch.cat([v[1] for v in views]), gq.expand(3, -1, -1, -1))
    for s, ids in ((0, "i_ids"), (1, "j_ids")):
        windows = lo.fine_windows(maps[s], b_ids, extra[ids].cpu(), (H // 8, Wi // 8), 5)
        forced = R.reference(sd, windows, extra[f"_feat_c{s}"].cpu(), b_ids, extra[ids].cpu())
        within_rows_bar("matcher, masks and scales, merged windows (forced)", extra[f"_fine_in{s}"], forced, f"image {s}")
    # full fine attention on the merged windows: the same merged windows, other fine features, finite results
    full = matcher_of(dev, sd, config(5, fine={"attention": "full"}))
    fdata = tgl._run(full, dev, zeros(3), zeros(1), batched_hook)
    assert torch.equal(fdata["_fine_in0"], batch["_fine_in0"]) and torch.equal(fdata["_fine_in1"], batch["_fine_in1"])
    assert not torch.equal(fdata["_fine_f0"], batch["_fine_f0"]) and bool(torch.isfinite(fdata["expec_f"]).all())
    d = (fdata["mkpts1_f"] - batch["mkpts1_f"]).abs().max().item()
    print(f"full against linear fine attention on the merged windows: max |mkpts1_f difference| = {d:.3e} px")


def test_the_empty_path(dev, sd):
    """no confidence (a product of two softmax values: 1 + a rounding at the most) passes a threshold of 2: the reference's empty shapes, and
    ``opfcx_merge`` is not reached"""
    m = matcher_of(dev, sd, config(9, match_coarse={"thr": 2.0}))
    pair = planted_pair((96, 128))
    img = torch.zeros(1, 1, 96, 128)
    data = tgl._run(m, dev, img, img, device_hook(pair, dev))
    assert data["b_ids"].shape == (0,) and data["expec_f"].shape == (0, 3) and data["mkpts0_f"].shape == (0, 2) and data["mkpts1_f"].shape == (0, 2)
    assert "_fine_in0" not in data
    with pytest.raises(NotImplementedError, match="provided coarse matches"):
        m({"image0": img.to(dev), "image1": img.to(dev), "mkpts0_c": torch.zeros(2, 2, device=dev), "mkpts1_c": torch.zeros(2, 2, device=dev)})
    assert data["bs"] == 1
