"""The fine stage on the device -- ``ophip_fine_refine`` (exact f32), ``ophip_fine_refine_bf16`` with nsplit 3 (split-bf16) and 1 (plain
bf16) and their ``_scaled`` forms, default pair kernel, debug outputs requested -- against the float64 restatement of
tests/bf16_faithful.py, over layer patterns, match counts, map layouts, planted heat maps and a count above the capacity.

Bounds.  f32 and split-bf16 against the UN-rounded float64 computation at the bars of test_gpu_parity.py::test_fine_refine_vs_oracle
(rtol 1e-4 / atol 2e-5, and 5e-4 / 2e-4).  Plain bf16 against the float64 computation that rounds where the kernel rounds, two statistics
at K = 256: (a) every match within the old 1e-1 / 1e-1; (b) the SHARE of matches whose windows and 3D token all meet the f32 bar.  A
match misses that bar only through a "flip" (a value within ~1e-7 of a bf16 rounding boundary rounds the other way in f32 than in float64
and the layer spreads 2^-8 over the match); tests/test_bf16_faithful_cpu.py shows that an f32 stand-in of the reference itself has shares
of 0.70 (two layers) and 0.81 / 0.89 (one layer), and that a computation which is off by the size of the rounding has a share of 0.  Caps:
>= 0.40 with two or more layers, >= 0.55 with one; with the encoder disabled nothing is rounded and every match meets the f32 bar.

Measured on the MI355X at K = 256 (max abs error of windows / 3D token / mkpts_f [px]; the module prints them):

    layers (cross_bits)   f32                        split-bf16                 plain bf16: worst match      share at the f32 bar
    2 (0b10, product)     3.8e-6 / 3.0e-6 / 1.1e-5   6.6e-5 / 5.6e-5 / 1.3e-4   1.2e-2 / 1.1e-2 / 1.1e-2     0.738
    1 (0b0, self)         2.4e-6 / 1.9e-6 / 5.1e-6   4.2e-5 / 3.2e-5 / 6.2e-5   6.4e-3 / 9.3e-5 / 7.9e-4     0.852
    1 (0b1, cross)        2.7e-6 / 2.5e-6 / 8.3e-6   4.6e-5 / 3.5e-5 / 5.2e-5   1.5e-3 / 5.9e-3 / 1.5e-3     0.914
    2 (0b01)              3.6e-6 / 3.4e-6 / 1.2e-5   6.4e-5 / 5.2e-5 / 1.1e-4   1.0e-2 / 1.1e-2 / 7.2e-3     0.695
    4 (0b1010)            5.4e-6 / 4.5e-6 / 2.0e-5   9.0e-5 / 7.5e-5 / 2.5e-4   2.2e-2 / 2.2e-2 / 2.2e-2     0.504
    encoder disabled      0 / 0 / 2.4e-6             0 / 0 / 1.9e-6             0 / 0 / 1.9e-6               1.000

The device's shares lie at or above the CPU stand-in's (0.70 / 0.81 / 0.89): ``__expf`` and ``v_rcp_f32`` move no more values across
rounding boundaries than accumulation order does, and the reference misses no rounding point.  The caps stay at the issue's 0.40 / 0.55.
Planted heat maps land within 9.0e-6 of their grid point in every mode and layout.
"""

import pytest
import torch

from onepose_st_amd import hip, matchcall, packing
from tests import bf16_faithful as bf

pytestmark = pytest.mark.gpu

PREFIX = "loftr_fine.layers."
MODES = ["f32", "bf16x3", "bf16"]
BAR = {"f32": (1e-4, 2e-5), "bf16x3": (5e-4, 2e-4), "bf16": (1e-1, 1e-1)}
# (nlayers, cross_bits, encoder_enable): the product's (self, cross) first
PATTERNS = [(2, 0b10, 1), (1, 0, 1), (1, 1, 1), (2, 0b01, 1), (4, 0b1010, 1), (2, 0b10, 0)]
FINE_SCALE = 4.0          # (W // 2) * image height / fine height = 2 * 2


@pytest.fixture(scope="module")
def dev():
    assert torch.cuda.is_available(), "these tests need the MI355X"
    hip.load()
    return torch.device("cuda:0")


@pytest.fixture(autouse=True)
def _no_precision_override(monkeypatch):
    monkeypatch.delenv("OPHIP_FINE_PRECISION", raising=False)      # (would turn every nsplit = 3 call into nsplit = 1)


@pytest.fixture(scope="module")
def sd4(sd):
    return bf.layer_state_dict(sd, 4, PREFIX)


@pytest.fixture(scope="module")
def weights(sd4, dev):
    cache = {}

    def get(mode, nl):
        if (mode, nl) not in cache:
            if mode == "f32":
                cache[mode, nl] = torch.cat([packing.pack_fine_layer(sd4, f"{PREFIX}{i}.") for i in range(nl)]).to(dev)
            else:
                cache[mode, nl] = packing.pack_fine_layers_bf16(sd4, PREFIX, nl).to(dev)
                assert cache[mode, nl].numel() == hip.load().ophip_fine_bf16_wpack_bytes(nl)
        return cache[mode, nl]
    return get


@pytest.fixture(scope="module")
def reference(sd4):
    """float64 references, computed once per (case, pattern, nsplit) and left unchanged"""
    cache = {}

    def get(name, c, nl, bits, enc, nsplit, qscale=None):
        key = (name, nl, bits, enc, nsplit if enc else 0, qscale is not None)
        if key not in cache:
            cache[key] = bf.fine_stage_faithful(sd4, c["feat"], c["desc"], c["b_ids"], c["i_ids"], c["j_ids"], c["mkc"], c["wc"], c["stride"],
                                                FINE_SCALE, [bool((bits >> l) & 1) for l in range(nl)], nsplit, bool(enc), qscale, PREFIX)
        return cache[key]
    return get


@pytest.fixture(scope="module")
def case256():
    return bf.random_case(256)


@pytest.fixture(scope="module")
def case64():
    return bf.random_case(64, seed=8)


def _edge_case():
    """B = 3 with ``b_ids`` that skip element 1, hf = 10 != wf = 12 at stride 2 (a window reaches two pixels from ``stride * cell``, so only a
    stride below 3 puts the bottom and right cells' windows across the map's edge): the four corner cells, one cell on each edge and one
    interior cell, in both batch elements -- an odd count of 19 with the last match alone in its workgroup"""
    g = torch.Generator().manual_seed(31)
    B, N, hc, wc, stride = 3, 40, 5, 6, 2
    cells = [0, wc - 1, (hc - 1) * wc, hc * wc - 1, 2, (hc - 1) * wc + 3, 2 * wc, 3 * wc - 1, 2 * wc + 3]
    j_ids = torch.tensor(cells + cells + [wc + 1])
    b_ids = torch.tensor([0] * 9 + [2] * 10)
    K = len(j_ids)
    c = dict(feat=torch.randn(B, bf.CF, hc * stride, wc * stride, generator=g), desc=torch.randn(B, bf.CF, N, generator=g), b_ids=b_ids,
             i_ids=torch.randint(0, N, (K,), generator=g), j_ids=j_ids, mkc=torch.stack([j_ids % wc, j_ids // wc], 1).float() * 8.0,
             hc=hc, wc=wc, hf=hc * stride, wf=wc * stride, stride=stride)
    return c


@pytest.fixture(scope="module")
def edge_case():
    return _edge_case()


@pytest.fixture(scope="module")
def planted():
    return bf.planted_case()


def _layout(feat, kind, dev):
    """the fine map as the kernel sees it: dense NCHW, dense channels-last, or a view of either cut out of a larger NaN-filled buffer"""
    B, C, hf, wf = feat.shape
    f = feat.to(dev)
    if kind == "nchw":
        return f
    if kind == "cl":
        f = f.contiguous(memory_format=torch.channels_last)
        assert f.stride(1) == 1
        return f
    if kind == "nchw_view":
        big = torch.full((B, C + 1, hf + 3, wf + 5), float("nan"), device=dev)
        v = big[:, :C, 1:1 + hf, 2:2 + wf]
        v.copy_(f)
        assert v.stride(2) == wf + 5 > wf and v.stride(0) > C * hf * wf and v.stride(3) == 1
        return v
    if kind == "cl_view":
        big = torch.full((B, hf + 2, wf + 3, C + 4), float("nan"), device=dev)
        v = big[:, 1:1 + hf, 1:1 + wf, :C].permute(0, 3, 1, 2)
        v.copy_(f)
        assert v.stride(1) == 1 and v.stride(3) == C + 4 and v.stride(2) == (wf + 3) * (C + 4) and v.stride(0) > C * hf * wf
        assert all(s % 4 == 0 for s in (v.stride(0), v.stride(2), v.stride(3))) and v.data_ptr() % 16 == 0
        return v
    raise ValueError(kind)


def run(dev, mode, c, w, nl, bits, enc, count, cap, rows=None, layout="nchw", qscale=None, dbg=True):
    """One call with ``max_matches = cap`` and the device count ``count``; every list and output has ``rows`` (default: cap) rows, outputs
    NaN-filled.  Returns the whole buffers."""
    rows = cap if rows is None else rows
    n = min(len(c["b_ids"]), rows)

    def pad(t):
        out = torch.zeros(rows, *t.shape[1:], dtype=t.dtype)
        out[:n] = t[:n]
        return out.to(dev)
    bd, idd, jd, mkd = pad(c["b_ids"]), pad(c["i_ids"]), pad(c["j_ids"]), pad(c["mkc"])
    ff, dd = _layout(c["feat"], layout, dev), c["desc"].to(dev)
    cnt = torch.tensor([count], dtype=torch.int32, device=dev)
    nan = lambda *s: torch.full(s, float("nan"), device=dev)
    expec, mkf, dw, d3 = nan(rows, 3), nan(rows, 2), nan(rows, 25, 128), nan(rows, 128)
    qd = None if qscale is None else qscale.to(dev)
    matchcall.fine_refine(ff, ff.stride(), c["hf"], c["wf"], dd, b_ids=bd, i_ids=idd, j_ids=jd, count=cnt, mkpts_c=mkd, max_matches=cap, wpack=w,
                          nlayers=nl, cross_bits=bits, encoder_enable=enc, nsplit={"f32": None, "bf16x3": 3, "bf16": 1}[mode], wc=c["wc"],
                          stride=c["stride"], fine_scale=FINE_SCALE, expec_f=expec, mkpts_f=mkf, dbg_win=dw if dbg else None,
                          dbg_f3=d3 if dbg else None, query_scale=qd)
    torch.cuda.synchronize()
    return {"expec_f": expec.cpu(), "mkpts_f": mkf.cpu(), "windows": dw.cpu(), "f3": d3.cpu()}


def _maxerr(got, ref, K):
    return {k: (got[k][:K].double() - ref[k][:K]).abs().max().item() for k in ("windows", "f3", "mkpts_f")} | {
        "expec_xy": (got["expec_f"][:K, :2].double() - ref["expec_f"][:K, :2]).abs().max().item(),
        "std": (got["expec_f"][:K, 2].double() - ref["expec_f"][:K, 2]).abs().max().item()}


def check(got, ref, K, rt, at, label):
    """the assertions of test_fine_refine_vs_oracle at (rt, at), against float64; std at the project's 1e-3 (ill-conditioned)"""
    errs = _maxerr(got, ref, K)
    print(f"{label}: max abs err " + ", ".join(f"{k} {v:.2e}" for k, v in errs.items()))
    for k, r, a in (("windows", rt, at), ("f3", rt, at), ("mkpts_f", rt, 4 * at)):
        assert bool(bf.meets(got[k][:K], ref[k][:K], r, a).all()), (label, k, errs)
    assert bool(bf.meets(got["expec_f"][:K, :2], ref["expec_f"][:K, :2], rt, at).all()), (label, "expec_xy", errs)
    assert bool(bf.meets(got["expec_f"][:K, 2:], ref["expec_f"][:K, 2:], max(rt, 1e-3), max(at, 1e-3)).all()), (label, "std", errs)


def _nan_from(got, K):
    return all(bool(torch.isnan(t[K:]).all()) for t in got.values())


@pytest.mark.parametrize("nl,bits,enc", PATTERNS)
@pytest.mark.parametrize("mode", MODES)
def test_layer_patterns(dev, weights, reference, case256, mode, nl, bits, enc):
    K = 256
    got = run(dev, mode, case256, weights(mode, nl), nl, bits, enc, K, K)
    label = f"{mode} layers {nl} cross_bits {bits:#b} encoder {enc}"
    if mode != "bf16":
        check(got, reference("c256", case256, nl, bits, enc, 0), K, *BAR[mode], label)
        return
    ref = reference("c256", case256, nl, bits, enc, 1)
    check(got, ref, K, *BAR["bf16"], label)                                      # (a) the old bound, every match
    share = bf.share_at_f32_bar(got["windows"], got["f3"], ref)                  # (b)
    cap = 1.0 if not enc else 0.40 if nl >= 2 else 0.55
    print(f"{label}: share of matches at the f32 bar {share:.3f} (required {cap})")
    assert share >= cap, (label, share)
    if not enc:
        check(got, ref, K, *BAR["f32"], label + " (nothing rounded)")


@pytest.mark.parametrize("cap", [64, 63])
@pytest.mark.parametrize("mode", MODES)
def test_counts_and_nan_fill(dev, weights, reference, case64, mode, cap):
    """count in {0, 1, 2, 37, cap}: rows >= count of every output keep their NaN fill (count 0: nothing is written), rows < count are the
    rows of the count = cap run bit for bit, and that run meets the mode's bar."""
    w = weights(mode, 2)
    full = run(dev, mode, case64, w, 2, 0b10, 1, cap, cap)
    assert _nan_from(full, cap) and all(bool(torch.isfinite(t).all()) for t in full.values())
    check(full, reference("c64", case64, 2, 0b10, 1, 1 if mode == "bf16" else 0), cap, *BAR[mode], f"{mode} cap {cap}")
    for count in (0, 1, 2, 37):
        got = run(dev, mode, case64, w, 2, 0b10, 1, count, cap)
        for k, t in got.items():
            assert bool(torch.isnan(t[count:]).all()), (k, count)
            assert torch.equal(t[:count], full[k][:count]), (k, count)


@pytest.mark.parametrize("cap", [64, 63])
@pytest.mark.parametrize("mode", MODES)
def test_count_above_capacity_is_clamped(dev, weights, case64, mode, cap):
    """A device count above ``max_matches`` (cap + 5): the kernels clamp it.  Every list and output has cap + 2 rows, so whatever row the
    unclamped pair kernel reaches (with an odd capacity its last workgroup takes row ``cap`` for a live second match: ids 0, outputs one
    row past the capacity) lies inside the test's buffers; rows >= cap must keep their NaN fill and rows < cap equal the count = cap run."""
    w = weights(mode, 2)
    want = run(dev, mode, case64, w, 2, 0b10, 1, cap, cap, rows=cap + 2)
    got = run(dev, mode, case64, w, 2, 0b10, 1, cap + 5, cap, rows=cap + 2)
    for k, t in got.items():
        assert bool(torch.isnan(t[cap:]).all()), f"{k}: rows past the capacity were written"
        assert torch.equal(t[:cap], want[k][:cap]) and bool(torch.isfinite(t[:cap]).all()), k


@pytest.mark.parametrize("mode", MODES)
def test_map_layouts_corners_and_edges(dev, weights, reference, edge_case, mode):
    """NCHW, channels-last, and views of both inside larger NaN-filled buffers (row / batch strides above the dense ones): with the encoder
    disabled the debug rows ARE the gather -- bit for bit, exact zeros in the padded window rows of corner and edge cells; with it enabled the
    NCHW result meets the mode's bar and the other three layouts reproduce it bit for bit (the gather only copies)."""
    c, K = edge_case, len(edge_case["b_ids"])
    tok = bf.gather_tokens(c["feat"], c["desc"], c["b_ids"], c["i_ids"], c["j_ids"], c["wc"], c["stride"], torch.float32)
    zero_rows = (tok[:, :25] == 0).all(2)
    assert [int(z.sum()) for z in zero_rows[:9]] == [16, 13, 13, 9, 10, 5, 10, 5, 0]      # corners TL TR BL BR, edges top bottom left right, interior
    # all four corners and all four edges: the padded rows of each are a different set
    assert len({tuple(r.tolist()) for r in zero_rows[:8]}) == 8
    w = weights(mode, 2)
    base = None
    for layout in ("nchw", "cl", "nchw_view", "cl_view"):
        raw = run(dev, mode, c, w, 2, 0b10, 0, K, K + 1, layout=layout)
        assert torch.equal(raw["windows"][:K], tok[:, :25]) and torch.equal(raw["f3"][:K], tok[:, 25]), layout
        assert _nan_from(raw, K)
        got = run(dev, mode, c, w, 2, 0b10, 1, K, K + 1, layout=layout)
        assert _nan_from(got, K)
        if base is None:
            base = got
            check(got, reference("edge", c, 2, 0b10, 1, 1 if mode == "bf16" else 0), K, *BAR[mode], f"{mode} corners and edges")
        else:
            for k in got:
                assert torch.equal(got[k][:K], base[k][:K]), (layout, k)


@pytest.mark.parametrize("layout", ["nchw", "cl"])
@pytest.mark.parametrize("mode", MODES)
def test_planted_heat_maps_land_on_their_grid_point(dev, weights, reference, planted, mode, layout):
    """Encoder disabled, window row r* = the match's 3D descriptor, every r* in 0..24 twice: the expectation must land on the (x, y) grid
    point of r* within 0.01 -- an axis or sign swap, which ``randn`` data averages away, moves it by >= 0.5."""
    c, K = planted, len(planted["b_ids"])
    got = run(dev, mode, c, weights(mode, 2), 2, 0b10, 0, K, K, layout=layout)
    err = (got["expec_f"][:, :2].double() - c["want_xy"]).abs().max().item()
    print(f"{mode} {layout}: planted heat maps, max |expectation - grid point| = {err:.2e}")
    assert err < 0.01
    check(got, reference("planted", c, 0, 0, 0, 0), K, *BAR["f32"], f"{mode} planted")      # nothing is rounded: the f32 bar in every mode


@pytest.mark.parametrize("enc", [1, 0])
@pytest.mark.parametrize("mode", MODES)
def test_scaled_form(dev, weights, reference, planted, mode, enc):
    """``query_scale`` differs per batch element and between its h and w factor; B = 3, ``b_ids`` skip element 1.  mkpts_f against the
    faithful formula at the mode's bar, and against the formula applied to the kernel's OWN expectation within the three f32 roundings
    the kernel spends on it (2^-24 each, of the larger term)."""
    c, K = planted, len(planted["b_ids"])
    qs = torch.tensor([[1.25, 0.75], [7.0, 9.0], [0.5, 2.0]])
    got = run(dev, mode, c, weights(mode, 2), 2, 0b10, enc, K, K, qscale=qs)
    ref = reference("planted", c, 2 if enc else 0, 0b10 if enc else 0, enc, 1 if mode == "bf16" else 0, qs)
    check(got, ref, K, *(BAR[mode] if enc else BAR["f32"]), f"{mode} scaled, encoder {enc}")
    own = bf.keypoints(c["mkc"], got["expec_f"].double(), FINE_SCALE, c["b_ids"], qs)
    mag = c["mkc"].double().abs() + (own - c["mkc"].double()).abs()
    assert bool(((got["mkpts_f"].double() - own).abs() <= 3 * 2.0 ** -24 * mag + 1e-30).all())
    plain = run(dev, mode, c, weights(mode, 2), 2, 0b10, enc, K, K)
    assert torch.equal(plain["expec_f"], got["expec_f"])                         # the scale only enters the keypoint
    assert (plain["mkpts_f"] - got["mkpts_f"]).abs().max().item() > 0.1


@pytest.mark.parametrize("mode", MODES)
def test_debug_buffers_do_not_change_the_result(dev, weights, case64, mode):
    w = weights(mode, 2)
    with_dbg = run(dev, mode, case64, w, 2, 0b10, 1, 37, 64)
    without = run(dev, mode, case64, w, 2, 0b10, 1, 37, 64, dbg=False)
    for k in ("expec_f", "mkpts_f"):
        assert torch.equal(with_dbg[k][:37], without[k][:37]) and bool(torch.isfinite(without[k][:37]).all()), k
    assert _nan_from(without, 37) and bool(torch.isnan(without["windows"]).all())
