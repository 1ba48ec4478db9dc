"""The four per-match kernels of the full-attention fine stage (csrc/fine_full.hip) at the kernel: ``ophip_fine_full_gather`` bit for bit against a
numpy gather, ``ophip_fine_full_attention`` and ``ophip_fine2_full_attention`` against float64 by ``ff.FINE_ATTENTION_BAR``,
``ophip_fine_full_match`` against the oracle's fine matching in float64 by ``ff.MATCH_BAR`` (tests/full_faithful.py; every bar is three times the
float32 stand-in's worst or, where said there, reasoned; tests/test_full_faithful_cpu.py pins them).  Every buffer is a region of one
``tests/guarded.Arena``, outputs start as NaN and carry spare rows."""
import numpy as np
import pytest
import torch

from onepose_st_amd import hip
from tests import full_faithful as ff
from tests.guarded import arena_for, is_fill as is_nan_fill

pytestmark = pytest.mark.gpu

CF = ff.CF
SPARE = 2


@pytest.fixture(scope="module")
def dev():
    assert torch.cuda.is_available(), "these tests need the MI355X"
    hip.load()
    return torch.device("cuda:0")


# ------------------------------------------------------------------------------------------------
# gather
# ------------------------------------------------------------------------------------------------
HF, WF, STRIDE = 23, 29, 2                              # a map whose sides are multiples of nothing; cells at stride 2 reach its last row and column
HC, WC = (HF + STRIDE - 1) // STRIDE, (WF + STRIDE - 1) // STRIDE
CELLS = [(0, 0), (0, WC - 1), (HC - 1, 0), (HC - 1, WC - 1), (0, 7), (HC - 1, 7), (5, 0), (5, WC - 1), (5, 7)]      # corners, edges, interior
NPTS = 13


def gather_case():
    g = torch.Generator().manual_seed(77)
    feat = torch.randn(2, CF, HF, WF, generator=g)
    desc = torch.randn(2, CF, NPTS, generator=g)
    j_ids = torch.tensor([cy * WC + cx for cy, cx in CELLS])
    b_ids = torch.tensor([0, 1, 1, 0, 1, 0, 0, 1, 1])
    i_ids = torch.randint(0, NPTS, (len(CELLS),), generator=g)
    return feat, desc, b_ids, i_ids, j_ids


def gather_numpy(feat, desc, b_ids, i_ids, j_ids, count, W, shared_desc):
    cap, half = len(j_ids), W // 2
    win, f3 = np.zeros((cap, W * W, CF), np.float32), np.zeros((cap, CF), np.float32)
    f, d = feat.numpy(), desc.numpy()
    for m in range(count):
        b, cell = int(b_ids[m]), int(j_ids[m])
        cy, cx = STRIDE * (cell // WC), STRIDE * (cell % WC)
        for r in range(W * W):
            y, x = cy + r // W - half, cx + r % W - half
            if 0 <= y < HF and 0 <= x < WF:
                win[m, r] = f[b, :, y, x]
        f3[m] = d[0 if shared_desc else b, :, int(i_ids[m])]
    return win, f3


@pytest.mark.parametrize("shared_desc", [False, True])
@pytest.mark.parametrize("layout", ["nchw", "channels_last"])
@pytest.mark.parametrize("W", [3, 5, 7, 9, 11])
def test_gather_is_a_plain_gather(dev, W, layout, shared_desc):
    feat, desc, b_ids, i_ids, j_ids = gather_case()
    cap, WW = len(j_ids), W * W
    if shared_desc:
        desc = desc[:1]
    stored = feat if layout == "nchw" else feat.permute(0, 2, 3, 1).contiguous()
    strides = (CF * HF * WF, HF * WF, WF, 1) if layout == "nchw" else (HF * WF * CF, 1, WF * CF, CF)          # of (b, c, y, x)
    for count in (0, cap - 1, cap):
        a = arena_for(dev, feat.numel() * 4, desc.numel() * 4, cap * 8, cap * 8, cap * 8, 16, (cap + SPARE) * WW * CF * 4, (cap + SPARE) * CF * 4)
        df, dd = a.put(stored, name="feat_f"), a.put(desc, name="desc3d_f")
        db, di, dj = a.put(b_ids, name="b_ids"), a.put(i_ids, name="i_ids"), a.put(j_ids, name="j_ids")
        dc = a.put(torch.tensor([count, 0, 0, 0], dtype=torch.int32), name="count")
        win, f3 = a.typed((cap + SPARE, WW, CF), torch.float32, name="windows"), a.typed((cap + SPARE, CF), torch.float32, name="feat3d")
        hip.launch("ophip_fine_full_gather", dict(feat_f=df, fs_b=strides[0], fs_c=strides[1], fs_y=strides[2], fs_x=strides[3], hf=HF, wf=WF,
                                                  desc3d_f=dd, d_bs=0 if shared_desc else CF * NPTS, d_cs=NPTS, b_ids=db, i_ids=di, j_ids=dj,
                                                  count=dc, cap=cap, wc=WC, stride=STRIDE, W=W, windows=win, feat3d=f3))
        torch.cuda.synchronize()
        want_win, want_f3 = gather_numpy(feat, desc, b_ids, i_ids, j_ids, count, W, shared_desc)
        assert is_nan_fill(win[cap:]) and is_nan_fill(f3[cap:]), "rows past the capacity were written"
        assert np.array_equal(win[:cap].cpu().numpy().view(np.int32), want_win.view(np.int32)), (W, layout, count)
        assert np.array_equal(f3[:cap].cpu().numpy().view(np.int32), want_f3.view(np.int32)), (W, layout, count)
        assert not win[count:cap].any() and not f3[count:cap].any()
        a.check()


# ------------------------------------------------------------------------------------------------
# the two attention kernels
# ------------------------------------------------------------------------------------------------
def run_fine_attention(dev, entry, c, count):
    """``count``: None (the pointer is NULL, or the entry takes none) or the device-side count"""
    K, L, S = c["q"].shape[0], c["q"].shape[1], c["k"].shape[1]
    a = arena_for(dev, K * L * CF * 4, K * S * CF * 4, K * S * CF * 4, 16, (K * L + SPARE) * CF * 4)
    q, k, v = (a.put(c[n], name=n) for n in ("q", "k", "v"))
    out = a.typed((K * L + SPARE, CF), torch.float32, name="msg")
    named = dict(q=q, k=k, v=v, K=K, L=L, S=S, msg=out)
    if entry == "ophip_fine_full_attention":
        named["count"] = None if count is None else a.put(torch.tensor([count, 0, 0, 0], dtype=torch.int32), name="count")
    hip.launch(entry, named)
    torch.cuda.synchronize()
    assert is_nan_fill(out[K * L:]), "rows past the output were written"
    o = out[:K * L].view(K, L, CF).cpu()
    assert not bool(torch.isnan(o).any())
    a.check()
    return o


def check_fine_attention(o, family, c, ref, live, label):
    bar = ff.FINE_ATTENTION_BAR[family]
    assert not o[live:].any(), f"{label}: matches at or past the count are zeros"
    if live == 0:
        return 0.0
    e = ff.attention_error(o[:live], ref[:live], c["v"][:live], ff.FNH)
    assert e <= bar, (label, e, bar)
    L, S = o.shape[1], c["k"].shape[1]
    if family == "peaked_last":                         # the output is the last value row
        es = ff.attention_error(o[:live], c["v"][:live, S - 1:].double().expand(-1, L, -1), c["v"][:live], ff.FNH)
        assert es <= bar + 2 * (1 - ff.SELECTED_WEIGHT), (label, es)
    if family == "uniform":
        em = ff.attention_error(o[:live], c["v"][:live].double().mean(1, keepdim=True).expand(-1, L, -1), c["v"][:live], ff.FNH)
        assert em <= bar, (label, em)
    if S == 1:
        assert torch.equal(o[:live], c["v"][:live].expand(-1, L, -1))
    return e


@pytest.mark.parametrize("family", ff.FINE_FAMILIES)
@pytest.mark.parametrize("L,S", ff.FINE_SHAPES)
def test_fine_full_attention(dev, family, L, S):
    K = ff.FINE_K
    c, ref = ff.attention_case(family, K, L, S, ff.FNH, ff.FDH), ff.attention_reference(family, K, L, S, ff.FNH, ff.FDH)
    for count in (None, 0, K - 1):
        o = run_fine_attention(dev, "ophip_fine_full_attention", c, count)
        e = check_fine_attention(o, family, c, ref, K if count is None else count, f"fine attention {family} L={L} S={S} count={count}")
        print(f"fine attention {family} L={L} S={S} count={count}: {e:.3e} (bar {ff.FINE_ATTENTION_BAR[family]:.2e})")


@pytest.mark.parametrize("family", ff.FINE_FAMILIES)
@pytest.mark.parametrize("L,S", ff.FINE2_SHAPES)
def test_fine2_full_attention(dev, family, L, S):
    K = ff.FINE_K
    c, ref = ff.attention_case(family, K, L, S, ff.FNH, ff.FDH), ff.attention_reference(family, K, L, S, ff.FNH, ff.FDH)
    o = run_fine_attention(dev, "ophip_fine2_full_attention", c, None)
    e = check_fine_attention(o, family, c, ref, K, f"window attention {family} L={L} S={S}")
    print(f"window attention {family} L={L} S={S}: {e:.3e} (bar {ff.FINE_ATTENTION_BAR[family]:.2e})")


# ------------------------------------------------------------------------------------------------
# matching
# ------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("scaled", [False, True])
@pytest.mark.parametrize("family", ff.MATCH_FAMILIES)
@pytest.mark.parametrize("W", ff.MATCH_WS)
def test_fine_full_match(dev, W, family, scaled):
    """``scaled``: ``query_scale`` given, with distinct h and w factors per batch element (the ``[1, 0]`` swap shows); else NULL.  The buffers hold
    two matches more than the count: their rows keep the NaN fill."""
    c = ff.match_case(family, W)
    K, WW = len(c["f3"]), W * W
    cap = K + 2
    a = arena_for(dev, cap * CF * 4, cap * WW * CF * 4, cap * 8, cap * 8, 16, 16, cap * 12, cap * 8)
    f3, win = a.typed((cap, CF), torch.float32, name="feat3d"), a.typed((cap, WW, CF), torch.float32, name="windows")
    mkc, b_ids = a.typed((cap, 2), torch.float32, name="mkpts_c"), a.typed((cap,), torch.int64, name="b_ids")
    for dst, src in ((f3, c["f3"]), (win, c["win"]), (mkc, c["mkc"]), (b_ids, c["b_ids"])):
        dst[:K].copy_(src)
    qs = a.put(c["qscale"], name="query_scale") if scaled else None
    count = a.put(torch.tensor([K, 0, 0, 0], dtype=torch.int32), name="count")
    expec, mkf = a.typed((cap, 3), torch.float32, name="expec_f"), a.typed((cap, 2), torch.float32, name="mkpts_f")
    hip.launch("ophip_fine_full_match", dict(feat3d=f3, windows=win, mkpts_c=mkc, b_ids=b_ids, query_scale=qs, count=count, cap=cap, W=W,
                                             scale=ff.MATCH_SCALE, expec_f=expec, mkpts_f=mkf))
    torch.cuda.synchronize()
    assert is_nan_fill(expec[K:]) and is_nan_fill(mkf[K:]), "rows at or past the count were written"
    e, m = expec[:K].cpu(), mkf[:K].cpu()
    assert not bool(torch.isnan(e).any()) and not bool(torch.isnan(m).any())
    a.check()
    ref_e, ref_m = ff.reference_match(c, W, scaled)
    got = ff.match_errors(e, m, ref_e, ref_m, c, W)
    bars = ff.MATCH_BAR[family]
    print(f"match {family} W={W} scaled={scaled}: coords {got[0]:.3e} std {got[1]:.3e} keypoints {got[2]:.3e} (bars {bars})")
    assert all(g <= b for g, b in zip(got, bars)), (got, bars)
    if family == "sharp":                               # the clamp acts on both axes: the std is 2 sqrt(1e-10)
        assert e[:, 2].min().item() >= 2e-5 * (1 - 1e-6)
    if family != "uniform":                             # the planted peak is where the expectation points
        step = 2.0 / (W - 1)
        for i, s in enumerate(c["spots"]):
            want = torch.tensor([-1 + step * (s % W), -1 + step * (s // W)])
            assert (e[i, :2] - want).abs().max().item() < (0.3 if family == "peak" else 1e-6), (i, s)
