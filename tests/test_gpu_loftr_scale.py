"""The LoFTR matcher's coarse path at working grid sizes on the MI355X (run with ``-m gpu``): 60 x 80 (a 480 x 640 frame), 64 x 64 (a 512²
crop), a ragged 61 x 79 against 59 x 83 and the detector's 64 x 64 view against a 180 x 240 frame (4096 x 43 200 elements, where the
two-pass form is the default).  The other LoFTR tests stay at or below 768 cells, where a row of the confidence matrix is one span of
``conf_kernel``, the similarity tiles are a handful and ``pad_limits_kernel`` never loops; the paths exercised here only run at size:

* dual softmax (``ophip_coarse_match_2d[_masked]``): one pass, two passes (``sim_frag_kernel<NS, 3>``) and the lazy form, against the
  float64 oracle: several spans per row merged by ``select_decide`` (exact ties across a span edge included), planted matches on tile
  edges, span edges, the all-sides border and each pair's padded border, per-pair masks (one with a one-row valid band, whose
  ``h - border_rm`` slice start is negative);
* Sinkhorn (``ophip_coarse_match_2d_sinkhorn[_masked]``) over 32 to 38 row chunks;
* the coarse encoder layer with and without masks at thousands of tokens per stream;
* the whole matcher on planted features, one pair and three padded views against one query.

The float64 references run the oracles' own torch expressions on the device where the matrices are large.  Bars: those of the
neighbouring files (conf_matrix rtol 1e-3 / atol 1e-6 in split bf16, index lists exact outside a relative band of 1e-4 around the
threshold or a tie); the decisions set aside inside the band are printed and bounded per case."""
import copy

import pytest
import torch

from onepose_st_amd import hip, layercall, loftr, matchcall, packing
from onepose_st_amd.synthetic import make_synthetic_loftr_state_dict
from tests import loftr_masked_oracle as lmo
from tests import test_gpu_loftr_masked as tglm
from tests import test_gpu_loftr_sinkhorn as tgls
from tests.loftr_helpers import planted_grids

pytestmark = pytest.mark.gpu

THR, BD, TEMP = 0.2, 2, 0.1
BAND = 1e-4
MAX_SET_ASIDE = 4           # decisions inside the band per case (planted matches sit far from the threshold and from any tie)


@pytest.fixture(scope="module")
def dev():
    assert torch.cuda.is_available(), "these tests need the MI355X"
    hip.load()
    return torch.device("cuda:0")


@pytest.fixture(scope="module")
def lsd():
    sd = dict(make_synthetic_loftr_state_dict(0))
    sd["coarse_matching.bin_score"] = torch.tensor(1.0)
    return sd


@pytest.fixture(scope="module")
def matchers(lsd, dev):
    out = {}

    def get(match_type):
        if match_type not in out:
            cfg = copy.deepcopy(loftr.default_cfg)
            cfg["match_coarse"]["match_type"] = match_type
            m = loftr.LoFTR_for_OnePose_Plus(cfg).eval()
            sd = lsd if match_type == "sinkhorn" else {k: v for k, v in lsd.items() if k != "coarse_matching.bin_score"}
            m.load_state_dict(sd, strict=True)
            out[match_type] = m.to(dev)
        return out[match_type]
    return get


# ------------------------------------------------------------------------------------------------
# inputs
# ------------------------------------------------------------------------------------------------
def _masks(hw, specs):
    """[B, h, w] bool per pair: ("rect", h, w) = the top-left extent LoFTR pads to; ("row", y) = a one-row valid band (extent height 1
    < border_rm: mask_border_with_padding's slice start h - border_rm is negative and counts from the end of the padded grid)"""
    m = torch.zeros(len(specs), *hw, dtype=torch.bool)
    for b, s in enumerate(specs):
        if s[0] == "rect":
            m[b, :s[1], :s[2]] = True
        else:
            m[b, s[1], :] = True
    return m


def _limits(hw, spec):
    """(row limit, column limit): cells inside the border of mask_border_with_padding, as Python slices read them"""
    H, W = hw
    if spec is None:
        return H - BD, W - BD
    h, w = (spec[1], spec[2]) if spec[0] == "rect" else (1, W)
    start = lambda e, n: e - BD if e - BD >= 0 else max(0, n + e - BD)
    return start(h, H), start(w, W)


def _inside(hw, spec, mask, c):
    """cell c is valid and survives the border (so a planted match there is kept)"""
    y, x = divmod(c, hw[1])
    ly, lx = _limits(hw, spec)
    return BD <= y < ly and BD <= x < lx and (mask is None or bool(mask.flatten()[c]))


def _spanw(M):
    """conf_kernel's span width (csrc/coarse_match.hip conf_spanw, CONF_U = 1)"""
    ns = (M + 1023) // 1024
    return ((M + ns - 1) // ns + 3) // 4 * 4


def _edge_cells(hw, spec):
    """cells on the all-sides border and on both sides of the padded border of one grid"""
    H, W = hw
    ly, lx = _limits(hw, spec)
    out = []
    for y in (0, 1, 2, ly - 1, ly, min(ly + 1, H - 1), H - 2, H - 1):
        for x in (0, 1, 2, W // 2, lx - 1, lx, min(lx + 1, W - 1), W - 1):
            if 0 <= y < H and 0 <= x < W:
                out.append(y * W + x)
    if spec is not None and spec[0] == "row":
        out += [spec[1] * W + x for x in range(0, W, 3)]         # the band itself: matches that only the negative slice keeps
    return out


def _pick(L, special, n, g):
    special = list(dict.fromkeys(int(s) for s in special if 0 <= s < L))
    perm = torch.randperm(L, generator=g)
    rest = perm[~torch.isin(perm, torch.tensor(special, dtype=torch.long))][:max(0, n - len(special))]
    return torch.cat([torch.tensor(special, dtype=torch.long), rest])


def _planted(B, hw0, hw1, specs0=None, specs1=None, n=320, seed=0, amp=1.2, ties=True):
    """random rows (scaled by amp); per pair n planted matches (image-1 cell j carries image-0 cell i plus noise) including tile edges
    (matrix rows / columns 127 / 128, 255 / 256), span edges (1023 / 1024, 2047 / 2048 and conf_kernel's actual span edges) and the
    border cells of both grids; with `ties`, one row per pair whose best entry is an exact tie of two valid columns in one similarity tile
    on both sides of a span edge (the reference takes the first).  -> f0, f1 (CPU), [(b, i, j_first, j_second)] of the ties"""
    L0, L1 = hw0[0] * hw0[1], hw1[0] * hw1[1]
    g = torch.Generator().manual_seed(seed)
    f0, f1 = torch.randn(B, L0, 256, generator=g) * amp, torch.randn(B, L1, 256, generator=g) * amp
    m0 = None if specs0 is None else _masks(hw0, specs0)
    m1 = None if specs1 is None else _masks(hw1, specs1)
    sw = _spanw(L1)
    tile_edges = [127, 128, 255, 256, 1023, 1024, 2047, 2048]
    tie_list = []
    for b in range(B):
        s0 = None if specs0 is None else specs0[b]
        s1 = None if specs1 is None else specs1[b]
        ii = _pick(L0, tile_edges + _edge_cells(hw0, s0), n, g)
        jj = _pick(L1, tile_edges + [sw - 1, sw, 2 * sw - 1, 2 * sw] + _edge_cells(hw1, s1), n, g)
        k = min(len(ii), len(jj))
        ii, jj = ii[:k], jj[:k]
        f1[b, jj] = f0[b, ii] + 0.1 * amp * torch.randn(k, 256, generator=g)
        if ties:
            used, mb = set(jj.tolist()), None if m1 is None else m1[b]
            cand = lambda r: [c for c in r if c not in used and _inside(hw1, s1, mb, c)]
            for edge in range(sw, L1, sw):                         # the first span edge inside a tile with valid columns on both sides
                t0 = edge // 128 * 128
                ja, jb = cand(range(edge - 1, t0 - 1, -1)), cand(range(edge, min(t0 + 128, L1)))
                if ja and jb and t0 < edge:
                    break
            else:
                continue                                           # (a one-row band of image 1 may hold no such tile)
            it = [c for c in [*range(L0 // 2, L0), *range(L0 // 2)] if c not in set(ii.tolist()) and _inside(hw0, s0, None if m0 is None else m0[b], c)]
            row = f0[b, it[0]] + 0.1 * amp * torch.randn(256, generator=g)
            f1[b, ja[0]] = row
            f1[b, jb[0]] = row
            tie_list.append((b, it[0], ja[0], jb[0]))
    assert tie_list or not ties, "no room for a tie"
    return f0, f1, m0, m1, tie_list


# ------------------------------------------------------------------------------------------------
# calls and checks
# ------------------------------------------------------------------------------------------------
def _pts(L0, w0, dev):
    ii = torch.arange(L0)
    return torch.stack([(ii % w0).float() * 8, (ii // w0).float() * 8, torch.zeros(L0)], 1)[None].contiguous().to(dev)


def _outputs(B, L0, dev):
    cap = B * L0
    ids = [torch.full((cap,), -1, dtype=torch.int64, device=dev) for _ in range(4)]
    return (ids, torch.empty(cap, device=dev), torch.empty(cap, 3, device=dev), torch.empty(cap, 2, device=dev),
            torch.empty(cap, dtype=torch.bool, device=dev), torch.zeros(4, dtype=torch.int32, device=dev))


def _collect(conf, ids, mconf, mk0, mk1, cnt):
    K = int(cnt[0])
    assert torch.equal(ids[3][:K], ids[0][:K]) and bool((ids[0][K:] == -1).all())      # m_bids = b_ids, nothing past K
    return {"conf": conf, "K": K, "lazy_tie": int(cnt[1]), "b_ids": ids[0][:K].cpu(), "i_ids": ids[1][:K].cpu(), "j_ids": ids[2][:K].cpu(),
            "mconf": mconf[:K].cpu(), "mkpts0_c": mk0[:K, :2].cpu(), "mkpts1_c": mk1[:K].cpu()}


def _dual(dev, d0, d1, w0, w1, masks=None, nsplit=3, lazy=False):
    B, L0, L1 = d0.shape[0], d0.shape[1], d1.shape[1]
    conf = None if lazy else torch.full((B, L0, L1), float("nan"), device=dev)
    ws = torch.full((hip.load().ophip_coarse_workspace_floats(B, L0, L1),), float("nan"), device=dev)
    ids, mconf, mk0, mk1, gt, cnt = _outputs(B, L0, dev)
    matchcall.coarse_match_2d(d0, d1, _pts(L0, w0, dev), w0c=w0, w1c=w1, temperature=TEMP, thr=THR, border_rm=BD, scale=8.0, nsplit=nsplit,
                              masks=masks, lists=matchcall.MatchLists(*ids[:3], mconf, mk0, mk1, ids[3], gt, cnt), conf=conf, workspace=ws)
    out = _collect(conf, ids, mconf, mk0, mk1, cnt)
    if conf is not None:
        assert bool(torch.isfinite(conf).all()), "conf_matrix has entries no kernel wrote"
    return out


def _skh(dev, d0, d1, w0, w1, iters, prefilter, masks=None, bin_score=1.0):
    B, L0, L1 = d0.shape[0], d0.shape[1], d1.shape[1]
    conf = torch.full((B, L0, L1), float("nan"), device=dev)
    ws = torch.full((hip.load().ophip_coarse_sinkhorn_workspace_floats(B, L0, L1),), float("nan"), device=dev)
    ids, mconf, mk0, mk1, gt, cnt = _outputs(B, L0, dev)
    matchcall.coarse_match_2d(d0, d1, _pts(L0, w0, dev), w0c=w0, w1c=w1, sinkhorn=(bin_score, iters, prefilter), thr=THR, border_rm=BD, scale=8.0,
                              masks=masks, lists=matchcall.MatchLists(*ids[:3], mconf, mk0, mk1, ids[3], gt, cnt), conf=conf, workspace=ws)
    assert bool(torch.isfinite(conf).all()), "conf_matrix has entries no kernel wrote"
    return _collect(conf, ids, mconf, mk0, mk1, cnt)


def _close_dev(got, ref, rtol, atol, tag, keep=None, rows=256):
    """|got - ref| <= atol + rtol |ref| everywhere (or where `keep`), on the device in row blocks (the matrices reach 177 M entries)"""
    B, L0 = ref.shape[:2]
    worst, nbad = 0.0, 0
    for b in range(B):
        for r in range(0, L0, rows):
            g, w = got[b, r:r + rows].double(), ref[b, r:r + rows]
            err = (g - w).abs()
            bad = err > atol + rtol * w.abs()
            if keep is not None:
                bad &= keep[b, r:r + rows]
            nbad += int(bad.sum())
            worst = max(worst, float((err / (atol + rtol * w.abs())).max()))
    assert nbad == 0, f"{tag}: {nbad} entries outside rtol {rtol} / atol {atol} (worst at {worst:.3g} x the bar)"


def _dual_ref(dev, f0, f1, hw0, hw1, m0=None, m1=None):
    """the masked oracle (tests/loftr_masked_oracle.py) in float64 on the device"""
    f0d, f1d = f0.to(dev).double(), f1.to(dev).double()
    m0d, m1d = (None, None) if m0 is None else (m0.to(dev), m1.to(dev))
    conf = lmo.dual_softmax_conf(f0d, f1d, TEMP, m0d, m1d)
    ref = lmo.get_coarse_match(conf, hw0, hw1, (8 * hw0[0], 8 * hw0[1]), THR, BD, m0d, m1d)
    return {k: (v.cpu() if torch.is_tensor(v) and k != "conf_matrix" else v) for k, v in ref.items()}


def _near_dual(conf, b, i, j, band=BAND):
    """a decision within the band: conf within `band` (relative) of the threshold, or of the best other entry of its row or column"""
    c = float(conf[b, i, j])
    if abs(c - THR) <= band * THR:
        return True
    row, col = conf[b, i].clone(), conf[b, :, j].clone()
    row[j], col[i] = -1, -1
    return float(row.max()) >= c * (1 - band) or float(col.max()) >= c * (1 - band)


def _triples(d):
    return list(zip(d["b_ids"].tolist(), d["i_ids"].tolist(), d["j_ids"].tolist()))


def _against_ref(out, ref, tag, near, rtol=1e-3, atol=1e-6, conf=True):
    """index lists equal to the reference's outside the band (set-aside counted and bounded), mconf 1e-3, coarse keypoints exact"""
    have, want = _triples(out), _triples(ref)
    diff = sorted(set(have) ^ set(want))
    assert all(near(*d) for d in diff), f"{tag}: matches differ outside the band: {[d for d in diff if not near(*d)][:6]}"
    print(f"{tag}: K = {len(want)}, set aside {len(diff)}")
    assert len(diff) <= MAX_SET_ASIDE, f"{tag}: {len(diff)} decisions inside the band"
    if conf:
        _close_dev(out["conf"], ref["conf_matrix"], rtol, atol, f"{tag}: conf_matrix")
    ws, rk = set(want), {t: k for k, t in enumerate(want)}
    ci = torch.tensor([k for k, t in enumerate(have) if t in ws], dtype=torch.long)
    ri = torch.tensor([rk[have[k]] for k in ci.tolist()], dtype=torch.long)
    torch.testing.assert_close(out["mconf"][ci].double(), ref["mconf"][ri].double(), rtol=max(rtol, 1e-4), atol=1e-6, msg=f"{tag}: mconf")
    assert torch.equal(out["mkpts0_c"][ci], ref["mkpts0_c"][ri]) and torch.equal(out["mkpts1_c"][ci], ref["mkpts1_c"][ri]), f"{tag}: keypoints"
    return len(want), len(diff)


def _padding_zero(conf, m0, m1, tag):
    """masked_fill then dual softmax: an entry where a valid cell meets a padded one is exactly 0"""
    v0, v1 = m0.flatten(1).to(conf.device), m1.flatten(1).to(conf.device)
    for b in range(conf.shape[0]):
        one = v0[b][:, None] ^ v1[b][None, :]
        assert not bool((conf[b][one] != 0).any()), f"{tag}: pair {b}: a valid cell against a padded one is not exactly 0"


# ------------------------------------------------------------------------------------------------
# A. dual-softmax coarse stage at working sizes
# ------------------------------------------------------------------------------------------------
GRIDS = {
    "60x80-60x80-B1": (1, (60, 80), (60, 80), [("rect", 57, 75)], [("rect", 52, 80)]),
    "64x64-60x80-B3": (3, (64, 64), (60, 80), [("rect", 64, 64), ("rect", 60, 61), ("row", 30)], [("rect", 60, 80), ("rect", 55, 70), ("rect", 58, 79)]),
    "61x79-59x83-B2": (2, (61, 79), (59, 83), [("rect", 58, 79), ("rect", 61, 70)], [("rect", 59, 81), ("row", 40)]),
}
_CACHE = {}


def _case(dev, name, masked):
    key = (name, masked)
    if key not in _CACHE:
        _CACHE.clear()                               # one case's float64 matrices at a time
        B, hw0, hw1, s0, s1 = GRIDS[name]
        f0, f1, m0, m1, ties = _planted(B, hw0, hw1, s0 if masked else None, s1 if masked else None, seed=len(name) + B)
        ref = _dual_ref(dev, f0, f1, hw0, hw1, m0, m1)
        _CACHE[key] = (f0.to(dev), f1.to(dev), m0, m1, ties, ref)
    return _CACHE[key]


@pytest.mark.parametrize("masked,nsplit", [(False, 3), (False, 1), (False, 0), (True, 3)])
@pytest.mark.parametrize("name", list(GRIDS))
def test_dual_softmax_stage_at_size(dev, monkeypatch, name, masked, nsplit):
    B, hw0, hw1, _, _ = GRIDS[name]
    d0, d1, m0, m1, ties, ref = _case(dev, name, masked)
    masks = None if m0 is None else (m0.flatten(1).to(dev), m1.flatten(1).to(dev))
    forms = {}
    if nsplit == 0:
        forms["one pass"] = _dual(dev, d0, d1, hw0[1], hw1[1], masks, nsplit)
    else:
        for form, two in (("one pass", "0"), ("two passes", "1")):
            monkeypatch.setenv("OPHIP_COARSE_TWO_PASS", two)
            forms[form] = _dual(dev, d0, d1, hw0[1], hw1[1], masks, nsplit)
        forms["lazy"] = _dual(dev, d0, d1, hw0[1], hw1[1], masks, nsplit, lazy=True)
    base = forms["one pass"]
    for form, out in forms.items():
        assert out["lazy_tie"] == 0, f"{form}: count[1] set without an unresolvable tie"
        for k in ("b_ids", "i_ids", "j_ids", "mkpts0_c", "mkpts1_c"):
            assert torch.equal(out[k], base[k]), f"{form} against one pass: {k}"
    if "two passes" in forms:
        two = forms["two passes"]
        assert torch.equal(two["conf"], base["conf"]), "conf_matrix of the two eager forms"
        assert torch.equal(two["mconf"], base["mconf"]), "mconf of the two eager forms"
    # bf16 (nsplit 1) rounds the features: conf within the bar of tests/test_gpu_parity.py, decisions within a band that wide
    rtol, band = {0: (1e-4, BAND), 1: (0.5, 5e-2), 3: (1e-3, BAND)}[nsplit]
    conf64 = ref["conf_matrix"]
    K, _ = _against_ref(base, ref, f"{name} masked={masked} nsplit={nsplit}", lambda b, i, j: _near_dual(conf64, b, i, j, band), rtol=rtol)
    assert K >= 100 * B // 2, "the planted matches must survive: the comparison would be vacuous"
    got = set(_triples(base))
    for b, i, ja, jb in ties:                        # exact tie across a span edge: the first valid column wins
        assert float(conf64[b, i, ja]) == float(conf64[b, i, jb])
        assert (b, i, ja) in got and (b, i, jb) not in got, f"tie in row {i} of pair {b}: {ja} (first) against {jb}"
    if masked:
        _padding_zero(base["conf"], m0, m1, name)
        assert set(b for b, _, _ in got) == set(range(B))
        for b in range(B):                           # the band pairs keep their matches (the negative slice start)
            if GRIDS[name][3][b][0] == "row":
                assert any(bb == b for bb, _, _ in got), f"pair {b}: no match in the one-row band"
        assert torch.equal(masks[0].cpu(), m0.flatten(1)) and torch.equal(masks[1].cpu(), m1.flatten(1))       # masks read only


@pytest.mark.parametrize("masked", [False, True])
def test_exact_tie_the_lazy_form_cannot_resolve(dev, monkeypatch, masked):
    """the row maximum tied between a column on the border (first, span 0) and a valid one (span 1) in one similarity tile: the eager
    forms walk the stored row and take the later, valid column; the lazy form never stored it and raises count[1]"""
    hw = (60, 80)
    L = hw[0] * hw[1]
    spec = [("rect", 57, 76)]
    f0, f1, m0, m1, _ = _planted(1, hw, hw, spec if masked else None, spec if masked else None, n=200, seed=21, ties=False)
    sw = _spanw(L)
    _, lx = _limits(hw, spec[0] if masked else None)
    ja = next(c for c in range(sw - 1, sw // 128 * 128, -1) if c % hw[1] >= lx and c % hw[1] < (76 if masked else hw[1]))
    jb = next(c for c in range(sw, sw // 128 * 128 + 128) if _inside(hw, spec[0] if masked else None, None, c))
    i = 30 * hw[1] + 40
    g = torch.Generator().manual_seed(5)
    f0[0, i] = 1.2 * torch.randn(256, generator=g)                # a fresh row: no planted copy of it elsewhere
    row = f0[0, i] + 0.12 * torch.randn(256, generator=g)
    f1[0, ja] = row
    f1[0, jb] = row
    ref = _dual_ref(dev, f0, f1, hw, hw, m0, m1)
    assert float(ref["conf_matrix"][0, i, ja]) == float(ref["conf_matrix"][0, i, jb]) > THR
    assert (0, i, jb) in set(_triples(ref))
    d0, d1 = f0.to(dev), f1.to(dev)
    masks = None if m0 is None else (m0.flatten(1).to(dev), m1.flatten(1).to(dev))
    for two in ("0", "1"):
        monkeypatch.setenv("OPHIP_COARSE_TWO_PASS", two)
        out = _dual(dev, d0, d1, hw[1], hw[1], masks)
        assert out["conf"][0, i, ja] == out["conf"][0, i, jb]
        assert out["lazy_tie"] == 0
        assert (0, i, jb) in set(_triples(out)), f"two passes={two}: the tie must resolve to the valid column {jb}"
        _against_ref(out, ref, f"tie, masked={masked}, two passes={two}", lambda b, ii, jj: _near_dual(ref["conf_matrix"], b, ii, jj))
    lazy = _dual(dev, d0, d1, hw[1], hw[1], masks, lazy=True)
    assert lazy["lazy_tie"] == 1, "the lazy form must flag the tie it cannot resolve"


# ------------------------------------------------------------------------------------------------
# B. the size where two passes become the default
# ------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("masked", [False, True])
def test_two_pass_default_at_the_detector_size(dev, monkeypatch, masked):
    """a 512² view (64 x 64) against a 1920 x 1440 frame (180 x 240): 4096 x 43 200 = 177 M elements >= 2^27, two passes by default"""
    hw0, hw1 = (64, 64), (180, 240)
    s0, s1 = [("rect", 60, 62)], [("rect", 171, 233)]
    f0, f1, m0, m1, ties = _planted(1, hw0, hw1, s0 if masked else None, s1 if masked else None, n=400, seed=7, amp=1.3)
    ref = _dual_ref(dev, f0, f1, hw0, hw1, m0, m1)
    d0, d1 = f0.to(dev), f1.to(dev)
    masks = None if m0 is None else (m0.flatten(1).to(dev), m1.flatten(1).to(dev))
    monkeypatch.delenv("OPHIP_COARSE_TWO_PASS", raising=False)
    monkeypatch.delenv("OPHIP_COARSE_TWO_PASS_MIN", raising=False)
    dflt = _dual(dev, d0, d1, hw0[1], hw1[1], masks)
    monkeypatch.setenv("OPHIP_COARSE_TWO_PASS", "0")
    one = _dual(dev, d0, d1, hw0[1], hw1[1], masks)
    for k in ("b_ids", "i_ids", "j_ids", "mconf", "mkpts0_c", "mkpts1_c"):
        assert torch.equal(dflt[k], one[k]), k
    assert torch.equal(dflt["conf"], one["conf"]), "conf_matrix of the default (two-pass) and the one-pass form"
    del one
    K, _ = _against_ref(dflt, ref, f"64x64-180x240 masked={masked}", lambda b, i, j: _near_dual(ref["conf_matrix"], b, i, j))
    assert K >= 200
    got = set(_triples(dflt))
    for b, i, ja, jb in ties:
        assert (b, i, ja) in got and (b, i, jb) not in got
    if masked:
        _padding_zero(dflt["conf"], m0, m1, "64x64-180x240")


# ------------------------------------------------------------------------------------------------
# C. Sinkhorn at size
# ------------------------------------------------------------------------------------------------
SKH_GRIDS = {
    "60x80-60x80-B1": (1, (60, 80), (60, 80), [("rect", 56, 77)], [("rect", 60, 74)]),
    "64x64-60x80-B3": (3, (64, 64), (60, 80), [("rect", 62, 64), ("row", 20), ("rect", 50, 57)], [("rect", 60, 80), ("rect", 59, 72), ("rect", 53, 80)]),
}


@pytest.mark.parametrize("masked", [False, True])
@pytest.mark.parametrize("iters", [0, 3, 10])
@pytest.mark.parametrize("name", list(SKH_GRIDS))
def test_sinkhorn_stage_at_size(dev, name, iters, masked):
    B, hw0, hw1, s0, s1 = SKH_GRIDS[name]
    f0, f1, m0, m1, _ = _planted(B, hw0, hw1, s0 if masked else None, s1 if masked else None, n=320, seed=iters + B, amp=4.0, ties=False)
    d0, d1 = f0.to(dev), f1.to(dev)
    f0d, f1d = d0.double(), d1.double()
    m0d, m1d = (None, None) if m0 is None else (m0.to(dev), m1.to(dev))
    masks = None if m0 is None else (m0.flatten(1).to(dev), m1.flatten(1).to(dev))
    for prefilter in (0, 1):
        tag = f"{name} iters={iters} prefilter={prefilter} masked={masked}"
        out = _skh(dev, d0, d1, hw0[1], hw1[1], iters, prefilter, masks)
        K = _check_sinkhorn(out, f0d, f1d, hw0, hw1, iters, prefilter, m0d, m1d, tag)
        assert K >= 50 * B, "the planted matches must survive: the comparison would be vacuous"
    if masked:
        assert torch.equal(masks[0].cpu(), m0.flatten(1)) and torch.equal(masks[1].cpu(), m1.flatten(1))


def _check_sinkhorn(out, f0d, f1d, hw0, hw1, iters, prefilter, m0d, m1d, tag, bin_score=1.0):
    """one Sinkhorn stage result (``_skh``'s dict) against the float64 oracle on the device (features float64, masks or None);
    -> the reference's match count"""
    conf64, assign = lmo.sinkhorn_conf(f0d, f1d, bin_score, iters, prefilter, m0d, m1d)
    ref = lmo.get_coarse_match(conf64, hw0, hw1, (8 * hw0[0], 8 * hw0[1]), THR, BD, m0d, m1d)
    ref = {k: (v.cpu() if torch.is_tensor(v) and k != "conf_matrix" else v) for k, v in ref.items()}
    near_r, near_c = tgls._near(assign, conf64, THR)
    keep = ~(near_r[:, :, None] | near_c[:, None, :])
    _close_dev(out["conf"], conf64, 1e-3 if iters == 0 else 0.0, 1e-4, f"{tag}: conf_matrix", keep=keep)
    nr, nc = near_r.cpu(), near_c.cpu()
    K, _ = _against_ref(out, ref, tag, lambda b, i, j: bool(nr[b, i] or nc[b, j]), rtol=1e-3 if iters == 0 else 1e-4, conf=False)
    return K


# ------------------------------------------------------------------------------------------------
# D. the coarse encoder layer at size
# ------------------------------------------------------------------------------------------------
ENC = {
    "4096-4800-B3": (3, (64, 64), (60, 80), [(64, 64), (60, 61), (47, 64)], [(60, 80), (55, 70), (58, 33)]),
    "4096-43200-B1": (1, (64, 64), (180, 240), [(60, 62)], [(171, 233)]),
}


@pytest.mark.parametrize("name", list(ENC))
def test_encoder_layer_at_size(lsd, dev, name):
    """self, both cross directions and one NULL mask through the two-mask entries, then the unmasked entries, against masked_layer in
    float64 on the device"""
    B, hw0, hw1, e0, e1 = ENC[name]
    L0, L1 = hw0[0] * hw0[1], hw1[0] * hw1[1]
    g = torch.Generator().manual_seed(L1 + B)
    x0, x1 = torch.randn(B, L0, 256, generator=g), torch.randn(B, L1, 256, generator=g)
    m0, m1 = tglm.rect_masks(B, hw0, e0).flatten(1), tglm.rect_masks(B, hw1, e1).flatten(1)
    p = "loftr_coarse.layers.3."
    sd = {k: v.to(dev).double() for k, v in lsd.items() if k.startswith(p)}
    w = packing.pack_coarse_layer_x3w8(lsd, p).to(dev)
    d0, d1, dm0, dm1 = x0.to(dev), x1.to(dev), m0.to(dev), m1.to(dev)
    r0, r1, rm0, rm1 = d0.double(), d1.double(), dm0, dm1
    kw = dict(mode="bf16x3", wpack=w, workspace=layercall.workspace("bf16x3", B, L0, L1, dev))
    layer = lambda x, s, mx=None, ms=None: lmo.masked_layer(sd, p, x, s, mx, ms)
    check = lambda got, want, what: _close_dev(got, want, 3e-4, 1e-4, f"{name}: {what}")
    # masked self
    y0, y1 = torch.full_like(d0, float("nan")), torch.full_like(d1, float("nan"))
    layercall.layer(d0, d1, y0, y1, is_cross=0, masks=(dm0, dm1), **kw)
    check(y0, layer(r0, r0, rm0, rm0), "masked self, stream 0")
    check(y1, layer(r1, r1, rm1, rm1), "masked self, stream 1")
    # masked cross, one direction per launch, then mask0 NULL
    n0, n1 = torch.full_like(d0, float("nan")), torch.full_like(d1, float("nan"))
    layercall.layer(d0, d1, n0, None, is_cross=1, streams=1, masks=(dm0, dm1), **kw)
    check(n0, layer(r0, r1, rm0, rm1), "masked cross, image 0 against image 1")
    layercall.layer(d0, d1, None, n1, is_cross=1, streams=2, masks=(dm0, dm1), **kw)
    check(n1, layer(r1, r0, rm1, rm0), "masked cross, image 1 against image 0")
    n0.fill_(float("nan"))
    layercall.layer(d0, d1, n0, None, is_cross=1, streams=1, masks=(None, dm1), **kw)
    check(n0, layer(r0, r1, None, rm1), "masked cross, mask0 NULL")
    assert torch.equal(dm0.cpu(), m0) and torch.equal(dm1.cpu(), m1)                # the masks are read only
    # the unmasked entries
    y0.fill_(float("nan"))
    y1.fill_(float("nan"))
    layercall.layer(d0, d1, y0, y1, is_cross=0, **kw)
    check(y0, layer(r0, r0), "self, stream 0")
    check(y1, layer(r1, r1), "self, stream 1")
    n0.fill_(float("nan"))
    n1.fill_(float("nan"))
    layercall.layer(d0, d1, n0, None, is_cross=1, streams=1, **kw)
    check(n0, layer(r0, r1), "cross, image 0 against image 1")
    layercall.layer(d0, d1, None, n1, is_cross=1, streams=2, **kw)
    check(n1, layer(r1, r0), "cross, image 1 against image 0")


# ------------------------------------------------------------------------------------------------
# E. the whole matcher at working size
# ------------------------------------------------------------------------------------------------
def _double(t):
    return t.double() if torch.is_tensor(t) and t.is_floating_point() else t


@pytest.mark.parametrize("match_type", ["dual_softmax", "sinkhorn"])
def test_matcher_one_480x640_pair(matchers, lsd, dev, match_type):
    m = matchers(match_type)
    amp = 1.0 if match_type == "dual_softmax" else 6.0
    x0, g0, x1, g1 = planted_grids((60, 80), (60, 80), seed=41)
    feats = (x0 * amp, g0, x1 * amp, g1)
    with torch.no_grad():
        ref = lmo.forward_from_features({k: _double(v) for k, v in lsd.items()}, m.config, *[t.double() for t in feats], (480, 640))
    data = tglm._run(m, dev, feats, (60, 80), (60, 80), None)
    K, _ = tglm._check(data, ref, f"{match_type}, 480 x 640")
    assert K >= 1000


def _views_against_a_query(seed=43, amp=1.0):
    """three 512 x 512 views (64 x 64 cells) with valid extents of their own against one 480 x 640 query (60 x 80): view k carries query
    cell (y + dy, x + dx) at its valid cell (y, x); padded cells hold random rows and zero fine maps"""
    hw0p, hw1 = (64, 64), (60, 80)
    views, shifts = ((60, 64), (56, 60), (50, 62)), ((2, 1), (1, 1), (0, 2))
    g = torch.Generator().manual_seed(seed)
    q = torch.randn(1, hw1[0] * hw1[1], 256, generator=g)
    gq = torch.randn(1, 128, 4 * hw1[0], 4 * hw1[1], generator=g)
    V = len(views)
    x0 = torch.randn(V, hw0p[0] * hw0p[1], 256, generator=g) * 2
    g0 = torch.zeros(V, 128, 4 * hw0p[0], 4 * hw0p[1])
    for k, ((h, w), (dx, dy)) in enumerate(zip(views, shifts)):
        y, x = torch.meshgrid(torch.arange(h), torch.arange(w), indexing="ij")
        y, x = y.flatten(), x.flatten()
        hit = (y + dy < hw1[0]) & (x + dx < hw1[1])
        cells = y * hw0p[1] + x
        x0[k, cells] = torch.randn(len(cells), 256, generator=g)
        x0[k, cells[hit]] = q[0, ((y + dy) * hw1[1] + x + dx)[hit]] + 0.1 * torch.randn(int(hit.sum()), 256, generator=g)
        g0[k, :, :4 * h, :4 * w] = torch.roll(gq[0], shifts=(-4 * dy, -4 * dx), dims=(1, 2))[:, :4 * h, :4 * w]
    masks = (tglm.rect_masks(V, hw0p, views), torch.ones(1, *hw1, dtype=torch.bool))
    return (x0 * amp, g0, q * amp, gq), hw0p, hw1, masks


@pytest.mark.parametrize("match_type", ["dual_softmax", "sinkhorn"])
def test_matcher_three_padded_views_against_one_query(matchers, lsd, dev, match_type):
    m = matchers(match_type)
    feats, hw0p, hw1, masks = _views_against_a_query(amp=1.0 if match_type == "dual_softmax" else 6.0)
    with torch.no_grad():
        ref = lmo.forward_from_features({k: _double(v) for k, v in lsd.items()}, m.config, *[t.double() for t in feats],
                                        (8 * hw0p[0], 8 * hw0p[1]), *masks)
    data = tglm._run(m, dev, feats, hw0p, hw1, masks, V=3, V1=1)
    K, _ = tglm._check(data, ref, f"{match_type}, three 512 x 512 views against a 480 x 640 query")
    assert K >= 1000 and set(data["b_ids"].tolist()) == {0, 1, 2}
    for k in range(3):                               # the batched call against one call per view
        one_feats = (feats[0][k:k + 1], feats[1][k:k + 1], feats[2], feats[3])
        one = tglm._run(m, dev, one_feats, hw0p, hw1, (masks[0][k:k + 1], masks[1]))
        sel = data["b_ids"] == k
        assert torch.equal(data["i_ids"][sel], one["i_ids"]) and torch.equal(data["j_ids"][sel], one["j_ids"]), k
        assert torch.equal(data["mkpts1_f"][sel], one["mkpts1_f"]), k
