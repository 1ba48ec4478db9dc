"""tests/full_faithful.py without a GPU: the reference against the oracle, the stand-in inside every bar and every bar within the two-to-four
factor of what the stand-in measures, seeded faults at least ten bars out, and the planted cases' constructions in float64."""
import math

import pytest
import torch

from tests import full_attention_oracle as foracle
from tests import full_faithful as ff

f32, f64 = torch.float32, torch.float64
P = ff.LAYER


# ---- 1. the reference is the oracle ------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("B,L,S", [(1, 1, 1), (2, 33, 31), (1, 129, 97)])
def test_reference_attention_is_the_oracle(B, L, S):
    c = ff.attention_case("soft", B, L, S)
    q, k, v = (c[n].to(f64).view(B, -1, 8, 32) for n in ("q", "k", "v"))
    want = foracle.full_attention(q, k, v).reshape(B, L, 256)
    assert (ff.reference_attention(c["q"], c["k"], c["v"]) - want).abs().max().item() <= 1e-12
    # and the plain formula, written out
    a = torch.softmax(torch.einsum("nlhd,nshd->nlsh", q, k) / math.sqrt(32.0), 2)
    assert (torch.einsum("nlsh,nshd->nlhd", a, v).reshape(B, L, 256) - want).abs().max().item() <= 1e-12


@pytest.mark.parametrize("shared", [False, True])
def test_reference_layer_is_the_oracle(sd, shared):
    x, src = ff.layer_inputs(2, 33, 31)
    if shared:
        src = src[:1]
    sd64 = {n: t.detach().double() for n, t in sd.items() if n.startswith(P)}
    with torch.no_grad():
        want = foracle.encoder_layer(sd64, P, x.double(), src.double().expand(2, -1, -1), 8)
    got = ff.reference_layer(sd, P, x, src)
    assert got.dtype == f64 and (got - want).abs().max().item() <= 1e-12
    # float64 of the f32 layer: the oracle in f32 is the same layer to f32 accuracy
    with torch.no_grad():
        assert ff.row_error(foracle.encoder_layer(sd, P, x, src.expand(2, -1, -1), 8), got) < 1e-4


# ---- 2. the stand-in sizes the bars --------------------------------------------------------------------------------------------------------
def standin_attention_worst(family):
    worst = (0.0, None)
    for B, L, S in ff.SHAPES:
        c = ff.attention_case(family, B, L, S)
        e = ff.attention_error(ff.standin_attention(c["q"], c["k"], c["v"]), ff.attention_reference(family, B, L, S), c["v"])
        assert e == e, (family, B, L, S)
        worst = max(worst, (e, (B, L, S)), key=lambda t: t[0])
    return worst


def layer_calls():
    """every ``(label, x, src)`` the layer bar is measured over: a two-stream call is two one-stream layers"""
    for L3, L2 in ff.LAYER_SHAPES:
        for B in (1, 2):
            x3, x2 = ff.layer_inputs(B, L3, L2)
            for cross in (0, 1):
                yield f"two-stream B={B} ({L3},{L2}) cross={cross} 3D", x3, (x2 if cross else x3)
                yield f"two-stream B={B} ({L3},{L2}) cross={cross} 2D", x2, (x3 if cross else x2)
    for L, S in ff.STREAM_SHAPES:
        for mode in ff.STREAM_MODES:
            yield (f"stream {mode} ({L},{S})",) + ff.stream_inputs(mode, L, S)


def standin_layer_worst(sd):
    worst = (0.0, None)
    for label, x, src in layer_calls():
        worst = max(worst, (ff.row_error(ff.standin_layer(sd, P, x, src), ff.reference_layer(sd, P, x, src)), label), key=lambda t: t[0])
    return worst


def standin_fine_worst(family):
    worst = (0.0, None)
    for L, S in ff.FINE_SHAPES + ff.FINE2_SHAPES:
        c = ff.attention_case(family, ff.FINE_K, L, S, ff.FNH, ff.FDH)
        e = ff.attention_error(ff.standin_fine_attention(c["q"], c["k"], c["v"]), ff.attention_reference(family, ff.FINE_K, L, S, ff.FNH, ff.FDH),
                               c["v"], ff.FNH)
        worst = max(worst, (e, (L, S)), key=lambda t: t[0])
    return worst


def standin_match_worst(family):
    worst = [0.0, 0.0, 0.0]
    for W in ff.MATCH_WS:
        c = ff.match_case(family, W)
        for scaled in (False, True):
            errs = ff.match_errors(*ff.standin_match(c, W, scaled), *ff.reference_match(c, W, scaled), c, W)
            worst = [max(a, b) for a, b in zip(worst, errs)]
    return worst


def _pinned(worst, bar, what):
    print(f"{what}: stand-in worst {worst:.3e}, bar {bar:.2e} = {bar / worst if worst else float('inf'):.2f} x")
    assert 2 * worst <= bar <= 4 * worst, (what, worst, bar)


@pytest.mark.parametrize("family", ff.FAMILIES)
def test_the_precision_bars_attention(family):
    worst, where = standin_attention_worst(family)
    _pinned(worst, ff.ATTENTION_BAR[family], f"attention {family} (worst at B, L, S = {where})")


def test_the_precision_bars_layer(sd):
    worst, where = standin_layer_worst(sd)
    _pinned(worst, ff.LAYER_BAR, f"layer rows (worst at {where})")


@pytest.mark.parametrize("family", ff.FINE_FAMILIES)
def test_the_precision_bars_fine_attention(family):
    worst, where = standin_fine_worst(family)
    _pinned(worst, ff.FINE_ATTENTION_BAR[family], f"fine attention {family} (worst at L, S = {where})")


@pytest.mark.parametrize("family", ff.MATCH_FAMILIES)
def test_the_precision_bars_match(family):
    worst = standin_match_worst(family)
    for w, bar, what in zip(worst, ff.MATCH_BAR[family], ("coords", "std", "keypoints")):
        if family == "sharp" and what != "keypoints":
            # by reasoning, not by measurement (see ff.MATCH_BAR): the stand-in must lie inside it
            print(f"match sharp {what}: stand-in worst {w:.3e}, bar {bar:.2e}")
            assert w <= bar
        else:
            _pinned(w, bar, f"match {family} {what}")


def test_the_cases_cover_the_edges():
    assert set(ff.SHAPES) >= {(1, L, S) for L in (1, 31, 32, 33, 127, 128, 129, 160) for S in (1, 31, 32, 33, 63, 64, 65, 97)}
    assert set(ff.SHAPES) >= {(3, L, S) for L in (1, 160) for S in (1, 97)} and len(ff.SHAPES) == 68
    assert set(ff.LAYER_SHAPES) == {(a, b) for a in (1, 31, 32, 33) for b in (1, 33)} | {(129, 65), (65, 129)}
    assert ff.STREAM_SHAPES == [(1, 1), (33, 31), (129, 65)] and ff.TOK == 32
    # the planted map sends the 32 queries of one wave to the three whole tiles, both k-steps and both 8-key groups of a k-step, and some query to
    # the one live key of the last tile
    pi = ff.planted_key(1, 32, 97)[0, :, 0]
    assert {int(s) // 32 for s in pi} >= {0, 1, 2} and {(int(s) % 32) // 16 for s in pi} == {0, 1} and {(int(s) % 16) // 8 for s in pi} == {0, 1}
    assert 96 in ff.planted_key(1, 160, 97)[0, :, 0].tolist()


# ---- 3. seeded faults ------------------------------------------------------------------------------------------------------------------------
# fault -> the named case (family, B, L, S) on which it must land at least ten bars out
FAULT_CASES = {"tail_unmasked": ("tail_bait", 1, 33, 33), "last_key_dropped": ("peaked_last", 1, 33, 65), "o_not_rescaled": ("growing", 1, 33, 97),
               "l_not_rescaled": ("growing", 1, 33, 97), "score_lohi_dropped": ("wide4", 1, 33, 97), "p_lo_dropped": ("soft", 1, 160, 33),
               "scale_16": ("soft", 1, 33, 33), "groups_swapped": ("planted", 1, 33, 97), "head_xor_1": ("soft", 1, 33, 33),
               "batch_0_keys": ("soft", 3, 160, 97)}
# a second named case where a fault's margin on the first is the smallest of the ten (P's lo plane: 23 and 26 bars; at (1, 33, 97) it is 12.5)
MORE_FAULT_CASES = {"p_lo_dropped": ("tail_bait", 1, 160, 33)}


@pytest.mark.parametrize("fault,case", [(f, FAULT_CASES[f]) for f in ff.FAULTS] + list(MORE_FAULT_CASES.items()))
def test_seeded_faults_lie_far_outside_the_bar(fault, case):
    family, B, L, S = case
    assert (B, L, S) in ff.SHAPES
    c = ff.attention_case(family, B, L, S)
    err = ff.attention_error(ff.standin_attention(c["q"], c["k"], c["v"], wrong=fault), ff.attention_reference(family, B, L, S), c["v"])
    print(f"{fault} on {family} B={B} L={L} S={S}: {err / ff.ATTENTION_BAR[family]:.3g} bars")
    assert err >= 10 * ff.ATTENTION_BAR[family], (fault, err)


def test_a_fault_in_the_attention_reaches_the_layer_rows(sd):
    x, src = ff.layer_inputs(1, 33, 33)
    err = ff.row_error(ff.standin_layer(sd, P, x, src, wrong="tail_unmasked"), ff.reference_layer(sd, P, x, src))
    print(f"tail_unmasked through the layer: {err / ff.LAYER_BAR:.3g} bars")
    assert err >= 10 * ff.LAYER_BAR


# ---- 4. the case generator -----------------------------------------------------------------------------------------------------------------------
def test_the_generator_is_deterministic():
    for family in ff.FAMILIES:
        a = ff.attention_case(family, 3, 160, 97)
        ff.attention_case.cache_clear()
        b = ff.attention_case(family, 3, 160, 97)
        assert a is not b and all(torch.equal(a[n], b[n]) for n in ("q", "k", "v")), family
    assert all(torch.equal(a, b) for a, b in zip(ff.layer_inputs(2, 33, 1), ff.layer_inputs(2, 33, 1)))
    assert torch.equal(ff.layer_inputs(1, 33, 1)[0], ff.layer_inputs(2, 33, 1)[0][:1])
    ff.match_case.cache_clear()
    a = ff.match_case("peak", 7)
    ff.match_case.cache_clear()
    assert torch.equal(a["win"], ff.match_case("peak", 7)["win"])


@pytest.mark.parametrize("family", ["planted", "peaked_last"])
def test_the_selected_key_owns_the_softmax(family):
    for B, L, S in ff.SHAPES:
        c = ff.attention_case(family, B, L, S)
        w = torch.softmax(ff.logits64(c), 2)                                                       # [B][L][S][H]
        own = torch.gather(w, 2, c["sel"][:, :, None, :]).min().item()
        assert own > ff.SELECTED_WEIGHT, (family, B, L, S, 1 - own)
        ref = ff.attention_reference(family, B, L, S)
        assert ff.attention_error(ff.selected_rows(c), ref, c["v"]) <= 2 * (1 - ff.SELECTED_WEIGHT)
        if family == "peaked_last":
            assert bool((c["sel"] == S - 1).all())
            if S > 1:                                                                              # the last value row differs from all the others
                v = c["v"].view(B, S, 256)
                assert (v[:, :-1] - v[:, -1:]).abs().amax(-1).min().item() > 1.0


def test_tail_bait_logits_lie_below_the_gap():
    for B, L, S in ff.SHAPES:
        t = ff.logits64(ff.attention_case("tail_bait", B, L, S))
        assert t.max().item() < -ff.TAIL_GAP, (B, L, S, t.max().item())


def test_fine_families_meet_their_constructions():
    for L, S in ff.FINE_SHAPES + ff.FINE2_SHAPES:
        c = ff.attention_case("peaked_last", ff.FINE_K, L, S, ff.FNH, ff.FDH)
        w = torch.softmax(ff.logits64(c, ff.FNH), 2)
        assert w[:, :, S - 1].min().item() > ff.SELECTED_WEIGHT, (L, S)
        u = ff.attention_case("uniform", ff.FINE_K, L, S, ff.FNH, ff.FDH)
        assert torch.equal(u["k"], u["k"][:, :1].expand(-1, S, -1))


def test_match_families_meet_their_constructions():
    for W in ff.MATCH_WS:
        for family, floor in (("peak", 3.0), ("sharp", 37.0)):
            c = ff.match_case(family, W)
            t = torch.einsum("mc,mrc->mr", c["f3"].double(), c["win"].double()) / math.sqrt(128.0)
            for m, s in enumerate(c["spots"]):
                others = torch.cat([t[m, :s], t[m, s + 1:]])
                assert (t[m, s] - others.max()).item() > floor, (family, W, m)
        ref, _ = ff.reference_match(ff.match_case("sharp", W), W, False)
        assert (ref[:, 2] - 2e-5).abs().max().item() < 1e-12                                       # the clamp acts on both axes
        uni, _ = ff.reference_match(ff.match_case("uniform", W), W, False)
        assert uni[:, :2].abs().max().item() < 1e-6 and uni[:, 2].min().item() > 1.0               # the largest std a window has
