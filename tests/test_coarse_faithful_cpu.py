"""tests/coarse_faithful.py checked on the CPU: the float64 restatement agrees with the oracle, every case of
tests/test_gpu_coarse_stage.py is decidable from the reference alone, an f32 stand-in of each mode meets that file's bars and reproduces
every list, four deliberately wrong variants do not, and the tie cases select what their docstring says."""
import functools

import numpy as np
import pytest
import torch

from oracle import onepose_oracle as orc
from tests import coarse_faithful as cf
from tests.bf16_faithful import bf16_round

CASES = sorted(cf.ALL_CASES)
TIES = [(p, v) for p in cf.TIE_PLACEMENTS for v in cf.TIE_VARIANTS]


@functools.lru_cache(maxsize=None)
def built(name):
    return cf.build(cf.ALL_CASES[name])


@functools.lru_cache(maxsize=None)
def ref(name, nsplit):
    """(float64 confidences, lists) of one table case: computed once, never changed"""
    return cf.reference(built(name), nsplit)


def test_the_bars_are_the_projects_own():
    from tests import test_gpu_parity as par
    assert cf.BAR[0] == dict(rtol=par.COARSE_RTOL[0], atol=1e-7) and cf.BAR[3] == dict(rtol=par.COARSE_RTOL[3], atol=1e-7)
    assert cf.BAR[1] == par.PLAIN_BF16_LIKE_FOR_LIKE_TOL and par.plain_bf16_confidence is cf.plain_bf16_confidence
    assert all(cf.MARGIN[ns] == 10 * cf.BAR[ns]["rtol"] for ns in cf.NSPLITS)
    assert all(cf.GPU_BAR[ns]["rtol"] <= cf.BAR[ns]["rtol"] and cf.GPU_BAR[ns]["atol"] == cf.BAR[ns]["atol"] for ns in cf.NSPLITS)      # tightened, never loosened


def test_exact_mode_agrees_with_the_oracle_in_float64():
    """temperature + 1e-4 = 0.125 is an f32 value, so the kernel's f32 temperature and the oracle's double are the same number"""
    g = torch.Generator().manual_seed(1)
    f3, f2 = torch.randn(2, 70, 256, generator=g).double() * 1.5, torch.randn(2, 45, 256, generator=g).double()
    mask = torch.rand(2, 45, generator=g) > 0.3
    for m in (None, mask):
        got, want = cf.confidence(f3, f2, 0.125 - 1e-4, 0, query_mask=m), orc.dual_softmax_confidence(f3, f2, 0.125 - 1e-4, mask_query=m)
        assert got.dtype == torch.float64 and float((got - want).abs().max()) < 1e-12
        assert float(((got - want).abs() / want)[want > 1e-200].max()) < 1e-12
    assert float(got.transpose(1, 2)[~mask].max()) == 0.0


def test_plain_bf16_is_the_formula_it_replaced():
    f3, f2 = cf.soft_case(1, 60, 5, 7, 3)
    inv_temp = float(np.float32(1.0) / np.float32(0.08 + 1e-4))
    sim = torch.einsum("nlc,nsc->nls", bf16_round(f3 * 0.0625).double(), bf16_round(f2 * 0.0625).double()) * inv_temp
    assert torch.equal(cf.plain_bf16_confidence(f3, f2), torch.softmax(sim, 1) * torch.softmax(sim, 2))


def test_split_mode_has_no_lo_lo_term_and_lies_between_the_other_two():
    f3, f2 = cf.soft_case(1, 60, 5, 7, 3)
    s0, s3, s1 = (cf.logits(f3, f2, 0.08, ns) for ns in (0, 3, 1))
    lo3, lo2 = cf._planes(f3, 3, torch.float64)[1], cf._planes(f2, 3, torch.float64)[1]
    lolo = torch.einsum("nlc,nsc->nls", lo3, lo2) * float(np.float32(1.0) / np.float32(0.08 + 1e-4))
    assert float((s3 - s0).abs().max()) < 2e-4 < 5e-3 < float((s1 - s0).abs().max())
    assert float((s3 + lolo - s0).abs().max()) < float((s3 - s0).abs().max())          # adding lo.lo back moves it towards the exact product


def test_the_gpu_file_runs_exactly_these_cases():
    from tests import test_gpu_coarse_stage as gpu
    assert sorted(gpu.SOFT) == sorted(cf.SOFT_CASES) and sorted(gpu.MASKED) == sorted(cf.MASK_CASES)
    assert sorted(gpu.TIES) == sorted(TIES)
    assert set(cf.SOFT_CASES[k]["shape"] for k in cf.SOFT_CASES) >= {(1, 1, 1, 1), (1, 127, 1, 129), (2, 257, 3, 43), (1, 256, 16, 16), (1, 1152, 8, 16),
                                                                      (1, 130, 25, 41), (1, 97, 54, 76), (33, 2000, 8, 8)}
    assert {c["thr"] for c in cf.SOFT_CASES.values()} == {0.05, 0.2, 0.5} and {c["border"] for c in cf.SOFT_CASES.values()} >= {0, 1, 2}


@pytest.mark.parametrize("nsplit", cf.NSPLITS)
@pytest.mark.parametrize("name", CASES)
def test_every_case_is_decidable(name, nsplit):
    """all three margins of the reference reach 10 x the mode's rtol; the soft inputs are soft (confidences in every band, a row that
    loses the mutual test wherever the threshold allows one)"""
    case, c = cf.ALL_CASES[name], built(name)
    conf, sel = ref(name, nsplit)
    m, good = cf.decidable(c, nsplit, conf)
    print(f"{name} nsplit {nsplit}: margins thr {m[0]:.3g} row {m[1]:.3g} col {m[2]:.3g}, {len(sel['i_ids'])} matches, "
          f"{cf.nonmutual_rows(conf, c['thr'])} non-mutual rows, |sim| max {float(cf.logits(c['f3'], c['f2'], 0.08, nsplit).abs().max()):.1f}")
    assert good, m
    assert case.get("nonmutual", True) == (c["thr"] < 0.5 and conf[0].numel() > 1 and c["border"] < min(c["hc"], c["wc"]))
    if case.get("nonmutual", True):
        assert cf.nonmutual_rows(conf, c["thr"]) >= 1
        for lo, hi in ((0.05, 0.2), (0.2, 0.5), (0.5, 0.9)):
            assert int(((conf > lo) & (conf <= hi)).sum()) >= 3, (lo, hi)
    if name == "b33":
        assert len(sel["i_ids"]) > 1000 and len(set(sel["b_ids"].tolist())) == 33
    if name == "border_takes_all":
        assert len(sel["i_ids"]) == 0 and int((conf > c["thr"]).sum()) > 10


@pytest.mark.parametrize("nsplit", cf.NSPLITS)
@pytest.mark.parametrize("name", CASES)
def test_the_bars_are_reachable(name, nsplit):
    """the same rounding points with f32 sums and an f32 softmax: inside the bars, every list reproduced"""
    c = built(name)
    conf32 = cf.confidence(c["f3"], c["f2"], cf.TEMPERATURE, nsplit, query_mask=c["mask"], dtype=torch.float32)
    assert conf32.dtype == torch.float32
    e = cf.compare(cf.as_outputs(conf32, cf.select(conf32, c)), *ref(name, nsplit), nsplit, cf.GPU_BAR[nsplit])
    print(f"{name} nsplit {nsplit}: f32 stand-in conf {e[0]:.2e} mconf {e[1]:.2e}")


def _rejected(got, name, nsplit):
    try:
        cf.compare(got, *ref(name, nsplit), nsplit)
    except AssertionError:
        return True
    return False


def _lists_differ(sel, want):
    return any(sel[k].shape != want[k].shape or not torch.equal(sel[k], want[k]) for k in cf.LIST_KEYS)


BITING = [k for k in CASES if k != "smallest"]            # one confidence is 1 whatever its logit: no wrong logit shows there


@pytest.mark.parametrize("name", BITING)
def test_wrong_temperature_and_missing_hi_lo_fail_the_conf_bar(name):
    """(a) temperature without the 1e-4 (every mode), (b) the split mode without its hi.lo term: outside the conf bar at every soft case"""
    c = built(name)
    for nsplit in cf.NSPLITS:
        conf = cf.confidence(c["f3"], c["f2"], cf.TEMPERATURE, nsplit, temp_eps=0.0, query_mask=c["mask"])
        with pytest.raises(AssertionError, match="conf_matrix|mconf"):
            cf.compare(cf.as_outputs(conf, ref(name, nsplit)[1]), *ref(name, nsplit), nsplit)           # (the reference's own lists: conf alone fails)
    conf = cf.confidence(c["f3"], c["f2"], cf.TEMPERATURE, 3, query_mask=c["mask"], fault="no_hi_lo")
    with pytest.raises(AssertionError, match="conf_matrix|mconf"):
        cf.compare(cf.as_outputs(conf, ref(name, 3)[1]), *ref(name, 3), 3)


def test_wrong_variants_change_a_list():
    """(c) the border removed on all four sides and (d) ``>=`` at the threshold leave conf alone and are caught by the lists"""
    # (c): a match in the bottom rows / right columns disappears.  Post-filtering the oracle's lists is the four-sided mask (no ties here)
    changed = []
    for name in ("interior_tiles", "nine_row_tiles", "two_spans", "b33"):
        c, (conf, want) = built(name), ref(name, 3)
        x, y = want["j_ids"] % c["wc"], want["j_ids"] // c["wc"]
        keep = (x < c["wc"] - c["border"]) & (y < c["hc"] - c["border"])
        sel = {k: (v[keep] if torch.is_tensor(v) else v) for k, v in want.items()}
        assert _rejected(cf.as_outputs(conf, sel), name, 3) == (not bool(keep.all()))
        changed.append(not bool(keep.all()))
    assert all(changed)
    # (d): thr set to a selected confidence.  The strict test drops that match; conf >= thr == conf > the next double below thr keeps it
    name = "interior_tiles"
    c, (conf, want) = built(name), ref(name, 0)
    k = int(torch.argsort(want["mconf"])[len(want["mconf"]) // 2])
    thr = float(want["mconf"][k])
    assert thr > c["thr"] and int((conf == thr).sum()) == 1
    strict, loose = cf.select(conf, c, thr=thr), cf.select(conf, c, thr=float(np.nextafter(thr, 0.0)))
    assert len(loose["i_ids"]) == len(strict["i_ids"]) + 1 and int(want["i_ids"][k]) in loose["i_ids"].tolist() and int(want["i_ids"][k]) not in strict["i_ids"].tolist()
    assert _lists_differ(loose, strict)
    with pytest.raises(AssertionError, match="ids"):
        cf.compare(cf.as_outputs(conf, loose), conf, strict, 0)


EXPECT = {   # (placement, variant): (i_ids, j_ids), written out
    ("one_tile", "valid"): ([0, 1, 3], [31, 71, 40]), ("one_tile", "border"): ([0, 1, 3], [31, 71, 40]), ("one_tile", "border2"): ([0, 1, 3], [31, 71, 40]),
    ("two_tiles", "valid"): ([0, 1, 3], [53, 511, 455]), ("two_tiles", "border"): ([0, 1, 3], [277, 511, 455]),
    ("two_tiles", "border2"): ([0, 1, 3], [277, 511, 455]),
    ("two_spans", "valid"): ([0, 1, 3], [215, 1024, 294]), ("two_spans", "border"): ([0, 1, 3], [830, 1024, 294]),
    ("two_spans", "border2"): ([0, 1, 3], [830, 1024, 294]),
}


@pytest.mark.parametrize("nsplit", cf.NSPLITS)
@pytest.mark.parametrize("placement,variant", TIES)
def test_tie_cases_select_what_they_say(placement, variant, nsplit):
    c = cf.tie_case(placement, variant)
    conf, sel = cf.reference(c, nsplit)
    vals = conf[0, 0, c["copies"]]
    assert bool((vals == vals[0]).all()) and float(vals[0]) == float(conf[0, 0].max()) > 0.3          # an exact tie of the row maximum
    assert (sel["i_ids"].tolist(), sel["j_ids"].tolist()) == EXPECT[placement, variant] and sel["b_ids"].tolist() == [0, 0, 0]
    lowest = c["copies"][0]
    assert (lowest // c["wc"] >= 2 and lowest % c["wc"] >= 2) == (variant == "valid") == (c["lazy_flag"] == 0)
    assert cf.decidable(c, nsplit, conf)[1]
    # the copies' column tiles hold no other strong logit (tie_case's docstring): the tied logit is the maximum of each
    sim = cf.logits(c["f3"], c["f2"], cf.TEMPERATURE, nsplit)[0]
    for j in c["copies"]:
        t = j // 128 * 128
        assert float(sim[:, t:t + 128].max()) == float(sim[0, j])
    if placement == "two_spans":
        assert min(c["copies"]) < 516 <= max(c["copies"])
    if placement == "two_tiles":
        assert c["copies"][-1] == c["copies"][0] + 256


@pytest.mark.parametrize("nsplit", cf.NSPLITS)
def test_two_identical_rows_match_the_same_cell(nsplit):
    c = cf.tie_case("two_rows", None)
    conf, sel = cf.reference(c, nsplit)
    assert float(conf[0, 5, 40]) == float(conf[0, 133, 40]) > 0.1
    assert sel["i_ids"].tolist() == [5, 133] and sel["j_ids"].tolist() == [40, 40]
    assert cf.decidable(c, nsplit, conf)[1]


@pytest.mark.parametrize("nsplit", cf.NSPLITS)
def test_wide_case(nsplit):
    c = cf.wide_case()
    conf, sel = cf.reference(c, nsplit)
    sim = cf.logits(c["f3"], c["f2"], cf.TEMPERATURE, nsplit)[0]
    lo, hi = cf.WIDE_LOW_TILE
    assert float(sim.max()) > 100 and bool((sim[cf.WIDE_ZERO_ROW] == 0).all()) and bool((sim[:, cf.WIDE_ZERO_COL] == 0).all())
    assert float(sim[:, lo:hi].max()) < min(float(sim[:, :lo].max()), float(sim[:, hi:2 * hi - lo].max())) - 59
    assert bool(torch.isfinite(conf).all()) and len(sel["i_ids"]) >= 10
    assert cf.decidable(c, nsplit, conf)[1]
    conf32 = cf.confidence(c["f3"], c["f2"], cf.TEMPERATURE, nsplit, dtype=torch.float32)
    cf.compare(cf.as_outputs(conf32, cf.select(conf32, c)), conf, sel, nsplit, cf.GPU_BAR[nsplit])
