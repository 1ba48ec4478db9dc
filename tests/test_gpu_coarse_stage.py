"""The 3D-2D coarse stage on the device -- ``ophip_coarse_match`` and ``ophip_coarse_match_masked``: frag_planes -> sim_frag / sim_frag3 /
sim_stats -> stat_combine -> conf or the second tile pass -> select_decide / select_place -- against the float64 restatement of
tests/coarse_faithful.py, in every form of every mode on both tile kernels:

    nsplit 0 (exact f32)            eager
    nsplit 3, 1 (split / plain bf16)  eager one-pass (OPHIP_COARSE_TWO_PASS=0), eager two-pass (=1), lazy (conf = NULL, count of 4 ints)

each with OPHIP_SIM_TILE unset and 3 (the exact mode has one tile kernel; it runs under both settings all the same).  The lazy form of
nsplit 0 does not exist: C refuses it, asserted once below and in test_gpu_parity.py::test_lazy_conf_matrix_exact_tie_raises_the_rerun_flag.

Every call starts from a NaN-filled conf_matrix and workspace and sentinel-filled lists, and nothing may be written past ``count`` in any
list.  conf_matrix and mconf are held to coarse_faithful.GPU_BAR: the project's bars (test_gpu_parity.py: COARSE_RTOL 1e-4 / 1e-3,
PLAIN_BF16_LIKE_FOR_LIKE_TOL 1e-3, atol 1e-7), the bf16 modes' tightened to rtol 2e-4 >= 10 x the largest error measured (1.53e-5, a tie case).
b_ids, i_ids, j_ids, m_bids, mkpts_3d and mkpts_c are compared exactly, nothing set aside: every decision of every case's reference has a
relative margin of ten times the mode's (un-tightened) rtol (tests/test_coarse_faithful_cpu.py::test_every_case_is_decidable).

Soft inputs: the shapes of coarse_faithful.SOFT_CASES (what each reaches is noted there).  Ties: exact duplicates of one 2D cell in one
column tile, in two (j and j + 256), and in conf_kernel's two spans at M = 1025, with the lowest copy selectable, in the removed border,
and two of three copies in the border; two identical 3D rows in different row tiles.  Wide logits: coarse_faithful.wide_case.  Query
mask: one whole interior column tile blanked, with and without per-image scales, and the stage in three calls (parts 4, 8, 2) against one.
Already pinned elsewhere and not repeated: a ragged mask with scales at three shapes, eager against lazy
(test_gpu_masked.py::test_coarse_match_masked_scaled_vs_oracle); the stage in two calls, parts 1 then 2
(test_gpu_workspace_contract.py::test_coarse_match_in_two_halves).

What the tie cases do NOT claim ("Coarse stage"): in the bf16 modes duplicate columns (or rows) are bit-equal only
while the statistics of their tiles use the same reference.  The fast statistics pass of an interior tile sums against the TILE's
maximum, so copies in two interior tiles with different maxima get column (row) sums that differ in the last bits; measured on the
MI355X with a stronger pair added to one copy's tile: confidences 0x1.00000cp-1 against 0x1.000004p-1, the larger copy then counts as
the only row maximum, and when it lies in the removed border the match is dropped where the reference emits it (the exact mode, whose
statistics use true maxima, keeps the tie).  tie_case keeps the ordinary matches out of the copies' tiles and the CPU file asserts that.

Measured on the MI355X (max relative error over reference elements above 1e-6 of conf_matrix / mconf, worst form and tile kernel; the
module prints them):

    case                matches   nsplit 0              nsplit 3              nsplit 1
    smallest                  1   0 / 0                 0 / 0                 0 / 0
    hc1_cut_tiles            61   1.14e-05 / 2.34e-06   5.23e-06 / 1.43e-06   4.98e-06 / 1.38e-06
    one_row_tails            73   9.53e-06 / 4.88e-06   7.59e-06 / 1.80e-06   6.24e-06 / 2.34e-06
    interior_tiles           92   8.86e-06 / 3.57e-06   7.59e-06 / 3.89e-06   6.06e-06 / 3.03e-06
    nine_row_tiles           49   8.14e-06 / 2.17e-06   8.92e-06 / 2.48e-06   6.13e-06 / 2.63e-06
    two_spans                46   1.05e-05 / 1.13e-06   9.45e-06 / 1.92e-06   6.84e-06 / 2.03e-06
    five_spans               44   1.18e-05 / 2.56e-06   8.32e-06 / 1.71e-06   6.93e-06 / 1.51e-06
    b33                    1570   1.40e-05 / 4.12e-06   8.50e-06 / 2.52e-06   6.58e-06 / 3.46e-06
    border_takes_all          0   9.04e-06 / -          6.03e-06 / -          5.62e-06 / -
    two_rows                  2   5.30e-06 / 5.8e-15    2.66e-06 / 5.8e-15    3.24e-06 / 5.8e-15
    wide                     15   1.04e-05 / 0          9.62e-06 / 0          4.32e-06 / 0
    masked_tile (_scaled)    63   9.73e-06 / 3.09e-06   1.02e-05 / 2.90e-06   7.44e-06 / 2.29e-06

    ties (nine cases)       3   6.53e-06 / 2.98e-08   1.53e-05 / 4.77e-07   1.46e-05 / 9.54e-07

Every list equal in all 14 calls of every case (2 in the exact mode); the whole module takes 4 s.
"""
import pytest
import torch

from onepose_st_amd import hip, matchcall
from tests import coarse_faithful as cf

pytestmark = pytest.mark.gpu

SOFT, MASKED = sorted(cf.SOFT_CASES), sorted(cf.MASK_CASES)
TIES = [(p, v) for p in cf.TIE_PLACEMENTS for v in cf.TIE_VARIANTS]
FORMS = {0: ("eager",), 3: ("one_pass", "two_pass", "lazy"), 1: ("one_pass", "two_pass", "lazy")}
TILES = (None, "3")
I64_SENTINEL, F32_SENTINEL, U8_SENTINEL, CNT_SENTINEL = -7, -123.0, 7, 77


@pytest.fixture(scope="module")
def dev():
    assert torch.cuda.is_available(), "these tests need the MI355X"
    hip.load()
    return torch.device("cuda:0")


@pytest.fixture(scope="module")
def cases():
    """inputs and float64 references, computed once per (case, nsplit) and left unchanged"""
    built, refs = {}, {}

    def get(key, nsplit):
        if key not in built:
            if isinstance(key, tuple):
                built[key] = cf.tie_case(*key)
            else:
                built[key] = cf.wide_case() if key == "wide" else cf.build(cf.ALL_CASES[key])
        if (key, nsplit) not in refs:
            refs[key, nsplit] = cf.reference(built[key], nsplit)
        return (built[key], *refs[key, nsplit])
    return get


def set_form(monkeypatch, form, tile):
    """both variables are read on every call"""
    if tile is None:
        monkeypatch.delenv("OPHIP_SIM_TILE", raising=False)
    else:
        monkeypatch.setenv("OPHIP_SIM_TILE", tile)
    if form in ("one_pass", "two_pass"):
        monkeypatch.setenv("OPHIP_COARSE_TWO_PASS", "1" if form == "two_pass" else "0")
    else:
        monkeypatch.delenv("OPHIP_COARSE_TWO_PASS", raising=False)


def run(dev, c, nsplit, form, parts=(3,)):
    """one call (or one per entry of ``parts``) on fresh buffers -> (outputs trimmed to the count, as coarse_faithful.compare takes them,
    count[1]); asserts what holds for every call: conf finite, nothing past the count in any list, count[2:] untouched"""
    B, N, _ = c["f3"].shape
    M, lazy = c["f2"].shape[1], form == "lazy"
    cap = B * N
    conf = None if lazy else torch.full((B, N, M), float("nan"), device=dev)
    ws = torch.full((hip.load().ophip_coarse_workspace_floats(B, N, M),), float("nan"), device=dev)
    ids = [torch.full((cap,), I64_SENTINEL, dtype=torch.int64, device=dev) for _ in range(4)]
    mconf, mk3, mkc = (torch.full(s, F32_SENTINEL, device=dev) for s in ((cap,), (cap, 3), (cap, 2)))
    gtm = torch.full((cap,), U8_SENTINEL, dtype=torch.uint8, device=dev)
    cnt = torch.full((4,), CNT_SENTINEL, dtype=torch.int32, device=dev)
    d3, d2, dk = c["f3"].to(dev), c["f2"].to(dev), c["kp"].to(dev)
    kw = {}
    if c["mask"] is not None:
        kw["query_mask"] = c["mask"].to(dev).view(torch.uint8).contiguous()
    if c["qscale"] is not None:
        kw["query_scale"] = c["qscale"].to(dev)
    for p in parts:
        matchcall.coarse_match(d3, d2, dk, kpts_bstride=0 if dk.shape[0] == 1 and B > 1 else N * 3, wc=c["wc"], temperature=cf.TEMPERATURE, thr=c["thr"],
                               border_rm=c["border"], scale=cf.SCALE, nsplit=nsplit, lists=matchcall.MatchLists(*ids[:3], mconf, mk3, mkc, ids[3], gtm, cnt),
                               conf=conf, workspace=ws, parts=p, **kw)
    torch.cuda.synchronize()
    count = cnt.tolist()
    K = count[0]
    assert 0 <= K <= cap and count[2:] == [CNT_SENTINEL] * 2 and (count[1] in (0, 1) if lazy else count[1] == CNT_SENTINEL), count
    for t in ids:
        assert bool((t[K:] == I64_SENTINEL).all())
    for t in (mconf, mk3, mkc):
        assert bool((t[K:] == F32_SENTINEL).all())
    assert bool((gtm[K:] == U8_SENTINEL).all())
    if conf is not None:
        assert bool(torch.isfinite(conf).all()), "conf_matrix has elements no kernel wrote"
    out = dict(conf=None if lazy else conf.cpu(), b_ids=ids[0][:K].cpu(), i_ids=ids[1][:K].cpu(), j_ids=ids[2][:K].cpu(), m_bids=ids[3][:K].cpu(),
               mconf=mconf[:K].cpu(), mkpts_3d_db=mk3[:K].cpu(), mkpts_query_c=mkc[:K].cpu(), gt_mask=gtm[:K].cpu())
    return out, count[1]


def every_form(dev, monkeypatch, c, ref_conf, ref, nsplit):
    """case ``c`` in every form of mode ``nsplit`` on both tile kernels against its reference -> {(form, tile): outputs}"""
    outs, worst = {}, (0.0, 0.0)
    for tile in TILES:
        for form in FORMS[nsplit]:
            set_form(monkeypatch, form, tile)
            out, flag = run(dev, c, nsplit, form)
            if form == "lazy":
                assert flag == 0, (form, tile)
            try:
                e = cf.compare(out, ref_conf, ref, nsplit, cf.GPU_BAR[nsplit])
            except AssertionError as err:
                raise AssertionError(f"{c['name']} nsplit {nsplit} {form} tile {tile}: {err}") from None
            worst = (max(worst[0], e[0]), max(worst[1], e[1]))
            outs[form, tile] = out
    print(f"coarse stage {c['name']} nsplit {nsplit}: conf max rel err {worst[0]:.2e}, mconf {worst[1]:.2e}, {len(ref['i_ids'])} matches")
    return outs


@pytest.mark.parametrize("nsplit", cf.NSPLITS)
@pytest.mark.parametrize("name", SOFT)
def test_soft_inputs(dev, monkeypatch, cases, name, nsplit):
    """confidences all over (0, 1) and rows that lose the mutual test: a confidence that is a few percent off changes a list"""
    c, ref_conf, ref = cases(name, nsplit)
    if cf.SOFT_CASES[name].get("nonmutual", True):
        assert cf.nonmutual_rows(ref_conf, c["thr"]) >= 1                       # the mutual test rejects something
    if name == "border_takes_all":
        assert len(ref["i_ids"]) == 0 and int((ref_conf > c["thr"]).sum()) > 10
    outs = every_form(dev, monkeypatch, c, ref_conf, ref, nsplit)
    for tile in TILES:                                                          # the two eager forms of one tile kernel: bit for bit
        if nsplit:
            assert torch.equal(outs["one_pass", tile]["conf"], outs["two_pass", tile]["conf"])
            assert torch.equal(outs["lazy", tile]["mconf"], outs["one_pass", tile]["mconf"])


def test_the_exact_mode_has_no_lazy_form(dev, cases):
    c = cases("hc1_cut_tiles", 0)[0]
    with pytest.raises(ValueError):
        run(dev, c, 0, "lazy")


@pytest.mark.parametrize("nsplit", cf.NSPLITS)
@pytest.mark.parametrize("placement,variant", TIES)
def test_exact_ties(dev, monkeypatch, cases, placement, variant, nsplit):
    """coarse_faithful.tie_case: the copies' confidences are bit-equal; the eager forms return the reference's first true j; the lazy form
    raises count[1] exactly when the lowest copy is not selectable, and returns the same lists when it is"""
    c, ref_conf, ref = cases((placement, variant), nsplit)
    worst = (0.0, 0.0)
    for tile in TILES:
        for form in FORMS[nsplit]:
            set_form(monkeypatch, form, tile)
            out, flag = run(dev, c, nsplit, form)
            if form == "lazy":
                assert flag == c["lazy_flag"], (form, tile)
                if flag:
                    continue                                                    # "run this frame again with a conf buffer": the lists are not final
            else:
                vals = out["conf"][0, 0, c["copies"]]
                assert bool((vals == vals[0]).all()) and float(vals[0]) == float(out["conf"][0, 0].max()), (form, tile, vals.tolist())
            try:
                e = cf.compare(out, ref_conf, ref, nsplit, cf.GPU_BAR[nsplit])
            except AssertionError as err:
                raise AssertionError(f"{c['name']} nsplit {nsplit} {form} tile {tile}: {err}") from None
            worst = (max(worst[0], e[0]), max(worst[1], e[1]))
    print(f"coarse stage tie {c['name']} nsplit {nsplit}: conf max rel err {worst[0]:.2e}, mconf {worst[1]:.2e}, j = {ref['j_ids'].tolist()}")


@pytest.mark.parametrize("nsplit", cf.NSPLITS)
def test_two_identical_rows_match_the_same_cell(dev, monkeypatch, cases, nsplit):
    c, ref_conf, ref = cases(("two_rows", None), nsplit)
    assert ref["i_ids"].tolist() == [5, 133] and ref["j_ids"].tolist() == [40, 40]
    outs = every_form(dev, monkeypatch, c, ref_conf, ref, nsplit)
    for (form, tile), out in outs.items():
        if form != "lazy":
            assert float(out["conf"][0, 5, 40]) == float(out["conf"][0, 133, 40]), (form, tile)


@pytest.mark.parametrize("nsplit", cf.NSPLITS)
def test_wide_logits(dev, monkeypatch, cases, nsplit):
    """coarse_faithful.wide_case: strong pairs that force the exact sweep in interior tiles (in MODE 0 and in MODE 1, the statistics-only
    pass of the lazy and two-pass forms, and in sim_frag3_kernel's own fallback), zero logits, a column tile far below its neighbours"""
    c, ref_conf, ref = cases("wide", nsplit)
    assert len(ref["i_ids"]) >= 10
    every_form(dev, monkeypatch, c, ref_conf, ref, nsplit)


@pytest.mark.parametrize("nsplit", cf.NSPLITS)
@pytest.mark.parametrize("name", MASKED)
def test_a_whole_column_tile_masked(dev, monkeypatch, cases, name, nsplit):
    c, ref_conf, ref = cases(name, nsplit)
    lo, hi = cf.MASK_CASES[name]["mask_cols"]
    assert float(ref_conf[:, :, lo:hi].max()) == 0.0 and len(ref["i_ids"]) > 20
    outs = every_form(dev, monkeypatch, c, ref_conf, ref, nsplit)
    for out in outs.values():
        if out["conf"] is not None:
            assert float(out["conf"][:, :, lo:hi].abs().max()) == 0.0              # padded cells: exactly 0
        assert not bool(((out["j_ids"] >= lo) & (out["j_ids"] < hi)).any())


@pytest.mark.parametrize("nsplit,form", [(0, "eager"), (3, "one_pass"), (3, "two_pass"), (3, "lazy")])
def test_the_stage_in_three_calls_equals_one(dev, monkeypatch, cases, nsplit, form):
    """parts 4 (similarity tiles), 8 (statistics merge and confidences), 2 (selection) in three calls: bit for bit what parts 3 gives"""
    c = cases("masked_tile_scaled", nsplit)[0]
    set_form(monkeypatch, form, None)
    (one, f1), (three, f3) = run(dev, c, nsplit, form), run(dev, c, nsplit, form, parts=(4, 8, 2))
    assert f1 == f3 and len(one["i_ids"]) > 20
    for k in one:
        assert (one[k] is None and three[k] is None) or torch.equal(one[k], three[k]), k
