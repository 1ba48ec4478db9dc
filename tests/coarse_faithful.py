"""Float64 restatement of the 3D-2D coarse stage (csrc/coarse_match.hip), its input generators, margins and case tables.  CPU only;
tests/test_coarse_faithful_cpu.py checks it, tests/test_gpu_coarse_stage.py compares the device with it.

``confidence`` rounds where the kernels round and nowhere else:

    nsplit 0  sim_stats_kernel: operands f / 16 (exact), products and sums unrounded, divided by float32(temperature + 1e-4)
    nsplit 1  frag_planes_kernel's hi plane bf16(f / 16), times the f32 factor 1 / float32(temperature + 1e-4)
    nsplit 3  hi = bf16(x), lo = bf16(x - hi) of x = f / 16; hi.hi + hi.lo + lo.hi (mma_bf16<3> issues no lo.lo); the same factor

then the dual softmax in float64.  The selection is ``oracle.onepose_oracle.coarse_match_select`` on that matrix (dtype-agnostic).

Soft inputs (``soft_case``) spread the confidences over (0, 1) and contain rows that pass the threshold and lose the mutual test, so a
confidence that is a few percent off changes a list -- and the seeds are chosen so that it must not: every decision of the reference
(threshold, row maximum, column maximum) has a relative margin of ten times the rtol of the mode under test (``margins``,
``MARGIN``).  A correct kernel is within rtol, a decision with ten times that gap cannot legitimately flip, so the lists are compared
exactly with nothing set aside."""
from __future__ import annotations

import numpy as np
import torch

from oracle import onepose_oracle as orc
from tests.bf16_faithful import bf16_round, split

TEMPERATURE, SCALE = 0.08, 8.0
# conf_matrix and mconf against confidence(nsplit): the bars of tests/test_gpu_parity.py (COARSE_RTOL[0], COARSE_RTOL[3] with atol 1e-7,
# PLAIN_BF16_LIKE_FOR_LIKE_TOL); test_coarse_faithful_cpu.py asserts they are the same numbers
BAR = {0: dict(rtol=1e-4, atol=1e-7), 3: dict(rtol=1e-3, atol=1e-7), 1: dict(rtol=1e-3, atol=1e-7)}
# what tests/test_gpu_coarse_stage.py holds the device to: the bf16 modes tightened to 10 x the largest error measured on the MI355X over all
# its cases (1.53e-5 in a tie case, rounded up); the exact mode's bar is already below 10 x its own (1.40e-5)
GPU_BAR = {0: BAR[0], 3: dict(rtol=2e-4, atol=1e-7), 1: dict(rtol=2e-4, atol=1e-7)}
# the least relative margin of every decision: 10 x the confidence rtol of the mode (1e-3 for exact f32, 1e-2 for the bf16 modes)
MARGIN = {0: 1e-3, 3: 1e-2, 1: 1e-2}
NSPLITS = (0, 3, 1)
LIST_KEYS = ("b_ids", "i_ids", "j_ids", "m_bids", "mkpts_3d_db", "mkpts_query_c")


def _planes(f, nsplit, dtype):
    """the operand planes of one input in mode ``nsplit``: [x] or [hi] or [hi, lo]"""
    if nsplit == 0:
        return [f.to(dtype) * 0.0625]                       # a power of two: exact in either dtype
    x = f.to(torch.float32) * 0.0625
    if nsplit == 1:
        return [bf16_round(x).to(dtype)]
    hi, lo = split(x)
    return [hi.to(dtype), lo.to(dtype)]


def logits(f3, f2, temperature, nsplit, temp_eps=1e-4, query_mask=None, dtype=torch.float64, fault=None):
    """the similarity matrix of mode ``nsplit`` with the arithmetic of ``dtype`` (float32: the stand-in of test_coarse_faithful_cpu.py).
    ``fault``: ``no_hi_lo`` drops the hi.lo term of the split mode (a deliberately wrong variant)"""
    a, b = _planes(f3, nsplit, dtype), _planes(f2, nsplit, dtype)
    dot = lambda x, y: torch.einsum("nlc,nsc->nls", x, y)
    temp = np.float32(temperature + temp_eps)               # SimArgs::temp = (float)(temperature + temp_eps)
    if nsplit == 0:
        sim = dot(a[0], b[0]) / float(temp)
    else:
        sim = dot(a[0], b[0])
        if nsplit == 3:
            sim = sim + dot(a[1], b[0]) if fault == "no_hi_lo" else sim + dot(a[0], b[1]) + dot(a[1], b[0])
        sim = sim * float(np.float32(1.0) / temp)           # inv_temp = 1.0f / p.temp
    if query_mask is not None:
        pad = torch.zeros_like(sim)
        pad[~query_mask.bool()[:, None, :].expand_as(sim)] = -1e9
        sim = sim + pad
    return sim


def confidence(f3, f2, temperature, nsplit, temp_eps=1e-4, query_mask=None, dtype=torch.float64, fault=None):
    """``[B, N, M]`` dual-softmax confidences of mode ``nsplit`` (module docstring); ``query_mask [B, M]`` adds -1e9 to the masked columns"""
    sim = logits(f3, f2, temperature, nsplit, temp_eps, query_mask, dtype, fault)
    return torch.softmax(sim, 1) * torch.softmax(sim, 2)


def plain_bf16_confidence(f3, f2, temperature=TEMPERATURE):
    """float64 confidences of plain bf16 (nsplit 1), rounded where the kernel rounds"""
    return confidence(f3, f2, temperature, 1)


def select(conf, c, thr=None, border=None):
    """the oracle's selection on ``conf`` for case ``c`` (``kp`` of a shared table is expanded over the batch)"""
    B, (hc, wc) = conf.shape[0], (c["hc"], c["wc"])
    kp = c["kp"].expand(B, -1, -1)
    return orc.coarse_match_select(conf, (hc, wc), (hc * SCALE, wc * SCALE), kp, c["thr"] if thr is None else thr,
                                   c["border"] if border is None else border, query_image_scale=c.get("qscale"))


def reference(c, nsplit, **kw):
    """(float64 confidences, the oracle's lists) of case ``c`` in mode ``nsplit``"""
    conf = confidence(c["f3"], c["f2"], TEMPERATURE, nsplit, query_mask=c.get("mask"), **kw)
    return conf, select(conf, c)


def margins(conf, hw_c, thr, border_rm, exempt_rows=(), exempt_cols=()):
    """From the reference alone, the three smallest relative margins of the selection's decisions:
      * |c - thr| / thr over the elements c > thr / 4 outside the removed border (inside it the threshold decides nothing);
      * (max - runner-up) / max over the rows whose maximum exceeds thr / 4, ``exempt_rows`` [(b, i)] -- planted exact ties -- left out;
      * the same over the columns, ``exempt_cols`` [(b, j)] left out.
    A set that is empty (or a row of one element) has the margin ``inf``."""
    B, N, M = conf.shape
    h, w = hw_c
    inside = torch.ones(h, w, dtype=torch.bool)
    inside[:border_rm] = False
    inside[:, :border_rm] = False
    el = conf[:, :, inside.flatten()]
    el = el[el > thr / 4]
    m_thr = float(((el - thr).abs() / thr).min()) if el.numel() else float("inf")

    def gap(x, dim, exempt):
        if x.shape[dim] < 2:
            return float("inf")
        top = torch.topk(x, 2, dim=dim)[0]
        first, second = top.select(dim, 0), top.select(dim, 1)
        live = first > thr / 4
        for b, k in exempt:
            live[b, k] = False
        return float(((first - second) / first)[live].min()) if bool(live.any()) else float("inf")
    return m_thr, gap(conf, 2, exempt_rows), gap(conf, 1, exempt_cols)


def nonmutual_rows(conf, thr):
    """rows whose maximum is above ``thr`` and is not its column's maximum: what the mutual test has to reject"""
    v, j = conf.max(dim=2)
    return int(((v > thr) & (v < conf.max(dim=1)[0].gather(1, j))).sum())


def _soft_batch(N, hc, wc, seed, n_plant):
    g = torch.Generator().manual_seed(seed)
    M = hc * wc
    f3, f2 = torch.randn(N, 256, generator=g), torch.randn(M, 256, generator=g)
    n = min(N, M) // 2 if n_plant is None else n_plant
    k = n // 4
    assert n + k <= N and n <= M
    if n:
        cells = torch.randperm(M, generator=g)[:n]
        s = torch.linspace(0.25, 1.0, n)[torch.randperm(n, generator=g)]
        f2[cells] = s[:, None] * f3[:n] + 0.1 * torch.randn(n, 256, generator=g)
        if k:
            f2[cells[:k]] += torch.linspace(0.3, 0.9, k)[:, None] * f3[n:n + k]          # a competing row on the first n // 4 cells
    return f3 * 1.5, f2


def soft_case(B, N, hc, wc, seed, n_plant=None):
    """Inputs whose confidences spread over (0, 1): n = min(N, M) // 2 (or ``n_plant``) pairs planted at strengths 0.25 .. 1.0, the
    first n // 4 cells with a second, competing row at 0.3 .. 0.9.  ``seed``: one int, or one per batch element (a decision margin is a
    property of one batch element, so a batch is assembled from elements that qualify)."""
    seeds = (seed,) * B if isinstance(seed, int) else tuple(seed)
    assert len(seeds) == B and (B == 1 or len(set(seeds)) == B)
    parts = [_soft_batch(N, hc, wc, s, n_plant) for s in seeds]
    return torch.stack([p[0] for p in parts]), torch.stack([p[1] for p in parts])


# --- the soft-input cases of tests/test_gpu_coarse_stage.py -------------------------------------------------------------------------
# name: (B, N, hc, wc), seed(s), thr, border_rm, and options: n_plant, shared_kpts (one keypoint table, kpts_bstride = 0), mask_cols (a
# query mask that blanks columns [lo, hi)), qscale, nonmutual (False: the shape cannot hold a row that loses the mutual test)
# seeds: found by a CPU search for the margin condition in all three modes (test_coarse_faithful_cpu.py::test_every_case_is_decidable)
SOFT_CASES = {}


def _case(name, shape, seed, thr, border, **opt):
    SOFT_CASES[name] = dict(name=name, shape=shape, seed=seed, thr=thr, border=border, **opt)


# A row above the threshold that loses the mutual test needs thr < 0.5: conf[i, j] = P_col(i | j) * P_row(j | i) > 0.5 makes i hold more
# than half of column j's softmax, so every other conf[i', j] <= P_col(i' | j) < 0.5 < conf[i, j].  The cases at thr 0.5 cannot show one.
_case("smallest", (1, 1, 1, 1), 1, 0.2, 0, nonmutual=False)                       # one confidence, exactly 1
_case("hc1_cut_tiles", (1, 127, 1, 129), 2, 0.2, 0)                               # hc = 1; both tiles cut; M % 4 = 1
_case("one_row_tails", (2, 257, 3, 43), (1, 2), 0.5, 1, nonmutual=False)          # last row tile / conf row block of one row; a selection workgroup across the batch boundary
_case("interior_tiles", (1, 256, 16, 16), 1, 0.05, 2)                             # 2 x 2 interior tiles: the fast statistics pass everywhere
_case("nine_row_tiles", (1, 1152, 8, 16), 2, 0.2, 1)                              # ntr = 9: xcd_tile's uneven deal; one column tile
_case("two_spans", (1, 130, 25, 41), 2, 0.5, 2, nonmutual=False)                  # M = 1025: two spans, non-vector path, second span unaligned
_case("five_spans", (1, 97, 54, 76), 1, 0.05, 0)                                  # M = 4104: a second round of records in select_decide; 33 column tiles
_case("b33", (33, 2000, 8, 8), (1, 2, 5, 7, 8, 9, 10, 12, 13, 14, 15, 16, 17, 18, 19, 20, 21, 22, 23, 24, 25, 26, 27, 28, 29, 31, 32, 33, 34, 35,
                                36, 37, 38), 0.05, 1, n_plant=64, shared_kpts=True)    # B N = 66000: 258 selection workgroups, ~1500 matches
_case("border_takes_all", (1, 300, 10, 13), 1, 0.2, 10, nonmutual=False)          # border_rm >= min(hc, wc): no match, conf finite
# the query-mask cases: one whole interior column tile (M = 384, columns 128 .. 255) blanked, then the same with per-image scales
MASK_CASES = {k: dict(name=k, shape=(1, 256, 12, 32), seed=2, thr=0.2, border=2, mask_cols=(128, 256), **opt)
              for k, opt in (("masked_tile", {}), ("masked_tile_scaled", dict(qscale=[[1.25, 1.5]])))}
ALL_CASES = {**SOFT_CASES, **MASK_CASES}


def build(case):
    """the inputs of one table entry: f3, f2, kp ([1, N, 3] for a shared table), mask, qscale, and the scalars of the call"""
    B, N, hc, wc = case["shape"]
    f3, f2 = soft_case(B, N, hc, wc, case["seed"], case.get("n_plant"))
    g = torch.Generator().manual_seed(4)
    kp = torch.randn(1 if case.get("shared_kpts") else B, N, 3, generator=g)
    c = dict(name=case["name"], f3=f3, f2=f2, kp=kp, hc=hc, wc=wc, thr=case["thr"], border=case["border"], mask=None, qscale=None,
             exempt_rows=(), exempt_cols=())
    if case.get("mask_cols"):
        lo, hi = case["mask_cols"]
        c["mask"] = torch.ones(B, hc * wc, dtype=torch.bool)
        c["mask"][:, lo:hi] = False
    if case.get("qscale"):
        c["qscale"] = torch.tensor(case["qscale"], dtype=torch.float32).reshape(B, 2).contiguous()
    return c


def decidable(c, nsplit, conf=None):
    """the three margins of case ``c`` in mode ``nsplit`` and whether all reach ``MARGIN[nsplit]``"""
    conf = reference(c, nsplit)[0] if conf is None else conf
    m = margins(conf, (c["hc"], c["wc"]), c["thr"], c["border"], c["exempt_rows"], c["exempt_cols"])
    return m, min(m) >= MARGIN[nsplit]


# --- exact ties ---------------------------------------------------------------------------------------------------------------------
# placement -> (N, hc, wc, {variant: columns of the copies}, cells of the three ordinary rows 1, 2, 3)
_cell = lambda wc, y, x: y * wc + x
TIE_PLACEMENTS = {
    # one column tile (M = 72), two row tiles
    "one_tile": (140, 8, 9, {"valid": [_cell(9, 3, 4), _cell(9, 5, 6)], "border": [_cell(9, 0, 4), _cell(9, 3, 4)],
                             "border2": [_cell(9, 0, 4), _cell(9, 2, 1), _cell(9, 3, 4)]},
                 [_cell(9, 7, 8), _cell(9, 5, 1), _cell(9, 4, 4)]),
    # M = 512: copies at j and j + 256 (column tiles 0 and 2; the middle copy of border2 in tile 1), ordinary matches in tile 3
    "two_tiles": (140, 32, 16, {"valid": [_cell(16, 3, 5), _cell(16, 3, 5) + 256], "border": [_cell(16, 1, 5), _cell(16, 1, 5) + 256],
                                "border2": [_cell(16, 1, 5), _cell(16, 9, 1), _cell(16, 1, 5) + 256]},
                  [_cell(16, 31, 15), _cell(16, 26, 1), _cell(16, 28, 7)]),
    # M = 1025: conf_kernel's two spans meet at column 516 (non-vector path); nine column tiles in the lazy and two-pass forms
    "two_spans": (130, 25, 41, {"valid": [_cell(41, 5, 10), _cell(41, 20, 10)], "border": [_cell(41, 1, 10), _cell(41, 20, 10)],
                                "border2": [_cell(41, 1, 10), _cell(41, 10, 1), _cell(41, 20, 10)]},
                  [_cell(41, 24, 40), _cell(41, 15, 1), _cell(41, 7, 7)]),
}
TIE_VARIANTS = ("valid", "border", "border2")


def tie_case(placement, variant):
    """Row 0's 2D cell exists two or three times (``copies``, exact duplicates: bit-equal confidences in every mode), thr 0.1, border 2:
      valid    every copy is selectable                     -> the reference's "first true j" is the lowest copy; the lazy form decides it
      border   the lowest copy lies in the removed border    -> the next copy; the lazy form cannot decide it and raises count[1]
      border2  three copies, the first two in the border     -> the third; count[1] likewise
    Rows 1, 2, 3 are ordinary: the bottom-right corner (kept: only top rows and left columns are removed), a left-border cell
    (removed) and an interior cell.  So the lists are i = [0, 1, 3], j = [the copy, the corner, the interior cell].
    The ordinary cells lie in other column tiles than the copies, so that the tied logit (~42 among |logit| < 7) is the maximum of each
    of its tiles: the fast statistics pass sums a column against its TILE's maximum, and duplicate columns are bit-equal across tiles only
    where those references coincide.
    ``placement`` ``two_rows``: rows 5 and 133 (two row tiles, M = 72: every tile takes the exact sweep) are identical and both match
    cell (4, 4), as the reference's mask has it: i = [5, 133], j = [40, 40]."""
    g = torch.Generator().manual_seed(5)
    if placement == "two_rows":
        N, hc, wc = 140, 8, 9
        f3 = torch.randn(1, N, 256, generator=g) * 1.5
        f2 = torch.randn(1, hc * wc, 256, generator=g)
        f3[0, 133] = f3[0, 5]
        f2[0, 40] = f3[0, 5] * 1.5
        return dict(name="two_rows", f3=f3, f2=f2, kp=torch.randn(1, N, 3, generator=g), hc=hc, wc=wc, thr=0.1, border=2, mask=None, qscale=None,
                    copies=[40], rows=[5, 133], exempt_rows=(), exempt_cols=((0, 40),), lazy_flag=0)
    N, hc, wc, variants, ordinary = TIE_PLACEMENTS[placement]
    copies = variants[variant]
    f3 = torch.randn(1, N, 256, generator=g) * 1.5
    f2 = torch.randn(1, hc * wc, 256, generator=g)
    for j in copies:
        f2[0, j] = f3[0, 0] * 1.5
    for i, j in zip((1, 2, 3), ordinary):
        f2[0, j] = f3[0, i] * 1.5
    return dict(name=f"{placement}-{variant}", f3=f3, f2=f2, kp=torch.randn(1, N, 3, generator=g), hc=hc, wc=wc, thr=0.1, border=2, mask=None,
                qscale=None, copies=copies, rows=[0], exempt_rows=((0, 0),), exempt_cols=(), lazy_flag=int(variant != "valid"))


# --- wide logits --------------------------------------------------------------------------------------------------------------------
WIDE_ZERO_ROW, WIDE_ZERO_COL, WIDE_LOW_TILE = 77, 333, (128, 256)


def wide_case():
    """test_coarse_match_wide_logit_range's construction -- 24 pairs at logit ~110 among |logit| < 10, N = M = 512: 4 x 4 interior tiles,
    whose rows and columns far below a strong pair force the exact sweep -- plus a zero 3D row and a zero 2D cell (every logit exactly 0)
    and one whole column tile (128 .. 255) scaled by 0.01, so that its maximum (~1) sits more than 59 below its neighbours' references"""
    hc, wc, N = 16, 32, 512
    g = torch.Generator().manual_seed(11)
    f3 = torch.randn(1, N, 256, generator=g) * 1.5
    f2 = torch.randn(1, hc * wc, 256, generator=g)
    rows = torch.randperm(N, generator=g)[:24]
    cells = torch.randperm(hc * wc, generator=g)[:24]
    f2[0, cells] = f3[0, rows] * 4.0
    kp = torch.randn(1, N, 3, generator=g)
    f3[0, WIDE_ZERO_ROW] = 0.0
    f2[0, WIDE_ZERO_COL] = 0.0
    f2[0, WIDE_LOW_TILE[0]:WIDE_LOW_TILE[1]] *= 0.01
    return dict(name="wide", f3=f3, f2=f2, kp=kp, hc=hc, wc=wc, thr=0.1, border=2, mask=None, qscale=None, exempt_rows=(), exempt_cols=())


# --- comparison ---------------------------------------------------------------------------------------------------------------------
def rel_err(got, want, floor=1e-6):
    """max relative error over the elements of the reference above ``floor`` (0 if there is none)"""
    got, want = got.double(), want.double()
    big = want > floor
    return float(((got - want).abs() / want)[big].max()) if bool(big.any()) else 0.0


def assert_close(got, want, rtol, atol, what):
    got, want = got.double(), want.double()
    bad = (got - want).abs() > atol + rtol * want.abs()
    assert not bool(bad.any()), f"{what}: {int(bad.sum())} of {bad.numel()} outside rtol {rtol:g} / atol {atol:g}, max rel err {rel_err(got, want):.3e}"


def compare(got, ref_conf, ref, nsplit, bar=None):
    """One call's outputs -- ``conf`` (None: the lazy form stores no matrix) and the lists under the oracle's names, trimmed to the count
    -- against the reference of mode ``nsplit``: every list exactly, conf and mconf at ``bar`` (default ``BAR[nsplit]``).
    -> (conf, mconf) max rel err"""
    bar = BAR[nsplit] if bar is None else bar
    for k in LIST_KEYS:
        assert got[k].shape == ref[k].shape and torch.equal(got[k], ref[k]), f"{k}: {got[k].shape[0]} against the reference's {ref[k].shape[0]} entries, or other values"
    assert torch.equal(got["gt_mask"].bool(), ref["mconf"] == 0)
    assert_close(got["mconf"], ref["mconf"], what="mconf", **bar)
    if got["conf"] is not None:
        assert bool(torch.isfinite(got["conf"]).all()), "conf_matrix is not finite"
        assert_close(got["conf"], ref_conf, what="conf_matrix", **bar)
    return (rel_err(got["conf"], ref_conf) if got["conf"] is not None else 0.0), rel_err(got["mconf"], ref["mconf"])


def as_outputs(conf, sel):
    """a selection ``sel`` on the matrix ``conf`` in the form ``compare`` takes (the CPU stand-ins and wrong variants)"""
    return dict(conf=conf, gt_mask=sel["gt_mask"], mconf=sel["mconf"], **{k: sel[k] for k in LIST_KEYS})
