"""tests/x3_faithful.py on the CPU: what tests/test_gpu_encoder_x3.py relies on, shown for the reference and the stand-in ALONE.

  * the two-mask reference is the oracle's layer; the block decoders invert the kernels' element order (lane-level emulation);
  * every bar: the stand-in's figure, recomputed over exactly the committed cases, lies under its constant and above a quarter of it;
  * the row bars against today's ``LAYER_TOL["bf16x3"]``;
  * the reference separates a right kernel from wrong ones (``test_the_reference_separates_wrong_kernels``, figures in its docstring);
  * the exact-f32 layer: an f32 restatement stays inside ``f32_kv_slack`` and ``LAYER_TOL["f32"]``.
"""
import functools

import numpy as np
import pytest
import torch

from oracle import onepose_oracle as orc
from tests import bf16_faithful as bf
from tests import x3_faithful as xf

P = xf.LAYER
_SD = {}


def _label(shape, regime, mcase, cross):
    return f"B={shape[0]} L=({shape[1]},{shape[2]}) {regime} mask={None if mcase is None else '/'.join(map(str, mcase))} cross={cross}"


@functools.lru_cache(maxsize=None)
def _standin_figures(shape, regime, mcase, cross):
    sd = _SD["sd"]
    x3, x2 = xf.inputs(*shape, regime=regime)
    masks = (None, None) if mcase is None else xf.masks_of(mcase, *shape)
    y3, y2, blocks = xf.standin_streams(sd, P, x3, x2, cross, masks)
    f = xf.figures(sd, P, x3, x2, cross, masks, y3, y2, blocks)
    f["family"] = tuple(xf.block_family(regime, x.shape[1], m) for x, m in ((x3, masks[0]), (x2, masks[1])))
    return f


@pytest.fixture()
def figs(sd):
    _SD["sd"] = sd
    return _standin_figures


def test_reference_with_a_mask_on_each_stream_is_the_oracle(sd):
    """``reference_streams`` (float64, nothing rounded) = oracle.onepose_oracle.encoder_layer (f32) within 2e-5 with a mask on the first stream, on
    the second, on both; and each mask matters."""
    B, L3, L2 = 2, 48, 49
    x3, x2 = xf.inputs(B, L3, L2)
    for mcase in xf.MASK_CASES:
        m3, m2 = xf.masks_of(mcase, B, L3, L2)
        f3, f2 = (None if m is None else m.float() for m in (m3, m2))
        for cross in (False, True):
            y3, y2, _ = xf.reference_streams(sd, P, x3, x2, cross, (m3, m2))
            if cross:
                r3, r2 = orc.encoder_layer(sd, P, x3, x2, 8, x_mask=f3, source_mask=f2), orc.encoder_layer(sd, P, x2, x3, 8, x_mask=f2, source_mask=f3)
            else:
                r3, r2 = orc.encoder_layer(sd, P, x3, x3, 8, f3, f3), orc.encoder_layer(sd, P, x2, x2, 8, f2, f2)
            assert max((y3 - r3).abs().max().item(), (y2 - r2).abs().max().item()) <= 2e-5, (mcase, cross)
            u3, u2, _ = xf.reference_streams(sd, P, x3, x2, cross)
            assert m3 is None or (u3 - y3).abs().max().item() > 1e-2
            assert m2 is None or (u2 - y2).abs().max().item() > 1e-2


def test_kv_block_decoder_inverts_the_kernels_element_order():
    """``decode_kv_block`` on a block written as ``kv_tail`` -> ``kv_sum_w8_kernel`` write it: the slab from the lane-level emulation of the matrix
    instruction and the slab -> fragment rule of tests/test_packing_emulation_x3.py::test_kv_tail_slab_kv_sum_attention_chain (which pins that
    order against attn_apply's reads), the byte addresses of encoder_x3w8.hip:438-453.  Integer operands: everything is exact in bf16."""
    from tests.test_packing_emulation_x3 import C16, L64, NTT, Q, mfma16
    rng = np.random.default_rng(1)
    blk = torch.zeros(xf.KV_BLOCK_BYTES, dtype=torch.uint8)
    planes = blk[:xf.KV_FRAG_BYTES].view(torch.bfloat16)              # 8 bf16 per 16-byte lane slot
    ksf = blk[xf.KV_FRAG_BYTES:].view(torch.float32)
    KV, Ksum = torch.zeros(8, 32, 32), torch.zeros(8, 32)
    z = np.zeros((64, 4))
    for head in range(8):
        Kt, Vt = rng.integers(0, 4, (48, 32)).astype(float), rng.integers(-3, 4, (48, 32)).astype(float)      # [tok][d], [tok][v]
        # kk[ft][tt]: D[token 16 tt + 4 q + r][feature 16 ft + c16]
        kk = [[np.stack([[Kt[16 * tt + 4 * Q[l] + r, 16 * ft + C16[l]] for r in range(4)] for l in range(64)]) for tt in range(NTT)] for ft in range(2)]
        vv = [[np.stack([[Vt[16 * tt + 4 * Q[l] + r, 16 * ft + C16[l]] for r in range(4)] for l in range(64)]) for tt in range(NTT)] for ft in range(2)]
        for dt in range(2):
            for vt in range(2):
                a0, a1 = np.concatenate([kk[dt][0], kk[dt][1]], 1), np.concatenate([kk[dt][2], z], 1)
                b0, b1 = np.concatenate([vv[vt][0], vv[vt][1]], 1), np.concatenate([vv[vt][2], z], 1)
                kvt = mfma16(a1, b1, mfma16(a0, b0, np.zeros((64, 4))))
                for ln in range(64):                                    # kv_tail's store (:126), then kv_sum's e -> block address (:439-450)
                    e = (((head * 2 + dt) * 2 + vt) * 64 + ln) * 4
                    assert ((e >> 2) & 63, (e >> 8) & 1, (e >> 9) & 1, e >> 10) == (ln, vt, dt, head)
                    for plane, val in ((0, kvt[ln]), (1, kvt[ln] / 512)):                # a lo plane that is told apart
                        byte = (((head * 2 + vt) * 2 + plane) * 64 + ln) * 16 + 8 * dt
                        planes[byte // 2:byte // 2 + 4] = torch.from_numpy(val).to(torch.bfloat16)
            s = sum(kk[dt][tt].sum(1) for tt in range(NTT))
            for c in range(16):                                         # (:132) -> (:452): Ksum keeps its slab order
                ksf[head * 32 + 16 * dt + c] = float(s[(L64 & 15) == c].sum())
        KV[head], Ksum[head] = torch.from_numpy(Kt.T @ Vt).float(), torch.from_numpy(Kt.sum(0)).float()
    hi, lo, ksum = xf.decode_kv_block(blk)
    assert torch.equal(hi, KV) and torch.equal(lo, KV / 512) and torch.equal(ksum, Ksum)
    assert not torch.equal(KV, KV.transpose(1, 2))
    assert xf.KV_BLOCK_BYTES == 33792
    # the block follows the two slab sets at the next 256-byte ADDRESS
    pf = 2 * (1 + 2) * xf.KV_PART_FLOATS
    assert xf.kv_block_offset(0, 2, 48, 49) == 2 * pf * 4 and xf.kv_block_offset(512 + 64, 2, 48, 49) == 2 * pf * 4 + 192 and (2 * pf * 4) % 256 == 0


def test_f32_kv_block_decoder_inverts_the_kernels_element_order():
    """``decode_f32_kv_block`` on a block written as ``kv_reduce_kernel`` writes it (encoder.hip:75-90), from the emulation of the 32 x 32 x 2
    instruction (tests/mfma_emul.py)."""
    from tests import mfma_emul as E
    rng = np.random.default_rng(2)
    blk = torch.zeros(xf.F32_KV_FLOATS)
    KV, Ksum = torch.zeros(8, 32, 32), torch.zeros(8, 32)
    for head in range(8):
        Kt, Vt = rng.integers(0, 4, (32, 32)).astype(float), rng.integers(-3, 4, (32, 32)).astype(float)      # [tok][d], [tok][v]
        kacc, vacc = Kt[E.ROWS, E.R[:, None]], Vt[E.ROWS, E.R[:, None]]                                       # D[token acc_row(reg, h)][feature r]
        kv, ks = np.zeros((64, 16)), np.zeros((64, 16))
        for reg in range(16):
            kv = E.mfma_32x32x2(kacc[:, reg], vacc[:, reg], kv)
            ks = E.mfma_32x32x2(kacc[:, reg], np.ones(64), ks)
        o = blk[head * 1056:(head + 1) * 1056]
        for kb in range(4):
            o[kb * 256:(kb + 1) * 256] = torch.from_numpy(kv[:, 4 * kb:4 * kb + 4].reshape(-1)).float()
        for h in range(2):
            for reg in range(16):
                o[1024 + E.acc_row(reg, h)] = float(ks[32 * h, reg])
        KV[head], Ksum[head] = torch.from_numpy(Kt.T @ Vt).float(), torch.from_numpy(Kt.sum(0)).float()
    got_kv, got_ks = xf.decode_f32_kv_block(blk)
    assert torch.equal(got_kv, KV) and torch.equal(got_ks, Ksum) and not torch.equal(KV, KV.transpose(1, 2))
    assert xf.f32_kv_block_offset(2, 33, 65) == 2 * (2 + 3) * xf.F32_KV_FLOATS


def test_masks_of_the_cases():
    for B, L3, L2 in xf.MASK_SHAPES:
        for kind in xf.MASK_KINDS:
            m = xf.mask(kind, B, L2)
            n = m.sum(1)
            assert bool((n >= 1).all()) and bool((n < L2).all())
            if kind == "single":
                assert bool((n == 1).all())
            if kind == "last_wg":                      # every cell of the last workgroup is padding
                assert not bool(m[:, xf.TOK * ((L2 - 1) // xf.TOK):].any())
            if kind == "mid_tile":                     # the real cells end inside a workgroup
                assert bool((n % xf.TOK != 0).all())


def test_standin_figures_pin_the_bars(figs):
    """Each constant of tests/x3_faithful.py against the stand-in's figure over exactly the committed cases: under the constant, above a quarter."""
    sd = _SD["sd"]
    worst = dict(deep=0.0, many=0.0, outliers=0.0, one_term=0.0)
    rows = {k: dict(forced=0.0, free=0.0) for k in ("unit", "scaled")}
    for shape, regime, mcase in xf.layer_cases():
        for cross in (0, 1):
            f = figs(shape, regime, mcase, cross)
            print(f"{_label(shape, regime, mcase, cross)}: block {f['block'][0]:.2e} ({f['family'][0]}) {f['block'][1]:.2e} ({f['family'][1]}), deep "
                  f"{max(f['deep']):.2e}, rows forced {f['forced']:.2e} free {f['free']:.2e}")
            for s in (0, 1):
                worst[f["family"][s]] = max(worst[f["family"][s]], f["block"][s])
            worst["deep"] = max(worst["deep"], *f["deep"])
            rf = xf.rows_family(regime)
            rows[rf] = {k: max(rows[rf][k], f[k]) for k in rows[rf]}
    for shape in xf.KV_SHAPES:
        for x in xf.inputs(*shape):
            blk, ref, L = xf.standin_kv(sd, P, x), xf.reference_kv(sd, P, x), x.shape[1]
            e, d = max(xf.block_error(blk, ref, xf.kv_terms(sd, P, x))), max(xf.block_error(blk, ref, xf.kv_terms_deep(sd, P, x)))
            print(f"K / V half, L = {L}: block {e:.2e} deep {d:.2e}")
            fam = xf.block_family("randn", L, None)
            worst[fam], worst["deep"] = max(worst[fam], e), max(worst["deep"], d)
    print("worst block:", {k: f"{v:.3e}" for k, v in worst.items()}, "rows:", {r: {k: f"{v:.3e}" for k, v in d.items()} for r, d in rows.items()})
    for k, c in dict(xf.STANDIN_BLOCK, deep=xf.STANDIN_BLOCK_DEEP).items():
        assert c / 4 < worst[k] <= c, (k, worst[k], c)
    for r in rows:
        for k, c in (("forced", xf.STANDIN_ROWS_FORCED[r]), ("free", xf.STANDIN_ROWS_FREE[r])):
            assert c / 4 < rows[r][k] <= c, (r, k, rows[r][k], c)
    assert xf.BLOCK_BAR == {k: 2 * v for k, v in xf.STANDIN_BLOCK.items()} and xf.BLOCK_DEEP_BAR == 2 * xf.STANDIN_BLOCK_DEEP
    assert xf.ROWS_FORCED_BAR == {k: 2 * v for k, v in xf.STANDIN_ROWS_FORCED.items()} and xf.ROWS_FREE_BAR == {k: 2 * v for k, v in xf.STANDIN_ROWS_FREE.items()}


def test_row_bars_against_todays_layer_bar(figs):
    """On unit-variance inputs the stand-in, un-forced, needs at most HALF of today's 3e-4 / 1e-4 at every element of every layer case (so twice
    the stand-in fits under it: no case is ill-conditioned); and what ROWS_FREE_BAR alone allows is printed as a multiple of today's bar per
    element -- above 1 near ``ref = 0`` in rows with a large maximum, which is why the GPU tests assert today's bar as well."""
    sd = _SD["sd"]
    need, ratio = 0.0, 0.0
    for shape, regime, mcase in xf.layer_cases():
        if regime != "randn":
            continue
        for cross in (0, 1):
            x3, x2 = xf.inputs(*shape)
            masks = (None, None) if mcase is None else xf.masks_of(mcase, *shape)
            ys = xf.standin_streams(sd, P, x3, x2, cross, masks)[:2]
            rs = xf.reference_streams(sd, P, x3, x2, cross, masks)[:2]
            for y, r in zip(ys, rs):
                old = xf.OLD_ATOL + xf.OLD_RTOL * r.abs()
                need = max(need, ((y.double() - r).abs() / old).max().item())
                ratio = max(ratio, (xf.ROWS_FREE_BAR["unit"] * r.abs().amax(-1, keepdim=True).clamp(min=1.0) / old).max().item())
    print(f"stand-in error / today's bar, worst element: {need:.3f}; ROWS_FREE_BAR['unit'] / today's bar, worst element: {ratio:.2f}")
    assert need <= 0.5



WRONG_CASES = [((2, 48, 49), "randn", None), ((1, 96, 97), "randn", None), ((3, 49, 130), "randn", None), ((2, 48, 49), "down", None)]


def test_the_reference_separates_wrong_kernels(figs):
    """Each wrong kernel, as a variant of the stand-in, against the bar of the statistic that should see it; "factor" = its figure / that bar, the
    largest over WRONG_CASES x self, cross (slabs: the 65- and 129-slab streams).  Required: a factor of at least 2 somewhere.  Measured:

        lo.hi term dropped in the Q GEMM         rows forced   factor  6.6       lo.hi dropped in the K|V GEMM      block  factor 66
        lo.hi dropped in the merge GEMM          rows forced   factor  75        1 / L with L rounded up to 48      block  factor 1.4e4
        lo.hi dropped in the W0 GEMM             rows forced   factor  89        a token >= L counted in Ksum       block  factor 829
        lo.hi dropped in the W2 GEMM             rows forced   factor  92        last slab left out, 65 slabs       block  factor 103
        the block's lo plane dropped             rows forced   factor  17        last slab left out, 129 slabs      block  factor 64
        srclen of the other stream (cross)       rows forced   factor  112       a masked cell counted as a source  block  factor 1.1e4

    Every variant is detected; none had to be reported as not detectable at its bar."""
    sd = _SD["sd"]
    factors = {}
    for shape, regime, mcase in WRONG_CASES:
        x3, x2 = xf.inputs(*shape, regime=regime)
        for cross in (0, 1):
            for w in xf.WRONG_ROWS:
                if w == "srclen" and not cross:
                    continue
                y3, y2, blocks = xf.standin_streams(sd, P, x3, x2, cross, wrong=w)
                f = xf.figures(sd, P, x3, x2, cross, (None, None), y3, y2, blocks)
                factors[w] = max(factors.get(w, 0.0), f["forced"] / xf.ROWS_FORCED_BAR[xf.rows_family(regime)])
        for w in ("lohi_kv", "len48", "pad_in_ksum"):
            for x in (x3, x2):
                e = max(xf.block_error(xf.standin_kv(sd, P, x, wrong=w), xf.reference_kv(sd, P, x), xf.kv_terms(sd, P, x)))
                factors[w] = max(factors.get(w, 0.0), e / xf.BLOCK_BAR[xf.block_family(regime, x.shape[1], None)])
    for L, name in ((3073, "slab_out_65"), (6145, "slab_out_129")):
        x = xf.inputs(1, L, 1)[0]
        assert (L + xf.TOK - 1) // xf.TOK == int(name.split("_")[-1])
        e = max(xf.block_error(xf.standin_kv(sd, P, x, wrong="slab_out"), xf.reference_kv(sd, P, x), xf.kv_terms(sd, P, x)))
        factors[name] = e / xf.BLOCK_BAR["many"]
    for B, L3, L2 in xf.MASK_SHAPES:                                   # the first padded cell of batch element 0 counted
        x2 = xf.inputs(B, L3, L2)[1]
        m = xf.mask("mid_tile", B, L2)
        leak = m.clone()
        leak[0, int(m[0].sum())] = True
        e = max(xf.block_error(xf.standin_kv(sd, P, x2, leak), xf.reference_kv(sd, P, x2, m), xf.kv_terms(sd, P, x2, m)))
        factors["mask_leak"] = max(factors.get("mask_leak", 0.0), e / xf.BLOCK_BAR["many"])
    for k, v in factors.items():
        print(f"wrong kernel {k}: figure / bar = {v:.3g}")
    assert set(factors) == set(xf.WRONG_ROWS + xf.WRONG_BLOCK) - {"slab_out"} | {"slab_out_65", "slab_out_129"}
    low = {k: v for k, v in factors.items() if v < 2.0}
    assert not low, low


# ---- the exact-f32 layer ---------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("B,L3,L2", xf.F32_SHAPES)
def test_f32_restatement_stays_inside_the_slack_and_the_layer_bar(sd, B, L3, L2):
    """The un-rounded restatement in float32 (a stand-in of ``encoder.hip``) against the float64 reference: its block within half of
    ``f32_kv_slack`` (reasoning, not a measurement; the GPU test allows the whole of it), its rows within half of ``LAYER_TOL["f32"]``."""
    x3, x2 = xf.inputs(B, L3, L2)
    for cross in (False, True):
        r3, r2, kv = xf.reference_streams(sd, P, x3, x2, cross)
        s3, s2, skv = bf.coarse_streams_faithful(sd, P, x3, x2, cross, dtype=torch.float32, rounded=False)
        use = 0.0
        for s, x in enumerate((x3, x2)):
            slack = xf.f32_kv_slack(sd, P, x)
            use = max(use, ((skv[s][0].double() - kv[s][0]).abs() / slack[0]).max().item(), ((skv[s][1].double() - kv[s][1]).abs() / slack[1]).max().item())
        rows = max(((s.double() - r).abs() / (xf.F32_ATOL + xf.F32_RTOL * r.abs())).max().item() for s, r in ((s3, r3), (s2, r2)))
        print(f"f32 restatement B={B} L=({L3},{L2}) cross={cross}: block error / slack {use:.3f}, row error / bar {rows:.3f}")
        assert use <= 0.5 and rows <= 0.5
