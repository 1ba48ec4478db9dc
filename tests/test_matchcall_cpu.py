"""onepose_st_amd/matchcall.py without a GPU: the pure ``plan_*`` step of the three calls, with CPU tensors.  Each plan names an entry of
include/onepose_hip.h and binds exactly that entry's header parameters (minus ``stream``), so a renamed header parameter, a forgotten
argument or a wrong entry choice fails here."""
import pytest
import torch

from onepose_st_amd import hip, matchcall as mc

B, N, HC, WC = 2, 7, 3, 4
M = HC * WC


def names(entry):
    return {n for _, n in hip.PROTOTYPES[entry].params} - {"stream"}


def lists(cap=B * N):
    return mc.MatchLists.empty(cap, "cpu")


def coarse(**kw):
    kw = {**dict(wc=WC, temperature=0.08, thr=0.1, border_rm=2, scale=8.0, nsplit=3, lists=lists(), conf=torch.empty(B, N, M),
                 workspace=torch.empty(16)), **kw}
    return mc.plan_coarse_match(torch.empty(B, N, 256), torch.empty(B, M, 256), torch.empty(B, N, 3), **kw), kw


QM, QS = torch.ones(B, M, dtype=torch.uint8), torch.ones(B, 2)
COARSE_ROWS = [(dict(query_mask=QM), "ophip_coarse_match_masked"), (dict(query_scale=QS, parts=1), "ophip_coarse_match_masked"),
               (dict(query_mask=QM, query_scale=QS, parts=2), "ophip_coarse_match_masked"),
               (dict(parts=1), "ophip_coarse_match_conf"), (dict(parts=2), "ophip_coarse_match_select"),
               (dict(parts=3), "ophip_coarse_match"), (dict(), "ophip_coarse_match"),
               (dict(parts=4), "ophip_coarse_match_masked"), (dict(parts=8), "ophip_coarse_match_masked")]


@pytest.mark.parametrize("kw,entry", COARSE_ROWS, ids=[f"{e[6:]}-{'-'.join(k) or 'default'}" for k, e in COARSE_ROWS])
def test_coarse_match_entry_and_names(kw, entry):
    (got, named), kw = coarse(**kw)
    assert got == entry and set(named) == names(entry)
    L = kw["lists"]
    for key, t in dict(conf=kw["conf"], workspace=kw["workspace"], b_ids=L.b_ids, i_ids=L.i_ids, j_ids=L.j_ids, mconf=L.mconf, mkpts3d=L.mk3d,
                       mkpts_c=L.mkc, m_bids=L.m_bids, gt_mask=L.gt_mask, count=L.count).items():
        assert named[key] is t, key                                        # supplied buffers by identity
    assert (named["B"], named["N"], named["M"], named["wc"], named["nsplit"], named["kpts_bstride"]) == (B, N, M, WC, 3, N * 3)
    if entry.endswith("_masked"):
        assert named["parts"] == kw.get("parts", 3) and named["query_mask"] is kw.get("query_mask") and named["query_scale"] is kw.get("query_scale")


def test_coarse_match_flag_bit_stride_and_what_c_refuses():
    (_, named), _ = coarse(planes_ready=True)
    assert named["nsplit"] == 3 | hip.COARSE_PLANES_READY
    (_, named), _ = coarse(nsplit=1)
    assert named["nsplit"] == 1
    (_, named), _ = coarse(kpts_bstride=0)
    assert named["kpts_bstride"] == 0
    shared = mc.plan_coarse_match(torch.empty(B, N, 256), torch.empty(B, M, 256), torch.empty(1, N, 3), wc=WC, temperature=0.08, thr=0.1,
                                  border_rm=2, scale=8.0, nsplit=3, lists=lists(), conf=None, workspace=None)[1]
    assert shared["kpts_bstride"] == 0                                     # hip.bstride: one object block for the batch
    (entry, named), _ = coarse(conf=None, nsplit=0)                        # the library refuses the lazy form in f32: the plan leaves it alone
    assert entry == "ophip_coarse_match" and named["conf"] is None and named["nsplit"] == 0


def coarse_2d(**kw):
    L0, L1 = 12, 20
    kw = {**dict(w0c=4, w1c=5, thr=0.2, border_rm=2, scale=8.0, lists=lists(B * L0), conf=torch.empty(B, L0, L1), workspace=torch.empty(16)), **kw}
    return mc.plan_coarse_match_2d(torch.empty(B, L0, 256), torch.empty(B, L1, 256), torch.empty(1, L0, 3), **kw), kw


MASKS = (torch.ones(B, 12, dtype=torch.bool), torch.ones(B, 20, dtype=torch.bool))
ROWS_2D = [(dict(temperature=0.1), "ophip_coarse_match_2d"), (dict(temperature=0.1, masks=MASKS), "ophip_coarse_match_2d_masked"),
           (dict(sinkhorn=(1.0, 3, 1)), "ophip_coarse_match_2d_sinkhorn"), (dict(sinkhorn=(1.0, 3, 1), masks=MASKS), "ophip_coarse_match_2d_sinkhorn_masked")]


@pytest.mark.parametrize("kw,entry", ROWS_2D, ids=[e[6:] for _, e in ROWS_2D])
def test_coarse_match_2d_entry_and_names(kw, entry):
    (got, named), kw = coarse_2d(**kw)
    assert got == entry and set(named) == names(entry)
    L = kw["lists"]
    assert named["conf"] is kw["conf"] and named["workspace"] is kw["workspace"] and named["mkpts0"] is L.mk3d and named["mkpts1_c"] is L.mkc
    assert named["count"] is L.count and named["m_bids"] is L.m_bids and named["gt_mask"] is L.gt_mask
    assert (named["B"], named["L0"], named["L1"], named["w0c"], named["w1c"], named["points_bstride"]) == (B, 12, 20, 4, 5, 0)
    if "sinkhorn" in kw:
        assert "temperature" not in named and "nsplit" not in named and (named["bin_score"], named["iters"], named["prefilter"]) == (1.0, 3, 1)
    else:
        assert named["temperature"] == 0.1 and named["nsplit"] == 3
    if "masks" in kw:
        assert named["mask0"] is MASKS[0] and named["mask1"] is MASKS[1]


def test_coarse_match_2d_leaves_what_c_refuses():
    (entry, named), _ = coarse_2d(temperature=0.1, masks=MASKS, nsplit=0)  # masks with nsplit 0: refused by the library, not here
    assert entry == "ophip_coarse_match_2d_masked" and named["nsplit"] == 0
    (entry, named), _ = coarse_2d(temperature=0.1, conf=None, nsplit=0)
    assert entry == "ophip_coarse_match_2d" and named["conf"] is None and named["nsplit"] == 0


FINE_ROWS = [(None, False, "ophip_fine_refine"), (None, True, "ophip_fine_refine_scaled"), (3, False, "ophip_fine_refine_bf16"),
             (1, True, "ophip_fine_refine_bf16_scaled")]


@pytest.mark.parametrize("by_lists", [True, False])
@pytest.mark.parametrize("nsplit,scaled,entry", FINE_ROWS, ids=[e[6:] for _, _, e in FINE_ROWS])
def test_fine_refine_entry_and_names(nsplit, scaled, entry, by_lists):
    cap, hf, wf = B * N, 12, 16
    ff, desc, L = torch.empty(B, 128, hf, wf), torch.empty(1, 128, N), lists()
    expec, mkf, wpack = torch.empty(cap, 3), torch.empty(cap, 2), torch.empty(8)
    src = dict(lists=L) if by_lists else dict(b_ids=L.b_ids, i_ids=L.i_ids, j_ids=L.j_ids, count=L.count, mkpts_c=L.mkc)
    got, named = mc.plan_fine_refine(ff, ff.stride(), hf, wf, desc, max_matches=cap, wpack=wpack, nlayers=2, cross_bits=2, encoder_enable=1,
                                     nsplit=nsplit, wc=WC, stride=4, fine_scale=5.0, expec_f=expec, mkpts_f=mkf,
                                     query_scale=QS if scaled else None, **src)
    assert got == entry and set(named) == names(entry)
    assert ("nsplit" in named) == (nsplit is not None) and named.get("nsplit") == nsplit
    assert (named["fs_b"], named["fs_c"], named["fs_y"], named["fs_x"]) == ff.stride() and (named["ds_b"], named["ds_c"]) == (0, N)
    for key, t in dict(feat_f=ff, desc3d_f=desc, b_ids=L.b_ids, i_ids=L.i_ids, j_ids=L.j_ids, count=L.count, mkpts_c=L.mkc, wpack=wpack,
                       expec_f=expec, mkpts_f=mkf).items():
        assert named[key] is t, key
    assert named["dbg_win"] is None and named["dbg_f3"] is None and named["max_matches"] == cap
    if scaled:
        assert named["query_scale"] is QS


def test_match_lists_empty_and_trim():
    L = mc.MatchLists.empty(10, "cpu", conf_shape=(2, 5, 6))
    assert [tuple(getattr(L, k).shape) for k in ("b_ids", "i_ids", "j_ids", "m_bids", "mconf", "mk3d", "mkc", "gt_mask", "count", "conf")] == \
        [(10,)] * 5 + [(10, 3), (10, 2), (10,), (4,), (2, 5, 6)]
    assert L.b_ids.dtype == L.m_bids.dtype == torch.int64 and L.gt_mask.dtype == torch.bool and L.count.dtype == torch.int32
    assert L.count.tolist() == [0, 0, 0, 0] and mc.MatchLists.empty(3, "cpu", count_ints=1).count.shape == (1,) and lists().conf is None
    got = L.trim(4)
    assert all(t.shape[0] == 4 and t.data_ptr() == getattr(L, k).data_ptr()
               for t, k in zip(got, ("b_ids", "i_ids", "j_ids", "m_bids", "gt_mask", "mconf", "mk3d", "mkc")))


def test_every_entry_of_the_two_stages_has_a_plan_and_a_converter():
    """the twelve entries and no more; the launch step's converters come from the header's C types, one per parameter but ``stream``"""
    planned = {e for _, e in COARSE_ROWS} | {e for _, e in ROWS_2D} | {e for _, _, e in FINE_ROWS}
    assert planned == {n for n in hip.PROTOTYPES if n.startswith(("ophip_coarse_match", "ophip_fine_refine"))}
    assert len(planned) == 12 and all(set(hip.converters(e)) == names(e) for e in planned) and mc.launch is hip.launch
    with pytest.raises(hip.HipLibraryError):                               # a CPU tensor reaches no kernel
        mc.launch(*coarse()[0])
