"""The lazy ``conf_matrix`` form of the LoFTR matcher and the detector's batch planning, the parts that need no GPU: the config key and
the per-call keyword, the byte estimate (``coarse_batch_bytes``: host arithmetic over three size queries, answered here by a stand-in
library), the chunk planner and the detector's gate."""
import copy

import numpy as np
import pytest
import torch

from onepose_st_amd import detector, hip, loftr


class _SizeLib:
    """in place of the library handle: answers the size queries by formulas of the right shape and records every other entry"""

    def __init__(self):
        self.entered = []

    def ophip_encoder_x3w8_workspace_bytes(self, B, L0, L1):
        return 2048 * B * (L0 + L1) + 4096

    def ophip_encoder_full_stream_workspace_bytes(self, B, L, S):
        return 4 * B * L * S + 1024 * B * L + 4096

    def ophip_coarse_workspace_floats(self, B, L0, L1):
        return 40 * B * (L0 + L1) + 1024

    def ophip_coarse_sinkhorn_workspace_floats(self, B, L0, L1):
        return 48 * B * (L0 + L1) + B * L0 * L1 + 1024

    def __getattr__(self, name):
        return lambda *args: self.entered.append(name) or 0


@pytest.fixture()
def lib(monkeypatch):
    stand_in = _SizeLib()
    monkeypatch.setattr(hip._BINDING, "handle", stand_in)
    return stand_in


def _cfg(**top):
    c = copy.deepcopy(loftr.default_cfg)
    c.update(top)
    return c


def _sinkhorn_cfg(**top):
    c = _cfg(**top)
    c["match_coarse"]["match_type"] = "sinkhorn"
    return c


def test_config_key_values():
    assert loftr.default_cfg["hip_conf_matrix"] == "eager"
    assert loftr.LoFTR_for_OnePose_Plus().conf_matrix_mode == "eager"
    assert loftr.LoFTR_for_OnePose_Plus(_cfg(hip_conf_matrix="lazy")).conf_matrix_mode == "lazy"
    old = dict(_cfg())                                              # a plain dict written before the key existed
    assert "hip_conf_matrix" not in old and loftr.LoFTR_for_OnePose_Plus(old).conf_matrix_mode == "eager"
    with pytest.raises(KeyError):
        loftr.default_cfg["no_such_key"]
    for bad in ("Lazy", "", None, True, "off"):
        with pytest.raises(ValueError, match="hip_conf_matrix"):
            loftr.LoFTR_for_OnePose_Plus(_cfg(hip_conf_matrix=bad))
    with pytest.raises(ValueError, match="sinkhorn"):
        loftr.LoFTR_for_OnePose_Plus(_sinkhorn_cfg(hip_conf_matrix="lazy"))
    assert loftr.LoFTR_for_OnePose_Plus(_sinkhorn_cfg()).conf_matrix_mode == "eager"


def test_keyword_is_checked_before_anything_runs(lib):
    data = {"image0": torch.zeros(1, 1, 64, 80), "image1": torch.zeros(1, 1, 96, 128)}
    m = loftr.LoFTR_for_OnePose_Plus().eval()
    for bad in ("Lazy", "", None, 1):
        with pytest.raises(ValueError, match="conf_matrix"):
            m(dict(data), conf_matrix=bad)
    s = loftr.LoFTR_for_OnePose_Plus(_sinkhorn_cfg()).eval()
    with pytest.raises(ValueError, match="sinkhorn"):
        s(dict(data), conf_matrix="lazy")
    assert lib.entered == []                                        # no entry point was reached
    for mm, kw in ((m, {"conf_matrix": "lazy"}), (m, {"conf_matrix": "eager"}), (s, {"conf_matrix": "eager"})):
        with pytest.raises(hip.HipLibraryError):                    # a good value goes on to the input checks: host tensors, no CPU fallback
            mm(dict(data), **kw)
    assert lib.entered == []


GRIDS = ((8, 10), (12, 16))                                         # views of 64 x 80 against a query of 96 x 128
L0, L1 = 80, 192


@pytest.mark.parametrize("cfg", ["linear", "full", "sinkhorn"])
def test_coarse_batch_bytes(lib, cfg):
    c = _sinkhorn_cfg() if cfg == "sinkhorn" else _cfg()
    if cfg == "full":
        c["coarse"]["attention"] = "full"
    m = loftr.LoFTR_for_OnePose_Plus(c)
    prev = {True: 0, False: 0}
    for V in range(1, 18):
        lazy, eager = m.coarse_batch_bytes(V, *GRIDS, True), m.coarse_batch_bytes(V, *GRIDS, False)
        assert isinstance(lazy, int) and isinstance(eager, int)
        assert eager - lazy == 4 * V * L0 * L1                      # exactly the matrix
        assert lazy >= prev[True] and eager >= prev[False]          # non-decreasing in V
        prev = {True: lazy, False: eager}
        enc = lib.ophip_encoder_full_stream_workspace_bytes(V, L1, L1) if cfg == "full" else lib.ophip_encoder_x3w8_workspace_bytes(V, L0, L1)
        cws = 4 * (lib.ophip_coarse_sinkhorn_workspace_floats if cfg == "sinkhorn" else lib.ophip_coarse_workspace_floats)(V, L0, L1)
        rows = 4 * V * (L0 + L1) * 256 * 4
        assert lazy >= rows + enc + cws + 57 * V * L0               # every term of the documented sum is in it
        assert lazy <= rows + enc + cws + 128 * V * L0 + (1 << 16)  # and nothing of the matrix's order besides
    assert lib.entered == []                                        # three size queries and host arithmetic


def _check_plan(V, estimate, budget):
    chunks = detector.plan_chunks(V, estimate, budget)
    assert [i for a, b in chunks for i in range(a, b)] == list(range(V))          # consecutive, every view once
    assert all(b > a for a, b in chunks)
    for a, b in chunks:
        assert b - a == 1 or estimate(b - a) <= budget
    sizes = [b - a for a, b in chunks]
    assert all(s == sizes[0] for s in sizes[:-1]) and sizes[-1] <= sizes[0]
    if sizes[0] < V:                                                # the largest Vc that fits: one more view would not
        assert estimate(sizes[0] + 1) > budget
    return chunks


def test_chunk_planner(lib):
    m = loftr.LoFTR_for_OnePose_Plus()
    for lazy in (True, False):
        est = lambda n: m.coarse_batch_bytes(n, *GRIDS, lazy)
        for V in (1, 2, 4, 5, 15):
            assert _check_plan(V, est, 0) == [(i, i + 1) for i in range(V)]              # below one view's estimate: one view per call
            assert _check_plan(V, est, est(1) - 1) == [(i, i + 1) for i in range(V)]
            assert _check_plan(V, est, est(V)) == [(0, V)]
            assert detector.plan_chunks(V, est, None) == [(0, V)]                        # no limit
            for vc in range(1, V + 1):
                for budget in (est(vc), est(vc) + 1, est(vc + 1) - 1):
                    chunks = _check_plan(V, est, budget)
                    assert chunks[0] == (0, vc)
    assert _check_plan(4, est, est(2)) == [(0, 2), (2, 4)]
    assert _check_plan(5, est, est(2)) == [(0, 2), (2, 4), (4, 5)]
    assert _check_plan(7, lambda n: 10 * n, 35) == [(0, 3), (3, 6), (6, 7)]              # a pure function of (V, estimate, budget)


def test_detector_gate_and_budget():
    views = [np.zeros((64, 80), np.uint8)] * 4
    det = detector.LocalFeatureObjectDetector(None, views, device="cpu")
    assert det.batch_budget_bytes == 4 << 30                        # the documented default
    assert det.common_view_size() == (64, 80)                       # one size, not the query's 96 x 128: the batched path
    assert det.plans_batch() and det.plans_batch(True) and not det.plans_batch(False)
    mixed = detector.LocalFeatureObjectDetector(None, views[:3] + [np.zeros((64, 88), np.uint8)], device="cpu")
    assert mixed.common_view_size() is None and not mixed.plans_batch()              # mixed sizes: the loop
    single = detector.LocalFeatureObjectDetector(None, views[:1], device="cpu")
    assert single.common_view_size() == (64, 80) and not single.plans_batch()        # one view: nothing to batch
    assert detector.LocalFeatureObjectDetector(None, views, device="cpu", batch_budget_bytes=None).batch_budget_bytes is None
    assert detector.LocalFeatureObjectDetector(None, views, device="cpu", batch_budget_bytes=0).batch_budget_bytes == 0
    with pytest.raises(ValueError):
        detector.LocalFeatureObjectDetector(None, views, device="cpu", batch_budget_bytes=-1)


def test_detector_chunks_and_keywords_without_a_device(lib):
    """the batched form against a recording matcher: chunk boundaries, the lazy request and the b_ids offsets"""
    real = loftr.LoFTR_for_OnePose_Plus()

    class Recorder:
        config = real.config
        coarse_batch_bytes = real.coarse_batch_bytes

        def __init__(self):
            self.calls = []

        def __call__(self, data, **kw):
            V = data["image0"].shape[0]
            self.calls.append((V, tuple(data["image1"].shape), dict(kw)))
            data.update({"b_ids": torch.arange(V), "mkpts0_f": torch.zeros(V, 2), "mkpts1_f": torch.zeros(V, 2)})
    query = torch.zeros(1, 1, 96, 128)
    views = [np.zeros((64, 80), np.uint8)] * 5
    est2 = real.coarse_batch_bytes(2, *GRIDS, True)
    for budget, want in ((None, [5]), (4 << 30, [5]), (est2, [2, 2, 1]), (0, [1] * 5)):
        rec = Recorder()
        det = detector.LocalFeatureObjectDetector(rec, views, device="cpu", batch_budget_bytes=budget)
        parts = list(det._batched_matches(query))
        assert [c[0] for c in rec.calls] == want and [p[0].shape[0] for p in parts] == want
        assert all(c[1] == (1, 1, 96, 128) and c[2] == {"conf_matrix": "lazy", "budget_bytes": budget} for c in rec.calls)
        assert torch.cat([p[2] for p in parts]).tolist() == list(range(5))          # b_ids counted from view 0
    rec = Recorder()
    rec.config = _sinkhorn_cfg()                                    # sinkhorn needs the matrix: nothing is asked for
    list(detector.LocalFeatureObjectDetector(rec, views, device="cpu")._batched_matches(query))
    assert rec.calls == [(5, (1, 1, 96, 128), {})]
