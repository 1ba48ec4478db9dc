"""The detector on views of one size against a query of another (the reference's 512 x 512 crops against a full frame, here 64 x 80
against 96 x 128) on the MI355X: the batched, chunked, lazy matcher calls against the view-by-view loop -- votes and ``DeviceDetection``
equal -- the number of matcher calls under each byte budget, the matcher's byte estimate against what its coarse stage allocates, and
views of mixed sizes."""
import numpy as np
import pytest
import torch

from onepose_st_amd import detector, hip, loftr
from onepose_st_amd.synthetic import make_synthetic_loftr_state_dict
from tests.loftr_helpers import planted_grids

pytestmark = pytest.mark.gpu

VIEW, QUERY = (64, 80), (96, 128)
G1 = (QUERY[0] // 8, QUERY[1] // 8)
DET_K = np.array([[300.0, 0, 64], [0, 300.0, 48], [0, 0, 1]])
# per view: (shift in coarse cells, noise).  Views 1 and 3 carry the query's content, view 1 best; 0 and 2 are unrelated (noise swamps the copy)
SCENE = (((0, 0), 3.0), ((2, 1), 0.1), ((0, 0), 3.0), ((3, 2), 0.25))


@pytest.fixture(scope="module")
def dev():
    if not torch.cuda.is_available():
        pytest.skip("needs the MI355X")
    hip.load()
    return torch.device("cuda:0")


@pytest.fixture(scope="module")
def matcher(dev):
    m = loftr.LoFTR_for_OnePose_Plus().eval()
    m.load_state_dict(make_synthetic_loftr_state_dict(0), strict=True)
    return m.to(dev)


class PlantedMatcher:
    """the detector's matcher with the planted scene behind it: a view is told by its grey level (view k is ``10 (k + 1)``), its planted
    features -- every pair with its own planted query, ``test_gpu_loftr.py``'s detector scene on two grid sizes -- go in through
    ``feature_hook``; counts the forward calls and what they were asked for"""

    def __init__(self, matcher, dev, view_sizes):
        self.matcher, self.dev, self.config, self.coarse_batch_bytes = matcher, dev, matcher.config, matcher.coarse_batch_bytes
        self.calls = []
        self.feats = []
        for k, ((shift, noise), hw) in enumerate(zip(SCENE, view_sizes)):
            x0, g0, x1, g1 = planted_grids((hw[0] // 8, hw[1] // 8), G1, shift_cells=shift, seed=20 + k, noise=noise)
            cl = lambda t: t.permute(0, 2, 3, 1).reshape(1, -1, 128).contiguous().to(dev)
            self.feats.append((x0.to(dev), cl(g0), x1.to(dev), cl(g1)))

    def parameters(self):
        return self.matcher.parameters()

    def __call__(self, data, **kw):
        ks = [int(round(v * 255.0 / 10.0)) - 1 for v in data["image0"][:, 0, 0, 0].tolist()]
        self.calls.append((ks, dict(kw)))
        self.matcher.feature_hook = lambda fc0, ff0, fc1, ff1: tuple(torch.cat([self.feats[k][n] for k in ks], 0) for n in range(4))
        try:
            self.matcher(data, **kw)
        finally:
            self.matcher.feature_hook = None


def _detector(matcher, dev, sizes=(VIEW,) * 4, **kw):
    pm = PlantedMatcher(matcher, dev, sizes)
    views = [np.full(hw, 10 * (k + 1), dtype=np.uint8) for k, hw in enumerate(sizes)]
    return detector.LocalFeatureObjectDetector(pm, views, **kw), pm


def _same_votes(got, want):
    assert sorted(got) == sorted(want) == list(range(len(want)))
    for k in want:
        assert np.array_equal(got[k]["bbox"], want[k]["bbox"]), k
        assert np.array_equal(np.asarray(got[k]["inliers"]), np.asarray(want[k]["inliers"])), k


def bits(a):
    return np.ascontiguousarray(a, dtype=np.float64).view(np.uint64)


def _device_outputs(d):
    host = lambda t: t.cpu().numpy()
    return dict(ranges=host(d.ranges), affine=host(d.affine), boxes=host(d.boxes), n_inliers=host(d.n_inliers), status=host(d.status),
                mask=host(d.inlier_mask), winner=int(host(d.winner)[0]), state=d.state.to_host(), votes=d.to_host())


def _same_detection(got, want):
    """every field exact or bit-equal, as ``test_gpu_detect_device.py`` compares them"""
    for k in ("ranges", "n_inliers", "status", "mask", "boxes"):
        assert np.array_equal(got[k], want[k]) and got[k].dtype == want[k].dtype, k
    assert np.array_equal(bits(got["affine"]), bits(want["affine"])) and got["winner"] == want["winner"]
    gs, ws = got["state"], want["state"]
    assert np.array_equal(gs[0], ws[0]) and gs[0].dtype == np.int32 and gs[1] == ws[1]
    assert np.array_equal(bits(gs[2]), bits(ws[2])) and np.array_equal(bits(gs[3]), bits(ws[3]))
    assert got["votes"][1] == want["votes"][1]
    _same_votes(got["votes"][0], want["votes"][0])


@pytest.fixture(scope="module")
def loop_results(matcher, dev):
    """the view-by-view loop on the scene, computed once: host votes and the device detection"""
    det, pm = _detector(matcher, dev, vote="device")
    query = torch.zeros(1, 1, *QUERY, device=dev)
    votes = det.match_worker(query, batched=False)
    assert [c[0] for c in pm.calls] == [[0], [1], [2], [3]] and all(c[1] == {} for c in pm.calls)
    det.plans_batch = lambda batched=True: False                    # the same detector forced onto the loop branch
    pm.calls.clear()
    dd = _device_outputs(det.match_worker_device(query, torch.as_tensor(DET_K).to(dev), 64))
    assert [c[0] for c in pm.calls] == [[0], [1], [2], [3]]
    n_in = [int(np.asarray(votes[k]["inliers"]).sum()) for k in range(4)]
    print(f"loop: inliers {n_in}, boxes {[votes[k]['bbox'].tolist() for k in range(4)]}")
    # a scene with something to vote on: two views that see the object, two that do not
    assert min(n_in[1], n_in[3]) >= 6 and max(n_in[1], n_in[3]) >= 12 and min(n_in[1], n_in[3]) > max(n_in[0], n_in[2])
    assert np.abs(votes[1]["bbox"] - np.array([16, 8, VIEW[1] + 16, VIEW[0] + 8])).max() <= 2
    return votes, dd


def _budget_for(matcher, vc):
    """a budget that admits ``vc`` views of the scene per call and not one more"""
    return matcher.coarse_batch_bytes(vc, (VIEW[0] // 8, VIEW[1] // 8), G1, True)


@pytest.mark.parametrize("budget,calls", [("default", [[0, 1, 2, 3]]), (None, [[0, 1, 2, 3]]), (2, [[0, 1], [2, 3]]), (3, [[0, 1, 2], [3]]),
                                          (0, [[0], [1], [2], [3]])], ids=["default", "unlimited", "two_views", "three_views", "zero"])
def test_batched_equals_loop_under_every_budget(matcher, dev, loop_results, budget, calls):
    kw = {} if budget == "default" else {"batch_budget_bytes": budget if budget in (None, 0) else _budget_for(matcher, budget)}
    det, pm = _detector(matcher, dev, vote="device", **kw)
    assert det.plans_batch()
    query = torch.zeros(1, 1, *QUERY, device=dev)
    want = {"conf_matrix": "lazy", "budget_bytes": det.batch_budget_bytes}
    votes = det.match_worker(query)
    assert [c[0] for c in pm.calls] == calls and all(c[1] == want for c in pm.calls)          # the batched path was taken, lazily
    _same_votes(votes, loop_results[0])
    pm.calls.clear()
    d = det.match_worker_device(query, torch.as_tensor(DET_K).to(dev), 64)
    assert [c[0] for c in pm.calls] == calls and all(c[1] == want for c in pm.calls)
    _same_detection(_device_outputs(d), loop_results[1])


def test_estimate_bounds_what_the_coarse_stage_allocates(matcher, dev, monkeypatch):
    """for the chunks the detector runs (two views, then a budget of one call for all four): the peak of allocated bytes inside the
    matcher's ``_coarse``, above what was live on entry (the features it is handed), is at most ``coarse_batch_bytes``"""
    seen = []
    real = matcher._coarse

    def measured(Wb, fc0, fc1, hw0_c, hw1_c, scale, s0, s1, masks, lazy=False, budget=None):
        torch.cuda.synchronize()
        torch.cuda.reset_peak_memory_stats()
        start = torch.cuda.memory_allocated()
        out = real(Wb, fc0, fc1, hw0_c, hw1_c, scale, s0, s1, masks, lazy, budget)
        torch.cuda.synchronize()
        seen.append((fc0.shape[0], tuple(hw0_c), tuple(hw1_c), lazy, torch.cuda.max_memory_allocated() - start))
        return out
    monkeypatch.setattr(matcher, "_coarse", measured)
    query = torch.zeros(1, 1, *QUERY, device=dev)
    for vc in (2, 4):
        det, pm = _detector(matcher, dev, batch_budget_bytes=_budget_for(matcher, vc))
        det.match_worker(query)
        assert len(pm.calls) == 4 // vc
    assert [s[0] for s in seen] == [2, 2, 4]
    for V, hw0_c, hw1_c, lazy, peak in seen:
        est = matcher.coarse_batch_bytes(V, hw0_c, hw1_c, lazy)
        print(f"V={V} {hw0_c} x {hw1_c} lazy={lazy}: _coarse peak {peak} bytes, estimate {est}")
        assert lazy and hw0_c == (8, 10) and hw1_c == (12, 16) and 0 < peak <= est
    # and the eager form of one call, the estimate's other branch
    seen.clear()
    pm = PlantedMatcher(matcher, dev, (VIEW,) * 4)
    pm({"image0": torch.cat([torch.full((1, 1, *VIEW), 10 * (k + 1) / 255.0, device=dev) for k in range(4)], 0), "image1": query})
    (V, hw0_c, hw1_c, lazy, peak), = seen
    est = matcher.coarse_batch_bytes(V, hw0_c, hw1_c, False)
    print(f"V={V} eager: _coarse peak {peak} bytes, estimate {est}")
    assert not lazy and V == 4 and 4 * V * 80 * 192 < peak <= est


def test_mixed_view_sizes_take_the_loop(matcher, dev):
    sizes = (VIEW, VIEW, (64, 88), VIEW)
    det, pm = _detector(matcher, dev, sizes, vote="device")
    assert not det.plans_batch() and det.common_view_size() is None
    query = torch.zeros(1, 1, *QUERY, device=dev)
    votes = det.match_worker(query)
    assert [c[0] for c in pm.calls] == [[0], [1], [2], [3]] and all(c[1] == {} for c in pm.calls)
    loop = det.match_worker(query, batched=False)
    _same_votes(votes, loop)
    n_in = [int(np.asarray(votes[k]["inliers"]).sum()) for k in range(4)]
    assert min(n_in[1], n_in[3]) >= 6 and max(n_in[1], n_in[3]) >= 12 and min(n_in[1], n_in[3]) > max(n_in[0], n_in[2])
    pm.calls.clear()
    d = det.match_worker_device(query, torch.as_tensor(DET_K).to(dev), 64)
    assert [c[0] for c in pm.calls] == [[0], [1], [2], [3]]
    host_votes, winner = d.to_host()
    assert sorted(host_votes) == [0, 1, 2, 3] and winner in (1, 3) and d.n_inliers.cpu().tolist()[winner] >= 12
