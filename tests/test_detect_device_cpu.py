"""Device detection without a GPU: the numpy oracle (``tests/detect_device_oracle.py``) against the host estimator on planted scenes, the
rules of the vote in the oracle, and the binding: the header parses, arities are checked, arguments are refused before the library is
loaded."""
import os
import sys

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import detect_device_oracle as orc  # noqa: E402

from onepose_st_amd import cabi, detect_device, detector, hip, pnp  # noqa: E402
from onepose_st_amd import frameloop as fl  # noqa: E402


@pytest.mark.parametrize("rows,seed", orc.HOST_SCENES)
def test_oracle_against_the_host_estimator(rows, seed):
    """3 views, 40 to 300 rows, noise at most 1 px, 30 % outliers at least 20 px off the model: the same inlier set, and the view's
    corners through both affinities within 1e-3 px (the bar: ``orc.CORNER_BAR``).  Measured: at most 3.1e-12 px."""
    sc = orc.planted_scene(rows, seed)
    out = orc.detect(sc["mk0"], sc["mk1"], sc["b_ids"], sc["view_hw"], orc.QUERY_HW, orc.SCENE_K)
    orc.assert_scene_condition(sc, out["affine"])
    for v, n in enumerate(rows):
        sel = sc["b_ids"] == v
        truth = orc.residuals(sc["truth"][v], sc["mk0"][sel], sc["mk1"][sel])
        assert ((truth <= 1.0) | (truth >= 20.0)).all() and abs(int((truth >= 20.0).sum()) - 0.3 * n) <= 0.5        # the scene is what it says
        A, inl = pnp.estimate_affine2d(sc["mk0"][sel], sc["mk1"][sel])
        assert A is not None and np.array_equal(inl[:, 0], out["mask"][sel]) and int(inl.sum()) == out["n_inliers"][v] == int((truth <= 1.0).sum())
        worst = max(abs(a - b) for p, q in zip(orc.corners_through(A.reshape(6), sc["view_hw"][v]), orc.corners_through(out["affine"][v], sc["view_hw"][v]))
                    for a, b in zip(p, q))
        print(f"rows {n}: {int(inl.sum())} inliers, corners through the oracle's and the host's affinity differ by {worst:.2e} px")
        assert worst < orc.CORNER_BAR
        # the host detector's box from its own affinity
        corners = (A @ np.array([[0, 0, 1], [640, 0, 1], [0, 480, 1], [640, 480, 1]], dtype=np.float64).T).T.astype(np.int32)
        assert out["boxes"][v].tolist() == [*corners.min(axis=0), *corners.max(axis=0)] and out["status"][v] == 0
    assert out["winner"] == int(np.argmax(rows))


@pytest.mark.parametrize("name", orc.RULES)
def test_rules_in_the_oracle(name):
    sc = orc.rule_scene(name)
    out = orc.detect(sc["mk0"], sc["mk1"], sc["b_ids"], sc["view_hw"], orc.QUERY_HW, orc.SCENE_K, trials=256)
    orc.check_rule(name, out)
    box, flag, K_crop, trans = out["state"]
    want_K, want_t = fl.crop_geometry(box, orc.SCENE_K, 512)
    assert np.allclose(K_crop, want_K, rtol=1e-12) and np.allclose(trans, want_t, rtol=1e-12)


def test_box_rules_one_at_a_time():
    assert orc.box_of(orc.NEGATIVE_CORNER_A, (480, 640)).tolist() == [10, -3, 330, 236]            # truncation toward zero, not floor
    assert orc.box_of([1.0, 0, -0.9, 0, 1.0, -0.9], (10, 10)).tolist() == [0, 0, 9, 9]
    assert orc.centre_box((480, 640)).tolist() == [320 - 500, 240 - 500, 320 + 500, 240 + 500]
    assert orc.centre_box((481, 641)).tolist() == [320 - 500, 240 - 500, 320 + 500, 240 + 500]
    for bad in ([4e6, 0, 0, 0, 1, 0], [1, 0, float("nan"), 0, 1, 0], [1, 0, 0, 0, 1, float("inf")], [1, 0, 0, 0, 1, -2147483649.0]):
        assert orc.box_of(bad, (480, 640)) is None
    assert orc.box_of([1, 0, 0, 0, 1, -2147483648.5], (480, 640)) is not None                      # truncates to INT32_MIN
    # the vote: most inliers, the first among equals; a degenerate winner takes the centre box, the others' boxes do not matter
    boxes = np.array([[5, 5, 5, 9], [1, 2, 30, 40], [3, 4, 50, 60]], dtype=np.int32)
    w, st, status = orc.vote(boxes, np.array([7, 9, 9]), np.zeros(3, np.int32), (480, 640), orc.SCENE_K, 512)
    assert w == 1 and st[0].tolist() == [1, 2, 30, 40] and st[1] == 0 and status.tolist() == [0, 0, 0]
    w, st, status = orc.vote(boxes, np.array([9, 9, 2]), np.zeros(3, np.int32), (480, 640), orc.SCENE_K, 512)
    assert w == 0 and st[0].tolist() == orc.centre_box((480, 640)).tolist() and status.tolist() == [orc.STATUS_DEGENERATE, 0, 0]
    w, _, _ = orc.vote(boxes, np.zeros(3, np.int32), np.zeros(3, np.int32), (480, 640), orc.SCENE_K, 512)
    assert w == 0
    # the sampler: three distinct rows, also in a view of three; a view below the floor runs no trials
    rng = np.array([[0, 3], [3, 8], [8, 14]], dtype=np.int32)
    smp = orc.sample(rng, 50, 2 ** 64 - 5, min_matches=6)
    assert (smp[:2] == -1).all() and all(len(set(t)) == 3 and min(t) >= 0 and max(t) < 6 for t in smp[2].tolist())
    assert all(sorted(t) == [0, 1, 2] for t in orc.sample(rng, 20, 1, min_matches=0)[0].tolist())
    assert orc.needs_more(5, 100, 0.99, 2048) and not orc.needs_more(70, 100, 0.99, 2048) and not orc.needs_more(100, 100, 0.99, 1)


def test_binding_reads_the_header_and_checks_arguments_before_loading(monkeypatch):
    dd = detect_device
    assert dd.ABI_VERSION == 1 and (dd.MAX_VIEWS, dd.DEFAULT_TRIALS, dd.MAX_TRIALS, dd.SCORE_CHUNK) == (256, 2048, 65536, 256)
    assert (dd.STATUS_NO_MODEL, dd.STATUS_DEGENERATE, dd.STATUS_NEEDS_MORE) == (orc.STATUS_NO_MODEL, orc.STATUS_DEGENERATE, orc.STATUS_NEEDS_MORE)
    entry, = [e for e in cabi.LIBRARIES if e.module == "detect_device"]
    assert (entry.prefix, entry.header, entry.so, entry.env) == ("opdet", "onepose_detect.h", "libonepose_detect.so", "OPDET_LIB")
    with pytest.raises(TypeError, match="takes 29 arguments"):
        dd.check_arity("opdet_detect", (1, 2, 3))
    with pytest.raises(TypeError, match="takes 6 arguments"):
        dd.check_arity("opdet_ranges", (1, 2, 3, 4, 5))

    def no_load():
        raise AssertionError("the library was loaded before the arguments were checked")
    monkeypatch.setattr(dd, "load", no_load)
    mk, ids, hw = torch.zeros(8, 2), torch.zeros(8, dtype=torch.int64), torch.tensor([[480, 640]], dtype=torch.int32)
    K = torch.eye(3, dtype=torch.float64)
    good = dict(mkpts0=mk, mkpts1=mk, b_ids=ids, view_hw=hw, query_hw=(480, 640), K=K)
    for change, match in ((dict(mkpts0=torch.zeros(8, 3)), "mkpts0 and mkpts1"), (dict(mkpts1=torch.zeros(7, 2)), "mkpts0 and mkpts1"),
                          (dict(mkpts0=mk.double()), "float32"), (dict(b_ids=ids.int()), "b_ids"), (dict(b_ids=ids[:5]), "b_ids"),
                          (dict(view_hw=hw.long()), "view_hw"), (dict(view_hw=torch.zeros(0, 2, dtype=torch.int32)), "view_hw"),
                          (dict(view_hw=torch.zeros(257, 2, dtype=torch.int32)), "view_hw"), (dict(query_hw=(0, 640)), "query_hw"),
                          (dict(K=K.float()), "K:"), (dict(K=torch.zeros(2, 3, dtype=torch.float64)), "K:"), (dict(crop_size=0), "crop_size"),
                          (dict(crop_size=dd.MAX_CROP + 1), "crop_size"), (dict(count=torch.zeros(1, dtype=torch.int64)), "count"),
                          (dict(trials=0), "trials"), (dict(trials=dd.MAX_TRIALS + 1), "trials"), (dict(ransac_reproj_threshold=0.0), "ransac_reproj_threshold"),
                          (dict(confidence=1.0), "confidence"), (dict(min_matches=-1), "min_matches")):
        with pytest.raises(ValueError, match=match):
            dd.vote(**{**good, **change})
    with pytest.raises(TypeError, match="mkpts0"):
        dd.vote(**{**good, "mkpts0": np.zeros((8, 2), np.float32)})
    with pytest.raises(hip.HipLibraryError, match="no CPU fallback"):           # well-formed CPU tensors: refused, never computed on the host
        dd.vote(**good)


class _NoState:
    def __call__(self, frame, t):
        return [0, 0, 4, 4]


class _WithState(_NoState):
    def detect_state(self, frame, K, crop_size):
        return None


def test_sequence_runner_and_detector_refuse_what_device_detection_cannot_use():
    block = {"keypoints3d": torch.zeros(1, 4, 3)}
    cube = np.zeros((8, 3))
    with pytest.raises(ValueError, match="detect='device' needs track='device'"):
        fl.SequenceRunner(None, block, np.eye(3), cube, _WithState(), detect="device")
    with pytest.raises(ValueError, match="detect='device' needs track='device'"):
        fl.SequenceRunner(None, block, np.eye(3), cube, _WithState(), pnp="device", detect="device")
    with pytest.raises(ValueError, match="needs a detector with detect_state"):
        fl.SequenceRunner(None, block, np.eye(3), cube, _NoState(), pnp="device", track="device", detect="device")
    with pytest.raises(ValueError, match="detect="):
        fl.SequenceRunner(None, block, np.eye(3), cube, _WithState(), detect="gpu")
    assert fl.SequenceRunner(None, block, np.eye(3), cube, _NoState()).detect == "host"
    # the detector: the device entries exist only with vote="device"
    lin = torch.nn.Linear(1, 1)
    views = [np.zeros((16, 24), np.uint8)] * 2
    host, dev = detector.LocalFeatureObjectDetector(lin, views), detector.LocalFeatureObjectDetector(lin, views, vote="device")
    assert host.vote == "host" and not hasattr(host, "detect_state") and not hasattr(host, "match_worker_device")
    assert dev.vote == "device" and callable(dev.detect_state) and callable(dev.match_worker_device)
    with pytest.raises(ValueError, match="vote="):
        detector.LocalFeatureObjectDetector(lin, views, vote="gpu")
    with pytest.raises(ValueError, match="detect='device' needs a detector"):
        fl.SequenceRunner(None, block, np.eye(3), cube, host, pnp="device", track="device", detect="device")
