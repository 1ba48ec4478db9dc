"""The temporal refinement without a GPU: the numpy restatement of its specification (tests/temporal_oracle.py) on the analytic scene,
the header and binding of ``libonepose_temporal.so`` (what tests/test_cabi_binding.py does not state for every row of
``cabi.LIBRARIES``), its argument checks (which come before any HIP call, so they answer on a machine with no device) and the ``refine``
option of ``SequenceRunner``."""
import ctypes
import os
import re

import numpy as np
import pytest
import torch

from onepose_st_amd import frameloop as fl, hip, temporal
from tests import temporal_oracle as to

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
# the oracle's own maximum error on the pure-shift scene (seed 0, 3 levels, window 15, 60 points): 0.0290 px
SHIFT_MAX_ERROR = 0.0290


@pytest.fixture(scope="module")
def shift_scene():
    src, dst, pts, truth = to.scene("shift")
    return {"src": src, "dst": dst, "pts": pts, "truth": truth, "S": to.pyramid(src, 3), "D": to.pyramid(dst, 3)}


def test_oracle_tracks_the_pure_shift(shift_scene):
    """Measured on the committed seed: max error 0.0290 px (median 0.0115), forward-backward error at most 0.00097 px, at most 12
    iterations, no flag.  The bar is twice the measured maximum: the margin for the uint8 quantisation of the two images."""
    s = shift_scene
    out = to.track(s["S"], s["D"], s["pts"], window=15)
    err = np.linalg.norm(out["pts"] - s["truth"], axis=1)
    print("max", err.max(), "median", np.median(err), "fb", out["fb_error"].max(), "iterations", out["iterations"].max())
    assert (out["flags"] == 0).all(), out["flags"]
    assert abs(err.max() - SHIFT_MAX_ERROR) < 5e-4                  # the docstring's figure is this run's
    assert (err <= 2 * SHIFT_MAX_ERROR).all()
    assert out["fb_error"].max() < 0.01 and out["iterations"].max() <= 12


def test_oracle_needs_the_pyramid(shift_scene):
    """a 6.3 px shift against wavelengths from 6 px: one level leaves points more than 1 px off, three levels none"""
    s = shift_scene
    one = to.track(to.pyramid(s["src"], 1), to.pyramid(s["dst"], 1), s["pts"], window=15, fb_threshold=None)
    err = np.linalg.norm(one["pts"] - s["truth"], axis=1)
    assert (np.isnan(err) | (err > 1.0)).sum() >= 1
    three = to.track(s["S"], s["D"], s["pts"], window=15, fb_threshold=None)
    assert (np.linalg.norm(three["pts"] - s["truth"], axis=1) <= 2 * SHIFT_MAX_ERROR).all()


def test_oracle_planted_flags():
    src, dst, pts = to.planted_scene("shift")
    out = to.track(to.pyramid(src, 3), to.pyramid(dst, 3), pts[60:], window=15)
    assert out["flags"][0] == to.DEGENERATE and out["flags"][1] == to.OUT_OF_IMAGE and out["flags"][2] == to.BAD_INPUT
    assert out["flags"][3] & to.FB_FAIL and not out["flags"][3] & (to.LOST & ~to.FB_FAIL)
    assert np.isnan(out["pts"][:3]).all() and np.isfinite(out["pts"][3]).all()
    assert out["iterations"][2] == 0                                # BAD_INPUT samples nothing
    # a planted case far on the other side of the threshold: the same constant-patch point in the untouched source tracks cleanly
    clean = to.scene("shift")
    ok = to.track(to.pyramid(clean[0], 3), to.pyramid(clean[1], 3), pts[60:61], window=15)
    assert ok["flags"][0] == 0


def test_oracle_forward_backward_check_finds_the_foreign_patch():
    """The target's 33 x 33 neighbourhood of a true location is replaced by an unrelated texture.  Inside: the points whose whole
    level-0 window (15: +-7 px, +1 for the bilinear support) lies in the patch, a 5 x 5 grid of step 4 around its centre.  Outside: the
    scene points whose level-2 window cannot touch it (patch half 16 + 4 * 7 window + 8 px of blur support = 52 px from the centre).
    fb_threshold is 0.1 px here: two orders above the 0.001 px a clean track of this scene closes with, and below the O(1) px by which
    forward and backward minimise different functions once the two images are unrelated."""
    src, dst, pts, truth = to.scene("shift")
    centre_src = np.array([80.0, 60.0])
    cx, cy = (int(round(v)) for v in centre_src + np.array(to.SHIFT))
    other = to.Texture(77).image(*src.shape)
    dst = dst.copy()
    dst[cy - 16:cy + 17, cx - 16:cx + 17] = other[cy - 16:cy + 17, cx - 16:cx + 17]
    gx, gy = np.meshgrid([-8.0, -4.0, 0.0, 4.0, 8.0], [-8.0, -4.0, 0.0, 4.0, 8.0])
    inside = centre_src + np.stack([gx.ravel(), gy.ravel()], axis=1)
    far = pts[np.abs(truth - np.array([cx, cy])).max(axis=1) > 52]
    assert len(far) >= 4
    S, D = to.pyramid(src, 3), to.pyramid(dst, 3)
    a, b = to.track(S, D, inside, window=15, fb_threshold=0.1), to.track(S, D, far, window=15, fb_threshold=0.1)
    print("inside fb_error", a["fb_error"], "outside", b["fb_error"])
    assert ((a["flags"] & to.FB_FAIL) != 0).all(), a["flags"]
    assert (b["flags"] == 0).all(), b["flags"]


def test_collect_and_inject_order_on_a_hand_written_case():
    trans = np.array([[2.0, 0.0, -10.0], [0.0, 2.0, 4.0], [0.0, 0.0, 1.0]])
    own2 = np.array([[0, 0], [2, 2], [4, 4], [6, 6]], np.float32)
    own3 = np.arange(12, dtype=np.float32).reshape(4, 3)
    q, q3, k = to.collect(own2, own3, trans, count=3, mask=np.array([1, 0, 1, 1], np.uint8))
    assert k == 2 and np.array_equal(q, [[5.0, -2.0], [7.0, 0.0]]) and np.array_equal(q3, own3[[0, 2]])       # row 3 is past the count
    flags_a = np.array([0, to.DEGENERATE, to.FLAG_MAX_ITERS, to.FB_FAIL], np.int32)
    src_a = (100 + own3, np.array([[5.0, -2.0], [0, 0], [6.0, 0.0], [1, 1]]), flags_a, None)
    src_b = (200 + own3, np.array([[7.0, 1.0], [8.0, 2.0], [9, 9], [9, 9]]), np.array([to.OUT_OF_IMAGE, 0, 0, 0], np.int32), 2)
    src_c = (300 + own3, np.zeros((4, 2)), np.full(4, to.BAD_INPUT, np.int32), None)          # contributes nothing
    out2, out3, n = to.inject(own2, own3, 3, [src_a, src_b, src_c], trans)
    assert n == 3 + 2 + 1
    assert np.array_equal(out2, np.array([[0, 0], [2, 2], [4, 4], [0, 0], [2, 4], [6, 8]], np.float32))
    assert np.array_equal(out3, np.concatenate([own3[:3], 100 + own3[[0, 2]], 200 + own3[[1]]]))
    assert out2.dtype == np.float32 and out3.dtype == np.float32
    assert to.inject(own2, own3, 3, [src_a, src_b], trans, cap_total=4)[2] == 4


def test_crop_mapping_round_trip():
    K = np.array([[900.0, 0, 320.0], [0, 900.0, 240.0], [0, 0, 1]])
    _, trans = fl.crop_geometry([203, 117, 398, 345], K, 512)
    x = np.random.default_rng(3).uniform(0, 512, size=(200, 2))
    back = to.map_to_crop(trans, to.map_to_original(trans, x))
    assert np.abs(back - x).max() <= 1e-12
    assert np.abs(to.inverse3(trans) - np.linalg.inv(trans)).max() <= 1e-12
    general = np.array([[1.1, 0.2, 3.0], [-0.1, 0.9, -2.0], [1e-4, -2e-4, 1.0]])
    assert np.abs(to.inverse3(general) @ general - np.eye(3)).max() <= 1e-12


def test_header_and_binding():
    assert temporal.ABI_VERSION == 1
    assert (temporal.DEGENERATE, temporal.OUT_OF_IMAGE, temporal.FB_FAIL, temporal.BAD_INPUT, temporal.FLAG_MAX_ITERS, temporal.LOST) == \
        (to.DEGENERATE, to.OUT_OF_IMAGE, to.FB_FAIL, to.BAD_INPUT, to.FLAG_MAX_ITERS, to.LOST)
    assert temporal.LOST == temporal.DEGENERATE | temporal.OUT_OF_IMAGE | temporal.FB_FAIL | temporal.BAD_INPUT
    for shape in ((37, 53, 4), (2, 2, 1), (120, 160, 3), (1080, 1440, 6), (2, 2, 2), (37, 53, 7), (1, 9, 1), (16, 16, 5)):
        assert temporal.load().optmp_pyramid_bytes(*shape) == to.pyramid_bytes(*shape), shape
    assert to.pyramid_bytes(2, 2, 2) == 0 and to.pyramid_bytes(16, 16, 4) > 0 and to.pyramid_bytes(16, 16, 5) == 0
    mk = open(os.path.join(REPO, "onepose_st_amd", "csrc", "Makefile")).read()
    assert re.search(r"^TMP_FLAGS := -ffp-contract=off$", mk, re.M) and not re.search(r"^(SRCS|HDRS) :=.*temporal", mk, re.M)
    assert "#pragma clang fp contract(off)" in open(os.path.join(REPO, "onepose_st_amd", "csrc", "temporal_refine.hip")).read()


def test_rejected_calls_answer_before_any_launch():
    _PTR = ctypes.c_void_p(256)          # not null and never followed: every call below returns from its argument checks
    protos = temporal._BINDING.header.prototypes

    def args(name, **given):
        return [given.get(n, None if c.endswith("*") else 0) for c, n in protos[name].params]

    def last_error():
        return temporal.load().optmp_last_error().decode()

    for name in ("optmp_pyramid", "optmp_track", "optmp_collect", "optmp_inject"):
        with pytest.raises(ValueError, match="null pointer"):
            temporal.call(name, *args(name))
        assert last_error() == f"{name}: null pointer"
    ptrs = {n: _PTR for c, n in protos["optmp_track"].params if c.endswith("*") and n not in ("guess", "pts_3d", "pose", "K", "count", "stream")}
    good = dict(H=120, W=160, levels=3, cap=8, scale=1.0, window=15, max_iters=30, eps=0.01, min_eig_threshold=1.0, fb_threshold=1.0)
    for change, text in ((dict(window=14), "window: odd"), (dict(window=33), "window: odd"), (dict(levels=7), "levels in [1, 6]"),
                         (dict(H=9, W=9, levels=5), "smallest level"), (dict(cap=0), "cap outside"), (dict(max_iters=0), "max_iters outside"),
                         (dict(eps=0.0), "eps > 0"), (dict(min_eig_threshold=float("nan")), "eps > 0"), (dict(fb_threshold=float("nan")), "eps > 0"),
                         (dict(pts_3d=_PTR), "all three or none"), (dict(scale=0.0), "scale"), (dict(src=ctypes.c_void_p(8)), "256-byte aligned")):
        with pytest.raises(ValueError, match=re.escape(text)):
            temporal.call("optmp_track", *args("optmp_track", **{**ptrs, **good, **change}))
        assert text in last_error()
    pyr = dict(frame=_PTR, pyramid=_PTR, H=120, W=160, levels=3, pyramid_bytes=1 << 20)
    for change, text in ((dict(levels=0), "levels in [1, 6]"), (dict(H=1), "levels in [1, 6]"), (dict(pyramid_bytes=16), "pyramid too small"),
                         (dict(pyramid=ctypes.c_void_p(8)), "256-byte aligned")):
        with pytest.raises(ValueError, match=re.escape(text)):
            temporal.call("optmp_pyramid", *args("optmp_pyramid", **{**pyr, **change}))
    col = {n: _PTR for c, n in protos["optmp_collect"].params if c.endswith("*") and n not in ("count", "mask", "stream")}
    with pytest.raises(ValueError, match="cap outside"):
        temporal.call("optmp_collect", *args("optmp_collect", **col, cap=0))
    inj = {n: _PTR for n in ("own_2d", "own_3d", "trans", "out_2d", "out_3d", "out_count")}
    for change, text in ((dict(n_sources=9), "n_sources outside"), (dict(n_sources=1), "null source table"), (dict(cap_total=3), "cap_own <= cap_total")):
        with pytest.raises(ValueError, match=re.escape(text)):
            temporal.call("optmp_inject", *args("optmp_inject", **{**inj, "cap_own": 4, "cap_total": 8, **change}))


def test_python_api_refuses_cpu_tensors_and_bad_options():
    frame = torch.zeros(16, 16, dtype=torch.uint8)
    with pytest.raises(hip.HipLibraryError):
        temporal.build_pyramid(frame)
    with pytest.raises(hip.HipLibraryError):
        temporal.collect(torch.zeros(4, 2), torch.zeros(4, 3), np.eye(3))
    with pytest.raises(hip.HipLibraryError):
        temporal.inject(torch.zeros(4, 2), torch.zeros(4, 3), None, [], np.eye(3))
    a, b = temporal.Pyramid(torch.zeros(1024, dtype=torch.uint8), 16, 16, 1), temporal.Pyramid(torch.zeros(2048, dtype=torch.uint8), 16, 32, 1)
    with pytest.raises(hip.HipLibraryError):
        temporal.track(a, a, torch.zeros(4, 2, dtype=torch.float64))
    with pytest.raises(ValueError, match="mismatched pyramids"):
        temporal.track(a, b, torch.zeros(4, 2, dtype=torch.float64))
    with pytest.raises(TypeError):
        temporal.track(a, frame, torch.zeros(4, 2, dtype=torch.float64))
    assert tuple(temporal.Pyramid(torch.zeros(to.pyramid_bytes(37, 53, 4), dtype=torch.uint8), 37, 53, 4).level(3).shape) == (5, 7)


class _Model:
    """the fake matcher of tests/test_frameloop.py's kind: the true pose's projections of a few object points, in the crop"""

    def __init__(self, pts3d, poses, K):
        self.pts3d, self.poses, self.K, self.t, self.trans = pts3d, poses, K, 0, None

    def __call__(self, data):
        pose = self.poses[self.t]
        cam = pose[:, :3] @ self.pts3d.T + pose[:, 3:4]
        uv = self.K @ cam
        uv = (uv[:2] / uv[2:]).T
        uvc = (self.trans @ np.concatenate([uv, np.ones((len(uv), 1))], axis=1).T).T[:, :2]
        data["mkpts_3d_db"], data["mkpts_query_f"] = torch.tensor(self.pts3d, dtype=torch.float32), torch.tensor(uvc, dtype=torch.float32)
        self.t += 1


def test_sequence_runner_refine_option():
    g = np.random.default_rng(1)
    K = np.array([[900.0, 0, 320.0], [0, 900.0, 240.0], [0, 0, 1]])
    pts = g.uniform(-0.08, 0.08, size=(100, 3))
    bbox3d = 0.1 * np.array([[i, j, k] for i in (-1, 1) for j in (-1, 1) for k in (-1, 1)], dtype=np.float64)
    poses = [np.concatenate([np.eye(3), [[0.01 * t], [0.0], [0.8]]], axis=1) for t in range(3)]
    fake = _Model(pts, poses, K)
    block = {"keypoints3d": torch.zeros(1, 100, 3), "descriptors3d_db": torch.zeros(1, 128, 100), "descriptors3d_coarse_db": torch.zeros(1, 256, 100)}
    detector = lambda frame, t: fl.project_bbox(K, poses[t], bbox3d)

    def crop_fn(dev_frame, bbox, S):
        fake.trans = fl.crop_geometry(bbox, K, S)[1]
        return torch.zeros(1, 1, S, S)

    with pytest.raises(ValueError, match="refine='device' needs pnp='device'"):
        fl.SequenceRunner(fake, block, K, bbox3d, detector, refine="device", pnp="host")
    with pytest.raises(ValueError, match="refine='host'"):
        fl.SequenceRunner(fake, block, K, bbox3d, detector, refine="host", pnp="device")
    with pytest.raises(ValueError, match="temp_thresh"):
        fl.SequenceRunner(fake, block, K, bbox3d, detector, temp_thresh=0)
    runner = fl.SequenceRunner(fake, block, K, bbox3d, detector, crop_fn=crop_fn)
    assert runner.refine is None and runner.temp_thresh == 5 and runner.inliers_only is True
    recs = runner.run([np.zeros((480, 640), np.uint8)] * 3)
    assert len(recs) == 3
    for r in recs:
        assert set(r) == {"pose", "inliers", "bbox", "K_crop", "trans", "num_matches", "redetected"}
