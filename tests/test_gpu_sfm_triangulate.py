"""``onepose_st_amd/sfm_triangulate.py`` on the MI355X against ``tests/sfm_triangulate_oracle.py``.

Every integer output is exact (labels, ``point3D_ids``, ``point_ids``, the track tables, ``n_rounds``), ``xys`` is bit-equal, two runs
give identical bytes, nothing is set aside.  ``xyz`` and ``point_error`` are held to 16 times the spread of the oracle against itself
with every sum taken in reversed element order, measured on the CPU on these same scenes
(tests/test_sfm_triangulate_cpu.py::test_spread_of_reversed_sums; the figures live in tests/sfm_triangulate_scenes.py): spread 1.33e-15 scene units for ``xyz`` and 1.19e-13 px for
``point_error``, so the bounds are ``BOUND_XYZ`` = 2.13e-14 (5.3e-15 of the scenes' extent of 4, against the 1e-6 that would mean an
ill-conditioned formulation) and ``BOUND_ERR`` = 1.91e-12 px.  That the device's order of sums cannot flip a decision is the CPU file's
``min_margin >= 1e-6`` on every scene.

The scenes: ``hand`` (3 images, 2 points), ``exact`` (noise-free: ``xyz`` also against the planted points, not through the oracle),
``small`` (8 images, tracks of 2 to 8: all pairs; one point seen by one image, one behind a camera), ``medium`` (40 images; 24 and 23
elements on either side of 256 hypotheses; every sampled hypothesis there has the same inliers, so it runs the sampled path without
checking the draw), ``sampled`` (12 components of four chained points of 12 elements each: 48, 36 and 24 candidates, sampled in every
round, and the earliest sampled hypothesis decides which point a round takes: a wrong seed, draw or tie-break changes the integer
outputs, as the CPU file shows with seeded faults), ``long`` (63, 64 | 65, 130 elements: either side of the one-wavefront limit
``OPSTR_SHORT_TRACK`` = 64, the 130 by 90 images plus second slots within an image), ``chained`` (wrong rows: rounds 2 and 3, a tie
between hypotheses, leftovers that fail the angle filter), ``empty`` (``Q = 0``, a pair with no rows).

The file fails without the feature: the module, its header and its library do not exist.
"""
import numpy as np
import pytest
import torch

from tests import sfm_triangulate_oracle as orc
from tests.sfm_triangulate_scenes import BOUND_ERR, BOUND_XYZ, INT_KEYS, nearest_planted, reference, scene

pytestmark = pytest.mark.gpu


def to_device(d, dev="cuda:0"):
    return {k: torch.from_numpy(np.ascontiguousarray(v)).to(dev) for k, v in d.items()}


def run_device(s, **options):
    from onepose_st_amd import sfm_triangulate as tri

    model = tri.triangulate(to_device(s["merged"]), to_device(s["cameras"]), **options)
    torch.cuda.synchronize()
    return model, {k: (v.cpu().numpy() if isinstance(v, torch.Tensor) else v) for k, v in model.items()}


def compare(got, want):
    from onepose_st_amd import sfm_tracks as st

    assert set(st.MODEL_KEYS) <= set(got)
    for k in INT_KEYS:
        g, w = np.asarray(got[k]), np.asarray(want[k])
        assert g.shape == w.shape and g.dtype == w.dtype, (k, g.shape, w.shape, g.dtype, w.dtype)
        diff = int((g != w).sum())
        print(k, g.shape, "differing elements:", diff)
        assert diff == 0, k
    assert got["n_rounds"] == want["n_rounds"], (got["n_rounds"], want["n_rounds"])
    g, w = np.ascontiguousarray(got["xys"]), np.ascontiguousarray(want["xys"])
    assert g.shape == w.shape and g.dtype == w.dtype == np.float64 and int((g.view(np.int64) != w.view(np.int64)).sum()) == 0
    for k, bound in (("xyz", BOUND_XYZ), ("point_error", BOUND_ERR)):
        g, w = got[k], want[k]
        assert g.shape == w.shape and g.dtype == w.dtype == np.float64, (k, g.shape, w.shape)
        err = float(np.abs(g - w).max()) if g.size else 0.0
        print(k, g.shape, "max |err|", err, "bound", bound, "err / bound", err / bound)
        assert np.isfinite(g).all() and err <= bound, k


def check(name, **options):
    s = scene(name)
    want = reference(name, **options)
    _, got = run_device(s, **options)
    compare(got, want)
    return s, got, want


def test_hand_case():
    _, got, _ = check("hand")
    assert got["point3D_ids"].tolist() == [1, 2, 2, 1, 2, 1] and got["labels"].tolist() == [0, 1, 1, 0, 1, 0]
    assert got["track_offsets"].tolist() == [0, 3, 6] and got["track_kpt"].tolist() == [0, 1, 1, 1, 0, 0]
    assert np.abs(got["xyz"][1] - [0.0, 0.0, 5.0]).max() < 1e-12


def test_noise_free_scene_against_the_planted_points():
    s, got, _ = check("exact")
    d = nearest_planted(s, got)
    print("largest distance to a planted point", d.max(), "bound", BOUND_XYZ)
    assert len(got["xyz"]) == 12 and d.max() <= BOUND_XYZ


def test_small_scene():
    check("small")


def test_medium_scene_sampled_hypotheses():
    check("medium")


def test_sampled_hypotheses_decide_the_outcome():
    """Components of 48, 36 and 24 candidates whose four points tie: the earliest sampled hypothesis decides which point a round takes,
    so the seed (label and round), the draw of ``a`` and ``b`` and the tie-break all reach the integer outputs"""
    _, got, _ = check("sampled")
    assert got["n_rounds"] == 3 and len(got["xyz"]) == 36
    check("sampled", max_rounds=1)


def test_long_tracks():
    from onepose_st_amd import sfm_triangulate as tri

    assert tri.SHORT_TRACK == 64
    _, got, _ = check("long")
    assert sorted(np.diff(got["track_offsets"]).tolist()) == [63, 64, 65, 130]


def test_chained_components():
    _, got, _ = check("chained")
    assert got["n_rounds"] == 3
    check("chained", max_rounds=1)                                         # which of two tied hypotheses wins shows after one round


def test_empty_outcomes():
    _, got, _ = check("empty")
    assert got["xyz"].shape == (0, 3) and got["point_ids"].shape == (0,) and (got["point3D_ids"] == -1).all()


def test_two_runs_are_identical():
    for name in ("medium", "long", "chained"):
        _, a = run_device(scene(name))
        _, b = run_device(scene(name))
        for k in a:
            if isinstance(a[k], np.ndarray):
                assert a[k].tobytes() == b[k].tobytes(), (name, k)


def test_chain_from_pair_matches_to_the_optimiser_rows():
    """merge_pair_matches -> triangulate -> assign_tracks, matching_pairs, optimisation_rows on the device; the plan equals the one the
    sfm_tracks oracle makes from the triangulation oracle's model"""
    from onepose_st_amd import sfm_coarse, sfm_tracks as st, sfm_triangulate as tri
    from tests import sfm_tracks_oracle as torc

    s = scene("small")
    mg = s["merged"]
    ko, pim, po = mg["kpt_offsets"], mg["pair_images"], mg["pair_offsets"]
    row_pair = np.repeat(np.arange(len(po) - 1), np.diff(po))
    rng = np.random.default_rng(8)
    mk0 = mg["keypoints"][ko[pim[row_pair, 0]] + mg["match_ids"][:, 0]] + np.float32(0.25)          # the matcher's sub-pixel positions
    mk1 = mg["keypoints"][ko[pim[row_pair, 1]] + mg["match_ids"][:, 1]] + np.float32(0.75)
    conf = rng.uniform(0.2, 1.0, len(mk0)).astype(np.float32)
    dev = "cuda:0"
    merged = sfm_coarse.merge_pair_matches(torch.from_numpy(mk0).to(dev), torch.from_numpy(mk1).to(dev), torch.from_numpy(conf).to(dev),
                                           torch.from_numpy(po).to(dev), torch.from_numpy(pim).to(dev), len(ko) - 1)
    merged["pair_images"] = torch.from_numpy(pim).to(dev)
    cams = to_device(s["cameras"])
    model = tri.triangulate(merged, cams)
    plan = st.assign_tracks(model)
    pairs = st.matching_pairs(plan, model)
    rows = st.optimisation_rows(plan, model, pairs)
    torch.cuda.synchronize()
    want_model = orc.triangulate({k: merged[k].cpu().numpy() for k in tri.MERGED_KEYS}, s["cameras"])
    assert want_model["min_margin"] >= 1e-6                                # the merge only reorders the slots of the small scene
    compare({k: (v.cpu().numpy() if isinstance(v, torch.Tensor) else v) for k, v in model.items()}, want_model)
    assert len(want_model["xyz"]) == 61
    want = torc.vectorised_form({k: want_model[k] for k in st.MODEL_KEYS})
    got = {k: plan[k].cpu().numpy() for k in st.PLAN_KEYS}
    got.update({k: pairs[k].cpu().numpy() for k in st.PAIR_KEYS})
    got.update({k: rows[k].cpu().numpy() for k in st.ROW_KEYS})
    for k in ("keyframes", "state", "is_keyframe", "assigned_image", "assigned_kpt", "pair_left", "pair_right", "pair_offsets", "mkpts0_idx",
              "fine_row", "ref_image", "ref_kpt", "n_query", "row_offsets"):
        assert np.array_equal(got[k], want[k]) and got[k].dtype == want[k].dtype, k
    for k in ("mkpts0_c", "mkpts1_c"):
        assert got[k].tobytes() == want[k].tobytes(), k


def test_cpu_tensors_are_refused():
    from onepose_st_amd import hip, sfm_triangulate as tri

    s = scene("hand")
    with pytest.raises(hip.HipLibraryError):
        tri.triangulate({k: torch.from_numpy(v) for k, v in s["merged"].items()}, to_device(s["cameras"]))
