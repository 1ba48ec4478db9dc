"""The triangulation oracle (tests/sfm_triangulate_oracle.py) and the input checks of ``onepose_st_amd/sfm_triangulate.py``, without a GPU.

The test scenes are those of tests/test_gpu_sfm_triangulate.py; what is derived here on the CPU and asserted, not measured there:

* every scene has ``min_margin >= 1e-6``: no decision of the specification lies within 1e-6 of its threshold, so the device's order of
  float sums cannot flip one (a condition on the committed seeds; no case is set aside);
* ``SPREAD_XYZ`` (scene units) and ``SPREAD_ERR`` (px) of tests/sfm_triangulate_scenes.py: the largest difference, over all scenes, of
  ``xyz`` and of ``point_error`` between the oracle and the oracle with every sum taken in reversed element order; the device test's
  bounds are 16 times these;
* the ``sampled`` scene tells the draws of the sampled hypotheses apart: a wrong draw, a seed without the round and a draw that does not
  skip ``a`` each change its outputs.
"""
import numpy as np
import pytest
import torch

from tests import sfm_triangulate_oracle as orc
from tests import sfm_triangulate_scenes as scenes
from tests.sfm_triangulate_scenes import BOUND_XYZ, INT_KEYS, SPREAD_ERR, SPREAD_XYZ, nearest_planted, reference, scene


def test_noise_free_scene_recovers_the_planted_points():
    s, m = scene("exact"), reference("exact")
    assert len(m["xyz"]) == len(s["planted"]["xyz"]) == 12 and m["n_rounds"] == 1
    d = nearest_planted(s, m)
    print("largest distance to a planted point", d.max())
    assert d.max() <= BOUND_XYZ
    for q, obs in enumerate(s["obs"]):                                     # every observation of a point carries one id
        assert len({int(m["point3D_ids"][slot]) for _, slot in obs}) == 1
    assert m["point_error"].max() < 1e-9


def test_second_round_recovers_the_chained_point():
    s, full, one = scene("chained"), reference("chained"), reference("chained", max_rounds=1)
    assert full["n_rounds"] == 3 and one["n_rounds"] == 1
    near_full, near_one = nearest_planted(s, full), nearest_planted(s, one)
    print("planted points found: all rounds", (near_full < 0.05).sum(), "one round", (near_one < 0.05).sum())
    assert (near_full[:8] < 0.05).all()                                    # the eight ordinary points, three of them chained 0-1-2
    assert (near_one[:3] < 0.05).sum() == 1 and (near_one[3:5] < 0.05).sum() == 1
    assert near_full[8] > 0.05                                             # the point of the two near cameras fails the angle filter
    narrow_slots = [slot for _, slot in s["obs"][8]]
    assert (full["point3D_ids"][narrow_slots] == -1).all()
    assert (full["labels"][narrow_slots] == full["labels"][s["obs"][0][0][1]]).all()


@pytest.mark.parametrize("name", sorted(scenes.SCENES))
def test_no_decision_near_its_threshold(name):
    m = reference(name)
    print(name, "min_margin", m["min_margin"])
    assert m["min_margin"] >= 1e-6


def test_spread_of_reversed_sums():
    worst, worst_err = 0.0, 0.0
    for name in sorted(scenes.SCENES):
        a, b = reference(name), reference(name, reverse=True)
        for k in INT_KEYS:
            assert np.array_equal(a[k], b[k]), (name, k)
        assert a["n_rounds"] == b["n_rounds"]
        if len(a["xyz"]):
            spread, spread_err = np.abs(a["xyz"] - b["xyz"]).max(), np.abs(a["point_error"] - b["point_error"]).max()
            print(name, "spread of xyz", spread, "of point_error", spread_err)
            worst, worst_err = max(worst, spread), max(worst_err, spread_err)
    print("largest spread", worst, worst_err, "bounds", 16 * worst, 16 * worst_err, "relative to the extent", 16 * worst / 4.0)
    assert worst <= SPREAD_XYZ and worst_err <= SPREAD_ERR and BOUND_XYZ <= 1e-6 * 4.0


def test_scene_shapes_cover_the_paths():
    small, medium, long_ = reference("small"), reference("medium"), reference("long")
    assert sorted(set(np.diff(small["track_offsets"]).tolist())) == [2, 3, 4, 5, 6, 7, 8] and len(small["xyz"]) == 61
    s = scene("small")
    assert (small["point3D_ids"][[slot for _, slot in s["obs"][61]]] == -1).all()                 # the point seen by one image
    behind = small["point3D_ids"][[slot for _, slot in s["obs"][60]]]
    assert behind[0] == behind[1] > 0 and behind[2] == -1                                          # the camera it lies behind stays out
    assert sorted(np.diff(medium["track_offsets"]).tolist())[:2] == [23, 24] and 24 * 23 // 2 > 256 >= 23 * 22 // 2
    assert sorted(np.diff(long_["track_offsets"]).tolist()) == [63, 64, 65, 130]
    assert len(set(long_["track_image"][long_["track_offsets"][2]:long_["track_offsets"][3]].tolist())) == 90
    empty = reference("empty")
    assert len(empty["xyz"]) == 0 and (empty["point3D_ids"] == -1).all() and empty["track_offsets"].tolist() == [0]


def test_sampled_scene_outputs_depend_on_the_draw():
    s, full, one = scene("sampled"), reference("sampled"), reference("sampled", max_rounds=1)
    G = scenes.SAMPLED_GROUPS
    sizes = np.bincount(full["labels"])
    assert sorted(sizes[sizes > 0].tolist()) == [4 * scenes.SAMPLED_TRACK] * G     # 48 candidates, then 36, then 24: every round samples
    assert 24 * 23 // 2 > 256 and full["n_rounds"] == 3
    assert len(full["xyz"]) == 3 * G and len(one["xyz"]) == G                       # a round takes one point of the four of a component
    assert set(np.diff(full["track_offsets"]).tolist()) == {scenes.SAMPLED_TRACK}
    near = nearest_planted(s, full) < 0.05
    missed = [int(np.nonzero(~near[4 * g:4 * g + 4])[0][0]) for g in range(G)]
    first = [int(np.nonzero((nearest_planted(s, one) < 0.05)[4 * g:4 * g + 4])[0][0]) for g in range(G)]
    print("the point three rounds leave over, per component", missed, "the point round 1 takes", first)
    assert all(near[4 * g:4 * g + 4].sum() == 3 for g in range(G))
    assert len(set(missed)) > 1 and len(set(first)) > 1                            # the draw's choice, not the scene's order
    for fault in ("wrong_draw", "seed_without_round", "draw_without_skip"):
        b = reference("sampled", fault=fault)
        assert not all(np.array_equal(full[k], b[k]) for k in INT_KEYS), fault


@pytest.mark.parametrize("name", ["hand", "exact", "small", "chained", "long", "sampled"])
def test_check_model_accepts_the_model(name):
    from onepose_st_amd import sfm_tracks as st

    m = reference(name)
    d = st.check_model({k: torch.from_numpy(np.ascontiguousarray(m[k])) for k in st.MODEL_KEYS})
    assert d["Q"] == len(m["xyz"]) and d["E"] == len(m["track_image"])


def test_hand_case():
    m = reference("hand")
    assert m["point3D_ids"].tolist() == [1, 2, 2, 1, 2, 1] and m["labels"].tolist() == [0, 1, 1, 0, 1, 0]
    assert m["track_image"].tolist() == [0, 1, 2, 0, 1, 2] and m["track_kpt"].tolist() == [0, 1, 1, 1, 0, 0]
    assert np.abs(m["xyz"][1] - [0.0, 0.0, 5.0]).max() < 1e-12 and np.abs(m["xyz"][0] - [0.6, 0.2, 4.0]).max() < 0.02
    assert m["point_error"][1] < 1e-10 and 0.1 < m["point_error"][0] < 1.0


def test_splitmix64_draw():
    # the first outputs of splitmix64 from the state 1234567, as published with the generator
    assert [orc.splitmix64(1234567, n) for n in range(3)] == [6457827717110365317, 3203168211198807973, 9817491932198370423]
    pairs = orc.hypothesis_pairs(30, 5, 1, 256)
    assert len(pairs) == 256 and all(0 <= a < 30 and 0 <= b < 30 and a != b for a, b in pairs)
    seed = 5 * 256 + 1
    assert pairs[0] == (orc.splitmix64(seed, 0) % 30, (lambda r, a: r + (r >= a))(orc.splitmix64(seed, 1) % 29, orc.splitmix64(seed, 0) % 30))
    assert orc.hypothesis_pairs(4, 0, 0, 256) == [(0, 1), (0, 2), (0, 3), (1, 2), (1, 3), (2, 3)]


@pytest.mark.parametrize("fault", orc.FAULTS)
def test_seeded_faults_change_the_outputs(fault):
    changed = []
    for name in sorted(scenes.SCENES):
        for rounds in (3, 1):                                              # one round: which of two tied points comes first shows
            a, b = reference(name, max_rounds=rounds), reference(name, fault=fault, max_rounds=rounds)
            same = all(np.array_equal(a[k], b[k]) for k in INT_KEYS + ("xyz", "xys", "point_error"))
            if not same:
                changed.append((name, rounds))
    print(fault, "changes", changed)
    assert changed


def _inputs(name="hand"):
    s = scene(name)
    return ({k: torch.from_numpy(v.copy()) for k, v in s["merged"].items()}, {k: torch.from_numpy(v.copy()) for k, v in s["cameras"].items()})


def test_input_checks():
    from onepose_st_amd import hip, sfm_triangulate as tri

    merged, cams = _inputs()
    d = tri.check_inputs(merged, cams)
    assert (d["I"], d["U"], d["T"], d["P"]) == (3, 6, 5, 3) and d["slot0"].tolist() == [1, 0, 1, 0, 3] and d["slot1"].tolist() == [2, 3, 4, 5, 5]
    with pytest.raises(hip.HipLibraryError):
        tri.triangulate(merged, cams)

    def broken(which, key, fn):
        m, c = _inputs()
        target = m if which == "merged" else c
        target[key] = fn(target[key])
        return m, c

    def poke(index, value):
        def fn(t):
            t = t.clone()
            t[index] = value
            return t
        return fn

    cases = [("merged", "keypoints", lambda t: t.double(), ValueError), ("merged", "keypoints", lambda t: t[:5], ValueError),
             ("merged", "kpt_offsets", poke(1, 5), ValueError), ("merged", "pair_offsets", poke(-1, 4), ValueError),
             ("merged", "keypoints", poke((0, 0), float("nan")), ValueError), ("cameras", "t", poke((0, 0), float("inf")), ValueError),
             ("cameras", "R", lambda t: t * 1.001, ValueError), ("cameras", "R", lambda t: -t, ValueError),
             ("cameras", "K", poke((0, 2, 2), 2.0), ValueError), ("cameras", "image_ids", poke(1, 7), ValueError),
             ("merged", "pair_images", poke((0, 1), 0), ValueError), ("merged", "pair_images", poke((0, 1), 3), IndexError),
             ("merged", "match_ids", poke((0, 0), 2), IndexError), ("merged", "match_ids", poke((0, 1), -1), IndexError),
             ("cameras", "K", lambda t: t.float(), ValueError)]
    for which, key, fn, exc in cases:
        with pytest.raises(exc):
            tri.check_inputs(*broken(which, key, fn))
    for bad in ({"max_hypotheses": 0}, {"max_rounds": 0}, {"refine_steps": -1}, {"max_reproj_error": float("nan")}, {"min_tri_angle": 200}):
        with pytest.raises(ValueError):
            tri.check_options(bad)
    with pytest.raises(TypeError):
        tri.check_options({"max_error": 1})
    assert tri.check_options({}) == tri.DEFAULTS == orc.DEFAULTS


def test_header_and_binding_agree():
    from onepose_st_amd import sfm_triangulate as tri

    assert tri.ABI_VERSION == 1 and tri.SHORT_TRACK == 64
    with pytest.raises(TypeError, match="takes 7 arguments"):
        tri.check_arity("opstr_components", (1, 2, 3))
