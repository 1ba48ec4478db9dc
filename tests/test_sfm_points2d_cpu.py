"""The SfM coarse-match merge without a GPU: the oracle (tests/sfm_points2d_oracle.py) on a hand-worked case, its vectorised form
against its dict form, the input checks of ``sfm_coarse.merge_pair_matches`` and ``to_reference_outputs`` on a hand-built result."""
import numpy as np
import pytest
import torch

from onepose_st_amd import hip, sfm_coarse
from tests import sfm_points2d_oracle as so


def hand_case():
    """3 images, 3 pairs: (0, 1) with 3 rows, (0, 2) with none, (2, 1) with 2 rows.

    image 0: (1, 2) from rows 0 and 2 (0.5 + 0.25), (-1, 0) from row 1 (-1.2 truncates to -1)  -> [(1, 2) 0.75, (-1, 0) 0.5]
    image 1: (0, 3) from rows 0, 2 (-0.5 -> 0, 3.9 -> 3; 0.75), (4, 4) from rows 1, 3 (1.25), (9, 9) from row 4 (0.75)
             -> [(4, 4), (0, 3), (9, 9)]: the 0.75 tie in (x, y) order
    image 2: (5, 5) row 3 and (-6, 1) row 4, both 0.75 -> [(-6, 1), (5, 5)]: the tie with a negative x first"""
    mk0 = [[1.5, 2.2], [-1.2, 0.0], [1.9, 2.7], [5.0, 5.0], [-6.5, 1.0]]
    mk1 = [[-0.5, 3.9], [4.0, 4.0], [0.3, 3.1], [4.5, 4.9], [9.0, 9.0]]
    conf = [0.5, 0.5, 0.25, 0.75, 0.75]
    return (np.array(mk0, np.float32), np.array(mk1, np.float32), np.array(conf, np.float32), np.array([0, 3, 3, 5], np.int64),
            np.array([[0, 1], [0, 2], [2, 1]], np.int64), 3)


HAND_KEYPOINTS = [[1, 2], [-1, 0], [4, 4], [0, 3], [9, 9], [-6, 1], [5, 5]]
HAND_SCORES = [0.75, 0.5, 1.25, 0.75, 0.75, 0.75, 0.75]
HAND_OFFSETS = [0, 2, 5, 7]
HAND_IDS = [[0, 1], [1, 0], [0, 1], [1, 0], [0, 2]]


def test_oracle_on_the_hand_worked_case():
    r = so.oracle_merge(*hand_case())
    assert r["keypoints"].dtype == np.float32 and r["scores"].dtype == np.float32 and r["match_ids"].dtype == np.int64
    assert r["keypoints"].tolist() == HAND_KEYPOINTS
    assert r["scores"].tolist() == HAND_SCORES
    assert r["kpt_offsets"].tolist() == HAND_OFFSETS
    assert r["match_ids"].tolist() == HAND_IDS
    v = so.oracle_merge_vectorised(*hand_case())
    for k in r:
        assert np.array_equal(r[k], v[k]), k


def test_oracle_reference_dicts_of_the_hand_case():
    matches, names, pair_names = so.reference_dicts(*hand_case())
    kp = {n: so.merge_points(p) for n, p in so.match_to_points(matches, names).items()}
    ids = so.index_matches(matches, kp)
    assert ids["0 2"].shape == (0, 2) and ids["0 2"].dtype == np.int64
    assert ids["2 1"].tolist() == [[1, 0], [0, 2]]
    kpts, scores = so.to_arrays(kp)
    assert kpts["2"].tolist() == [[-6, 1], [5, 5]] and scores["1"].tolist() == [1.25, 0.75, 0.75]


def order_case(first_big: bool):
    """image 0: key (5, 5) seen in three pairs with mconf 1, 2^-53, 2^-53 (or the reverse order), key (0, 0) once with 1.0.  In float64,
    (1 + 2^-53) + 2^-53 = 1 (ties to even, twice) but (2^-53 + 2^-53) + 1 = 1 + 2^-52: the order decides whether (5, 5) ties (0, 0) --
    and then ranks after it -- or beats it"""
    tiny = 2.0 ** -53
    conf = [1.0, tiny, tiny] if first_big else [tiny, tiny, 1.0]
    mk0 = np.array([[5, 5], [5, 5], [5, 5], [1, 1]], np.float32)
    mk1 = np.array([[1, 1], [1, 1], [1, 1], [0, 0]], np.float32)
    return mk0, mk1, np.array(conf + [1.0], np.float32), np.array([0, 1, 2, 3, 4], np.int64), np.array([[0, 1], [0, 2], [0, 3], [1, 0]]), 4


def image0_ids(r):
    return r["match_ids"][:3, 0].tolist() + r["match_ids"][3:, 1].tolist()


def test_oracle_sums_in_occurrence_order():
    tie = so.oracle_merge(*order_case(True))
    assert tie["keypoints"][:2].tolist() == [[0, 0], [5, 5]] and image0_ids(tie) == [1, 1, 1, 0]
    win = so.oracle_merge(*order_case(False))
    assert win["keypoints"][:2].tolist() == [[5, 5], [0, 0]] and image0_ids(win) == [0, 0, 0, 1]
    for first_big in (True, False):
        v = so.oracle_merge_vectorised(*order_case(first_big))
        assert np.array_equal(v["match_ids"], (tie if first_big else win)["match_ids"])


def random_case(seed, n_images=12, n_pairs=40, max_rows=300, grid=8.0):
    rng = np.random.default_rng(seed)
    all_pairs = [(a, b) for a in range(n_images) for b in range(n_images) if a != b]
    pick = rng.choice(len(all_pairs), n_pairs, replace=False)
    pim = np.array([all_pairs[i] for i in pick], np.int64)
    rows = rng.integers(0, max_rows, n_pairs)
    rows[rng.random(n_pairs) < 0.1] = 0
    off = np.concatenate([[0], np.cumsum(rows)]).astype(np.int64)
    T = int(off[-1])
    scale = rng.uniform(0.6, 1.7, (n_images, 2)).astype(np.float32)
    pair_of_row = np.repeat(np.arange(n_pairs), rows)
    cells = lambda: rng.integers(-3, 40, (T, 2)).astype(np.float32) * np.float32(grid)
    mk0 = cells() * scale[pim[pair_of_row, 0]]
    mk1 = cells() * scale[pim[pair_of_row, 1]]
    conf = rng.uniform(0.2, 1.0, T).astype(np.float32)
    return mk0, mk1, conf, off, pim, n_images


@pytest.mark.parametrize("seed", [0, 1, 2])
def test_vectorised_oracle_equals_the_dict_oracle(seed):
    case = random_case(seed)
    try:
        a = so.oracle_merge(*case)
    except AssertionError:
        pytest.fail("the random case leaves an image without observations")
    b = so.oracle_merge_vectorised(*case)
    for k in a:
        assert a[k].dtype == b[k].dtype and np.array_equal(a[k], b[k]), k


# ---- input checks -----------------------------------------------------------------------------------------------------------------------
def _t(case):
    mk0, mk1, conf, off, pim, I = case
    return torch.from_numpy(mk0), torch.from_numpy(mk1), torch.from_numpy(conf), torch.from_numpy(off), torch.from_numpy(pim), I


def test_check_inputs_accepts_the_hand_case():
    assert sfm_coarse.check_inputs(*_t(hand_case())) == (5, 3, 3)


def test_cpu_tensors_raise_the_library_error():
    with pytest.raises(hip.HipLibraryError):
        sfm_coarse.merge_pair_matches(*_t(hand_case()))


def test_an_image_without_observations_raises_the_reference_assert():
    mk0, mk1, conf, off, pim, I = hand_case()
    with pytest.raises(AssertionError, match="corner-case n_kpts=0 not handled."):
        sfm_coarse.check_inputs(*_t((mk0, mk1, conf, off, pim, 4)))
    # image 2 only in the empty pair
    pim2 = np.array([[0, 1], [0, 2], [0, 1]], np.int64)
    with pytest.raises(AssertionError, match="corner-case"):
        sfm_coarse.check_inputs(*_t((mk0, mk1, conf, off, pim2, 3)))


def test_self_pair_raises_value_error():
    mk0, mk1, conf, off, pim, I = hand_case()
    pim = pim.copy()
    pim[1] = [2, 2]
    with pytest.raises(ValueError, match="both sides"):
        sfm_coarse.check_inputs(*_t((mk0, mk1, conf, off, pim, I)))


@pytest.mark.parametrize("bad", [-1, 3])
def test_image_index_outside_the_range_raises_index_error(bad):
    mk0, mk1, conf, off, pim, I = hand_case()
    pim = pim.copy()
    pim[2, 1] = bad
    with pytest.raises(IndexError):
        sfm_coarse.check_inputs(*_t((mk0, mk1, conf, off, pim, I)))


@pytest.mark.parametrize("where,value", [("mk0", np.nan), ("mk1", np.inf), ("mk0", -np.inf), ("conf", np.nan), ("conf", np.inf)])
def test_non_finite_values_raise_value_error(where, value):
    mk0, mk1, conf, off, pim, I = (a.copy() if isinstance(a, np.ndarray) else a for a in hand_case())
    {"mk0": mk0, "mk1": mk1, "conf": conf}[where].reshape(-1)[3] = value
    with pytest.raises(ValueError, match="non-finite"):
        sfm_coarse.check_inputs(*_t((mk0, mk1, conf, off, pim, I)))


@pytest.mark.parametrize("value,ok", [(2.0 ** 20 - 0.5, True), (-(2.0 ** 20) + 0.5, True), (2.0 ** 20, False), (-(2.0 ** 20), False),
                                      (3e9, False)])
def test_coordinate_range(value, ok):
    mk0, mk1, conf, off, pim, I = (a.copy() if isinstance(a, np.ndarray) else a for a in hand_case())
    mk1[4, 0] = value
    args = _t((mk0, mk1, conf, off, pim, I))
    if ok:
        sfm_coarse.check_inputs(*args)
    else:
        with pytest.raises(ValueError, match="truncates outside"):
            sfm_coarse.check_inputs(*args)


@pytest.mark.parametrize("off", [[0, 3, 3, 4], [1, 3, 3, 5], [0, 3, 2, 5]])
def test_malformed_offsets_raise_value_error(off):
    mk0, mk1, conf, _, pim, I = hand_case()
    with pytest.raises(ValueError, match="pair_offsets"):
        sfm_coarse.check_inputs(*_t((mk0, mk1, conf, np.array(off, np.int64), pim, I)))


def test_malformed_shapes_and_dtypes_raise_value_error():
    mk0, mk1, conf, off, pim, I = hand_case()
    with pytest.raises(ValueError):
        sfm_coarse.check_inputs(*_t((mk0.astype(np.float64), mk1, conf, off, pim, I)))
    with pytest.raises(ValueError):
        sfm_coarse.check_inputs(*_t((mk0[:4], mk1, conf, off, pim, I)))
    with pytest.raises(ValueError):
        sfm_coarse.check_inputs(*_t((mk0, mk1, conf, off, pim.astype(np.int32), I)))


# ---- reference outputs ---------------------------------------------------------------------------------------------------------------
def test_to_reference_outputs_on_a_hand_built_result():
    res = {"keypoints": torch.tensor(HAND_KEYPOINTS, dtype=torch.float32), "scores": torch.tensor(HAND_SCORES, dtype=torch.float32),
           "kpt_offsets": torch.tensor(HAND_OFFSETS), "match_ids": torch.tensor(HAND_IDS), "pair_offsets": torch.tensor([0, 3, 3, 5])}
    names = ["a", "b", "c"]
    kp, sc, um = sfm_coarse.to_reference_outputs(res, names, [("a", "b"), ("a", "c"), "c b"])
    assert list(kp) == names and list(sc) == names
    assert kp["b"].dtype == np.float32 and kp["b"].tolist() == [[4, 4], [0, 3], [9, 9]]
    assert sc["c"].tolist() == [0.75, 0.75]
    assert list(um) == ["a b", "a c", "c b"]
    assert um["a c"].shape == (0, 2) and um["a c"].dtype == np.int64
    assert um["a b"].tolist() == [[0, 1], [1, 0], [0, 1]] and um["c b"].tolist() == [[1, 0], [0, 2]]
    with pytest.raises(ValueError):
        sfm_coarse.to_reference_outputs(res, names[:2], [("a", "b"), ("a", "c"), "c b"])


def test_match_pairs_wants_the_coarse_only_matcher():
    class M:
        enable_fine_matching = True
    with pytest.raises(ValueError, match="enable_fine_matching=False"):
        sfm_coarse.match_pairs(M(), [], [(0, 1)])
