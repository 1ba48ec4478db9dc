"""The SfM coarse-match merge on the MI355X (run with ``-m gpu``): ``sfm_coarse.merge_pair_matches`` bit-exact against the oracle
(tests/sfm_points2d_oracle.py) -- keypoints, scores as float32 bits, match_ids and per-image counts -- on the hand-worked case, a seeded
realistic case, planted ties, order-dependent sums, truncation, an image seen only as img1, one image with more than 100 k keys and
2T above 2^24; two runs bitwise equal; ``match_pairs`` batched against one matcher call per pair; ``detector_free_coarse_matching``
against the oracle on the per-pair matches."""
import numpy as np
import pytest
import torch

from onepose_st_amd import hip, sfm_coarse
from onepose_st_amd.synthetic import make_synthetic_loftr_state_dict
from tests import sfm_points2d_oracle as so
from tests.loftr_helpers import planted_grids
from tests.test_sfm_points2d_cpu import HAND_IDS, HAND_KEYPOINTS, hand_case, order_case

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def dev():
    if not torch.cuda.is_available():
        pytest.skip("needs the MI355X")
    hip.load()
    return torch.device("cuda:0")


def run(dev, case):
    mk0, mk1, conf, off, pim, I = case
    t = lambda a: torch.from_numpy(np.ascontiguousarray(a)).to(dev)
    r = sfm_coarse.merge_pair_matches(t(mk0), t(mk1), t(conf), t(off), t(pim), I)
    torch.cuda.synchronize()
    return {k: v.cpu().numpy() for k, v in r.items()}


def assert_bit_exact(got, want, what=""):
    assert got["kpt_offsets"].tolist() == want["kpt_offsets"].tolist(), f"{what}: per-image counts"
    assert got["keypoints"].dtype == np.float32 and np.array_equal(got["keypoints"].view(np.uint32), want["keypoints"].view(np.uint32)), \
        f"{what}: keypoints"
    assert got["scores"].dtype == np.float32 and np.array_equal(got["scores"].view(np.uint32), want["scores"].view(np.uint32)), \
        f"{what}: scores"
    assert got["match_ids"].dtype == np.int64 and np.array_equal(got["match_ids"], want["match_ids"]), f"{what}: match_ids"


def realistic_case(seed=5, n_images=60, n_pairs=600, max_rows=3000):
    """keypoints on coarse grids (8 px cells, image 480 x 640) times per-image float scales, so that truncation matters; ~10 % empty
    pairs; every image in some non-empty pair"""
    rng = np.random.default_rng(seed)
    all_pairs = [(a, b) for a in range(n_images) for b in range(n_images) if a != b]
    pim = np.array([all_pairs[i] for i in rng.choice(len(all_pairs), n_pairs, replace=False)], np.int64)
    rows = rng.integers(1, max_rows + 1, n_pairs)
    rows[rng.random(n_pairs) < 0.1] = 0
    covered = np.zeros(n_images, bool)
    covered[pim[rows > 0].reshape(-1)] = True
    for g in np.flatnonzero(~covered):
        rows[np.flatnonzero((pim == g).any(1))[0]] = 50
    off = np.concatenate([[0], np.cumsum(rows)]).astype(np.int64)
    T = int(off[-1])
    scale = rng.uniform(0.55, 1.8, (n_images, 2)).astype(np.float32)
    pr = np.repeat(np.arange(n_pairs), rows)
    cells = lambda: np.stack([rng.integers(0, 80, T), rng.integers(0, 60, T)], 1).astype(np.float32) * np.float32(8)
    mk0 = cells() * scale[pim[pr, 0]]
    mk1 = cells() * scale[pim[pr, 1]]
    conf = rng.uniform(0.2, 1.0, T).astype(np.float32)
    return mk0, mk1, conf, off, pim, n_images


def test_hand_worked_case(dev):
    got = run(dev, hand_case())
    assert got["keypoints"].tolist() == HAND_KEYPOINTS and got["match_ids"].tolist() == HAND_IDS
    assert_bit_exact(got, so.oracle_merge(*hand_case()), "hand case")


def test_realistic_case_and_determinism(dev):
    case = realistic_case()
    assert 500_000 < len(case[2]) and len(case[4]) == 600
    want = so.oracle_merge(*case)
    a = run(dev, case)
    assert_bit_exact(a, want, "realistic")
    b = run(dev, case)
    for k in a:
        assert np.array_equal(a[k], b[k]), f"second run differs: {k}"


def test_planted_exact_ties_with_negative_x(dev):
    """every key of image 0 scores exactly 1.5 (three 0.5 observations in different pairs); x from -40 to 40: the ranks must follow
    signed (x, y) order"""
    rng = np.random.default_rng(2)
    xs = rng.permutation(np.arange(-40, 41)).astype(np.float32)
    keys = np.stack([xs + 0.25, (-xs * 0.5).astype(np.float32) + 0.75], 1).astype(np.float32)
    mk0 = np.concatenate([keys, keys[::-1], keys[rng.permutation(len(keys))]], 0)
    mk1 = rng.integers(-5, 5, (len(mk0), 2)).astype(np.float32) + 0.5
    conf = np.full(len(mk0), 0.5, np.float32)
    n = len(keys)
    case = (mk0, mk1, conf, np.array([0, n, 2 * n, 3 * n], np.int64), np.array([[0, 1], [0, 2], [0, 3]], np.int64), 4)
    want = so.oracle_merge(*case)
    kp0 = want["keypoints"][:want["kpt_offsets"][1]]
    assert (want["scores"][:len(kp0)] == 1.5).all() and kp0[:, 0].tolist() == sorted(kp0[:, 0].tolist()) and kp0[0, 0] < 0
    assert_bit_exact(run(dev, case), want, "ties")


@pytest.mark.parametrize("first_big", [True, False])
def test_order_dependent_sums(dev, first_big):
    case = order_case(first_big)
    want = so.oracle_merge(*case)
    got = run(dev, case)
    assert_bit_exact(got, want, "order")
    assert got["keypoints"][:2].tolist() == ([[0, 0], [5, 5]] if first_big else [[5, 5], [0, 0]])


def test_order_dependent_sums_spread_over_many_pairs(dev):
    """1.0 and many 2^-53 / 2^-30 / 2^-60 terms on one key, spread over pairs in a fixed order, against a rival key at exactly the
    float64 sum the wrong order would give"""
    tiny = [1.0] + [2.0 ** -53] * 6 + [2.0 ** -30, 2.0 ** -60] + [2.0 ** -53] * 4
    n = len(tiny)
    mk0 = np.array([[3, 3]] * n + [[2, 2]], np.float32)
    mk1 = np.array([[1, 1]] * (n + 1), np.float32)
    conf = np.array(tiny + [1.0 + 2.0 ** -30], np.float32)
    pim = np.array([[0, g] for g in range(1, n + 2)], np.int64)
    case = (mk0, mk1, conf, np.arange(n + 2, dtype=np.int64), pim, n + 2)
    assert_bit_exact(run(dev, case), so.oracle_merge(*case), "spread order")


def test_truncation_toward_zero(dev):
    vals = np.array([-0.5, -1.5, 7.9999995, -7.9999995, 0.99999994, -0.99999994, 1.0, -1.0, 2.0 ** 20 - 1, -(2.0 ** 20) + 1], np.float32)
    mk0 = np.stack([vals, vals[::-1]], 1)
    mk1 = np.stack([vals[::-1], vals], 1)
    conf = np.linspace(0.2, 1.0, len(vals)).astype(np.float32)
    case = (mk0, mk1, conf, np.array([0, 5, 10], np.int64), np.array([[0, 1], [1, 2]], np.int64), 3)
    want = so.oracle_merge(*case)
    assert {0.0, -1.0, 7.0, -7.0} <= set(want["keypoints"][:, 0].tolist())
    assert_bit_exact(run(dev, case), want, "truncation")


def test_image_seen_only_as_img1(dev):
    rng = np.random.default_rng(4)
    rows = [30, 0, 45, 20]
    pim = np.array([[0, 3], [3, 1], [1, 3], [2, 3]], np.int64)
    T = sum(rows)
    case = ((rng.integers(0, 9, (T, 2)) * 1.3).astype(np.float32), (rng.integers(-9, 9, (T, 2)) * 0.7).astype(np.float32),
            rng.uniform(0.2, 1, T).astype(np.float32), np.concatenate([[0], np.cumsum(rows)]).astype(np.int64), pim, 4)
    assert_bit_exact(run(dev, case), so.oracle_merge(*case), "img1 only")


def test_one_image_with_more_than_100k_keys(dev):
    """image 0 against 8 others, 160 k distinct keys on a 400 x 400 grid (negative half included), plus repeats"""
    rng = np.random.default_rng(6)
    gx, gy = np.meshgrid(np.arange(-200, 200), np.arange(-150, 250))
    keys = np.stack([gx.reshape(-1), gy.reshape(-1)], 1).astype(np.float32) + np.float32(0.5)
    mk1 = np.concatenate([keys, keys[rng.permutation(len(keys))[:40_000]]], 0)
    T = len(mk1)
    rows = np.full(8, T // 8)
    rows[-1] += T - rows.sum()
    pim = np.array([[g, 0] for g in range(1, 9)], np.int64)
    mk0 = rng.integers(0, 300, (T, 2)).astype(np.float32)
    conf = rng.choice(np.array([0.25, 0.5, 0.75, 1.0], np.float32), T)      # many exact ties
    case = (mk0, mk1, conf, np.concatenate([[0], np.cumsum(rows)]).astype(np.int64), pim, 9)
    want = so.oracle_merge_vectorised(*case)
    assert want["kpt_offsets"][1] > 100_000
    assert_bit_exact(run(dev, case), want, "100k keys")


def test_more_than_2_pow_24_observations(dev):
    rng = np.random.default_rng(7)
    T = (1 << 23) + 4097
    n_images, n_pairs = 40, 800
    all_pairs = [(a, b) for a in range(n_images) for b in range(n_images) if a != b]
    pim = np.array([all_pairs[i] for i in rng.choice(len(all_pairs), n_pairs, replace=False)], np.int64)
    cuts = np.sort(rng.integers(0, T, n_pairs - 1))
    off = np.concatenate([[0], cuts, [T]]).astype(np.int64)
    mk0 = (rng.integers(0, 640, (T, 2), dtype=np.int32).astype(np.float32) * np.float32(0.75))
    mk1 = (rng.integers(-10, 480, (T, 2), dtype=np.int32).astype(np.float32) * np.float32(1.25))
    conf = rng.uniform(0.2, 1.0, T).astype(np.float32)
    case = (mk0, mk1, conf, off, pim, n_images)
    want = so.oracle_merge_vectorised(*case)
    assert 2 * T > (1 << 24)
    assert_bit_exact(run(dev, case), want, "2T > 2^24")


# ---- the matcher over a pair list ------------------------------------------------------------------------------------------------------
SIZES = {"A": (96, 128), "B": (80, 112)}
IMAGE_SIZES = ["A", "A", "B", "A", "B", "A"]
PAIRS = [(0, 1), (2, 4), (1, 3), (0, 2), (3, 0), (4, 1), (2, 1), (5, 3), (1, 5), (4, 0)]


@pytest.fixture(scope="module")
def coarse_matcher(dev):
    return sfm_coarse.build_model(make_synthetic_loftr_state_dict(0)).to(dev)


def planted_hook(dev):
    """the same planted features for every pair of a call, chosen by the two coarse grids (the real backbone finds no matches)"""
    feats = {}
    for h0, w0 in SIZES.values():
        for h1, w1 in SIZES.values():
            x0, g0, x1, g1 = planted_grids((h0 // 8, w0 // 8), (h1 // 8, w1 // 8))
            cl = lambda g: g.permute(0, 2, 3, 1).reshape(1, -1, 128)
            feats[((h0 // 8) * (w0 // 8), (h1 // 8) * (w1 // 8))] = [t.contiguous().to(dev) for t in (x0, cl(g0), x1, cl(g1))]

    def hook(fc0, ff0, fc1, ff1):
        V = fc0.shape[0]
        x0, f0, x1, f1 = feats[(fc0.shape[1], fc1.shape[1])]
        if V == 1:
            return x0, f0[0], x1, f1[0]
        return tuple(t.expand(V, -1, -1).contiguous() for t in (x0, f0, x1, f1))
    return hook


def make_images(dev):
    rng = np.random.default_rng(9)
    out = []
    for s in IMAGE_SIZES:
        H, W = SIZES[s]
        out.append((torch.zeros(1, 1, H, W, device=dev), torch.from_numpy(rng.uniform(0.5, 2.0, (1, 2)).astype(np.float32)).to(dev)))
    return out


def per_pair_matches(m, images):
    mk0, mk1, conf, counts = [], [], [], [0]
    for a, b in PAIRS:
        data = {"image0": images[a][0], "image1": images[b][0], "scale0": images[a][1], "scale1": images[b][1]}
        m(data)
        mk0.append(data["mkpts0_f"].cpu())
        mk1.append(data["mkpts1_f"].cpu())
        conf.append(data["mconf"].cpu())
        counts.append(len(conf[-1]))
    return torch.cat(mk0).numpy(), torch.cat(mk1).numpy(), torch.cat(conf).numpy(), np.cumsum(counts).astype(np.int64)


def test_match_pairs_batched_equals_one_call_per_pair(dev, coarse_matcher):
    images = make_images(dev)
    coarse_matcher.feature_hook = planted_hook(dev)
    try:
        got = sfm_coarse.match_pairs(coarse_matcher, images, PAIRS, max_batch=2)
        mk0, mk1, conf, off = per_pair_matches(coarse_matcher, images)
    finally:
        coarse_matcher.feature_hook = None
    assert (np.diff(off) >= 20).all()
    assert got["pair_offsets"].cpu().numpy().tolist() == off.tolist()
    assert got["pair_images"].cpu().numpy().tolist() == [list(p) for p in PAIRS]
    for k, want in (("mkpts0", mk0), ("mkpts1", mk1), ("mconf", conf)):
        g = got[k].cpu().numpy()
        assert g.dtype == np.float32 and np.array_equal(g.view(np.uint32), want.view(np.uint32)), k
    # the scales reach the keypoints: the same cells, another image's scale
    assert not np.array_equal(mk0[off[0]:off[1]], mk0[off[4]:off[5]])


def test_detector_free_coarse_matching_against_the_oracle(dev, coarse_matcher):
    images = make_images(dev)
    names = [f"img/{i:03d}.png" for i in range(len(images))]
    coarse_matcher.feature_hook = planted_hook(dev)
    try:
        final_keypoints, updated_matches = sfm_coarse.detector_free_coarse_matching(coarse_matcher, names, images, PAIRS)
        mk0, mk1, conf, off = per_pair_matches(coarse_matcher, images)
    finally:
        coarse_matcher.feature_hook = None
    want = so.oracle_merge(mk0, mk1, conf, off, np.array(PAIRS, np.int64), len(names))
    ko = want["kpt_offsets"]
    assert list(final_keypoints) == names
    for g, n in enumerate(names):
        assert np.array_equal(final_keypoints[n].view(np.uint32), want["keypoints"][ko[g]:ko[g + 1]].view(np.uint32)), n
    assert list(updated_matches) == [f"{names[a]} {names[b]}" for a, b in PAIRS]
    for p, (a, b) in enumerate(PAIRS):
        ids = updated_matches[f"{names[a]} {names[b]}"]
        assert ids.dtype == np.int64 and np.array_equal(ids, want["match_ids"][off[p]:off[p + 1]])
