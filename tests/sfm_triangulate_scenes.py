"""Seeded scenes for the triangulation tests: cameras on a ring around a box of points, observations projected, perturbed and truncated
to integer pixels as ``sfm_coarse.merge_pair_matches`` produces them (one slot per image and integer pixel), match rows that join the
observations of a point across a pair list, optionally wrong rows that chain two points together.

Every scene is a dict: ``merged`` (``keypoints``, ``kpt_offsets``, ``match_ids``, ``pair_offsets``, ``pair_images``), ``cameras``
(``image_ids``, ``K``, ``R``, ``t``), ``planted`` (``xyz [N, 3]``) and ``obs`` (per planted point the list of ``(image, slot)``), ``extent``.
The seeds of ``SCENES`` were chosen on the CPU so that the oracle's ``min_margin`` is at least 1e-6 on each
(tests/test_sfm_triangulate_cpu.py asserts it).

Shared by the CPU and the GPU tests: ``scene(name)`` and ``reference(name, ...)`` (the oracle's model, computed once and not to be
written to), and what the CPU file derives and asserts for the GPU file to use --

* ``SPREAD_XYZ`` (scene units) and ``SPREAD_ERR`` (px): the largest difference, over all scenes, of ``xyz`` and of ``point_error``
  between the oracle and the oracle with every sum taken in reversed element order
  (tests/test_sfm_triangulate_cpu.py::test_spread_of_reversed_sums);
* ``BOUND_XYZ``, ``BOUND_ERR``: 16 times these, the device test's bounds.
"""
import functools

import numpy as np

from tests import sfm_triangulate_oracle as orc

W, H, F = 640.0, 480.0, 600.0


def look_at(centre, target=(0.0, 0.0, 0.0)):
    centre, target = np.asarray(centre, float), np.asarray(target, float)
    z = target - centre
    z /= np.linalg.norm(z)
    x = np.cross([0.0, 0.0, 1.0], z)
    x /= np.linalg.norm(x)
    y = np.cross(z, x)
    R = np.stack([x, y, z])
    return R, -R @ centre


def ring_cameras(angles_deg, radius=6.0, height=1.0):
    Rs, ts = [], []
    for k, a in enumerate(angles_deg):
        a = np.radians(a)
        R, t = look_at([radius * np.cos(a), radius * np.sin(a), height * (1 + 0.3 * np.sin(3 * a + k))])
        Rs.append(R)
        ts.append(t)
    n = len(Rs)
    K = np.tile(np.array([[F, 0.0, W / 2], [0.0, F, H / 2], [0.0, 0.0, 1.0]]), (n, 1, 1))
    return K, np.array(Rs), np.array(ts)


def _assemble(K, R, t, observations, pairs, wrong_rows=(), extra_rows=(), shuffle_seed=None, image_ids=None, planted=None):
    """observations: per point a list of (image, x, y) float pixel positions (already perturbed).  Slots: one per (image, integer pixel),
    within an image in a seeded shuffled order.  Rows: for every pair (i, j) of ``pairs`` in order, every point seen in both.
    ``wrong_rows``: (point p, image i, point q, image j) joins p's observation in i with q's in j; ``extra_rows`` likewise"""
    I = len(K)
    per_image = [dict() for _ in range(I)]
    for obs in observations:
        for i, x, y in obs:
            per_image[i].setdefault((int(x), int(y)), None)
    rng = np.random.default_rng(0 if shuffle_seed is None else shuffle_seed)
    kpts, offsets = [], [0]
    for i in range(I):
        keys = list(per_image[i])
        for rank, k in enumerate(rng.permutation(len(keys)).tolist()):
            per_image[i][keys[k]] = rank
        inv = sorted(per_image[i], key=per_image[i].get)
        kpts += inv
        offsets.append(len(kpts))
    seen = [{i: per_image[i][(int(x), int(y))] for i, x, y in obs} for obs in observations]
    rows_of = {}
    for p, s in enumerate(seen):
        imgs = sorted(s)
        for a in range(len(imgs)):
            for b in range(a + 1, len(imgs)):
                rows_of.setdefault((imgs[a], imgs[b]), []).append((s[imgs[a]], s[imgs[b]]))
    for p, i, q, j in list(wrong_rows) + list(extra_rows):
        key, row = ((i, j), (seen[p][i], seen[q][j])) if i < j else ((j, i), (seen[q][j], seen[p][i]))
        rows_of.setdefault(key, []).append(row)
    match_ids, pair_offsets = [], [0]
    for i, j in pairs:
        match_ids += rows_of.get((i, j), []) if i < j else [(b, a) for a, b in rows_of.get((j, i), [])]
        pair_offsets.append(len(match_ids))
    ko = np.array(offsets, np.int64)
    merged = {"keypoints": np.array(kpts, np.float32).reshape(-1, 2), "kpt_offsets": ko,
              "match_ids": np.array(match_ids, np.int64).reshape(-1, 2), "pair_offsets": np.array(pair_offsets, np.int64),
              "pair_images": np.array(pairs, np.int64).reshape(-1, 2)}
    cameras = {"image_ids": np.arange(1, I + 1, dtype=np.int64) if image_ids is None else np.asarray(image_ids, np.int64), "K": K, "R": R, "t": t}
    obs = [[(i, int(ko[i] + r)) for i, r in sorted(s.items())] for s in seen]
    return {"merged": merged, "cameras": cameras, "planted": {"xyz": np.asarray(planted, float)}, "obs": obs, "extent": 4.0}


def project(K, R, t, X):
    q = K @ (R @ X + t)
    return q[0] / q[2], q[1] / q[2], q[2]


def make_scene(seed, n_images, visible, noise=0.3, chains=(), angles=None, all_pairs=True, neighbours=2, behind=False, lonely=False,
               narrow=None, duplicates=0):
    """``visible``: per point the number of images that see it (a random subset), or a list of image indices.  ``chains``: (p, q) plants
    one wrong row between p and q.  ``behind``: one more point seen by cameras 0 and 1 that lies behind the opposite camera, observed there at its
    mirrored projection.  ``lonely``: one more point seen by one image only.  ``narrow = (i, j)``: one more point seen only by the (nearly coincident)
    cameras i and j, chained to point 0.  ``duplicates``: the last point gets that many second slots (one pixel to the right) in its
    first images, joined to its observation in its last image."""
    rng = np.random.default_rng(seed)
    angles = np.linspace(0, 360, n_images, endpoint=False) if angles is None else np.asarray(angles, float)
    K, R, t = ring_cameras(angles)
    X = rng.uniform(-1.0, 1.0, (len(visible), 3))
    observations = []
    for p, vis in enumerate(visible):
        imgs = sorted(rng.choice(n_images, vis, replace=False).tolist()) if np.isscalar(vis) else list(vis)
        obs = []
        for i in imgs:
            u, v, z = project(K[i], R[i], t[i], X[p])
            assert z > 0 and 2 < u < W - 2 and 2 < v < H - 2
            obs.append((i, u + rng.uniform(-noise, noise), v + rng.uniform(-noise, noise)))
        observations.append(obs)
    X = list(X)
    wrong, extra = [], []
    for p, q in chains:
        i = observations[p][0][0]
        j = next(j for j, _, _ in observations[q] if j != i)
        wrong.append((p, i, q, j))
    if behind:
        # in front of cameras 0 and 1, behind the opposite camera (beyond it, seen from the origin), which records the mirrored projection
        back = n_images // 2
        Xb = -R[back].T @ t[back] * 1.17 + np.array([0.05, 0.2, 0.03])
        obs = []
        for i in (0, 1, back):
            u, v, z = project(K[i], R[i], t[i], Xb)
            assert (z < 0) == (i == back) and 2 < u < W - 2 and 2 < v < H - 2, (i, u, v, z)
            obs.append((i, u, v))
        observations.append(obs)
        X.append(Xb)
    if lonely:
        Xl = np.array([0.9, -0.9, 0.9])
        u, v, _ = project(K[0], R[0], t[0], Xl)
        observations.append([(0, u, v)])
        X.append(Xl)
    if narrow is not None:
        Xn = np.array([-0.8, 0.7, -0.6])
        observations.append([(i, *project(K[i], R[i], t[i], Xn)[:2]) for i in narrow])
        X.append(Xn)
        wrong.append((0, observations[0][0][0] if observations[0][0][0] != narrow[1] else observations[0][1][0], len(X) - 1, narrow[1]))
    if duplicates:
        p = len(visible) - 1
        last = observations[p][-1][0]
        for i, u, v in observations[p][:duplicates]:
            observations.append([(i, u + 1.0, v)])
            X.append(X[p])
            extra.append((len(X) - 1, i, p, last))
    if all_pairs:
        pairs = [(i, j) for i in range(n_images) for j in range(i + 1, n_images)]
    else:
        pairs = sorted({(min(i, (i + k) % n_images), max(i, (i + k) % n_images)) for i in range(n_images) for k in range(1, neighbours + 1)})
    return _assemble(K, R, t, observations, pairs, wrong, extra, shuffle_seed=seed, planted=X)


def exact_scene():
    """The noise-free scene: every observation is the exact projection of its planted point and exactly representable in float32 (all
    cameras look along +z, rolled by multiples of 90 degrees, centres on a ring in the plane z = 0 at multiples of 1/4, points at depth 2
    or 4 at multiples of 1/16, focal length 512): the planted points are the exact minimisers."""
    rolls = [np.eye(3), np.array([[0.0, -1, 0], [1, 0, 0], [0, 0, 1]]), np.array([[-1.0, 0, 0], [0, -1, 0], [0, 0, 1]]),
             np.array([[0.0, 1, 0], [-1, 0, 0], [0, 0, 1]])]
    centres = [(2.0, 0.0), (1.5, 1.5), (0.0, 2.0), (-1.5, 1.5), (-2.0, 0.0), (-1.5, -1.5), (0.0, -2.0), (1.5, -1.5)]
    R = np.array([rolls[k % 4] for k in range(8)])
    t = np.array([-(R[k] @ np.array([cx, cy, 0.0])) for k, (cx, cy) in enumerate(centres)])
    K = np.tile(np.array([[512.0, 0.0, 1024.5], [0.0, 512.0, 1024.5], [0.0, 0.0, 1.0]]), (8, 1, 1))
    rng = np.random.default_rng(10)
    X = np.concatenate([rng.integers(-16, 17, (12, 2)) / 16.0, rng.choice([2.0, 4.0], (12, 1))], 1)
    observations = []
    for p in range(12):
        imgs = sorted(rng.choice(8, 3 + p % 5, replace=False).tolist())
        obs = []
        for i in imgs:
            u, v, z = project(K[i], R[i], t[i], X[p])
            assert z > 0 and float(np.float32(u - 0.5)) == u - 0.5 and float(np.float32(v - 0.5)) == v - 0.5
            obs.append((i, u - 0.5, v - 0.5))                              # import_features adds the half pixel back
        observations.append(obs)
    pairs = [(i, j) for i in range(8) for j in range(i + 1, 8)]
    return _assemble(K, R, t, observations, pairs, shuffle_seed=5, planted=X)


def hand_scene():
    """3 images, 2 points, written out by hand: cameras at (-1, 0, 0), (1, 0, 0), (0, 1, 0) looking along +z, focal length 500, principal
    point (320.5, 240.5).  Point A = (0, 0, 5): pixels (420, 240), (220, 240), (320, 140).  Point B = (0.6, 0.2, 4): (520, 265),
    (270, 265), (395, 140), stored one pixel off in y in image 2 (a reprojection error the refinement has to spread).
    Image 0 lists B before A, so its slots are B, A."""
    K = np.tile(np.array([[500.0, 0.0, 320.5], [0.0, 500.0, 240.5], [0.0, 0.0, 1.0]]), (3, 1, 1))
    R = np.tile(np.eye(3), (3, 1, 1))
    t = np.array([[1.0, 0.0, 0.0], [-1.0, 0.0, 0.0], [0.0, -1.0, 0.0]])
    merged = {"keypoints": np.array([[520, 265], [420, 240], [220, 240], [270, 265], [320, 140], [395, 141]], np.float32),
              "kpt_offsets": np.array([0, 2, 4, 6], np.int64),
              "match_ids": np.array([[1, 0], [0, 1], [1, 0], [0, 1], [1, 1]], np.int64),          # pairs (0, 1): A, B; (0, 2): A, B; (1, 2): B
              "pair_offsets": np.array([0, 2, 4, 5], np.int64), "pair_images": np.array([[0, 1], [0, 2], [1, 2]], np.int64)}
    cameras = {"image_ids": np.array([7, 3, 5], np.int64), "K": K, "R": R, "t": t}
    return {"merged": merged, "cameras": cameras, "planted": {"xyz": np.array([[0.6, 0.2, 4.0], [0.0, 0.0, 5.0]])},
            "obs": [[(0, 0), (1, 3), (2, 5)], [(0, 1), (1, 2), (2, 4)]], "extent": 5.0}


def empty_scene():
    """Nothing triangulates: two images, each row joins pixels whose rays diverge; the second pair has no rows"""
    K = np.tile(np.array([[500.0, 0.0, 320.5], [0.0, 500.0, 240.5], [0.0, 0.0, 1.0]]), (3, 1, 1))
    R = np.tile(np.eye(3), (3, 1, 1))
    t = np.array([[1.0, 0.0, 0.0], [-1.0, 0.0, 0.0], [0.0, -1.0, 0.0]])
    merged = {"keypoints": np.array([[100, 100], [120, 300], [500, 100], [520, 30], [320, 240]], np.float32),
              "kpt_offsets": np.array([0, 2, 4, 5], np.int64), "match_ids": np.array([[0, 0], [1, 1]], np.int64),
              "pair_offsets": np.array([0, 2, 2], np.int64), "pair_images": np.array([[0, 1], [1, 2]], np.int64)}
    return {"merged": merged, "cameras": {"image_ids": np.array([1, 2, 3], np.int64), "K": K, "R": R, "t": t},
            "planted": {"xyz": np.zeros((0, 3))}, "obs": [], "extent": 5.0}


# the test scenes: name -> builder (seeds chosen so that min_margin >= 1e-6: tests/test_sfm_triangulate_cpu.py)
def small_scene():
    """8 images, 60 points with tracks of 2 to 8 (all-pairs hypotheses), one point seen by one image only, one behind a camera"""
    rng = np.random.default_rng(100)
    return make_scene(11, 8, [int(v) for v in rng.integers(2, 9, 60)], behind=True, lonely=True)


def medium_scene():
    """40 images, 30 points seen by all, one by 24 (276 pairs: sampled) and one by 23 (253 pairs: all pairs)"""
    return make_scene(12, 40, [40] * 30 + [24, 23])


def long_scene():
    """90 images, tracks of 63, 64, 65 elements and one of 130: 90 images plus 40 second slots within an image"""
    return make_scene(13, 90, [63, 64, 65, 90], duplicates=40)


def chained_scene():
    """10 images (two of them 0.4 degrees apart); wrong rows chain points 0-1-2 (three rounds), 3-4, 5-7 (three
    elements each: a tie between their hypotheses), and a point seen only by the two
    near cameras to point 0 (its leftovers fail the angle filter)"""
    angles = [0, 36, 72, 108, 144, 180, 216, 252, 288, 288.4]
    vis = [[0, 1, 2, 3, 4, 5], [1, 2, 3, 6, 7], [0, 4, 5, 6], [2, 3, 4, 5, 6, 7], [0, 1, 7], [0, 1, 2], [0, 2, 4, 6], [5, 6, 7]]
    return make_scene(14, 10, vis, chains=[(0, 1), (1, 2), (3, 4), (5, 7)], angles=angles, narrow=(8, 9))


SAMPLED_SEED, SAMPLED_GROUPS, SAMPLED_TRACK = 21, 12, 12


def sampled_scene(seed=SAMPLED_SEED, groups=SAMPLED_GROUPS):
    """16 images; ``groups`` components, each four points seen by 12 images and chained 0-1-2-3 by wrong rows: 48 candidates in round 1,
    36 in round 2, 24 in round 3, all above the 23 that all-pairs hypotheses reach, so every round samples.  A hypothesis from two
    elements of one point has that point's 12 elements as inliers, one from two points next to none: the four inlier sets tie, the
    earliest sampled hypothesis decides which point a round takes, and the point left over after three rounds is the draw's choice"""
    chains = [(4 * g + k, 4 * g + k + 1) for g in range(groups) for k in range(3)]
    return make_scene(seed, 16, [SAMPLED_TRACK] * (4 * groups), chains=chains)


SCENES = {"hand": hand_scene, "exact": exact_scene, "small": small_scene, "medium": medium_scene, "long": long_scene,
          "chained": chained_scene, "sampled": sampled_scene, "empty": empty_scene}

SPREAD_XYZ = 1.3322676295501878e-15      # measured by test_spread_of_reversed_sums (6 ulp of 1.0; the exact scene), scene units
SPREAD_ERR = 1.1920384820585433e-13      # px: an ulp of a pixel coordinate near 1000 (the exact scene, whose true error is 0)
BOUND_XYZ = 16 * SPREAD_XYZ              # 2.13e-14: 5.3e-15 of the scenes' extent (4), far below the 1e-6 that would mean ill-conditioning
BOUND_ERR = 16 * SPREAD_ERR              # 1.91e-12 px
INT_KEYS = ("labels", "point3D_ids", "point_ids", "track_offsets", "track_image", "track_kpt", "kpt_offsets", "image_ids")


@functools.lru_cache(maxsize=None)
def scene(name):
    return SCENES[name]()


@functools.lru_cache(maxsize=None)
def reference(name, fault=None, reverse=False, max_rounds=3):
    s = scene(name)
    return orc.triangulate(s["merged"], s["cameras"], fault=fault, reverse=reverse, max_rounds=max_rounds)


def nearest_planted(s, m):
    """per planted point the distance to the nearest triangulated point"""
    if not len(m["xyz"]):
        return np.full(len(s["planted"]["xyz"]), np.inf)
    return np.abs(s["planted"]["xyz"][:, None, :] - m["xyz"][None, :, :]).max(2).min(1)


def timing_scene(n_images=150, n_points=60000, track=20, seed=21):
    """150 images, 60 000 points each seen by 20 consecutive images of the ring (about 1.2 M observations), rows between ring neighbours at
    distance 1 and 2; built with numpy (no per-observation Python loop)"""
    rng = np.random.default_rng(seed)
    angles = np.linspace(0, 360, n_images, endpoint=False)
    K, R, t = ring_cameras(angles)
    K[:, :2, :] *= 6.0                                                     # 3840 x 2880 images: few observations share a pixel
    X = rng.uniform(-1.0, 1.0, (n_points, 3))
    start = rng.integers(0, n_images, n_points)
    img = (start[:, None] + np.arange(track)[None, :]) % n_images                                  # [N, track]
    pc = np.einsum("ntij,nj->nti", R[img], X) + t[img]
    uv = np.einsum("ntij,ntj->nti", K[img], pc)
    uv = uv[..., :2] / uv[..., 2:] + rng.uniform(-0.3, 0.3, (n_points, track, 2))
    pix = np.floor(uv).astype(np.int64)
    key = (img * 4096 + pix[..., 0]) * 4096 + pix[..., 1]
    uniq, slot = np.unique(key.reshape(-1), return_inverse=True)                                    # slots ascend by (image, x, y)
    slot = slot.reshape(n_points, track)
    slot_img = uniq // (4096 * 4096)
    ko = np.concatenate([[0], np.cumsum(np.bincount(slot_img, minlength=n_images))]).astype(np.int64)
    keypoints = np.stack([(uniq // 4096) % 4096, uniq % 4096], 1).astype(np.float32)
    rows = []
    for k in (1, 2):
        a_img, b_img = img[:, :-k].reshape(-1), img[:, k:].reshape(-1)
        a_id, b_id = slot[:, :-k].reshape(-1) - ko[a_img], slot[:, k:].reshape(-1) - ko[b_img]
        swap = a_img > b_img
        rows.append(np.stack([np.where(swap, b_img, a_img), np.where(swap, a_img, b_img), np.where(swap, b_id, a_id), np.where(swap, a_id, b_id)], 1))
    rows = np.concatenate(rows)
    pair_key = rows[:, 0] * n_images + rows[:, 1]
    order = np.argsort(pair_key, kind="stable")
    rows, pair_key = rows[order], pair_key[order]
    pk, counts = np.unique(pair_key, return_counts=True)
    merged = {"keypoints": keypoints, "kpt_offsets": ko, "match_ids": np.ascontiguousarray(rows[:, 2:]),
              "pair_offsets": np.concatenate([[0], np.cumsum(counts)]).astype(np.int64),
              "pair_images": np.stack([pk // n_images, pk % n_images], 1).astype(np.int64)}
    cameras = {"image_ids": np.arange(1, n_images + 1, dtype=np.int64), "K": K, "R": R, "t": t}
    return {"merged": merged, "cameras": cameras, "planted": {"xyz": X}, "extent": 4.0}
