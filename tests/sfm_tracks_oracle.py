"""CPU oracle of ``onepose_st_amd/sfm_tracks.py``, numpy only.

Two forms that must agree wherever both run:

* ``reference_form``: the reference's three classes (``CoarseReconDataset.get_keyframes_greedy`` / ``build_initial_depth_pose`` /
  ``extract_corresponding_frames``, ``MatchingPairData``, ``ConstructOptimizationData``) restated on dicts keyed by COLMAP ids, in the
  reference's own loop form: a sorted dict carried from round to round, one ``argwhere`` per row, float64 state arrays, the depth through
  numpy's matmul.  Quadratic in places, for small cases.
* ``vectorised_form``: the same results from sorts and segment operations, for the 60 000-point case.  Its depth is written out term by
  term, ``((r0 x + r1 y) + r2 z) + t`` and ``(k0 cx + k1 cy) + k2 cz``, the order the device uses.

Both return one flat dict (``PLAN_KEYS + PAIR_KEYS + ROW_KEYS``).  ``fault=`` seeds one of ``FAULTS`` into ``reference_form`` so that the
CPU tests can show that the GPU tests' inputs tell each fault from the truth.
"""
from __future__ import annotations

import numpy as np

MODEL_KEYS = ("image_ids", "kpt_offsets", "xys", "point3D_ids", "K", "R", "t", "point_ids", "xyz", "track_offsets", "track_image", "track_kpt")
PLAN_KEYS = ("keyframes", "state", "is_keyframe", "assigned_image", "assigned_kpt", "initial_depth")
PAIR_KEYS = ("pair_left", "pair_right", "pair_offsets", "mkpts0_c", "mkpts1_c", "mkpts0_idx")
ROW_KEYS = ("fine_row", "ref_image", "ref_kpt", "n_query", "row_offsets")
FAULTS = ("tie_initial_order", "first_keypoint_wins", "right_by_index", "last_occurrence", "robbed_is_owned")
EPS = 2.0 ** -52


# ---- models ----------------------------------------------------------------------------------------------------------------------------
def _poses(rng, I):
    K = np.zeros((I, 3, 3))
    K[:, 0, 0] = 480 + 40 * rng.random(I)
    K[:, 1, 1] = 480 + 40 * rng.random(I)
    K[:, 0, 2], K[:, 1, 2], K[:, 2, 2] = 250 + 10 * rng.random(I), 250 + 10 * rng.random(I), 1.0
    w = rng.standard_normal((I, 3)) * 0.3
    R = np.empty((I, 3, 3))
    for i in range(I):
        th = np.linalg.norm(w[i])
        k = w[i] / th
        S = np.array([[0, -k[2], k[1]], [k[2], 0, -k[0]], [-k[1], k[0], 0]])
        R[i] = np.eye(3) + np.sin(th) * S + (1 - np.cos(th)) * (S @ S)
    t = rng.standard_normal((I, 3)) * 0.1 + np.array([0.0, 0.0, 3.0])
    return K, R, t


def build_model(observations, n_kpt, image_ids, point_ids, rng, xyz=None):
    """observations: per point a list of (image index, keypoint index) in track order; n_kpt [I] keypoints per image (the slots no
    observation names are unregistered) -> the flat model (numpy)"""
    I, Q = len(n_kpt), len(observations)
    ko = np.concatenate([[0], np.cumsum(n_kpt)]).astype(np.int64)
    U = int(ko[-1])
    p3d = np.full(U, -1, np.int64)
    ti, tk, to = [], [], [0]
    for q, obs in enumerate(observations):
        for i, k in obs:
            p3d[ko[i] + k] = point_ids[q]
            ti.append(i)
            tk.append(k)
        to.append(len(ti))
    K, R, t = _poses(rng, I)
    return {"image_ids": np.asarray(image_ids, np.int64), "kpt_offsets": ko, "xys": rng.random((U, 2)) * 500, "point3D_ids": p3d, "K": K,
            "R": R, "t": t, "point_ids": np.asarray(point_ids, np.int64), "xyz": rng.standard_normal((Q, 3)) * 0.3 if xyz is None else xyz,
            "track_offsets": np.asarray(to, np.int64), "track_image": np.asarray(ti, np.int64), "track_kpt": np.asarray(tk, np.int64)}


def make_model(seed, Q, I, mean_track, n_dup=0, long_track=0, shuffle_ids=False, empty_images=(), unregistered=0.2):
    """A seeded consistent model: point q is seen in ``2 + Poisson(mean_track - 2)`` distinct images (at most the images that take
    keypoints), ``n_dup`` points are seen twice in one of their images (a duplicate keypoint in an image = a repeated image in the track),
    one track of ``long_track`` elements spread over all images, track elements in random order, a share of unregistered slots,
    ``empty_images`` without any registered keypoint, ids shuffled on request."""
    rng = np.random.default_rng(seed)
    live = np.array([i for i in range(I) if i not in set(empty_images)])
    # images differ in how often they are drawn, so that the counts spread and some image ends without a track of its own
    weight = rng.random(len(live)) ** 2 + 0.02
    weight /= weight.sum()
    lens = np.minimum(2 + rng.poisson(max(mean_track - 2, 0), Q), len(live))
    per_image = [[] for _ in range(I)]                                     # (point, position in its track)
    tracks = []
    for q in range(Q):
        imgs = rng.choice(live, size=lens[q], replace=False, p=weight).tolist()
        if q < n_dup:
            imgs.insert(int(rng.integers(0, len(imgs) + 1)), imgs[int(rng.integers(0, len(imgs)))])
        if q == Q - 1 and long_track:
            imgs = rng.choice(live, size=long_track, replace=True).tolist()
        tracks.append(imgs)
        for pos, i in enumerate(imgs):
            per_image[i].append((q, pos))
    n_kpt = np.zeros(I, np.int64)
    observations = [[None] * len(tr) for tr in tracks]
    for i in range(I):
        n_reg = len(per_image[i])
        n = n_reg + int(np.ceil(unregistered * n_reg)) + (3 if i in set(empty_images) else 0)
        n_kpt[i] = n
        where = rng.permutation(n)[:n_reg]
        for (q, pos), k in zip(per_image[i], where.tolist()):
            observations[q][pos] = (i, k)
    image_ids = np.arange(1, I + 1)
    point_ids = np.arange(1, Q + 1) * 3 + 7
    if shuffle_ids:
        image_ids = rng.permutation(np.arange(1, 4 * I + 1))[:I]
        point_ids = rng.permutation(point_ids)
    return build_model(observations, n_kpt, image_ids, point_ids, rng)


def with_projected_keypoints(m, noise=0.0, seed=0):
    """the model with every registered keypoint at the projection of its point (plus noise in pixels): a geometrically sound model for
    the optimiser"""
    slot_image, _, slot_point, _ = _tables(m)
    reg = slot_point >= 0
    X = m["xyz"][slot_point[reg]]
    cam = np.einsum("nij,nj->ni", m["R"][slot_image[reg]], X) + m["t"][slot_image[reg]]
    h = np.einsum("nij,nj->ni", m["K"][slot_image[reg]], cam)
    out = dict(m)
    out["xys"] = m["xys"].copy()
    out["xys"][reg] = h[:, :2] / h[:, 2:] + noise * np.random.default_rng(seed).standard_normal((int(reg.sum()), 2))
    return out


def hand_case():
    """Four images (ids 30, 10, 20, 40 in this order), five points, small enough to work on paper (tests/test_sfm_tracks_cpu.py):

    image 0 (id 30): k0 -> A, k1 -> B, k2 unregistered, k3 -> C
    image 1 (id 10): k0 -> A, k1 -> D, k2 -> D (D twice), k3 -> E
    image 2 (id 20): k0 -> B, k1 -> A, k2 -> A (A twice), k3 unregistered, k4 -> E
    image 3 (id 40): k0 -> C, k1 unregistered, k2 -> D
    The tracks, as (image, keypoint) in track order, are the table below; the ids of A .. E are 5, 9, 2, 7, 4 in this dict order."""
    obs = [[(2, 2), (0, 0), (1, 0), (2, 1)],        # A: image 2 twice, the later element names the earlier keypoint
           [(0, 1), (2, 0)],                        # B
           [(3, 0), (0, 3)],                        # C
           [(1, 2), (1, 1), (3, 2)],                # D: image 1 twice
           [(1, 3), (2, 4)]]                        # E
    n_kpt = [4, 4, 5, 3]                            # image 0 k2, image 2 k3, image 3 k1 are unregistered
    return build_model(obs, np.array(n_kpt), [30, 10, 20, 40], [5, 9, 2, 7, 4], np.random.default_rng(0),
                       xyz=np.array([[0.1, 0.2, 0.3], [-0.2, 0.1, 0.0], [0.3, -0.1, 0.2], [0.0, 0.0, 0.1], [0.2, 0.2, -0.2]]))


def tie_case():
    """Four images whose counts tie in a way the initial order would resolve differently from the carried order; every point is seen in
    two images.

    counts at round 1: [4, 5, 6, 5] -> order 2, 1, 3, 0; image 2 is taken and robs two slots of image 1, three of image 3 and one of image
    0: counts 1: 3, 3: 2, 0: 3 -> the carried order 1, 3, 0 sorts (stably) to 1, 0, 3: image 1 is the second keyframe, where the initial
    order would take image 0.  Image 1 robs two slots of image 0 and one of image 3; image 0 takes the last point; image 3 is never a
    keyframe."""
    obs = [[(2, 0), (1, 0)], [(2, 1), (1, 1)], [(2, 2), (3, 0)], [(2, 3), (3, 1)], [(2, 4), (3, 2)], [(2, 5), (0, 2)],     # image 2's six
           [(1, 2), (0, 0)], [(1, 3), (0, 1)], [(1, 4), (3, 3)],                                                         # image 1's other three
           [(0, 3), (3, 4)]]                                                                                               # images 0 and 3
    return build_model(obs, np.array([4, 5, 6, 5]), [1, 2, 3, 4], np.arange(100, 110), np.random.default_rng(1))


# ---- the reference's loop form ---------------------------------------------------------------------------------------------------------
def reference_form(m, fault=None):
    ids = m["image_ids"].tolist()
    ko, to = m["kpt_offsets"], m["track_offsets"]
    I, Q, U = len(ids), len(m["point_ids"]), len(m["point3D_ids"])
    index_of = {cid: i for i, cid in enumerate(ids)}
    images = {cid: {"xys": m["xys"][ko[i]:ko[i + 1]], "p3d": m["point3D_ids"][ko[i]:ko[i + 1]]} for i, cid in enumerate(ids)}
    points = {}
    for q, pid in enumerate(m["point_ids"].tolist()):
        sl = slice(to[q], to[q + 1])
        points[pid] = {"xyz": m["xyz"][q], "image_ids": m["image_ids"][m["track_image"][sl]], "kpts": m["track_kpt"][sl]}
    # get_keyframes_greedy
    st = {}
    for cid, im in images.items():
        s = -2 * np.ones((im["xys"].shape[0],))
        s[im["p3d"] == -1] = -1
        st[cid] = {"state": s, "n": (s == -2).sum()}
    p_state = {pid: (-1,) for pid in points}
    keyframe_dict = {}
    while any(len(v) == 1 for v in p_state.values()):
        assert len(st) != 0
        if fault == "tie_initial_order":
            st = {k: v for k, v in sorted(st.items(), key=lambda kv: (-kv[1]["n"], index_of[kv[0]]))}
        else:
            st = {k: v for k, v in sorted(st.items(), key=lambda kv: kv[1]["n"], reverse=True)}
        cur = list(st.keys())[0]
        cur_state = st.pop(cur)
        mask = cur_state["state"] == -2
        if fault == "robbed_is_owned":
            mask = mask | (cur_state["state"] == -3)
        cur_state["state"][mask] = images[cur]["p3d"][mask]
        keyframe_dict[cur] = cur_state
        taken = images[cur]["p3d"][mask]
        kpts = np.arange(images[cur]["xys"].shape[0])[mask]
        seen = set()
        for n, pid in enumerate(taken.tolist()):
            if not (fault == "first_keypoint_wins" and pid in seen):
                p_state[pid] = (cur, kpts[n])
            seen.add(pid)
            for img_id, k in zip(points[pid]["image_ids"].tolist(), points[pid]["kpts"].tolist()):
                if img_id == cur:
                    continue
                if fault == "robbed_is_owned" and img_id not in st:
                    continue
                assert st[img_id]["state"][k] != -1
                st[img_id]["state"][k] = -3
        for v in st.values():
            v["n"] = (v["state"] == -2).sum()
    # build_initial_depth_pose
    state = np.empty(U, np.int64)
    depth = -np.ones(U)
    for i, cid in enumerate(ids):
        if cid in keyframe_dict:
            s = keyframe_dict[cid]["state"]
            occ = s >= 0
            cloud = np.concatenate([points[int(pid)]["xyz"][None] for pid in s[occ]])
            cam = m["R"][i] @ cloud.T + m["t"][i][:, None]
            d = -np.ones(len(s))
            d[occ] = (m["K"][i] @ cam).T[:, 2]
            depth[ko[i]:ko[i + 1]] = d
        else:
            s = st[cid]["state"]
        state[ko[i]:ko[i + 1]] = s.astype(np.int64)
    out = {"keyframes": np.array([index_of[c] for c in keyframe_dict], np.int64), "state": state,
           "is_keyframe": np.array([c in keyframe_dict for c in ids]), "initial_depth": depth,
           "assigned_image": np.array([index_of[p_state[pid][0]] for pid in points], np.int64),
           "assigned_kpt": np.array([p_state[pid][1] for pid in points], np.int64)}
    # extract_corresponding_frames + MatchingPairData
    all_pairs = []
    for cid in ids:
        if cid not in keyframe_dict:
            continue
        s = keyframe_dict[cid]["state"]
        related = np.concatenate([points[int(pid)]["image_ids"] for pid in s[s >= 0]])
        if fault == "right_by_index":
            uniq = [ids[i] for i in sorted({index_of[c] for c in related.tolist()})]
        else:
            uniq = np.unique(related).tolist()
        uniq.remove(cid)
        all_pairs += [(cid, r) for r in uniq]
    fine, pl, pr, po, mk0, mk1, idx = {}, [], [], [0], [], [], []
    for left, right in all_pairs:
        s = keyframe_dict[left]["state"]
        valid = np.arange(len(s))[s >= 0]
        a, b, c = [], [], []
        for k in valid.tolist():
            pt = points[int(s[k])]
            hit = np.argwhere(pt["image_ids"] == right)
            if len(hit) != 0:
                e = int(hit[-1 if fault == "last_occurrence" else 0, 0])
                a.append(images[left]["xys"][k])
                b.append(images[right]["xys"][pt["kpts"][e]])
                c.append(k)
        fine[f"{left}-{right}"] = {"mkpts0_idx": np.array(c), "first_row": po[-1]}
        pl.append(index_of[left])
        pr.append(index_of[right])
        mk0 += a
        mk1 += b
        idx += c
        po.append(len(idx))
    out.update(pair_left=np.array(pl, np.int64), pair_right=np.array(pr, np.int64), pair_offsets=np.array(po, np.int64),
               mkpts0_c=np.stack(mk0), mkpts1_c=np.stack(mk1), mkpts0_idx=np.array(idx, np.int64))
    # ConstructOptimizationData
    fr, ri, rk, nq = [], [], [], []
    for pid, pt in points.items():
        a_img, a_kpt = p_state[pid]
        pairs_dict = {}
        for img_id, k in zip(pt["image_ids"].tolist(), pt["kpts"].tolist()):
            if img_id != a_img:
                pairs_dict[f"{a_img}-{img_id}"] = k
        for name, k in pairs_dict.items():
            assert name in fine, name
            hit = np.argwhere(fine[name]["mkpts0_idx"] == a_kpt)
            assert len(hit) == 1, len(hit)
            fr.append(fine[name]["first_row"] + int(hit[0, 0]))
            ri.append(index_of[int(name.split("-")[1])])
            rk.append(k)
        nq.append(len(pairs_dict))
    out.update(fine_row=np.array(fr, np.int64), ref_image=np.array(ri, np.int64), ref_kpt=np.array(rk, np.int64),
               n_query=np.array(nq, np.int64), row_offsets=np.concatenate([[0], np.cumsum(nq)]).astype(np.int64))
    return out


# ---- the vectorised form -----------------------------------------------------------------------------------------------------------------
def _tables(m):
    ko, to = m["kpt_offsets"], m["track_offsets"]
    I, Q = len(m["image_ids"]), len(m["point_ids"])
    slot_image = np.repeat(np.arange(I), np.diff(ko))
    elem_point = np.repeat(np.arange(Q), np.diff(to))
    order = np.argsort(m["point_ids"])
    where = np.clip(np.searchsorted(m["point_ids"][order], m["point3D_ids"]), 0, Q - 1)
    slot_point = np.where(m["point_ids"][order][where] == m["point3D_ids"], order[where], -1)
    return slot_image, elem_point, slot_point, ko[m["track_image"]] + m["track_kpt"]


def _gather_ranges(starts, ends):
    """concatenated aranges [starts[n], ends[n])"""
    lens = ends - starts
    total = int(lens.sum())
    base = np.repeat(starts - np.concatenate([[0], np.cumsum(lens)[:-1]]), lens)
    return base + np.arange(total)


def vectorised_form(m):
    ko, to = m["kpt_offsets"], m["track_offsets"]
    I, Q, U, E = len(m["image_ids"]), len(m["point_ids"]), len(m["point3D_ids"]), len(m["track_image"])
    slot_image, elem_point, slot_point, elem_slot = _tables(m)
    state = np.where(slot_point >= 0, -2, -1).astype(np.int64)            # point INDEX where owned, until the end
    order = np.arange(I)
    a_img, a_kpt = np.full(Q, -1, np.int64), np.full(Q, -1, np.int64)
    keyframes = []
    count = np.bincount(slot_image[state == -2], minlength=I)
    while (a_img < 0).any():
        order = order[np.argsort(-count[order], kind="stable")]
        kf, order = int(order[0]), order[1:]
        keyframes.append(kf)
        sl = np.arange(ko[kf], ko[kf + 1])
        take = sl[state[sl] == -2]
        pts = slot_point[take]
        state[take] = pts
        a_img[pts] = kf
        np.maximum.at(a_kpt, pts, take - ko[kf])
        upts = np.unique(pts)
        el = _gather_ranges(to[upts], to[upts + 1])
        el = el[m["track_image"][el] != kf]
        state[elem_slot[el]] = -3
        count = np.bincount(slot_image[state == -2], minlength=I)
    occ = state >= 0
    K, R, t, X = m["K"][slot_image[occ]], m["R"][slot_image[occ]], m["t"][slot_image[occ]], m["xyz"][state[occ]]
    cam = [((R[:, r, 0] * X[:, 0] + R[:, r, 1] * X[:, 1]) + R[:, r, 2] * X[:, 2]) + t[:, r] for r in range(3)]
    depth = -np.ones(U)
    depth[occ] = (K[:, 2, 0] * cam[0] + K[:, 2, 1] * cam[1]) + K[:, 2, 2] * cam[2]
    is_kf = np.zeros(I, bool)
    is_kf[keyframes] = True
    out = {"keyframes": np.array(keyframes, np.int64), "state": np.where(occ, m["point_ids"][np.maximum(state, 0)], state), "is_keyframe": is_kf,
           "assigned_image": a_img, "assigned_kpt": a_kpt, "initial_depth": depth}
    # first / last occurrence of each (point, image) among the track elements
    by = np.lexsort((np.arange(E), m["track_image"], elem_point))
    new = np.ones(E, bool)
    new[1:] = (elem_point[by][1:] != elem_point[by][:-1]) | (m["track_image"][by][1:] != m["track_image"][by][:-1])
    group = np.cumsum(new) - 1
    first_e = by[new]
    last_e = by[np.concatenate([np.nonzero(new)[0][1:] - 1, [E - 1]])]
    is_first = np.zeros(E, bool)
    is_first[first_e] = True
    last_of = np.empty(E, np.int64)
    last_of[by] = last_e[group]
    other = is_first & (m["track_image"] != a_img[elem_point])
    rows_e = np.nonzero(other)[0]
    n_query = np.bincount(elem_point[rows_e], minlength=Q)
    row_offsets = np.concatenate([[0], np.cumsum(n_query)]).astype(np.int64)
    ref_image, ref_kpt = m["track_image"][rows_e], m["track_kpt"][last_of[rows_e]]
    # pair rows: every owned slot x the rows of its point
    owned = np.nonzero(occ)[0]
    p_of = state[owned]
    per = n_query[p_of]
    which = np.repeat(np.arange(len(owned)), per)
    e_of = rows_e[_gather_ranges(row_offsets[p_of], row_offsets[p_of + 1])]
    left, right = slot_image[owned[which]], m["track_image"][e_of]
    kpt = owned[which] - ko[left]
    perm = np.lexsort((kpt, m["image_ids"][right], left))
    left, right, kpt, e_of, slot = left[perm], right[perm], kpt[perm], e_of[perm], owned[which][perm]
    newp = np.ones(len(perm), bool)
    newp[1:] = (left[1:] != left[:-1]) | (right[1:] != right[:-1])
    starts = np.nonzero(newp)[0]
    out.update(pair_left=left[starts], pair_right=right[starts], pair_offsets=np.concatenate([starts, [len(perm)]]).astype(np.int64),
               mkpts0_c=m["xys"][slot], mkpts1_c=m["xys"][ko[right] + m["track_kpt"][e_of]], mkpts0_idx=kpt)
    # fine_row: the pair row with (assigned image, ref image, assigned keypoint)
    stride = int(np.diff(ko).max())
    row_key = (left * I + right) * stride + kpt
    assert (np.diff(np.sort(row_key)) > 0).all()
    by_key = np.argsort(row_key)
    want = (a_img[elem_point[rows_e]] * I + ref_image) * stride + a_kpt[elem_point[rows_e]]
    pos = np.clip(np.searchsorted(row_key[by_key], want), 0, len(by_key) - 1)
    assert (row_key[by_key][pos] == want).all()
    out.update(fine_row=by_key[pos].astype(np.int64), ref_image=ref_image, ref_kpt=ref_kpt, n_query=n_query.astype(np.int64), row_offsets=row_offsets)
    return out


# ---- bounds and adapters -------------------------------------------------------------------------------------------------------------------
def depth_bound(m, state):
    """Per slot the forward-error bound of z of K (R X + t) in float64: ``8 * 2^-52 * (|K| (|R| |X| + |t|))_z`` (three-term dot products,
    one addition, a three-term dot product: at most 6 roundings per path, whatever the order of the sums), 0 on slots without a point"""
    slot_image, _, slot_point, _ = _tables(m)
    occ = state >= 0
    bound = np.zeros(len(state))
    K, R, t, X = np.abs(m["K"][slot_image[occ]]), np.abs(m["R"][slot_image[occ]]), np.abs(m["t"][slot_image[occ]]), np.abs(m["xyz"][slot_point[occ]])
    cam = np.einsum("nij,nj->ni", R, X) + t
    bound[occ] = 8 * EPS * np.einsum("nj,nj->n", K[:, 2, :], cam)
    return bound


def update_model(m, res, depth, R, t):
    """update_optimize_results_to_colmap on the flat model: every point unprojected from its assigned keypoint with the new pose, every
    registered slot reprojected (float64, numpy's matmul and inverse as the reference)"""
    slot_image, _, slot_point, _ = _tables(m)
    ko = m["kpt_offsets"]
    Q = len(m["point_ids"])
    xyz = np.empty((Q, 3))
    for q in range(Q):
        i = res["assigned_image"][q]
        kp = m["xys"][ko[i] + res["assigned_kpt"][q]][None]
        T = np.concatenate([np.concatenate([R[i], t[i][:, None]], axis=1), [[0, 0, 0, 1]]], axis=0)
        Ti = np.linalg.inv(T)
        kpt_h = (np.concatenate([kp, np.ones((1, 1))], axis=-1) * depth[q]).T
        xyz[q] = (Ti[:3, :3] @ (np.linalg.inv(m["K"][i]) @ kpt_h) + Ti[:3, 3][:, None]).squeeze(-1)
    xys = m["xys"].copy()
    for i in range(len(ko) - 1):
        reg = np.nonzero(slot_point[ko[i]:ko[i + 1]] >= 0)[0] + ko[i]
        if len(reg) == 0:
            continue
        cam = R[i] @ xyz[slot_point[reg]].T + t[i][:, None]
        h = (m["K"][i] @ cam).T
        xys[reg] = h[:, :2] / (h[:, [2]] + 1e-4)
    return {"xyz": xyz, "xys": xys}


def optimizer_inputs(m, res, mkpts1_f):
    """the ``aggregated`` arrays of ``start_optimize`` from the oracle's rows (numpy)"""
    fr = res["fine_row"]
    row_left = np.repeat(res["pair_left"], np.diff(res["pair_offsets"]))
    row_right = np.repeat(res["pair_right"], np.diff(res["pair_offsets"]))
    slots = m["kpt_offsets"][res["assigned_image"]] + res["assigned_kpt"]
    return {"depth": res["initial_depth"][slots][:, None], "n_query": res["n_query"], "intrinsic0": m["K"][row_left[fr]],
            "intrinsic1": m["K"][row_right[fr]], "mkpts0_c": res["mkpts0_c"][fr], "mkpts1_c": res["mkpts1_c"][fr], "mkpts1_f": mkpts1_f[fr],
            "left_colmap_ids": m["image_ids"][row_left[fr]], "right_colmap_ids": m["image_ids"][row_right[fr]], "point_cloud_id": m["point_ids"]}


def golden_model(npz):
    return {k: npz["model_" + k] for k in MODEL_KEYS}
