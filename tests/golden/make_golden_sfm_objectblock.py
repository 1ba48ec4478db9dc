"""Generate ``sfm_objectblock_small.npz`` FROM THE REFERENCE ITSELF.

Run in the build container only (needs ``/root/reference``; the GPU box never sees the reference):

    python tests/golden/make_golden_sfm_objectblock.py

The reference's own ``feature_aggregation_and_update`` (feature_aggregation.py), ``filter_bbox`` / ``filter_track_length`` / ``merge``
(filter_points.py), ``get_tkl`` (filter_tkl.py) and ``id_mapping`` / ``count_features`` / ``gather_3d_ann`` /
``mean_descriptors_and_scores`` (feature_process.py) run on the seeded small case of ``tests/sfm_objectblock_oracle.make_case``
(312 points, 12 images, planted close pairs, chains and a cluster, colliding writers, a box that cuts points).

* The COLMAP model is real: the reference's ``read_write_model`` (numpy + struct only) writes the case as ``.bin`` files into a temporary
  directory and the reference's functions read it back, as ``postprocess`` does.  ``filter_bbox`` reads the box with ``np.loadtxt`` and
  writes the filtered model, which the later steps read.
* Import shims, behaviour-neutral, for what is not installed: ``loguru`` (logging), ``cv2``, ``ray`` (a pass-through ``remote``
  decorator; the Ray branch is not run), ``pytorch3d`` (imported by geometry_utils, unused here), ``matplotlib`` when absent, the
  reference's ``vis_utils`` / ``ray_utils`` (visualisation, Ray helpers), and ``h5py``: an in-memory ``File`` with groups and datasets,
  through which the reference's own ``feature_load`` / ``feature_save`` run.
* The ``__init__`` files of ``src.KeypointFreeSfM``, ``.post_optimization``, ``src.sfm_utils`` and ``.postprocess`` are bypassed (they import
  the whole pipeline: open3d, the matcher); the modules themselves are the reference's files, unchanged.
* ``get_kpt_ann`` itself is not called: between the steps pinned here it writes the training annotations (``save_2d_anno``, out of
  scope) and files.  Its four arithmetic steps are called in its order with its arguments.
* The feature files start with 1-row descriptor tables, as the coarse keypoint file does not carry 256 / 128-dimensional descriptors:
  the reference's ``np.zeros`` branch then makes the float64 tables.

Stored: sha256 of every input array (generator drift shows), the outputs of every step, and for the two [U, dim] feature tables their
sha256 as float32 after checking that the float64 tables hold float32 values only (2.5 MB otherwise).
"""
from __future__ import annotations

import hashlib
import importlib.util
import logging
import os
import sys
import tempfile
import types

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
REPO = os.path.abspath(os.path.join(HERE, "..", ".."))
REF = "/root/reference"
sys.dont_write_bytecode = True
sys.path.insert(0, REPO)

CASE_ARGS = dict(seed=5, Q=300, I=12, mean_track=6, max_num_kp3d=150, n_close=12, n_chains=5, cluster=8, collisions=40)
H5_STORE = {}


class _Group(dict):
    def create_dataset(self, name, data=None):
        self[name] = np.array(data)

    def create_group(self, name):
        self[name] = _Group()
        return self[name]


class _File:
    def __init__(self, path, mode="r"):
        if mode == "w":
            H5_STORE[path] = _Group()
        self._g = H5_STORE[path]

    def __enter__(self):
        return self._g

    def __exit__(self, *a):
        return False

    def __getitem__(self, k):
        return self._g[k]


def _install_shims():
    def mod(name, **attrs):
        m = types.ModuleType(name)
        m.__dict__.update(attrs)
        sys.modules[name] = m
        return m

    mod("loguru", logger=logging.getLogger("ref"))
    mod("cv2")
    mod("h5py", File=_File)
    ray = mod("ray", remote=lambda *a, **k: (a[0] if a and callable(a[0]) else (lambda f: f)))
    ray.actor = mod("ray.actor", ActorHandle=object)
    mod("pytorch3d", transforms=mod("pytorch3d.transforms"))
    if importlib.util.find_spec("matplotlib") is None:
        mod("matplotlib", pyplot=mod("matplotlib.pyplot"))
    mod("src.utils.vis_utils", add_pointcloud_to_vis3d=lambda *a, **k: None)
    mod("src.utils.ray_utils", ProgressBar=object, chunks=None, chunk_index=None, split_dict=None)
    # the packages' own __init__ files import the whole SfM pipeline (open3d, COLMAP wrappers, the matcher): plain namespace packages
    # over the same directories let the four modules above be imported on their own
    for name in ("src.KeypointFreeSfM", "src.KeypointFreeSfM.post_optimization", "src.sfm_utils", "src.sfm_utils.postprocess"):
        mod(name, __path__=[os.path.join(REF, *name.split("."))])


def sha(a) -> str:
    return hashlib.sha256(np.ascontiguousarray(a).tobytes()).hexdigest()


def main():
    _install_shims()
    sys.path.insert(0, REF)
    from src.KeypointFreeSfM.post_optimization import feature_aggregation
    from src.sfm_utils.postprocess import feature_process, filter_points, filter_tkl
    from src.utils.colmap import read_write_model as rw
    from tests import sfm_objectblock_oracle as orc

    case = orc.make_case(**CASE_ARGS)
    ko = case["kpt_offsets"]
    I, U = len(ko) - 1, int(ko[-1])
    names = [f"color/{i}.png" for i in range(I)]                           # image i of the flat case = COLMAP image id i + 1
    slot_img = np.repeat(np.arange(I), np.diff(ko))
    slot_kpt = np.arange(U) - ko[slot_img]

    # ---- the COLMAP model of stages B and C, written and read by the reference's own read_write_model
    rng = np.random.default_rng(0)
    xys = rng.random((U, 2)) * 500
    images = {i + 1: rw.Image(id=i + 1, qvec=np.array([1.0, 0, 0, 0]), tvec=np.zeros(3), camera_id=1, name=names[i],
                              xys=xys[ko[i]:ko[i + 1]], point3D_ids=case["point3D_ids"][ko[i]:ko[i + 1]].copy()) for i in range(I)}
    cameras = {1: rw.Camera(id=1, model="PINHOLE", width=512, height=512, params=np.array([500.0, 500.0, 256.0, 256.0]))}
    points3D = {}
    for q, pid in enumerate(case["point_ids"]):
        seen = np.nonzero(case["point3D_ids"] == pid)[0]
        assert len(seen) == case["track_len"][q]
        points3D[int(pid)] = rw.Point3D(id=int(pid), xyz=case["xyz"][q], rgb=np.zeros(3, int), error=0.0, image_ids=slot_img[seen] + 1,
                                        point2D_idxs=slot_kpt[seen])
    tmp = tempfile.mkdtemp()
    model, filtered, box = os.path.join(tmp, "model"), os.path.join(tmp, "model_filted_bbox"), os.path.join(tmp, "box3d_corners.txt")
    os.makedirs(model)
    rw.write_model(cameras, images, points3D, model, ext=".bin")
    np.savetxt(box, case["bbox_corners"], fmt="%.17g")
    assert np.array_equal(np.loadtxt(box), case["bbox_corners"])

    # ---- stage A: feature_aggregation_and_update
    ro = case["row_offsets"]
    colmap_3ds, assigned, fmr = {}, {}, {}
    for p in range(len(ro) - 1):
        rows = np.arange(ro[p], ro[p + 1])
        q_img, q_kpt = int(case["assigned_image"][p]) + 1, int(case["assigned_kpt"][p])
        colmap_3ds[p + 1] = rw.Point3D(id=p + 1, xyz=np.zeros(3), rgb=np.zeros(3, int), error=0.0,
                                       image_ids=np.concatenate([[q_img], case["ref_image"][rows] + 1]),
                                       point2D_idxs=np.concatenate([[q_kpt], case["ref_kpt"][rows]]))
        assigned[p + 1] = (q_img, q_kpt)
        for r in rows:
            d = fmr.setdefault(f"{q_img}-{int(case['ref_image'][r]) + 1}", {"mkpts0_idx": [], "rows": []})
            d["mkpts0_idx"].append(q_kpt)
            d["rows"].append(int(r))
    for d in fmr.values():
        rows = np.array(d.pop("rows"))
        d["mkpts0_idx"] = np.array(d["mkpts0_idx"])
        for k in ("feature_c0", "feature_c1", "feature0", "feature1"):
            d[k] = case[k][rows]
    dataset = types.SimpleNamespace(colmap_3ds=colmap_3ds, colmap_images=images, point_cloud_assigned_imgID_kptID=assigned)
    feat_fine, feat_coarse = os.path.join(tmp, "feats.h5"), os.path.join(tmp, "feats_coarse.h5")
    g = H5_STORE[feat_coarse] = _Group()
    for i, n in enumerate(names):
        k = int(ko[i + 1] - ko[i])
        g[n] = _Group(keypoints=xys[ko[i]:ko[i + 1]].copy(), descriptors=np.zeros((1, k)), scores=np.ones(k))
    open(feat_coarse, "w").close()                                         # feature_load asserts that the path exists
    feature_aggregation.feature_aggregation_and_update(dataset, fmr, feat_fine, names, verbose=False)
    out = {}
    for key, path, dim in (("desc_coarse", feat_coarse, 256), ("desc_fine", feat_fine, 128)):
        tabs = [H5_STORE[path][n]["descriptors"] for n in names]
        assert all(t.shape[0] == dim and t.dtype == np.float64 for t in tabs), "an image no writer reached"
        t64 = np.concatenate([t.T for t in tabs], axis=0)
        assert np.array_equal(t64.astype(np.float32).astype(np.float64), t64)
        out[key + "_sha256"] = sha(t64.astype(np.float32))
        out[key + "_written"] = t64.any(axis=1)
    out["scores_cleared"] = np.concatenate([H5_STORE[feat_coarse][n]["scores"] for n in names]) == 0
    assert np.array_equal(out["scores_cleared"], np.concatenate([H5_STORE[feat_fine][n]["scores"] for n in names]) == 0)

    # ---- stage B: postprocess' calls, in its order
    filter_points.filter_bbox(model, filtered, box, box_trans_path=None)
    track_length, _ = filter_tkl.get_tkl(filtered, thres=case["max_num_kp3d"], show=False)
    xyzs, points_ids = filter_points.filter_track_length(filtered, track_length)
    merge_xyzs, merge_idxs = filter_points.merge(xyzs, points_ids)
    _, images_f, points_f = rw.read_model(filtered, ext=".bin")
    out.update(after_bbox=len(points_f), track_length=int(track_length), after_track_length=len(points_ids), keypoints3d=merge_xyzs,
               group_offsets=np.concatenate([[0], np.cumsum([len(v) for v in merge_idxs.values()])]).astype(np.int64),
               group_members=np.concatenate([np.asarray(v) for v in merge_idxs.values()]).astype(np.int64))
    assert list(merge_idxs) == list(range(len(merge_idxs)))

    # ---- stage C: get_kpt_ann's steps 1 and 2 and its mean, for the coarse and the fine file
    for key, path in (("descriptors3d_coarse", feat_coarse), ("descriptors3d_fine", feat_fine)):
        features = _File(path, "r")
        mapping = feature_process.id_mapping(merge_idxs)
        _, kp3d_id_feature, kp3d_id_score, _ = feature_process.count_features(names, features, images_f, mapping, verbose=False)
        f_xyzs, f_desc, f_scores, idxs = feature_process.gather_3d_ann(kp3d_id_feature, kp3d_id_score, merge_xyzs, merge_idxs, verbose=False)
        avg, avg_scores, _ = feature_process.mean_descriptors_and_scores(f_desc, f_scores, idxs)
        assert np.array_equal(f_xyzs, merge_xyzs)
        out[key], out["scores3d"] = avg, avg_scores
    for k, v in case.items():
        if isinstance(v, np.ndarray):
            out["input_sha256_" + k] = sha(v)
    out["case_args"] = np.array(repr(sorted(CASE_ARGS.items())))
    path = os.path.join(HERE, "sfm_objectblock_small.npz")
    np.savez_compressed(path, **out)
    print("wrote", path, os.path.getsize(path), "bytes;", {k: (out[k] if np.ndim(out[k]) == 0 else np.shape(out[k])) for k in
                                                          ("after_bbox", "track_length", "after_track_length", "keypoints3d", "group_members")})


if __name__ == "__main__":
    main()
