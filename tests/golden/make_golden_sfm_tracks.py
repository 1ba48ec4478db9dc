"""Generate ``sfm_tracks_small.npz`` FROM THE REFERENCE ITSELF.

Run in the build container only (needs the reference checkout beside the repository; the GPU box never sees it):

    python tests/golden/make_golden_sfm_tracks.py

The reference's own ``CoarseReconDataset`` (dataset/coarse_colmap_dataset.py), ``MatchingPairData`` (construct_matching_data.py) and
``ConstructOptimizationData`` (construct_optimization_data.py) run on the seeded small model of
``tests/sfm_tracks_oracle.make_model`` (12 images with shuffled ids, 300 points, 25 of them seen twice in one image, one image without a
registered keypoint).

* The COLMAP model is real: the reference's ``read_write_model`` writes it as ``.bin`` files into a temporary directory (one PINHOLE
  camera per image, the rotation as the quaternion of ``rotmat2qvec``) and ``CoarseReconDataset`` reads it back.  The stored model is
  what the reference works with: ``R`` is ``qvec2rotmat`` of the stored quaternion, ``K`` its ``get_intrinsic_from_colmap_camera``.
* ``ConstructOptimizationData``'s padded ``__getitem__`` output is reduced as ``Optimizer.start_optimize`` reduces a batch: the first
  ``n_query`` rows of every padded entry, concatenated over the points.
* The fine-match dict is seeded random ``mkpts1_f`` keyed by the pair names, beside the pair's own ``mkpts0_c / mkpts1_c / mkpts0_idx``;
  the matcher itself is not run.
* Import shims, behaviour-neutral, for what is not installed or out of scope: ``loguru`` (logging), ``pytorch3d`` (imported by
  geometry_utils, unused here), the reference's ``vis3d`` (visualisation) and ``src.utils.data_io`` (image reading: ``read_grayscale``
  returns a 1 x 1 image, which nothing pinned here looks at).  The ``__init__`` files of ``src.KeypointFreeSfM`` and its sub-packages are
  bypassed (they import the whole pipeline); the modules themselves are the reference's files, unchanged.

Stored: the model (``model_*``), sha256 of every model array (generator drift shows), ``mkpts1_f``, and the outputs of the three classes.
"""
from __future__ import annotations

import hashlib
import logging
import os
import sys
import tempfile
import types

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
REPO = os.path.abspath(os.path.join(HERE, "..", ".."))
REF = os.environ.get("ONEPOSE_REFERENCE", "/root/reference")
sys.dont_write_bytecode = True
sys.path.insert(0, REPO)

CASE_ARGS = dict(seed=5, Q=300, I=12, mean_track=6, n_dup=25, shuffle_ids=True, empty_images=(4,))


def _install_shims():
    def mod(name, **attrs):
        m = types.ModuleType(name)
        m.__dict__.update(attrs)
        sys.modules[name] = m
        return m

    mod("loguru", logger=logging.getLogger("ref"))
    mod("pytorch3d", transforms=mod("pytorch3d.transforms"))
    mod("src.utils.data_io", read_grayscale=lambda *a, **k: (np.zeros((1, 1, 1), np.float32), np.ones((2,), np.float32)))
    for name in ("src.KeypointFreeSfM", "src.KeypointFreeSfM.dataset", "src.KeypointFreeSfM.post_optimization",
                 "src.KeypointFreeSfM.post_optimization.utils", "src.KeypointFreeSfM.post_optimization.data_construct"):
        mod(name, __path__=[os.path.join(REF, *name.split("."))])
    mod("src.KeypointFreeSfM.post_optimization.utils.vis3d", vis_cameras_point_clouds=lambda *a, **k: None)


def sha(a) -> str:
    return hashlib.sha256(np.ascontiguousarray(a).tobytes()).hexdigest()


def main():
    _install_shims()
    sys.path.insert(0, REF)
    from src.KeypointFreeSfM.dataset.coarse_colmap_dataset import CoarseReconDataset
    from src.KeypointFreeSfM.post_optimization.data_construct.construct_matching_data import MatchingPairData
    from src.KeypointFreeSfM.post_optimization.data_construct.construct_optimization_data import ConstructOptimizationData
    from src.utils.colmap import read_write_model as rw
    from tests import sfm_tracks_oracle as orc

    m = orc.make_model(**CASE_ARGS)
    ko, to = m["kpt_offsets"], m["track_offsets"]
    ids, pids = m["image_ids"].tolist(), m["point_ids"].tolist()
    I = len(ids)
    names = [f"color/{n}.png" for n in range(I)]
    cameras, images, points3D = {}, {}, {}
    for n, cid in enumerate(ids):
        K = m["K"][n]
        cameras[n + 1] = rw.Camera(id=n + 1, model="PINHOLE", width=512, height=512, params=np.array([K[0, 0], K[1, 1], K[0, 2], K[1, 2]]))
        images[cid] = rw.Image(id=cid, qvec=rw.rotmat2qvec(m["R"][n]), tvec=m["t"][n], camera_id=n + 1, name=names[n],
                               xys=m["xys"][ko[n]:ko[n + 1]], point3D_ids=m["point3D_ids"][ko[n]:ko[n + 1]])
    for q, pid in enumerate(pids):
        sl = slice(to[q], to[q + 1])
        points3D[pid] = rw.Point3D(id=pid, xyz=m["xyz"][q], rgb=np.zeros(3, int), error=0.0, image_ids=m["image_ids"][m["track_image"][sl]],
                                   point2D_idxs=m["track_kpt"][sl])
    tmp = tempfile.mkdtemp()
    rw.write_model(cameras, images, points3D, tmp, ext=".bin")

    args = {"img_resize": None, "df": 8, "feature_track_assignment_strategy": "greedy", "verbose": False}
    ds = CoarseReconDataset(args, names, [], tmp, os.path.join(tmp, "refined"))
    assert list(ds.colmap_images) == ids and list(ds.colmap_3ds) == pids
    index_of = {cid: n for n, cid in enumerate(ids)}
    # the model as the reference holds it
    model = dict(m)
    model["R"] = np.stack([rw.qvec2rotmat(ds.colmap_images[c].qvec) for c in ids])
    model["K"] = np.stack([ds.colmap_frame_dict[c]["intrinsic"] for c in ids]).astype(np.float64)
    model["t"] = np.stack([ds.colmap_images[c].tvec for c in ids])
    for k in ("xys", "point3D_ids"):
        assert np.array_equal(np.concatenate([getattr(ds.colmap_images[c], k) for c in ids]), m[k]), k
    assert np.array_equal(np.stack([ds.colmap_3ds[p].xyz for p in pids]), m["xyz"]) and np.array_equal(model["t"], m["t"])
    assert np.abs(model["R"] - m["R"]).max() < 1e-12 and np.array_equal(model["K"], m["K"])

    out = {"model_" + k: v for k, v in model.items()}
    out.update({"input_sha256_" + k: np.array(sha(v)) for k, v in model.items()})
    state = np.concatenate([(ds.keyframe_dict[c]["state"] if c in ds.keyframe_dict else -np.ones(ko[n + 1] - ko[n])) for n, c in enumerate(ids)])
    # a frame that is no keyframe keeps its state inside get_keyframes_greedy only (-1 / -3): the stored state covers keyframes, -9 elsewhere
    covered = np.concatenate([np.full(ko[n + 1] - ko[n], c in ds.keyframe_dict) for n, c in enumerate(ids)])
    assert np.array_equal(state, state.astype(np.int64))
    out["state_keyframes"] = np.where(covered, state.astype(np.int64), -9)
    out["keyframes"] = np.array([index_of[c] for c in ds.keyframe_dict], np.int64)
    out["is_keyframe"] = np.array([ds.colmap_frame_dict[c]["is_keyframe"] for c in ids])
    out["assigned_image"] = np.array([index_of[ds.point_cloud_assigned_imgID_kptID[p][0]] for p in pids], np.int64)
    out["assigned_kpt"] = np.array([ds.point_cloud_assigned_imgID_kptID[p][1] for p in pids], np.int64)
    out["initial_depth"] = np.concatenate([(ds.colmap_frame_dict[c]["initial_depth"] if c in ds.keyframe_dict else -np.ones(ko[n + 1] - ko[n]))
                                           for n, c in enumerate(ids)])

    pairs = MatchingPairData(ds)
    rng = np.random.default_rng(11)
    fine, pl, pr, po, mk0, mk1, idx, mk1f = {}, [], [], [0], [], [], [], []
    for n in range(len(pairs)):
        item = pairs[n]
        a, b = item["frame0_colmap_id"], item["frame1_colmap_id"]
        k0, k1, ki = item["mkpts0_c"].numpy(), item["mkpts1_c"].numpy(), item["mkpts0_idx"].numpy()
        f = k1 + rng.standard_normal(k1.shape)
        fine[f"{a}-{b}"] = {"mkpts0_c": k0, "mkpts1_c": k1, "mkpts1_f": f, "mkpts0_idx": ki, "scale0": np.ones((1, 2)), "scale1": np.ones((1, 2))}
        pl.append(index_of[a])
        pr.append(index_of[b])
        mk0.append(k0)
        mk1.append(k1)
        idx.append(ki)
        mk1f.append(f)
        po.append(po[-1] + len(ki))
    out.update(pair_left=np.array(pl, np.int64), pair_right=np.array(pr, np.int64), pair_offsets=np.array(po, np.int64),
               mkpts0_c=np.concatenate(mk0), mkpts1_c=np.concatenate(mk1), mkpts0_idx=np.concatenate(idx).astype(np.int64),
               mkpts1_f=np.concatenate(mk1f))

    opt = ConstructOptimizationData(ds, fine)
    agg = {}
    for n in range(len(opt)):
        item = opt[n]
        nq = int(item["n_query"][0])
        for k, v in item.items():
            v = v.numpy()
            agg.setdefault(k, []).append(v[:nq] if k not in ("depth", "point_cloud_id", "n_query") else v.reshape(1, -1) if k == "depth" else v)
    for k, v in agg.items():
        out["agg_" + k] = np.concatenate(v).astype(np.float64)
    out["case_args"] = np.array(repr(sorted(CASE_ARGS.items())))
    path = os.path.join(HERE, "sfm_tracks_small.npz")
    np.savez_compressed(path, **out)
    print("wrote", path, os.path.getsize(path), "bytes; keyframes", out["keyframes"], "pairs", len(pl), "rows", len(out["mkpts0_idx"]),
          "optimiser rows", len(out["agg_mkpts1_f"]), "max track", opt.max_track_length)


if __name__ == "__main__":
    main()
