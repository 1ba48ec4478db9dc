"""CPU side of the SfM track assignment: the oracle equals the reference's golden, its two forms agree, a
hand-worked case, every input check, the header / binding / library, the kernels' resource usage, and that the GPU tests' inputs tell
every seeded fault from the truth."""
import os
import re
import shutil
import subprocess
import tempfile

import numpy as np
import pytest
import torch

from onepose_st_amd import cabi, hip
from tests import sfm_tracks_oracle as orc

REPO = os.path.abspath(os.path.join(os.path.dirname(__file__), ".."))
OBJDUMP = "/opt/rocm/lib/llvm/bin/llvm-objdump"
ALL_KEYS = orc.PLAN_KEYS + orc.PAIR_KEYS + orc.ROW_KEYS


def _same(a, b):
    a, b = np.asarray(a), np.asarray(b)
    return a.shape == b.shape and a.dtype == b.dtype and a.tobytes() == b.tobytes()


def forms_agree(m, r, v):
    """every key bit for bit, but the depth: numpy's matmul against the written-out sums, inside the forward-error bound"""
    bad = [k for k in ALL_KEYS if k != "initial_depth" and not _same(r[k], v[k])]
    bound = orc.depth_bound(m, v["state"])
    if not (np.abs(r["initial_depth"] - v["initial_depth"]) <= bound).all() or not _same(r["initial_depth"] == -1, v["initial_depth"] == -1):
        bad.append("initial_depth")
    return bad


def golden_mismatches(npz, m, got, agg=None):
    """keys of ``got`` (the flat result dict) that differ from what the reference's classes gave; with ``agg`` also the optimiser's
    aggregated arrays.  Integers and keypoint copies exactly, the depth inside ``oracle.depth_bound``."""
    bad = [k for k in ("keyframes", "is_keyframe", "assigned_image", "assigned_kpt", "pair_left", "pair_right", "pair_offsets", "mkpts0_c",
                       "mkpts1_c", "mkpts0_idx") if not _same(got[k], npz[k])]
    covered = npz["state_keyframes"] != -9
    if not np.array_equal(got["state"][covered], npz["state_keyframes"][covered]) or (got["state"][~covered] >= 0).any():
        bad.append("state")
    bound = orc.depth_bound(m, got["state"])
    if not (np.abs(got["initial_depth"] - npz["initial_depth"]) <= bound).all() or not np.array_equal(got["initial_depth"] == -1, npz["initial_depth"] == -1):
        bad.append("initial_depth")
    if not np.array_equal(got["n_query"], npz["agg_n_query"]) or not np.array_equal(m["image_ids"][got["ref_image"]], npz["agg_right_colmap_ids"]):
        bad.append("rows")
    if got["fine_row"].max() >= len(npz["mkpts1_f"]) or not _same(npz["mkpts1_f"][got["fine_row"]], npz["agg_mkpts1_f"]):
        bad.append("fine_row")
    if agg is not None:
        slots = m["kpt_offsets"][got["assigned_image"]] + got["assigned_kpt"]
        for k in ("n_query", "intrinsic0", "intrinsic1", "mkpts0_c", "mkpts1_c", "mkpts1_f", "left_colmap_ids", "right_colmap_ids", "point_cloud_id"):
            if not _same(np.asarray(agg[k], dtype=np.float64), npz["agg_" + k]):
                bad.append("agg_" + k)
        if agg["depth"].shape != npz["agg_depth"].shape or not (np.abs(agg["depth"] - npz["agg_depth"])[:, 0] <= bound[slots]).all():
            bad.append("agg_depth")
    return bad


def test_product_module_exists_and_keeps_to_itself():
    import onepose_st_amd.sfm_tracks as st

    src = open(st.__file__).read()
    assert "import oracle" not in src and "from tests" not in src and "from oracle" not in src


def test_hand_case():
    """What ``oracle.hand_case`` must give, worked by hand.

    Unoccupied counts: image 0: 3, image 1: 4, image 2: 4, image 3: 2.  Round 1: stable descending order 1, 2, 0, 3: image 1 takes A (k0), D
    (k1 and k2: the later keypoint 2 is assigned) and E (k3), and robs A's (2, 2), (0, 0), (2, 1), D's (3, 2) and E's (2, 4).  Counts: image
    2: 1, image 0: 2, image 3: 1; the carried order 2, 0, 3 sorts to 0, 2, 3: image 0 takes B (k1) and C (k3) and robs (2, 0) and (3, 0).
    Every point is assigned: two keyframes."""
    m = orc.hand_case()
    r = orc.reference_form(m)
    assert r["keyframes"].tolist() == [1, 0] and r["is_keyframe"].tolist() == [True, True, False, False]
    assert r["state"].tolist() == [-3, 9, -1, 2, 5, 7, 7, 4, -3, -3, -3, -1, -3, -3, -1, -3]
    assert r["assigned_image"].tolist() == [1, 0, 0, 1, 1] and r["assigned_kpt"].tolist() == [0, 1, 3, 2, 3]
    # left images in image order (0, then 1); right images by id: for image 1 (id 10) ids 20, 30, 40 = images 2, 0, 3
    assert r["pair_left"].tolist() == [0, 0, 1, 1, 1] and r["pair_right"].tolist() == [2, 3, 2, 0, 3]
    assert r["pair_offsets"].tolist() == [0, 1, 2, 4, 5, 7] and r["mkpts0_idx"].tolist() == [1, 3, 0, 3, 0, 1, 2]
    ko = m["kpt_offsets"]
    assert _same(r["mkpts0_c"][2], m["xys"][ko[1] + 0]) and _same(r["mkpts1_c"][2], m["xys"][ko[2] + 2])      # A in image 2: first occurrence k2
    assert _same(r["mkpts1_c"][6], m["xys"][ko[3] + 2]) and _same(r["mkpts1_c"][5], m["xys"][ko[3] + 2])      # D's two slots, one partner
    # rows: A -> images 2 (the keypoint of its LAST occurrence, 1) and 0; B -> 2; C -> 3; D -> 3; E -> 2
    assert r["n_query"].tolist() == [2, 1, 1, 1, 1] and r["row_offsets"].tolist() == [0, 2, 3, 4, 5, 6]
    assert r["ref_image"].tolist() == [2, 0, 2, 3, 3, 2] and r["ref_kpt"].tolist() == [1, 0, 0, 0, 2, 4]
    assert r["fine_row"].tolist() == [2, 4, 0, 1, 6, 3]                    # D is assigned keypoint 2: row 6, not row 5
    # the depth of slot 4 = (image 1, k0) = point A
    X, K, R, t = m["xyz"][0], m["K"][1], m["R"][1], m["t"][1]
    assert abs(r["initial_depth"][4] - (K @ (R @ X + t))[2]) <= orc.depth_bound(m, r["state"])[4]
    assert (r["initial_depth"][r["state"] < 0] == -1).all() and (r["initial_depth"][r["state"] >= 0] > 0).all()
    assert forms_agree(m, r, orc.vectorised_form(m)) == []


def test_carried_order_tie():
    """``oracle.tie_case``: after round 1 the counts of images 0 and 1 tie at 3; the carried order 1, 3, 0 puts image 1 first, the initial
    order would put image 0 first"""
    m = orc.tie_case()
    r = orc.reference_form(m)
    assert r["keyframes"].tolist() == [2, 1, 0]
    assert orc.reference_form(m, fault="tie_initial_order")["keyframes"].tolist()[:2] == [2, 0]
    assert forms_agree(m, r, orc.vectorised_form(m)) == []


def test_oracle_equals_the_reference_golden(golden_dir):
    """both forms of the oracle against what the reference's own classes gave (tests/golden/make_golden_sfm_tracks.py); the depth of the
    oracle against the golden stays inside the bound the GPU test applies"""
    import hashlib

    npz = np.load(os.path.join(golden_dir, "sfm_tracks_small.npz"))
    m = orc.golden_model(npz)
    for k, v in m.items():
        assert hashlib.sha256(np.ascontiguousarray(v).tobytes()).hexdigest() == str(npz["input_sha256_" + k]), k
    for form in (orc.reference_form, orc.vectorised_form):
        res = form(m)
        agg = orc.optimizer_inputs(m, res, npz["mkpts1_f"])
        assert golden_mismatches(npz, m, res, agg) == [], form.__name__
    assert len(npz["keyframes"]) >= 2 and (~npz["is_keyframe"]).sum() >= 2 and (np.diff(m["image_ids"]) < 0).any()
    for f in orc.FAULTS:
        if f != "tie_initial_order":                                       # the golden model holds no such tie: tie_case does
            assert golden_mismatches(npz, m, orc.reference_form(m, fault=f)) != [], f


@pytest.mark.parametrize("kw", [dict(seed=5, Q=300, I=12, mean_track=6, n_dup=25, shuffle_ids=True, empty_images=(4,)),
                                dict(seed=13, Q=300, I=10, mean_track=5, n_dup=60), dict(seed=9, Q=200, I=12, mean_track=5, n_dup=10, long_track=1300),
                                dict(seed=31, Q=200, I=8, mean_track=5, n_dup=10, shuffle_ids=True), dict(seed=41, Q=300, I=10, mean_track=5, shuffle_ids=True)])
def test_vectorised_form_equals_reference_form(kw):
    m = orc.make_model(**kw)
    assert forms_agree(m, orc.reference_form(m), orc.vectorised_form(m)) == []


def test_inputs_discriminate_faults():
    """the tests that tests/test_gpu_sfm_tracks.py lists per fault: the oracle with that fault differs from the oracle on their inputs"""
    cases = {"hand": orc.hand_case(), "tie": orc.tie_case(), "duplicates": orc.make_model(13, 300, 10, 5, n_dup=60),
             "shuffled": orc.make_model(5, 300, 12, 6, n_dup=25, shuffle_ids=True, empty_images=(4,)),
             "long_track": orc.make_model(9, 200, 12, 5, n_dup=10, long_track=1300)}
    listed = {"tie_initial_order": ("tie", "long_track"), "first_keypoint_wins": ("hand", "duplicates", "shuffled", "long_track"),
              "right_by_index": ("hand", "shuffled"), "last_occurrence": ("hand", "duplicates", "shuffled", "long_track"),
              "robbed_is_owned": tuple(cases)}
    truth = {k: orc.reference_form(m) for k, m in cases.items()}
    for fault, names in listed.items():
        for n in names:
            try:
                bad = orc.reference_form(cases[n], fault=fault)
            except (AssertionError, KeyError):
                continue                                                   # the fault breaks the reference's own invariants: told apart
            assert any(not _same(truth[n][k], bad[k]) for k in ALL_KEYS), (fault, n)


def _tensors(m):
    return {k: torch.from_numpy(np.ascontiguousarray(v)) for k, v in m.items()}


def test_input_checks():
    from onepose_st_amd import sfm_tracks as st

    t = _tensors(orc.hand_case())
    d = st.check_model(t)
    assert (d["I"], d["U"], d["Q"], d["E"], d["max_slots"]) == (4, 16, 5, 13, 5)
    assert d["slot_point"].tolist() == [0, 1, -1, 2, 0, 3, 3, 4, 1, 0, 0, -1, 4, 2, -1, 3]
    with pytest.raises(hip.HipLibraryError):
        st.assign_tracks(t)
    with pytest.raises(NotImplementedError):
        st.assign_tracks(t, feature_track_assignment_strategy="balanced")
    with pytest.raises(ValueError, match="lacks"):
        st.check_model({k: v for k, v in t.items() if k != "xyz"})

    def model(**kw):
        return dict(t, **kw)

    def changed(key, index, value):
        v = t[key].clone()
        v[index] = value
        return model(**{key: v})

    for bad in (model(xys=t["xys"].float()), model(point3D_ids=t["point3D_ids"].int()), model(K=t["K"][:3]), model(xyz=t["xyz"][:, :2]),
                model(kpt_offsets=torch.tensor([0, 4, 3, 13, 16])), model(kpt_offsets=torch.tensor([0, 4, 8, 13, 15])),
                model(track_offsets=torch.tensor([0, 4, 4, 8, 11, 13])),                            # a point without element
                model(track_offsets=torch.tensor([0, 4, 6, 8, 11, 12])),
                changed("xys", (3, 0), float("nan")), changed("xyz", (1, 2), float("inf")), changed("t", (0, 0), float("nan")),
                changed("point_ids", 1, 5), changed("image_ids", 2, 30), changed("point_ids", 0, -5), changed("point3D_ids", 2, -2),
                changed("point_ids", 0, 2 ** 53), changed("image_ids", 0, 2 ** 53),
                changed("point3D_ids", 2, 77),                                                      # an id no point carries
                changed("point3D_ids", 2, 9),                                                       # a slot of B that B's track does not hold
                changed("point3D_ids", 0, -1),                                                      # A's track names a slot without A
                changed("track_kpt", 1, 1)):                                                        # A's element (0, 1) is B's slot
        with pytest.raises(ValueError):
            st.check_model(bad)
    for bad in (changed("track_image", 0, 4), changed("track_image", 0, -1), changed("track_kpt", 4, 5), changed("track_kpt", 0, -1)):
        with pytest.raises(IndexError):
            st.check_model(bad)
    big = orc.make_model(1, 10, 4, 2)
    big["image_ids"] = np.arange(st.MAX_IMAGES + 1)
    with pytest.raises(ValueError, match="at most"):
        st.check_model(_tensors(big))


def test_header_and_binding():
    from onepose_st_amd import sfm_tracks as st

    header = cabi.parse(open(os.path.join(REPO, "include", "onepose_sfm_tracks.h")).read())
    assert header.defines["OPSFT_ABI_VERSION"] == st.ABI_VERSION == 1
    assert header.defines["OPSFT_MAX_IMAGES"] == st.MAX_IMAGES == 1024
    with pytest.raises(TypeError, match="takes 13 arguments"):
        st.check_arity("opsft_finish", (1, 2, 3, 4))
    # the other headers are not the place of these entry points, and the library has a source list of its own
    for other in ("onepose_hip.h", "onepose_sfm.h"):
        assert "opsft_" not in open(os.path.join(REPO, "include", other)).read()
    mk = open(os.path.join(REPO, "onepose_st_amd", "csrc", "Makefile")).read()
    srcs = re.search(r"^SRCS := (.*)$", mk, re.M).group(1).split()
    assert "sfm_tracks.hip" not in srcs and re.search(r"^SFT_SRCS := sfm_tracks.hip$", mk, re.M)


def test_built_library_exports_every_prototype():
    from onepose_st_amd import sfm_tracks as st

    assert os.path.exists(st.library_path()), "libonepose_sfm_tracks.so: run __graft_entry__.build()"


@pytest.fixture(scope="module")
def tracks_asm():
    """{kernel symbol: [instruction lines]} of the gfx950 code object bundled in libonepose_sfm_tracks.so"""
    from onepose_st_amd import sfm_tracks as st

    if not os.path.exists(OBJDUMP):
        pytest.skip("llvm-objdump of the ROCm install not found")
    out = {}
    with tempfile.TemporaryDirectory() as tmp:
        so = os.path.join(tmp, "lib.so")
        shutil.copy(st.library_path(), so)
        subprocess.run([OBJDUMP, "--offloading", so], cwd=tmp, check=True, capture_output=True)
        for name in sorted(os.listdir(tmp)):
            if not name.endswith("gfx950"):
                continue
            text = subprocess.run([OBJDUMP, "-d", os.path.join(tmp, name)], check=True, capture_output=True, text=True).stdout
            cur = None
            for line in text.splitlines():
                hit = re.match(r"^[0-9a-f]+ <(\S+)>:$", line)
                if hit:
                    cur = out.setdefault(hit.group(1), [])
                elif cur is not None and line.startswith("\t"):
                    cur.append(line.strip().split("//")[0].strip())
    return out


def test_kernels_do_not_spill(tracks_asm):
    names = ("select_kernel", "take_kernel", "finish_kernel", "track_rows_kernel", "pair_keys_kernel", "pair_emit_kernel", "fine_rows_kernel")
    for n in names:
        hits = [k for k in tracks_asm if n in k]
        assert len(hits) == 1, (n, sorted(tracks_asm))
        spills = [t for t in tracks_asm[hits[0]] if t.startswith("scratch_")]
        assert not spills, (n, spills[:4])
    # the rounds use integer atomics only, and no workgroup waits for another: no sleep loop in the two kernels of a round
    for n in ("select_kernel", "take_kernel"):
        ins = tracks_asm[[k for k in tracks_asm if n in k][0]]
        assert not any(t.startswith("s_sleep") for t in ins), n
        assert not any(re.match(r"(global|flat)_atomic_\w*(f32|f64|pk)", t) for t in ins), n
