"""Device PnP without a GPU: the numpy oracle of its specification (``tests/pnp_device_oracle.py``) against the host solver, and the
interface of ``onepose_st_amd/pnp_device.py`` (header, binding, policy errors).  The kernels themselves: ``tests/test_gpu_pnp_device.py``.
"""
import os
import re
import subprocess
import sys

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import pnp_device_oracle as orc  # noqa: E402

from onepose_st_amd import cabi, hip, pnp  # noqa: E402

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
REPROJ = 5.0
POSE_BAR = 1e-4                  # the project's pose bar on |dR| and |dt| / |t|


# ---- sampler -----------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("n", [4, 5, 400])
def test_oracle_sampler_draws_three_distinct_rows(n):
    seen = set()
    for f in (0, 1, 3):
        for t in range(300):
            s = orc.sample_one(1, f, t, n)
            assert len(set(s)) == 3 and all(0 <= i < n for i in s), (f, t, s)
            seen.update(s)
    assert seen == set(range(n)) if n <= 5 else len(seen) > n // 2           # every row can be drawn
    assert orc.sample_one(1, 0, 0, 3) == (-1, -1, -1)


def test_oracle_sampler_pinned_values():
    # mix(G) is the first output of splitmix64 seeded with 0 (the published test vector of the generator)
    assert orc.mix(orc.G) == 0xE220A8397B1DCDAF
    pinned = {(1, 0, 0, 400): (65, 218, 334), (1, 0, 1, 400): (361, 317, 332), (1, 2, 1023, 65): (29, 24, 26), (12345, 1, 7, 5): (2, 4, 3),
              (2 ** 64 - 1, 3, 65535, 4): (3, 0, 1), (0, 0, 0, 4): (3, 0, 2)}
    for args, want in pinned.items():
        assert orc.sample_one(*args) == want, args
    # the third pick steps past the two earlier ones in ascending order: all (n - 2) values of the last draw reach distinct free rows
    rng = np.array([[0, 6]], dtype=np.int32)
    s = orc.sample(rng, 2000, 9)[0]
    assert {tuple(r) for r in s.tolist()} == {(a, b, c) for a in range(6) for b in range(6) for c in range(6) if len({a, b, c}) == 3}


# ---- P3P ---------------------------------------------------------------------------------------------------------------------------------------
def test_oracle_p3p_matches_the_host_solver_root_for_root():
    """200 seeded well-conditioned samples (``orc.p3p_samples``): the same number of roots as ``pnp.p3p`` and the poses matched root
    for root.  The host roots of a sample lie at least 1e-6 apart, so a difference below 1e-6 pairs them unambiguously: that is the
    assertion.  Measured here (x86-64, the AVX2 + FMA build of the host library): e_p3p = 2.61e-08, the largest relative pose
    difference (``orc.pose_distance``) over all roots; both sides are float64, the host compiled with contraction, and the worst
    sample's quartic amplifies a rounding by ~1e8.  DESIGN.md section 6l quotes it; the GPU test bounds the kernel by 10 x e_p3p."""
    samples = orc.p3p_samples()
    assert len(samples) == 200
    e_p3p, n_roots = 0.0, 0
    for ray, X, host in samples:
        mine = orc.p3p_one(ray, X)
        assert len(mine) == len(host) >= 1
        for a, b in zip(mine, host):
            e_p3p = max(e_p3p, orc.pose_distance(a, b))
        n_roots += len(host)
    print(f"e_p3p = {e_p3p:.3e} over {n_roots} roots")
    assert e_p3p < 1e-6


# ---- end to end ----------------------------------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def host_runs():
    """per frame kind: (K, pts2d, pts3d, [three host results])"""
    out = {}
    for hard in (False, True):
        K, p2, p3, _ = orc.c1_frame(hard, orc.FRAME_SEED)
        runs = [pnp.ransac_PnP(K, p2, p3, pnp_reprojection_error=REPROJ, use_pycolmap_ransac=True, seed=s) for s in (1, 2, 3)]
        out[hard] = (K, p2, p3, runs)
    return out


@pytest.mark.parametrize("hard", [False, True], ids=["planted", "hard"])
def test_oracle_end_to_end_matches_the_host_solver(host_runs, hard):
    """The planted c1 frame (563 matches, all correct) and the ``HARD_PROFILE`` c1 frame (563 matches, 197 of them wrong), object seed
    ``orc.FRAME_SEED``: three host runs agree on the inlier set and no match lies within 1e-6 thr2 of the threshold, so the set is a
    property of the frame; the oracle (1 024 trials, seeds 1 - 3) then returns that set and a pose within the pose bar.
    Measured: planted max 3.5e-12, hard max 2.1e-13 (oracle seed 1; the other seeds within 1e-10)."""
    K, p2, p3, runs = host_runs[hard]
    sets = [tuple(r[2].tolist()) for r in runs]
    assert sets[0] == sets[1] == sets[2] and len(sets[0]) >= 300
    rows = orc.prep(K, p2, p3, len(p2), None, 1)
    _, e2 = orc.residuals(runs[0][0][None], rows, orc._intr(K, 0))
    thr2 = REPROJ * REPROJ
    assert np.abs(e2[0] - thr2).min() > 1e-6 * thr2
    for seed in (1, 2, 3):
        o = orc.solve(K, p2, p3, reproj=REPROJ, trials=1024, seed=seed)
        assert o["status"][0] == 0 and o["n_inliers"][0] == len(sets[0])
        assert tuple(np.nonzero(o["mask"])[0].tolist()) == sets[0]
        d = orc.pose_distance(o["pose"][0], runs[0][0])
        print(f"{'hard' if hard else 'planted'} frame, oracle seed {seed}: pose distance to the host {d:.2e}")
        assert d < POSE_BAR


def test_oracle_edges():
    K, p2, p3, _ = orc.c1_frame(False, orc.FRAME_SEED)
    for n in (0, 3):
        o = orc.solve(K, p2[:n], p3[:n], trials=8)
        assert o["status"][0] == orc.STATUS_NO_POSE and np.array_equal(o["pose"][0], orc.IDENTITY) and o["n_inliers"][0] == 0
    # the confidence formula, at its three branches
    assert orc.needed_for(10, 10, 0.99) == 1 and orc.needed_for(0, 10, 0.99) == orc.MAX_NEEDED
    assert orc.needed_for(5, 10, 0.99) == np.ceil(np.log(0.01) / np.log(1 - 0.125)) == 35


# ---- interface ---------------------------------------------------------------------------------------------------------------------------------
def test_header_and_binding():
    from onepose_st_amd import pnp_device as pd

    header = cabi.parse(open(os.path.join(REPO, "include", "onepose_pnp_device.h")).read())
    assert header.defines["OPPNPD_ABI_VERSION"] == pd.ABI_VERSION == 1
    assert pd.DEFAULT_TRIALS == 10240 and pd.DEFAULT_TRIALS % 256 == 0 and pd.MAX_TRIALS == 65536
    assert (pd.STATUS_NO_POSE, pd.STATUS_NEEDS_MORE, pd.MIN_INLIERS, pd.MAX_NEEDED) == (orc.STATUS_NO_POSE, orc.STATUS_NEEDS_MORE, orc.MIN_INLIERS,
                                                                                      orc.MAX_NEEDED)
    for name, n_args in (("oppnpd_solve", 20), ("oppnpd_select", 20), ("oppnpd_refine", 16), ("oppnpd_score", 12), ("oppnpd_p3p", 9),
                         ("oppnpd_sample", 6), ("oppnpd_prep", 11), ("oppnpd_ranges", 6)):
        pd.check_arity(name, (0,) * n_args)
        with pytest.raises(TypeError, match=f"takes {n_args} arguments"):
            pd.check_arity(name, (0,) * (n_args + 1))
    # a library and a source list of its own; the host solver's header and the other device headers do not know these entry points
    for other in ("onepose_hip.h", "onepose_pnp.h", "onepose_sfm.h", "onepose_sfm_tracks.h", "onepose_sfm_triangulate.h", "onepose_sfm_fine.h"):
        assert "oppnpd_" not in open(os.path.join(REPO, "include", other)).read()
    mk = open(os.path.join(REPO, "onepose_st_amd", "csrc", "Makefile")).read()
    srcs = re.search(r"^SRCS := (.*)$", mk, re.M).group(1).split()
    assert "pnp_device.hip" not in srcs and re.search(r"^PND_SRCS := pnp_device.hip$", mk, re.M)

    def compile_line(obj):                       # what make would run for one object, however the Makefile writes its rules
        out = subprocess.run(["make", "-n", "-B", obj], cwd=os.path.join(REPO, "onepose_st_amd", "csrc"), check=True, capture_output=True, text=True)
        line, = [ln for ln in out.stdout.splitlines() if ln.endswith(f" -o {obj}")]
        return line.split()

    for obj in ("build/pnd/pnp_device.o", "build/sfm/sfm_objectblock.o", "build/sft/sfm_tracks.o", "build/str/sfm_triangulate.o", "build/trk/track_box.o"):
        assert "-ffp-contract=off" in compile_line(obj), obj
    assert "-ffp-contract=off" not in compile_line("build/trk/track_crop.o")      # that file writes its fused operations out itself
    # the package does not import the oracle
    for root, _, files in os.walk(os.path.join(REPO, "onepose_st_amd")):
        for fn in files:
            if fn.endswith(".py"):
                assert not re.search(r"^\s*(import|from)\s[^\n]*pnp_device_oracle", open(os.path.join(root, fn)).read(), re.M), fn


def test_built_library_exports_every_prototype():
    from onepose_st_amd import pnp_device as pd

    assert os.path.exists(pd.library_path()), "libonepose_pnp_device.so: run __graft_entry__.build()"
    # the argument checks run before any launch, so they answer without a device: -1 and a message
    assert pd.load().oppnpd_workspace_bytes(3000, 1, 10240) > 0 and pd.load().oppnpd_workspace_bytes(3000, 1, 65537) == 0
    with pytest.raises(ValueError, match="table sizes"):
        pd.call("oppnpd_solve", None, None, None, 0, None, 1, None, 1, 1.0, 5.0, 0.99, 1024, 1, None, 0, None, None, None, None, None)
    with pytest.raises(ValueError, match="null pointer"):
        pd.call("oppnpd_solve", None, None, None, 8, None, 1, None, 1, 1.0, 5.0, 0.99, 1024, 1, None, 0, None, None, None, None, None)
    with pytest.raises(ValueError, match="table sizes"):
        pd.call("oppnpd_sample", None, 1, 65537, 1, None, None)


def test_policy_and_cpu_tensors_raise():
    from onepose_st_amd import frameloop, pnp_device as pd

    K = np.eye(3)
    p2, p3 = torch.zeros(8, 2), torch.zeros(8, 3)
    with pytest.raises(NotImplementedError, match="dlt6"):
        pd.ransac_pnp(K, p2, p3, solver="dlt6")
    with pytest.raises(NotImplementedError, match="adaptive"):
        pd.ransac_pnp(K, p2, p3, use_pycolmap_ransac=False)
    with pytest.raises(hip.HipLibraryError, match="no CPU fallback"):
        pd.ransac_pnp(K, p2, p3)
    for bad in (dict(trials=0), dict(trials=65537), dict(confidence=1.0), dict(scale=0.0), dict(pnp_reprojection_error=-1.0)):
        with pytest.raises(ValueError):
            pd.ransac_pnp(K, p2, p3, **bad)
    with pytest.raises(ValueError, match="'host' or 'device'"):
        frameloop.SequenceRunner(None, {"keypoints3d": torch.zeros(1, 4, 3)}, K, np.zeros((8, 3)), None, pnp="gpu")
    import inspect
    assert inspect.signature(frameloop.SequenceRunner.__init__).parameters["pnp"].default == "host"
