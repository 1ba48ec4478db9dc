"""bench.py --dump-outputs without a GPU: what output_arrays keeps of a step's results, in which dtypes, within which size, and that the
conf_matrix sample is the same draw every time."""
import os
import subprocess
import sys

import numpy as np
import torch

import bench

REPO = os.path.abspath(os.path.join(os.path.dirname(__file__), ".."))


def _step(B=1, N=50, M=40, K=30, seed=0):
    g = torch.Generator().manual_seed(seed)
    data = {
        "keypoints3d": torch.rand(B, N, 3, generator=g),          # an input that travels in the same dict: not an output
        "conf_matrix": torch.rand(B, N, M, generator=g),
        "b_ids": torch.zeros(K, dtype=torch.int64), "i_ids": torch.randperm(N, generator=g)[:K], "j_ids": torch.randint(M, (K,), generator=g),
        "m_bids": torch.zeros(K, dtype=torch.int64), "gt_mask": torch.zeros(K, dtype=torch.bool), "mconf": torch.rand(K, generator=g),
        "mkpts_3d_db": torch.rand(K, 3, generator=g), "mkpts_query_c": torch.rand(K, 2, generator=g),
        "mkpts_query_f": torch.rand(K, 2, generator=g), "expec_f": torch.rand(K, 3, generator=g),
    }
    poses = [(np.eye(3, 4) + b, 20 + b, 0) for b in range(B)]
    return data, poses


def test_outputs_are_float32_or_float64_and_exact():
    data, poses = _step()
    out = bench.output_arrays(data, poses)
    assert set(out) == set(bench.MATCH_KEYS) | {"conf_matrix", "pose", "pnp_inliers", "pnp_status"}
    assert all(a.dtype in (np.float32, np.float64) for a in out.values())
    assert out["i_ids"].dtype == np.float64 and np.array_equal(out["i_ids"], data["i_ids"].numpy())
    assert out["mconf"].dtype == np.float32 and np.array_equal(out["mconf"], data["mconf"].numpy())
    assert np.array_equal(out["conf_matrix"], data["conf_matrix"].numpy())
    assert out["pose"].shape == (1, 3, 4) and out["pnp_inliers"].tolist() == [20.0]


def test_large_conf_matrix_is_a_fixed_sample_of_whole_rows(monkeypatch):
    monkeypatch.setattr(bench, "DUMP_CONF_ENTRIES", 400)
    data, _ = _step(B=2)
    a, b = bench.output_arrays(data), bench.output_arrays(dict(data))
    assert "conf_matrix" not in a
    rows = a["conf_matrix_row_index"].astype(np.int64)
    assert len(rows) == 400 // 40 and np.array_equal(rows, np.sort(rows)) and np.array_equal(rows, b["conf_matrix_row_index"])
    assert np.array_equal(a["conf_matrix_rows"], data["conf_matrix"].reshape(100, 40).numpy()[rows])


def test_total_stays_within_the_budget(monkeypatch):
    data, poses = _step(K=2000, N=3000, M=4)
    full = bench.output_arrays(data, poses)
    cap = sum(v.nbytes for v in full.values()) // 2
    monkeypatch.setattr(bench, "DUMP_BYTES_MAX", cap)
    out = bench.output_arrays(data, poses)
    assert sum(v.nbytes for v in out.values()) <= cap
    pick = out["match_index"].astype(np.int64)
    assert 0 < len(pick) < 2000 and all(len(out[k]) == len(pick) for k in bench.MATCH_KEYS)
    assert np.array_equal(out["mkpts_query_f"], full["mkpts_query_f"][pick])


def test_lazy_conf_matrix_is_not_computed_for_the_dump():
    data, _ = _step()
    data["conf_matrix"] = object()          # the lazy form: never computed by the timed path
    assert not any(k.startswith("conf_matrix") for k in bench.output_arrays(data))


def test_write_outputs_round_trip(tmp_path):
    data, poses = _step()
    arrays = bench.output_arrays(data, poses)
    info = bench.write_outputs(str(tmp_path / "out"), arrays)
    assert info["files"] == sorted(arrays) and info["bytes"] == sum(a.nbytes for a in arrays.values())
    for name, a in arrays.items():
        back = np.load(tmp_path / "out" / f"{name}.npy")
        assert back.dtype == a.dtype and np.array_equal(back, a)


def test_steps_below_one_is_refused():
    p = subprocess.run([sys.executable, os.path.join(REPO, "bench.py"), "--steps", "0"], capture_output=True, text=True, timeout=120)
    assert p.returncode == 2 and "--steps" in p.stderr
