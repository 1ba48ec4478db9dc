"""CPU side of the SfM fine matching over a pair list: the chunk / bucket planner, every input check, the header /
binding / library, the kernels' resource usage, ``to_reference_outputs`` on hand-made arrays, and that the GPU tests' pair list holds what
they rely on.  The file fails without the feature: the module, its header and its library do not exist."""
import os
import re
import shutil
import subprocess
import tempfile

import numpy as np
import pytest
import torch

from onepose_st_amd import cabi, hip, loftr
from tests import loftr_sfm_oracle as lsf
from tests import sfm_fine_cases as cases

REPO = os.path.abspath(os.path.join(os.path.dirname(__file__), ".."))
OBJDUMP = "/opt/rocm/lib/llvm/bin/llvm-objdump"


def test_product_module_exists_and_keeps_to_itself():
    import onepose_st_amd.sfm_fine as sf

    src = open(sf.__file__).read()
    assert "import oracle" not in src and "from tests" not in src and "from oracle" not in src


# ---- the planner ---------------------------------------------------------------------------------------------------------------------------
def _covered(chunks, M, chunk_rows, keys=None):
    """every row exactly once; chunks consecutive and in order, none above chunk_rows; buckets of one key each, ascending rows"""
    seen, at = [], 0
    for a, b, buckets in chunks:
        assert a == at and a < b <= M and b - a <= chunk_rows
        at = b
        rows_of_chunk = []
        assert [k for k, _ in buckets] == sorted({k for k, _ in buckets})
        for key, rows in buckets:
            assert rows.dtype == np.int64 and len(rows) and (np.diff(rows) > 0).all() and rows[0] >= a and rows[-1] < b
            if keys is not None:
                assert (np.asarray(keys)[rows] == key).all()
            rows_of_chunk += rows.tolist()
        assert sorted(rows_of_chunk) == list(range(a, b))
        seen += rows_of_chunk
    assert at == M and sorted(seen) == list(range(M))


@pytest.mark.parametrize("M,chunk_rows", [(0, 8), (1, 8), (1, 1), (8, 8), (9, 8), (300, 64), (300, 1 << 20), (300, 7)])
def test_planner_covers_every_row_once_in_order(M, chunk_rows):
    from onepose_st_amd import sfm_fine as sf

    chunks = sf.plan_chunks(M, chunk_rows)
    _covered(chunks, M, chunk_rows)
    assert len(chunks) == -(-M // chunk_rows)
    for a, b, buckets in chunks:                  # one bucket of consecutive rows
        assert len(buckets) == 1 and buckets[0][0] == 0 and buckets[0][1].tolist() == list(range(a, b))
    if M == 0:
        assert chunks == []


def test_planner_splits_pairs_and_separates_size_groups():
    from onepose_st_amd import sfm_fine as sf

    pairs = cases.pair_list()
    keys = cases.bucket_keys(pairs)
    off = pairs["pair_offsets"].tolist()
    M = off[-1]
    assert M == 300 and sorted(set(keys.tolist())) == [0, 1, 2, 3]          # all four (left group, right group) buckets occur
    for chunk_rows in (64, 100, 1 << 20):
        chunks = sf.plan_chunks(M, chunk_rows, keys)
        _covered(chunks, M, chunk_rows, keys)
    chunks = sf.plan_chunks(M, 64, keys)
    starts = [a for a, _, _ in chunks]
    assert starts == [0, 64, 128, 192, 256] and not set(starts[1:]) & set(off)      # every boundary falls inside a pair
    assert chunks[0][2][0][0] == 0 and len(chunks[0][2]) == 1                        # rows 0 .. 63: the pair (0, 1) alone
    # the whole list in one chunk: bucket (0, 0) holds the rows of pairs 0, 1, 2 and the single row of pair 5 (not consecutive)
    (_, _, buckets), = sf.plan_chunks(M, 1 << 20, keys)
    rows00 = dict(buckets)[0]
    assert rows00.tolist() == list(range(0, 155)) + [240]
    assert dict(buckets)[1].tolist() == list(range(155, 195)) and dict(buckets)[3].tolist() == list(range(195, 240))
    assert dict(buckets)[2].tolist() == list(range(241, 300))
    with pytest.raises(ValueError):
        sf.plan_chunks(M, 0, keys)
    with pytest.raises(ValueError):
        sf.plan_chunks(M, 64, keys[:-1])


def test_pair_list_holds_what_the_gpu_tests_rely_on():
    """both sides of every clip limit, the ties, a single-row pair, two pairs between the size groups, and no id outside its grid"""
    sc = cases.scales()
    for dtype in (torch.float32, torch.float64):
        p = cases.pair_list(dtype)
        off = p["pair_offsets"].tolist()
        assert (np.diff(off) == 1).sum() == 1
        n_clipped = 0
        for n, (l, r, _) in enumerate(cases.PAIRS):
            a, b = off[n], off[n + 1]
            data = {"mkpts0_c": p["mkpts0_c"][a:b].clone(), "mkpts1_c": p["mkpts1_c"][a:b].clone(), "hw0_i": cases.SIZES[l], "hw1_i": cases.SIZES[r],
                    "hw0_c": (cases.SIZES[l][0] // 8, cases.SIZES[l][1] // 8), "hw1_c": (cases.SIZES[r][0] // 8, cases.SIZES[r][1] // 8),
                    "scale0": sc[l:l + 1], "scale1": sc[r:r + 1]}
            _, ii, jj = lsf.coarse_ids(data)
            assert (ii >= 0).all() and (ii < data["hw0_c"][0] * data["hw0_c"][1]).all(), n
            assert (jj >= 0).all() and (jj < data["hw1_c"][0] * data["hw1_c"][1]).all(), n
            n_clipped += int((data["mkpts0_c"] != p["mkpts0_c"][a:b]).any(1).sum())
            if (l, r) == (0, 1):                  # half to even at unit scale: 0.5 -> 0, 1.5 -> 2, 2.5 -> 2
                assert (ii[:cases.N_TIES] % 16 == 2 * ((torch.arange(cases.N_TIES) + 1) // 2)).all()
        x, y = p["mkpts0_c"][:, 0], p["mkpts0_c"][:, 1]
        W = torch.tensor([cases.SIZES[i][1] for i in p["row_left"].tolist()])
        H = torch.tensor([cases.SIZES[i][0] for i in p["row_left"].tolist()])
        assert (x < 0).sum() >= 5 and (x > W - 2).sum() >= 5 and (y < 0).sum() >= 5 and (y > H - 2).sum() >= 3 and n_clipped >= 20


# ---- input checks --------------------------------------------------------------------------------------------------------------------------
def _matcher():
    return loftr.LoFTR_for_OnePose_Plus().eval()


def test_input_checks():
    from onepose_st_amd import sfm_fine as sf

    p = {k: v for k, v in cases.pair_list().items() if k in sf.PAIR_KEYS}
    assert sf.check_pairs(p, 5) == 300
    assert sf.check_pairs({k: v[:0] for k, v in p.items()}, 5) == 0
    for bad in (dict(p, mkpts0_c=p["mkpts0_c"].half()), dict(p, mkpts1_c=p["mkpts1_c"].long()), dict(p, row_left=p["row_left"].int()),
                dict(p, row_right=p["row_right"].double()), dict(p, mkpts0_c=p["mkpts0_c"][:, :1]), dict(p, row_left=p["row_left"][:, None]),
                dict(p, mkpts1_c=p["mkpts1_c"][:-1]), dict(p, row_left=p["row_left"][:-1]), dict(p, row_right=p["row_right"][:5]),
                {k: v for k, v in p.items() if k != "row_right"}):
        with pytest.raises(ValueError):
            sf.check_pairs(bad, 5)
    with pytest.raises(ValueError, match="unequal lengths"):
        sf.check_pairs(dict(p, mkpts1_c=p["mkpts1_c"][:-1]), 5)
    with pytest.raises(TypeError):
        sf.check_pairs(dict(p, row_left=p["row_left"].numpy()), 5)
    for key, value in (("row_left", 5), ("row_right", 7), ("row_left", -1)):          # an image index past the bank
        t = p[key].clone()
        t[17] = value
        with pytest.raises(IndexError, match=rf"{key}.*\[17\] = {value}"):
            sf.check_pairs(dict(p, **{key: t}), 5)
    assert sf.check_pairs(p, 4, ranges=False) == 300
    with pytest.raises(IndexError):
        sf.check_pairs(p, 4)
    # host tensors: no CPU fallback
    m = _matcher()
    with pytest.raises(hip.HipLibraryError):
        sf.fine_match_pairs(m, {"n_images": 5}, p)
    with pytest.raises(hip.HipLibraryError):
        sf.build_feature_bank(m, cases.images())
    with pytest.raises(ValueError, match="chunk_rows"):
        sf.fine_match_pairs(m, {"n_images": 5}, p, chunk_rows=0)
    # the bank's own checks come before anything runs
    with pytest.raises(ValueError, match="max_bytes"):
        sf.build_feature_bank(m, cases.images(), max_bytes=1000)
    assert sf.bank_bytes(cases.SIZES) == 4 * (3 * (48 * 64 * 128 + 12 * 16 * 256) + 2 * (32 * 48 * 128 + 8 * 12 * 256))
    with pytest.raises(ValueError, match="multiples of 8"):
        sf.build_feature_bank(m, [torch.zeros(1, 1, 60, 96)])
    with pytest.raises(ValueError):
        sf.build_feature_bank(m, cases.images(), scales=torch.ones(4, 2))
    with pytest.raises(ValueError):
        sf.build_feature_bank(m, cases.images(), scales=torch.ones(5, 2, dtype=torch.float64))
    with pytest.raises(ValueError):
        sf.build_feature_bank(m, cases.images(), max_batch=0)
    with pytest.raises(ValueError):
        sf.build_feature_bank(m, [])
    m.feature_hook = lambda *a: a
    with pytest.raises(NotImplementedError):
        sf.build_feature_bank(m, cases.images())
    with pytest.raises(NotImplementedError):
        sf.fine_match_pairs(m, {"n_images": 5}, p)
    with pytest.raises(NotImplementedError):
        sf.fine_match_pairs(loftr.LoFTR_for_OnePose_Plus(enable_fine_matching=False).eval(), {"n_images": 5}, p)


# ---- header, binding, library ----------------------------------------------------------------------------------------------------------------
def test_header_and_binding():
    from onepose_st_amd import sfm_fine as sf

    header = cabi.parse(open(os.path.join(REPO, "include", "onepose_sfm_fine.h")).read())
    assert header.defines["OPSFF_ABI_VERSION"] == sf.ABI_VERSION == 1
    assert header.defines["OPSFF_CTRL_INTS"] == sf.CTRL_INTS == 2 and header.defines["OPSFF_NO_ROW"] == sf.NO_ROW == 2 ** 31 - 1
    with pytest.raises(TypeError, match="takes 17 arguments"):
        sf.check_arity("opsff_row_ids", (1, 2, 3, 4))
    with pytest.raises(TypeError, match="takes 32 arguments"):
        sf.check_arity("opsff_sample_rows", (1,))
    # the other headers are not the place of these entry points, and the library has a source list of its own
    for other in ("onepose_hip.h", "onepose_sfm.h", "onepose_sfm_tracks.h", "onepose_sfm_triangulate.h"):
        assert "opsff_" not in open(os.path.join(REPO, "include", other)).read()
    mk = open(os.path.join(REPO, "onepose_st_amd", "csrc", "Makefile")).read()
    srcs = re.search(r"^SRCS := (.*)$", mk, re.M).group(1).split()
    assert "sfm_fine.hip" not in srcs and re.search(r"^SFF_SRCS := sfm_fine.hip$", mk, re.M)
    out = subprocess.run(["make", "-n", "-B", "build/sff/sfm_fine.o"], cwd=os.path.join(REPO, "onepose_st_amd", "csrc"), check=True, capture_output=True, text=True)
    line, = [ln for ln in out.stdout.splitlines() if ln.endswith(" -o build/sff/sfm_fine.o")]         # what make would run for the object
    assert "-ffp-contract=off" in line.split()


def test_built_library_exports_every_prototype():
    from onepose_st_amd import sfm_fine as sf

    assert os.path.exists(sf.library_path()), "libonepose_sfm_fine.so: run __graft_entry__.build()"


def test_fine_stage_takes_the_batch_indices_of_each_side():
    """``LoFTR_for_OnePose_Plus._fine``: the optional arguments default to today's behaviour"""
    import inspect

    sig = inspect.signature(loftr.LoFTR_for_OnePose_Plus._fine)
    assert sig.parameters["b_ids1"].default is None and sig.parameters["scale_ids"].default is None


@pytest.fixture(scope="module")
def fine_asm():
    """{kernel symbol: [instruction lines]} of the gfx950 code object bundled in libonepose_sfm_fine.so"""
    from onepose_st_amd import sfm_fine as sf

    if not os.path.exists(OBJDUMP):
        pytest.skip("llvm-objdump of the ROCm install not found")
    out = {}
    with tempfile.TemporaryDirectory() as tmp:
        so = os.path.join(tmp, "lib.so")
        shutil.copy(sf.library_path(), so)
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


def test_kernels_do_not_spill_and_keep_their_shape(fine_asm):
    for n, count in (("row_ids_kernel", 4), ("sample_rows_kernel", 1), ("init_ctrl_kernel", 1)):
        hits = [k for k in fine_asm if n in k]
        assert len(hits) == count, (n, sorted(fine_asm))
        for h in hits:
            spills = [t for t in fine_asm[h] if t.startswith("scratch_")]
            assert not spills, (h, spills[:4])
    sampler = fine_asm[[k for k in fine_asm if "sample_rows_kernel" in k][0]]
    # 16-byte row loads and stores (the correctly rounded divisions expand into FMA sequences, so contraction is pinned on the GPU)
    assert any(t.startswith("global_load_dwordx4") for t in sampler) and any(t.startswith("global_store_dwordx4") for t in sampler)


# ---- the reference's form ------------------------------------------------------------------------------------------------------------------
def test_to_reference_outputs_on_hand_made_arrays():
    from onepose_st_amd import sfm_fine as sf

    rng = np.random.default_rng(3)
    M = 6
    pairs = {"pair_left": torch.tensor([0, 2, 2]), "pair_right": torch.tensor([1, 0, 1]), "pair_offsets": torch.tensor([0, 3, 4, 6]),
             "mkpts0_idx": torch.tensor([4, 5, 9, 0, 1, 2])}
    model = {"image_ids": torch.tensor([30, 10, 20])}
    result = {"mkpts0_c": rng.standard_normal((M, 2)), "mkpts1_c": rng.standard_normal((M, 2)), "mkpts1_f": rng.standard_normal((M, 2)),
              "expec_f": rng.standard_normal((M, 3)).astype(np.float32), "i_ids": np.arange(M), "j_ids": np.arange(M),
              "feature_c0": rng.standard_normal((M, 256)).astype(np.float32), "feature_c1": rng.standard_normal((M, 256)).astype(np.float32),
              "feature0": rng.standard_normal((M, 128)).astype(np.float32), "feature1": rng.standard_normal((M, 128)).astype(np.float32)}
    result["mkpts0_f"] = result["mkpts0_c"]
    result = {k: torch.from_numpy(v) for k, v in result.items()}
    scales = torch.tensor([[1.0, 1.0], [1.25, 0.8], [0.5, 2.0]])
    out = sf.to_reference_outputs(result, pairs, model, scales)
    assert list(out) == ["30-10", "20-30", "20-10"]
    for (name, entry), (a, b), (l, r) in zip(out.items(), ((0, 3), (3, 4), (4, 6)), ((0, 1), (2, 0), (2, 1))):
        assert tuple(entry) == sf.REFERENCE_KEYS and len(entry) == 11
        for k in ("mkpts0_c", "mkpts1_c", "mkpts0_f", "mkpts1_f", "feature_c0", "feature_c1", "feature0", "feature1"):
            assert isinstance(entry[k], np.ndarray) and np.array_equal(entry[k], result[k].numpy()[a:b]) and entry[k].dtype == result[k].numpy().dtype, k
        assert entry["mkpts0_idx"].tolist() == pairs["mkpts0_idx"].tolist()[a:b]
        assert entry["scale0"].shape == (1, 2) and np.array_equal(entry["scale0"][0], scales[l].numpy())
        assert np.array_equal(entry["scale1"][0], scales[r].numpy()) and entry["scale1"].dtype == np.float32
        assert entry["feature_c0"].shape == (b - a, 256) and entry["feature1"].shape == (b - a, 128)
    ones = sf.to_reference_outputs(result, pairs, model)
    assert np.array_equal(ones["20-30"]["scale0"], np.ones((1, 2), np.float32))
    with pytest.raises(ValueError):
        sf.to_reference_outputs(dict(result, feature0=result["feature0"][:-1]), pairs, model, scales)
    with pytest.raises(ValueError):
        sf.to_reference_outputs(result, pairs, model, scales[:2])
