"""The SfM calls of the LoFTR matcher without a GPU: the oracle sampler (tests/loftr_sfm_oracle.py) against hand-computed samples of
the reference formula, the input forms that still raise, a well-formed call on CPU tensors, the new C entries in the header, the binding
and the built library, and the emitted code of the new kernels."""
import ctypes
import os

import pytest
import torch

from onepose_st_amd import hip, loftr
from tests import loftr_sfm_oracle as lsf
from tests.test_disasm_guards import device_asm  # noqa: F401  (fixture)

NEW_ENTRIES = ("ophip_loftr_coarse_ids", "ophip_sample_features", "ophip_fine2_match_scaled")


def _ramp_map(C, h, w, dtype=torch.float32):
    """map[c, y, x] = 100 c + 10 y + x: bilinear sampling inside the map is exact on it"""
    c, y, x = torch.meshgrid(torch.arange(C), torch.arange(h), torch.arange(w), indexing="ij")
    return (100.0 * c + 10.0 * y + x).to(dtype)[None]


@pytest.mark.parametrize("kdtype", [torch.float32, torch.float64])
def test_oracle_sampler_against_the_reference_formula(kdtype):
    """map 5 x 9 against an image extent of 9 x 17 (scale (1.5, 0.5) on 6 x 34): a keypoint k lands on map pixel k / 2, exactly in
    float32 (the extents minus one are powers of two), so half-integer map coordinates stay exact"""
    C, h, w = 3, 5, 9
    fmap = _ramp_map(C, h, w)
    scale = torch.tensor([[1.5, 0.5]])
    hw = lsf.imghw(scale, (6, 34))
    assert hw.tolist() == [9.0, 17.0]
    kp = torch.tensor([[0.0, 0.0], [2.0, 4.0], [12.0, 8.0], [3.0, 5.0], [1.0, 1.0], [5.0, 3.0], [2.5, 7.0], [-1.0, 2.0], [14.0, 2.0],
                       [4.0, -3.0], [-3.0, -3.0], [0.5, 8.5], [17.0, 3.0], [-1.5, 3.0], [16.0, 9.0]], dtype=kdtype)
    u, v = kp[:, 0].double() / 2, kp[:, 1].double() / 2                      # map coordinates
    bil = lsf.sample_feature_from_featuremap(fmap, kp, hw, "bilinear")
    near = lsf.sample_feature_from_featuremap(fmap, kp, hw, "nearest")
    assert bil.shape == (len(kp), C) and bil.dtype == torch.float32 and near.dtype == torch.float32
    for r in range(len(kp)):
        x, y = float(u[r]), float(v[r])
        want_b = torch.zeros(C, dtype=torch.float64)
        if 0 <= x <= w - 1 and 0 <= y <= h - 1:
            want_b = (100.0 * torch.arange(C) + 10 * y + x).double()
        elif -1 < x < w and -1 < y < h:                  # partly outside: zero padding weighs the missing corners with 0
            x0, y0 = int(torch.floor(torch.tensor(x))), int(torch.floor(torch.tensor(y)))
            for yy, xx, wt in ((y0, x0, (x0 + 1 - x) * (y0 + 1 - y)), (y0, x0 + 1, (x - x0) * (y0 + 1 - y)),
                               (y0 + 1, x0, (x0 + 1 - x) * (y - y0)), (y0 + 1, x0 + 1, (x - x0) * (y - y0))):
                if 0 <= yy < h and 0 <= xx < w:
                    want_b += wt * (100.0 * torch.arange(C) + 10 * yy + xx).double()
        assert torch.allclose(bil[r].double(), want_b, atol=1e-4), (r, bil[r], want_b)
        rx, ry = round(x), round(y)                      # Python's round: half to even, as grid_sample's nearbyint
        want_n = torch.zeros(C, dtype=torch.float64)
        if 0 <= rx <= w - 1 and 0 <= ry <= h - 1:
            want_n = (100.0 * torch.arange(C) + 10 * ry + rx).double()
        assert torch.equal(near[r].double(), want_n), (r, near[r], want_n)
    # the exact half-integers: 0.5 -> 0, 1.5 -> 2, 2.5 -> 2 (kp (1, 1), (3, 5), (5, 3))
    assert near[4].tolist() == [0.0, 100.0, 200.0] and near[3].tolist()[0] == 10 * 2 + 2 and near[5].tolist()[0] == 10 * 2 + 2
    assert (bil[9:11] == 0).all() and (near[9:11] == 0).all()                      # above / left of the image: zero padding
    # the normalised grid is computed in the keypoints' dtype, then cast
    g = lsf.sample_grid(kp, hw)
    assert g.dtype == torch.float32 and g.shape == (1, len(kp), 1, 2)
    assert torch.equal(g[0, :, 0], ((((kp - 0.5) + 0.5) / torch.tensor([16.0, 8.0], dtype=kdtype)) * 2 - 1).float())


def _images(V=1, V1=1, H=64, W=96):
    return torch.zeros(V, 1, H, W), torch.zeros(V1, 1, H, W)


def _well_formed(kdtype=torch.float32):
    i0, i1 = _images()
    return {"image0": i0, "image1": i1, "scale0": torch.tensor([[1.0, 1.25]]), "scale1": torch.tensor([[0.8, 1.0]]),
            "mkpts0_c": torch.rand(5, 2, dtype=kdtype) * 50, "mkpts1_c": torch.rand(5, 2, dtype=torch.float64) * 50}


def test_input_forms_that_still_raise():
    m = loftr.LoFTR_for_OnePose_Plus().eval()
    i0, i1 = _images()
    for k in ("mask0", "mask1", "scale0", "scale1", "mkpts0_c", "mkpts1_c"):        # the zeros(1) forms: wrong shape or no partner
        with pytest.raises(NotImplementedError):
            m({"image0": i0, "image1": i1, k: torch.zeros(1)})
    bad = [
        {"mask0": torch.ones(1, 64, 96), "mask1": torch.ones(1, 64, 96)},
        {"scale0": torch.ones(1, 2)},                                               # no partner
        {"scale0": torch.ones(1, 2, dtype=torch.float64), "scale1": torch.ones(1, 2, dtype=torch.float64)},
        {"scale0": torch.ones(2), "scale1": torch.ones(2)},
        {"scale0": torch.ones(1, 3), "scale1": torch.ones(1, 3)},
        {"mkpts0_c": torch.ones(4, 2)},
        {"mkpts0_c": torch.ones(4, 2, dtype=torch.float16), "mkpts1_c": torch.ones(4, 2, dtype=torch.float16)},
        {"mkpts0_c": torch.ones(4, 3), "mkpts1_c": torch.ones(4, 3)},
        {"mkpts0_c": torch.ones(4, 2), "mkpts1_c": torch.ones(5, 2)},
        {"mkpts0_c": torch.ones(4, 2, dtype=torch.int64), "mkpts1_c": torch.ones(4, 2, dtype=torch.int64)},
    ]
    for extra in bad:
        with pytest.raises(NotImplementedError):
            m({"image0": i0, "image1": i1, **extra})
    # V > 1 with provided matches or with extraction; scale1 [1, 2] against a batch-V image1
    i0v, i1v = _images(V=2, V1=1)
    with pytest.raises(NotImplementedError):
        m({"image0": i0v, "image1": i1v, "mkpts0_c": torch.ones(3, 2), "mkpts1_c": torch.ones(3, 2)})
    with pytest.raises(NotImplementedError):
        m({"image0": i0v, "image1": i1v, "scale0": torch.ones(2, 2), "scale1": torch.ones(1, 2)}, extract_fine_feature=True)
    i0v, i1v = _images(V=2, V1=2)
    with pytest.raises(NotImplementedError):
        m({"image0": i0v, "image1": i1v, "scale0": torch.ones(2, 2), "scale1": torch.ones(1, 2)})
    with pytest.raises(NotImplementedError):
        m({"image0": i0v, "image1": i1v, "scale0": torch.ones(1, 2), "scale1": torch.ones(2, 2)})
    # coarse extraction with a feature hook
    m.feature_hook = lambda *a: a
    with pytest.raises(NotImplementedError):
        m(_well_formed(), extract_coarse_feature=True)
    m.feature_hook = None
    # extraction without scales: the reference's KeyError
    with pytest.raises(KeyError):
        m({"image0": i0, "image1": i1}, extract_fine_feature=True)
    with pytest.raises(KeyError):
        m({"image0": i0, "image1": i1, "mkpts0_c": torch.ones(3, 2), "mkpts1_c": torch.ones(3, 2)}, extract_coarse_feature=True)


@pytest.mark.parametrize("kdtype", [torch.float32, torch.float64])
def test_a_well_formed_call_on_cpu_tensors_raises_the_library_error(kdtype):
    m = loftr.LoFTR_for_OnePose_Plus().eval()
    for kwargs in ({}, {"extract_coarse_feature": True, "extract_fine_feature": True}, {"extract_fine_feature": False}):
        with pytest.raises(hip.HipLibraryError):
            m(_well_formed(kdtype), **kwargs)
    d = _well_formed()
    del d["mkpts0_c"], d["mkpts1_c"]                       # the SfM coarse call: scales only
    with pytest.raises(hip.HipLibraryError):
        m(d)
    m2 = loftr.LoFTR_for_OnePose_Plus(enable_fine_matching=False).eval()
    i0v, i1v = _images(V=3, V1=1)
    with pytest.raises(hip.HipLibraryError):               # batched pairs with one shared scale for the query
        m2({"image0": i0v, "image1": i1v, "scale0": torch.ones(3, 2), "scale1": torch.ones(1, 2)})


def test_new_entries_are_declared_registered_and_exported():
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    with open(os.path.join(root, "include", "onepose_hip.h")) as f:
        header = f.read()
    with open(os.path.join(root, "onepose_st_amd", "csrc", "Makefile")) as f:
        assert "loftr_sfm.hip" in f.read()
    lib = ctypes.CDLL(hip.library_path())
    for name in NEW_ENTRIES:
        assert f"int {name}(" in header, name
        assert name in hip.EXPORTED_SYMBOLS, name
        assert hasattr(lib, name), name
    assert "ophip_sample_job" in header and hip.SAMPLE_MAX_JOBS == 4 and "#define OPHIP_SAMPLE_MAX_JOBS 4" in header
    assert ctypes.sizeof(hip.SampleJob) == 4 * 8 + 8 * 4
    assert hip.ABI_VERSION == 4


def test_new_kernels_do_not_spill(device_asm):  # noqa: F811
    ks = {k: v for k, v in device_asm.items() if "sfm_" in k or "fine2_match_kernel" in k}
    assert len([k for k in ks if "sfm_coarse_ids_kernel" in k]) == 4, sorted(ks)          # float / double per image
    assert len([k for k in ks if "sfm_sample_kernel" in k]) == 1, sorted(ks)
    assert len([k for k in ks if "fine2_match_kernel" in k]) == 3, sorted(ks)             # plain float, scaled float / double
    for sym, ins in ks.items():
        spills = [t for t in ins if t.startswith("scratch_")]
        assert not spills, (sym, spills[:4])
