"""The product's own allocations under guard (run with ``-m gpu`` on the MI355X): for the duration of a call, ``torch.empty`` /
``torch.empty_like`` as ``onepose_st_amd.model``, ``.loftr``, ``.matchcall`` and ``.layercall`` look them up hand out regions of a ``tests.guarded.Arena``
-- every workspace, intermediate, output and frame block of the call at exactly the size the product asks for, 1 MiB of guard on each
side, filled 0xFF (NaN / -1) or 0x00 instead of whatever the caching allocator last held there.

Per run: the guards are intact, and every key that tests/test_gpu_parity.py::test_frame_call_equals_the_stage_by_stage_path compares is
bit-identical between the two fills and to an unpatched run.  The product reuses one block for every frame of a pipeline, so the
pipelined frames run twice: from the fill, and again with frame t in the very blocks frame t + 1 has just used (``guarded_empty``'s
``reuse``), where the stale bytes are another frame's results; both times every frame equals its single-frame run."""
import copy

import pytest
import torch

from onepose_st_amd import loftr as loftr_module
from onepose_st_amd import hip, layercall as layercall_module, matchcall as matchcall_module, model as model_module
from onepose_st_amd.model import OnePosePlus_model
from onepose_st_amd.synthetic import make_synthetic_inputs, make_synthetic_loftr_state_dict
from tests import test_gpu_loftr_masked as tglm
from tests.guarded import Arena, guarded_empty
from tests.test_gpu_workspace_contract import FILLS, FRAME_KEYS, same_bits

pytestmark = pytest.mark.gpu

MODULES = [model_module, loftr_module, matchcall_module, layercall_module]
ARENA_BYTES = 320 << 20


@pytest.fixture(scope="module")
def dev():
    assert torch.cuda.is_available(), "these tests need the MI355X"
    hip.load()
    return torch.device("cuda:0")


def _model(sd, cfg, dev, frame_call):
    c = copy.deepcopy(cfg)
    c["hip_frame_call"] = frame_call
    m = OnePosePlus_model(c).eval()
    m.load_state_dict(sd, strict=True)
    return m.to(dev)


@pytest.fixture(scope="module")
def frames(sd, cfg, dev):
    """the 128 x 160, 900-point frames of test_frame_call_equals_the_stage_by_stage_path"""
    fr = [make_synthetic_inputs(sd, n_points=900, image_hw=(128, 160), n_plant=350, seed=47, config=cfg, frame=f) for f in range(3)]
    obj = {k: fr[0][k].to(dev) for k in ("keypoints3d", "descriptors3d_db", "descriptors3d_coarse_db")}
    return obj, [(f["feat_c"].to(dev), f["feat_f"].to(dev)) for f in fr], fr[0]["image_hw"]


def under_guard(dev, fill, call):
    arena = Arena(dev, ARENA_BYTES)
    with guarded_empty(arena, fill, MODULES):
        out = call()
        torch.cuda.synchronize()
    print(f"fill {fill:#04x}: {len(arena.regions)} allocations of the call went through the arena")
    assert len(arena.regions) >= 1, "no allocation of the call went through the arena"
    arena.check()
    return out


def assert_same(got, want, keys, what):
    for k in keys:
        assert same_bits(got[k], want[k]), f"{what}: {k}"


@pytest.mark.parametrize("frame_call", [False, True], ids=["stage_by_stage", "frame_call"])
def test_forward_features(sd, cfg, dev, frames, frame_call):
    obj, feats, image_hw = frames
    m = _model(sd, cfg, dev, frame_call)
    assert m.frame_call == frame_call

    def forward():
        d = dict(obj)
        m.forward_features(d, *feats[0], image_hw)
        return {k: d[k].clone() for k in FRAME_KEYS}
    plain = forward()
    torch.cuda.synchronize()
    assert len(plain["i_ids"]) > 150
    for fill in FILLS:
        assert_same(under_guard(dev, fill, forward), plain, FRAME_KEYS, f"fill {fill:#04x} against the unpatched run")


def test_three_pipelined_frames(sd, cfg, dev, frames):
    obj, feats, image_hw = frames
    m = _model(sd, cfg, dev, True)
    keys = FRAME_KEYS
    single = []
    for fc, ff in feats:
        d = dict(obj)
        m.enqueue_features(d, fc, ff, image_hw, host_copy=True).finish()
        torch.cuda.synchronize()
        single.append({k: d[k].clone() for k in keys})
    assert not torch.equal(single[0]["j_ids"], single[1]["j_ids"]) and not torch.equal(single[1]["j_ids"], single[2]["j_ids"])

    def pipeline():
        datas = [dict(obj) for _ in feats]
        pend = [m.enqueue_features(d, fc, ff, image_hw, inputs_ready=True, host_copy=True) for d, (fc, ff) in zip(datas, feats)]
        for p in pend:
            p.finish()
        return [{k: d[k].clone() for k in keys} for d in datas]
    for fill in FILLS:
        arena, log = Arena(dev, ARENA_BYTES), []
        with guarded_empty(arena, fill, MODULES, log=log):
            first = pipeline()
            torch.cuda.synchronize()
        arena.check()
        for t, (got, want) in enumerate(zip(first, single)):
            assert_same(got, want, keys, f"fill {fill:#04x}, pipelined frame {t} against its single-frame run")
        # the product reuses one block for every frame: the same pipeline again, frame t in the blocks frame t + 1 has just used, so the
        # stale bytes it finds are another frame's results
        per_frame = len(log) // len(feats)
        print(f"fill {fill:#04x}: {len(arena.regions)} allocations of the three frames went through the arena")
        assert per_frame >= 1 and len(log) == per_frame * len(feats)
        assert all(a.shape == b.shape and a.dtype == b.dtype for a, b in zip(log, log[per_frame:]))
        with guarded_empty(arena, fill, MODULES, reuse=log[per_frame:] + log[:per_frame]):
            second = pipeline()
            torch.cuda.synchronize()
        arena.check()
        for t, (got, want) in enumerate(zip(second, single)):
            assert_same(got, want, keys, f"fill {fill:#04x}, frame {t} in another frame's used blocks against its single-frame run")


LOFTR_KEYS = ("b_ids", "i_ids", "j_ids", "mconf", "conf_matrix", "mkpts0_c", "mkpts1_c", "mkpts0_f", "mkpts1_f", "expec_f")


@pytest.fixture(scope="module")
def lsd():
    sd = dict(make_synthetic_loftr_state_dict(0))
    sd["coarse_matching.bin_score"] = torch.tensor(1.0)
    return sd


@pytest.mark.parametrize("masked", [False, True])
@pytest.mark.parametrize("match_type", ["dual_softmax", "sinkhorn"])
def test_loftr_matcher_forward(lsd, dev, match_type, masked):
    """one batch of two views against a shared query (tests/test_gpu_loftr_masked.py's planted views), with and without padding masks"""
    cfg = copy.deepcopy(loftr_module.default_cfg)
    cfg["match_coarse"]["match_type"] = match_type
    m = loftr_module.LoFTR_for_OnePose_Plus(cfg).eval()
    m.load_state_dict(lsd if match_type == "sinkhorn" else {k: v for k, v in lsd.items() if k != "coarse_matching.bin_score"}, strict=True)
    m.to(dev)
    (x0, g0, q, gq), hw0p, hw1, masks = tglm._shared_query(amp=1.0 if match_type == "dual_softmax" else 6.0)
    feats = (x0[:2].contiguous(), g0[:2].contiguous(), q, gq)
    masks = (masks[0][:2].contiguous(), masks[1]) if masked else None

    def forward():
        data = tglm._run(m, dev, feats, hw0p, hw1, masks, V=2, V1=1)
        return {k: data[k].clone() for k in LOFTR_KEYS}
    plain = forward()
    torch.cuda.synchronize()
    assert len(plain["i_ids"]) > 20 and set(plain["b_ids"].tolist()) == {0, 1}
    for fill in FILLS:
        assert_same(under_guard(dev, fill, forward), plain, LOFTR_KEYS, f"{match_type} masked={masked} fill {fill:#04x} against the unpatched run")
