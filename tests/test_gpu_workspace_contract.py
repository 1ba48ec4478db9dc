"""The workspace contract of include/onepose_hip.h on the MI355X (run with ``-m gpu``): every entry point that takes a caller-sized
workspace (or the frame block) writes nothing outside the buffers it is given and reads no workspace byte it has not written.

Every buffer of a call -- inputs, outputs, the workspace at EXACTLY the size its helper returns -- is a region of one ``tests.guarded.Arena``
with 1 MiB of guard on each side; outputs start as 0xFF bytes (NaN / -1).  Each row runs four times: workspace filled 0xFF and 0x00, at a
256-byte aligned base and at the minimum alignment the header states (16 bytes: base address 16 mod 256, which is what makes the
address-dependent round-ups inside the x3w8 encoder, coarse matching and Sinkhorn workspaces non-zero; 256 bytes: base 256 mod 512).
Per row:

  (a) the guards are intact after every run;
  (b) every output is bit-identical across the two fills and the two bases;
  (c) one run meets the bar of the test that already covers the entry -- its oracle call and its tolerance, imported, not restated --
      so that (b) does not compare garbage with garbage.

Carried state is run as the documented sequence on one workspace poisoned once: the fused K|V tail (kv_from_prev = 1), ``kv_first``
(kv_from_prev = 2), the fragment planes of ``_frag`` into ``COARSE_PLANES_READY``, ``_conf`` then ``_select``, ``points2d_group`` then
``_rank``, and the Sinkhorn potentials the header promises on return.  ``ENTRY_ROWS`` names the rows of every entry point;
tests/test_workspace_sizes_cpu.py checks it against the header's prototypes."""
import copy
import ctypes

import numpy as np
import pytest
import torch

from oracle import onepose_oracle as orc
from onepose_st_amd import hip, layercall, matchcall, model as model_module, packing, postopt
from onepose_st_amd.model import OnePosePlus_model
from onepose_st_amd.synthetic import make_synthetic_inputs, make_synthetic_sfm_tracks
from tests import bf16_faithful as bf
from tests import full_attention_oracle as foracle
from tests import sfm_points2d_oracle as so
from tests import test_gpu_encoder_bf16 as tbf
from tests import test_gpu_loftr_scale as tls
from tests import test_gpu_loftr_sinkhorn as tsk
from tests import test_gpu_masked as tmk
from tests import test_gpu_parity as par
from tests import test_gpu_postopt as tpo
from tests import test_gpu_sfm_points2d as tp2
from tests.guarded import Arena, guarded_empty
from tests.test_sfm_points2d_cpu import hand_case

pytestmark = pytest.mark.gpu

FILLS = (0xFF, 0x00)
P = hip.ptr
U8, I32, I64, F32, F64 = torch.uint8, torch.int32, torch.int64, torch.float32, torch.float64

# entry point -> the tests below that run it; tests/test_workspace_sizes_cpu.py holds this against the header
ENTRY_ROWS = {}


def rows(*entries):
    def mark(fn):
        for e in entries:
            ENTRY_ROWS.setdefault(e, []).append(fn.__name__)
        return fn
    return mark


@pytest.fixture(scope="module")
def dev():
    assert torch.cuda.is_available(), "these tests need the MI355X"
    hip.load()
    return torch.device("cuda:0")


def bases(min_align):
    """(align, shift) of the workspace region: 256-byte aligned, then the stated minimum and no more"""
    return {16: ((256, 0), (256, 16)), 256: ((512, 0), (512, 256))}[min_align]


def same_bits(a, b):
    return a.shape == b.shape and a.dtype == b.dtype and torch.equal(a.contiguous().view(-1).view(U8), b.contiguous().view(-1).view(U8))


def contract(dev, min_align, run, bar, arena_bytes=48 << 20):
    """``run(arena, ws)``: makes its regions (``ws(nbytes)`` -> the workspace region of this run), enqueues the entry (or its documented
    sequence) and returns {name: output tensor}.  (a), (b), then ``bar(outputs of the first run)`` for (c)."""
    outs = {}
    for align, shift in bases(min_align):
        for fill in FILLS:
            arena = Arena(dev, arena_bytes)
            made = []

            def ws(nbytes, name="workspace"):
                made.append(arena.region(nbytes, align, shift, fill, name))
                return made[-1]
            out = run(arena, ws)
            torch.cuda.synchronize()
            arena.check()                                                                           # (a)
            assert made and all(t.data_ptr() % align == shift for t in made)
            outs[shift, fill] = {k: v.clone() for k, v in out.items() if v is not None}
    first = outs[bases(min_align)[0][1], FILLS[0]]
    for key, out in outs.items():                                                                   # (b)
        assert out.keys() == first.keys()
        for k in first:
            assert same_bits(out[k], first[k]), f"output {k!r} differs at (base shift, fill) = {key} from the aligned 0xFF run"
    bar(first)                                                                                      # (c)


_WEIGHTS = {}


def weights(sd, dev, packer, prefix):
    key = (packer, prefix)
    if key not in _WEIGHTS:
        _WEIGHTS[key] = getattr(packing, packer)(sd, prefix).to(dev)
    return _WEIGHTS[key]


# ------------------------------------------------------------------------------------------------
# encoder layers
# ------------------------------------------------------------------------------------------------
ENC_SHAPES = [(2, 70, 45), (3, 49, 97), (1, 1, 32)]          # ragged tiles of 32 and 48 tokens, batch strides, a one-token stream
LAYER = bf.COARSE_LAYER
# variant -> (entry, arithmetic mode of par.LAYER_TOL, packer, workspace helper, stated alignment)
ENC = {
    "f32": ("ophip_encoder_layer", "f32", "pack_coarse_layer", "ophip_encoder_workspace_floats", 16),
    "f32_masked": ("ophip_encoder_layer_masked", "f32", "pack_coarse_layer", "ophip_encoder_workspace_floats", 16),
    "bf16": ("ophip_encoder_layer_bf16", "bf16", "pack_coarse_layer_bf16", "ophip_encoder_bf16_workspace_bytes", 256),
    "bf16_masked": ("ophip_encoder_layer_bf16_masked", "bf16", "pack_coarse_layer_bf16", "ophip_encoder_bf16_workspace_bytes", 256),
    "x3w8": ("ophip_encoder_layer_x3w8", "bf16x3", "pack_coarse_layer_x3w8", "ophip_encoder_x3w8_workspace_bytes", 16),
    "x3w8_masked": ("ophip_encoder_layer_x3w8_masked", "bf16x3", "pack_coarse_layer_x3w8", "ophip_encoder_x3w8_workspace_bytes", 16),
    "x3w8_masks": ("ophip_encoder_layer_x3w8_masks", "bf16x3", "pack_coarse_layer_x3w8", "ophip_encoder_x3w8_workspace_bytes", 16),
    "x3w8_masks_null0": ("ophip_encoder_layer_x3w8_masks", "bf16x3", "pack_coarse_layer_x3w8", "ophip_encoder_x3w8_workspace_bytes", 16),
    "x3w8_masks_null1": ("ophip_encoder_layer_x3w8_masks", "bf16x3", "pack_coarse_layer_x3w8", "ophip_encoder_x3w8_workspace_bytes", 16),
    "x3w8_streams1": ("ophip_encoder_layer_x3w8_streams", "bf16x3", "pack_coarse_layer_x3w8", "ophip_encoder_x3w8_workspace_bytes", 16),
    "x3w8_streams2": ("ophip_encoder_layer_x3w8_streams", "bf16x3", "pack_coarse_layer_x3w8", "ophip_encoder_x3w8_workspace_bytes", 16),
    "x3w8_streams3": ("ophip_encoder_layer_x3w8_streams", "bf16x3", "pack_coarse_layer_x3w8", "ophip_encoder_x3w8_workspace_bytes", 16),
    "x3w8_streams_masks1": ("ophip_encoder_layer_x3w8_streams_masks", "bf16x3", "pack_coarse_layer_x3w8", "ophip_encoder_x3w8_workspace_bytes", 16),
    "x3w8_streams_masks2": ("ophip_encoder_layer_x3w8_streams_masks", "bf16x3", "pack_coarse_layer_x3w8", "ophip_encoder_x3w8_workspace_bytes", 16),
    "x3w8_streams_masks3": ("ophip_encoder_layer_x3w8_streams_masks", "bf16x3", "pack_coarse_layer_x3w8", "ophip_encoder_x3w8_workspace_bytes", 16),
    "x3w8_kv_first": ("ophip_encoder_kv_first_x3w8", "bf16x3", "pack_coarse_layer_x3w8", "ophip_encoder_x3w8_workspace_bytes", 16),
    "full": ("ophip_encoder_layer_full_x3", "bf16x3", "pack_coarse_layer", "ophip_encoder_full_workspace_bytes", 16),
    "full_stream": ("ophip_encoder_layer_full_x3_stream", "bf16x3", "pack_coarse_layer", "ophip_encoder_full_stream_workspace_bytes", 16),
}
# variant -> what ``layercall.layer`` is given beside the rows, the weights, ``is_cross`` and the workspace region; M3 / M2 stand for the
# arena's copies of the 3D / 2D stream's mask.  (full_stream: ``layercall.layer_full_stream``, which has no options)
M3, M2 = "mask0", "mask1"
X3 = dict(mode="bf16x3")
ENC_KW = {
    "f32": dict(mode="f32"), "f32_masked": dict(mode="f32", query_mask=M2),
    "bf16": dict(mode="bf16"), "bf16_masked": dict(mode="bf16", query_mask=M2),
    "x3w8": X3, "x3w8_masked": dict(X3, query_mask=M2),
    "x3w8_masks": dict(X3, masks=(M3, M2)), "x3w8_masks_null0": dict(X3, masks=(None, M2)), "x3w8_masks_null1": dict(X3, masks=(M3, None)),
    **{f"x3w8_streams{s}": dict(X3, streams=s) for s in (1, 2, 3)},
    **{f"x3w8_streams_masks{s}": dict(X3, streams=s, masks=(M3, M2)) for s in (1, 2, 3)},
    "x3w8_kv_first": dict(X3, kv_from_prev=2),                    # after layercall.kv_first: "the summed block is there"
    "full": dict(mode="full"), "full_stream": {},
}
assert set(ENC_KW) == set(ENC)
_ENC_CASES = {}


def enc_case(B, L3, L2):
    """the streams of the tests that own the bars (seed 2) and one padding mask per stream"""
    key = (B, L3, L2)
    if key not in _ENC_CASES:
        x3, x2 = bf.coarse_inputs(B, L3, L2)
        _ENC_CASES[key] = (x3, x2, tmk._mask(B, L3, 13), tmk._mask(B, L2, 11))
    return _ENC_CASES[key]


def layer_oracle(sd, x3, x2, cross, m3=None, m2=None, full=False):
    """both streams of one layer: each stream's own mask is its x_mask, its source's mask the source_mask"""
    s3, s2, ms3, ms2 = (x2, x3, m2, m3) if cross else (x3, x2, m3, m2)
    if full:
        with torch.no_grad():
            return foracle.encoder_layer(sd, LAYER, x3, s3, 8), foracle.encoder_layer(sd, LAYER, x2, s2, 8)
    return orc.encoder_layer(sd, LAYER, x3, s3, 8, m3, ms3), orc.encoder_layer(sd, LAYER, x2, s2, 8, m2, ms2)


@rows(*sorted({v[0] for v in ENC.values()}), "ophip_encoder_layer_x3w8")
@pytest.mark.parametrize("cross", [0, 1])
@pytest.mark.parametrize("B,L3,L2", ENC_SHAPES)
@pytest.mark.parametrize("variant", list(ENC))
def test_encoder_layer(sd, dev, variant, B, L3, L2, cross):
    entry, mode, packer, helper, min_align = ENC[variant]
    x3, x2, m3, m2 = enc_case(B, L3, L2)
    w = weights(sd, dev, packer, LAYER)
    lib = hip.load()
    kw = ENC_KW[variant]
    masked2 = "query_mask" in kw
    use3, use2 = M3 in kw.get("masks", ()), masked2 or M2 in kw.get("masks", ())
    streams = kw.get("streams", 3)
    S3 = L2 if cross else L3                                    # full_stream: the 3D rows against their source
    nbytes = getattr(lib, helper)(B, L3, S3 if variant == "full_stream" else L2) * (4 if helper.endswith("floats") else 1)
    seen = {}

    def run(arena, ws):
        d3, d2 = arena.put(x3, name="x3d"), arena.put(x2, name="x2d")
        y3, y2 = arena.typed(x3.shape, F32, name="y3d"), arena.typed(x2.shape, F32, name="y2d")
        dm3 = arena.put(m3.view(U8), name="mask0") if use3 else None
        dm2 = arena.put(m2.view(U8), name="mask1") if use2 else None
        wsp = ws(nbytes)
        region = wsp.view(F32) if helper.endswith("floats") else wsp                 # the f32 entries take float*
        if variant == "full_stream":                              # the 3D rows as the query stream
            layercall.layer_full_stream(d3, d2 if cross else d3, y3, wpack=w, workspace=region)
        else:
            put = {M3: dm3, M2: dm2}
            call = {k: tuple(put.get(m) for m in v) if k == "masks" else put.get(v, v) for k, v in kw.items()}
            if variant == "x3w8_kv_first":                        # the K / V half first
                layercall.kv_first(d3, d2, wpack=w, slot=0, workspace=region)
            plan = layercall.plan_layer(d3, d2, y3 if streams & 1 else None, y2 if streams & 2 else None, wpack=w, is_cross=cross,
                                        workspace=region, **call)
            assert plan[0] == ("ophip_encoder_layer_x3w8" if variant == "x3w8_kv_first" else entry)      # the row's entry is the one that runs
            hip.launch(*plan)
        if mode == "bf16" and "block" not in seen:                # (c) of the plain-bf16 layer reads the K^T V | Ksum block of the first run
            torch.cuda.synchronize()
            off = bf.kv_block_offset(wsp.data_ptr(), B, L3, L2)
            seen["block"] = bf.decode_kv_block(wsp[off:off + B * 2 * bf.KV_BLOCK_BYTES].cpu().view(B, 2, bf.KV_BLOCK_BYTES))
        return {"y3d": y3, "y2d": y2}

    def bar(out):
        runs3, runs2 = (streams & 1) != 0, (streams & 2) != 0 and variant != "full_stream"
        if mode == "bf16":
            tbf.check(sd, LAYER, x3, x2, cross, m2 if masked2 else None, out["y3d"], out["y2d"], seen["block"], f"{variant} {B, L3, L2} cross={cross}")
            return
        r3, r2 = layer_oracle(sd, x3, x2, cross, m3 if use3 else None, m2 if use2 else None, full=variant.startswith("full"))
        for name, on, got, want in (("3D", runs3, out["y3d"], r3), ("2D", runs2, out["y2d"], r2)):
            if on:
                par.close(got, want, msg=f"{name} stream", **par.LAYER_TOL[mode])
            else:
                assert bool(torch.isnan(got).all()), f"{name} stream does not run in this call and must stay untouched"

    contract(dev, min_align, run, bar, arena_bytes=24 << 20)


CHAIN = ["self", "cross", "self"]


@rows("ophip_encoder_layer_x3w8", "ophip_encoder_layer_bf16")
@pytest.mark.parametrize("B,L3,L2", ENC_SHAPES)
@pytest.mark.parametrize("kind", ["x3w8", "bf16"])
def test_fused_chain(sd, dev, kind, B, L3, L2):
    """three layers, each handing the next its K|V slabs (wpack_next, kv_from_prev = 1, alternating slot): ONE workspace, poisoned once
    before the first call -- the slab set a layer reads was written by the layer before it, never by an earlier run"""
    entry, mode, packer, helper, min_align = ENC[kind]
    x3, x2 = bf.coarse_inputs(B, L3, L2, seed=5)
    ps = [f"loftr_coarse.layers.{li}." for li in range(3)]
    ws_ = [weights(sd, dev, packer, p) for p in ps]
    nbytes = getattr(hip.load(), helper)(B, L3, L2)
    seen = {}

    def run(arena, ws):
        a3, a2 = arena.put(x3, name="x3d"), arena.put(x2, name="x2d")
        b3, b2 = arena.typed(x3.shape, F32, name="y3d"), arena.typed(x2.shape, F32, name="y2d")
        wsp = ws(nbytes)
        layers = []
        for li, nm in enumerate(CHAIN):
            nxt = ws_[li + 1] if li + 1 < 3 else None
            layercall.layer(a3, a2, b3, b2, wpack=ws_[li], wpack_next=nxt, is_cross=1 if nm == "cross" else 0, kv_from_prev=1 if li > 0 else 0,
                            slot=li & 1, workspace=wsp, **ENC_KW[kind])
            if kind == "bf16" and "layers" not in seen:
                torch.cuda.synchronize()
                off = bf.kv_block_offset(wsp.data_ptr(), B, L3, L2)
                block = bf.decode_kv_block(wsp[off:off + B * 2 * bf.KV_BLOCK_BYTES].cpu().view(B, 2, bf.KV_BLOCK_BYTES))
                layers.append((a3.cpu(), a2.cpu(), b3.clone(), b2.clone(), block))
            a3, b3, a2, b2 = b3, a3, b2, a2
        seen.setdefault("layers", layers)
        return {"y3d": a3, "y2d": a2}

    def bar(out):
        if kind == "bf16":
            for li, (i3, i2, y3, y2, block) in enumerate(seen["layers"]):
                tbf.check(sd, ps[li], i3, i2, CHAIN[li] == "cross", None, y3, y2, block, f"chain {B, L3, L2} layer {li} ({CHAIN[li]})")
            return
        r3, r2 = x3, x2
        for p, nm in zip(ps, CHAIN):
            if nm == "cross":
                r2, r3 = orc.encoder_layer(sd, p, r2, r3, 8), orc.encoder_layer(sd, p, r3, r2, 8)
            else:
                r2, r3 = orc.encoder_layer(sd, p, r2, r2, 8), orc.encoder_layer(sd, p, r3, r3, 8)
        par.close(out["y3d"], r3, msg="3D stream after 3 layers", **par.CHAIN_TOL)
        par.close(out["y2d"], r2, msg="2D stream after 3 layers", **par.CHAIN_TOL)

    contract(dev, min_align, run, bar, arena_bytes=24 << 20)


@rows("ophip_encoder_object_x3w8")
@pytest.mark.parametrize("masked_frames", [0, 1])
@pytest.mark.parametrize("Bo,N", [(2, 70), (3, 49), (1, 1)])
def test_encoder_object(sd, dev, Bo, N, masked_frames):
    """the object cache's build: workspace sized (Bo, N, 1); y3d0 and kv1 are guarded outputs"""
    lib = hip.load()
    x3, _ = bf.coarse_inputs(Bo, N, 32)
    w0, w1 = (weights(sd, dev, "pack_coarse_layer_x3w8", f"loftr_coarse.layers.{li}.") for li in (0, 1))
    nbytes, kvb = lib.ophip_encoder_x3w8_workspace_bytes(Bo, N, 1), lib.ophip_encoder_x3w8_kv_block_bytes()

    def run(arena, ws):
        d3 = arena.put(x3, name="x3d")
        y3d0, kv1 = arena.typed(x3.shape, F32, name="y3d0"), arena.typed((Bo, kvb), U8, align=256, shift=16, name="kv1")
        layercall.object_rows(d3, wpack0=w0, wpack1=w1, workspace=ws(nbytes), y3d0=y3d0, kv1=kv1, masked_frames=masked_frames)
        return {"y3d0": y3d0, "kv1": kv1}

    def bar(out):
        par.close(out["y3d0"], orc.encoder_layer(sd, "loftr_coarse.layers.0.", x3, x3, 8), msg="first layer's 3D rows", **par.LAYER_TOL["bf16x3"])
        assert bool((out["kv1"] != 0xFF).any(dim=1).all())
        if not masked_frames:           # tests/test_gpu_parity.py::test_object_cache_is_bit_identical: the rows ARE the plain layer's 3D rows
            d3, d2 = x3.to(dev), torch.randn(Bo, 32, 256, device=dev)
            y3, y2 = torch.empty_like(d3), torch.empty_like(d2)
            layercall.layer(d3, d2, y3, y2, wpack=w0, wpack_next=w1, is_cross=0, workspace=layercall.workspace("bf16x3", Bo, N, 32, dev), **X3)
            torch.cuda.synchronize()
            assert torch.equal(y3, out["y3d0"])

    contract(dev, 16, run, bar, arena_bytes=24 << 20)


# ------------------------------------------------------------------------------------------------
# coarse matching
# ------------------------------------------------------------------------------------------------
COARSE_SHAPES = [(2, 129, 9, 9), (1, 300, 10, 13), (1, 1408, 24, 32)]      # the last: no ragged tile, the counter-case
_COARSE_CASES = {}


def coarse_case(B, N, hc, wc):
    """the planted features of tests/test_gpu_parity.py's coarse tests and their oracles, computed once"""
    key = (B, N, hc, wc)
    if key not in _COARSE_CASES:
        f3, f2 = par._planted_features(B, N, hc, wc, 3, min(N, hc * wc) // 2)
        kp = torch.randn(B, N, 3, generator=torch.Generator().manual_seed(4))
        _COARSE_CASES[key] = {"f3": f3, "f2": f2, "kp": kp, "refs": {}}
    return _COARSE_CASES[key]


def coarse_ref(case, hc, wc, nsplit):
    like = nsplit == 1                                           # plain bf16 against the reference that rounds where the kernel rounds
    if like not in case["refs"]:
        conf = par.plain_bf16_confidence(case["f3"], case["f2"]) if like else orc.dual_softmax_confidence(case["f3"], case["f2"], 0.08)
        case["refs"][like] = (conf, orc.coarse_match_select(conf, (hc, wc), (hc * 8, wc * 8), case["kp"], 0.1, 2))
    return case["refs"][like]


def coarse_buffers(arena, B, N, M, lazy):
    cap = B * N
    return {"conf": None if lazy else arena.typed((B, N, M), F32, name="conf"),
            "b_ids": arena.typed((cap,), I64, name="b_ids"), "i_ids": arena.typed((cap,), I64, name="i_ids"),
            "j_ids": arena.typed((cap,), I64, name="j_ids"), "mconf": arena.typed((cap,), F32, name="mconf"),
            "mk3": arena.typed((cap, 3), F32, name="mkpts3d"), "mkc": arena.typed((cap, 2), F32, name="mkpts_c"),
            "m_bids": arena.typed((cap,), I64, name="m_bids"), "gt_mask": arena.typed((cap,), U8, name="gt_mask"),
            "count": arena.typed((4,), I32, name="count")}


def coarse_outputs(o, wsp):
    """the buffers of ``coarse_buffers`` and the workspace region as every coarse-matching call of ``matchcall`` takes them"""
    lists = matchcall.MatchLists(*(o[k] for k in ("b_ids", "i_ids", "j_ids", "mconf", "mk3", "mkc", "m_bids", "gt_mask", "count")))
    return dict(lists=lists, conf=o["conf"], workspace=wsp.view(F32))


def coarse_lists(out):
    """(conf, [b, i, j], mconf, mk3, mkc) as tests/test_gpu_parity.py::_coarse_match returns them, with its own checks of what lies past K"""
    K = int(out["count"][0])
    assert 0 <= K <= out["b_ids"].numel()
    assert torch.equal(out["m_bids"][:K], out["b_ids"][:K]) and bool((out["m_bids"][K:] == -1).all()) and bool((out["b_ids"][K:] == -1).all())
    assert torch.equal(out["gt_mask"][:K].bool(), out["mconf"][:K] == 0) and bool((out["gt_mask"][K:] == 0xFF).all())
    if "conf" in out:
        assert bool(torch.isfinite(out["conf"]).all()), "conf_matrix has elements no kernel wrote"
    return out.get("conf"), [out[k][:K] for k in ("b_ids", "i_ids", "j_ids")], out["mconf"][:K], out["mk3"][:K], out["mkc"][:K]


def coarse_bar(case, hc, wc, nsplit):
    ref_conf, ref = coarse_ref(case, hc, wc, nsplit)
    if nsplit == 1:
        tol = par.PLAIN_BF16_LIKE_FOR_LIKE_TOL
        return lambda out: par.coarse_equals_oracle(*coarse_lists(out), ref_conf, ref, tol["rtol"], mconf_atol=tol["atol"])
    return lambda out: par.coarse_equals_oracle(*coarse_lists(out), ref_conf, ref, par.COARSE_RTOL[nsplit])


def coarse_kw(wc):
    return dict(wc=wc, temperature=0.08, thr=0.1, border_rm=2, scale=8.0)


COARSE_FORMS = [("f32", 0, None, None), ("x3", 3, None, None), ("bf16", 1, None, None), ("x3_lazy", 3, None, None), ("bf16_lazy", 1, None, None)] + \
               [(f"{'x3' if ns == 3 else 'bf16'}_tile{tile}_twopass{two}", ns, tile, two) for ns in (3, 1) for tile in ("2", "3") for two in ("0", "1")]


@rows("ophip_coarse_match")
@pytest.mark.parametrize("form,nsplit,tile,two", COARSE_FORMS, ids=[f[0] for f in COARSE_FORMS])
@pytest.mark.parametrize("B,N,hc,wc", COARSE_SHAPES)
def test_coarse_match(dev, monkeypatch, B, N, hc, wc, form, nsplit, tile, two):
    """nsplit 0 / 1 / 3, the lazy form (conf == NULL), and in the bf16 modes both tile kernels in both eager forms, set as
    tests/test_gpu_parity.py::test_coarse_match_tile_kernels_and_two_pass_form_agree sets them"""
    if tile is not None:
        monkeypatch.setenv("OPHIP_SIM_TILE", tile)
        monkeypatch.setenv("OPHIP_COARSE_TWO_PASS", two)
    M, case, lazy = hc * wc, coarse_case(B, N, hc, wc), form.endswith("lazy")
    nfloats = hip.load().ophip_coarse_workspace_floats(B, N, M)

    def run(arena, ws):
        f3, f2, kp = (arena.put(case[k], name=k) for k in ("f3", "f2", "kp"))
        o = coarse_buffers(arena, B, N, M, lazy)
        matchcall.coarse_match(f3, f2, kp, kpts_bstride=N * 3, nsplit=nsplit, **coarse_kw(wc), **coarse_outputs(o, ws(4 * nfloats)))
        return o

    def bar(out):
        if lazy:
            assert int(out["count"][1]) == 0                     # no unresolvable tie in these inputs
        coarse_bar(case, hc, wc, nsplit)(out)

    contract(dev, 16, run, bar)


@rows("ophip_coarse_match_conf", "ophip_coarse_match_select")
@pytest.mark.parametrize("nsplit", [0, 3])
@pytest.mark.parametrize("B,N,hc,wc", COARSE_SHAPES)
def test_coarse_match_in_two_halves(dev, B, N, hc, wc, nsplit):
    """_conf then _select with identical arguments: the second call reads what the first left in the workspace"""
    M, case = hc * wc, coarse_case(B, N, hc, wc)
    nfloats = hip.load().ophip_coarse_workspace_floats(B, N, M)

    def run(arena, ws):
        f3, f2, kp = (arena.put(case[k], name=k) for k in ("f3", "f2", "kp"))
        o = coarse_buffers(arena, B, N, M, False)
        outputs = coarse_outputs(o, ws(4 * nfloats))
        for parts in (1, 2):                                          # _conf, then _select
            matchcall.coarse_match(f3, f2, kp, kpts_bstride=N * 3, nsplit=nsplit, parts=parts, **coarse_kw(wc), **outputs)
        return o

    contract(dev, 16, run, coarse_bar(case, hc, wc, nsplit))


@rows("ophip_coarse_match_masked")
@pytest.mark.parametrize("form,nsplit", [("f32", 0), ("x3", 3), ("x3_lazy", 3)])
@pytest.mark.parametrize("B,N,hc,wc", COARSE_SHAPES)
def test_coarse_match_masked(dev, B, N, hc, wc, form, nsplit):
    """a query mask and per-image scales, as tests/test_gpu_masked.py::test_coarse_match_masked_scaled_vs_oracle"""
    M, case, lazy = hc * wc, coarse_case(B, N, hc, wc), form.endswith("lazy")
    mask = torch.ones(B, hc, wc, dtype=torch.bool)
    mask[0, :, wc - 3:] = False
    mask[B - 1, hc - 2:, :] = False
    qs = torch.tensor([[1.25, 1.5], [0.8, 1.0], [2.0, 3.0]])[:B].contiguous()
    nfloats = hip.load().ophip_coarse_workspace_floats(B, N, M)

    def run(arena, ws):
        f3, f2, kp = (arena.put(case[k], name=k) for k in ("f3", "f2", "kp"))
        dm, dq = arena.put(mask.flatten(1).view(U8), name="query_mask"), arena.put(qs, name="query_scale")
        o = coarse_buffers(arena, B, N, M, lazy)
        matchcall.coarse_match(f3, f2, kp, kpts_bstride=N * 3, nsplit=nsplit, query_mask=dm, query_scale=dq, **coarse_kw(wc),
                               **coarse_outputs(o, ws(4 * nfloats)))
        return o

    def bar(out):
        conf_ref = orc.dual_softmax_confidence(case["f3"], case["f2"], 0.08, mask_query=mask.flatten(1))
        want = orc.coarse_match_select(conf_ref, (hc, wc), (hc * 8, wc * 8), case["kp"], 0.1, 2, query_image_scale=qs)
        if lazy:
            assert int(out["count"][1]) == 0
        else:
            assert float(out["conf"].cpu().transpose(1, 2)[~mask.flatten(1)].abs().max()) == 0.0      # padded cells: exactly 0
        par.coarse_equals_oracle(*coarse_lists(out), conf_ref, want, par.COARSE_RTOL[nsplit])

    contract(dev, 16, run, bar)


@rows("ophip_encoder_layer_x3w8_frag", "ophip_coarse_frag_planes", "ophip_coarse_match")
@pytest.mark.parametrize("B,N,hc,wc", COARSE_SHAPES)
def test_fragment_planes_carried_into_coarse_matching(sd, dev, B, N, hc, wc):
    """the last encoder layer writes the similarity operands into the COARSE workspace (ophip_coarse_frag_planes says where), coarse
    matching is told they are there: two guarded workspaces, the second poisoned once before the layer writes into it.  The bar is the one of
    tests/test_gpu_parity.py::test_encoder_layer_writes_the_similarity_fragments: bit for bit what coarse matching gives from the same rows."""
    M, lib = hc * wc, hip.load()
    g = torch.Generator().manual_seed(9)
    x3, x2, kp = torch.randn(B, N, 256, generator=g), torch.randn(B, M, 256, generator=g), torch.randn(B, N, 3, generator=g)
    w = weights(sd, dev, "pack_coarse_layer_x3w8", "loftr_coarse.layers.5.")
    enc_bytes, nfloats = lib.ophip_encoder_x3w8_workspace_bytes(B, N, M), lib.ophip_coarse_workspace_floats(B, N, M)

    def run(arena, ws):
        d3, d2, dk = arena.put(x3, name="x3d"), arena.put(x2, name="x2d"), arena.put(kp, name="kp")
        y3, y2 = arena.typed(x3.shape, F32, name="y3d"), arena.typed(x2.shape, F32, name="y2d")
        o = coarse_buffers(arena, B, N, M, False)
        ews, cws = ws(enc_bytes, "encoder workspace"), ws(4 * nfloats, "coarse workspace")
        pa, pb = ctypes.c_void_p(), ctypes.c_void_p()
        hip.call("ophip_coarse_frag_planes", P(cws, None), B, N, M, ctypes.byref(pa), ctypes.byref(pb))
        lo, hi = cws.data_ptr(), cws.data_ptr() + cws.numel()
        assert lo <= pa.value < pb.value < hi and pa.value % 64 == 0
        layercall.layer(d3, d2, y3, y2, wpack=w, is_cross=1, workspace=ews, frag=(pa, pb), **X3)
        matchcall.coarse_match(y3, y2, dk, kpts_bstride=N * 3, nsplit=3, planes_ready=True, **coarse_kw(wc), **coarse_outputs(o, cws))
        return {**o, "y3d": y3, "y2d": y2}

    def bar(out):
        d3, d2, dk = x3.to(dev), x2.to(dev), kp.to(dev)
        y3, y2 = torch.empty_like(d3), torch.empty_like(d2)
        layercall.layer(d3, d2, y3, y2, wpack=w, is_cross=1, workspace=torch.empty(enc_bytes, dtype=U8, device=dev), **X3)
        conf, ids, mconf, mk3, mkc = par._coarse_match(dev, y3, y2, dk, wc, nsplit=3)
        got = coarse_lists(out)
        assert torch.equal(out["y3d"], y3) and torch.equal(out["y2d"], y2)
        assert torch.equal(got[0], conf) and all(torch.equal(a, b) for a, b in zip(got[1], ids)) and torch.equal(got[2], mconf)
        assert torch.equal(got[3], mk3) and torch.equal(got[4], mkc)

    contract(dev, 16, run, bar)


# the two-image matcher's grids: N = h0c x w0c with an interior left after the all-sides border (129 = 3 x 43 has none: 130)
GRIDS_2D = [(2, (10, 13), (9, 9)), (1, (15, 20), (10, 13)), (1, (32, 44), (24, 32))]
SPECS_2D = {(10, 13): [("rect", 9, 12), ("rect", 10, 11)], (9, 9): [("rect", 9, 8), ("rect", 8, 9)], (15, 20): [("rect", 14, 18)],
            (32, 44): [("rect", 30, 41)], (24, 32): [("rect", 24, 29)]}
SPECS_2D[(10, 13, 1)] = [("rect", 10, 12)]


def specs_2d(hw, B, second):
    return (SPECS_2D[(*hw, 1)] if second and (*hw, 1) in SPECS_2D else SPECS_2D[hw])[:B]


def pts0(L0, w0):
    ii = torch.arange(L0)
    return torch.stack([(ii % w0).float() * 8, (ii // w0).float() * 8, torch.zeros(L0)], 1)[None].contiguous()


def planted_2d(B, hw0, hw1, s0, s1, seed, amp=1.2):
    """random rows; per pair, half of the cells that are valid and inside the border on the smaller side carry a match (the planting of
    tests/test_gpu_loftr_scale.py puts its matches on tile and span edges that grids this small do not have)"""
    L0, L1 = hw0[0] * hw0[1], hw1[0] * hw1[1]
    g = torch.Generator().manual_seed(seed)
    f0, f1 = torch.randn(B, L0, 256, generator=g) * amp, torch.randn(B, L1, 256, generator=g) * amp
    m0, m1 = (None, None) if s0 is None else (tls._masks(hw0, s0), tls._masks(hw1, s1))
    for b in range(B):
        inside = [[c for c in range(hw[0] * hw[1]) if tls._inside(hw, None if s is None else s[b], None if m is None else m[b], c)]
                  for hw, s, m in ((hw0, s0, m0), (hw1, s1, m1))]
        n = min(len(inside[0]), len(inside[1])) // 2
        ii, jj = (torch.tensor(c)[torch.randperm(len(c), generator=g)[:n]] for c in inside)
        f1[b, jj] = f0[b, ii] + 0.1 * amp * torch.randn(n, 256, generator=g)
    return f0, f1, m0, m1


def lists_2d(out):
    ids = [out[k] for k in ("b_ids", "i_ids", "j_ids", "m_bids")]
    return tls._collect(out.get("conf"), ids, out["mconf"], out["mk3"], out["mkc"], out["count"])


@rows("ophip_coarse_match_2d", "ophip_coarse_match_2d_masked")
@pytest.mark.parametrize("form", ["eager", "lazy"])
@pytest.mark.parametrize("masked", [False, True])
@pytest.mark.parametrize("B,hw0,hw1", GRIDS_2D)
def test_coarse_match_2d(dev, B, hw0, hw1, masked, form):
    """LoFTR's dual softmax between two grids, with and without the padding masks, against the float64 oracle and the bars of
    tests/test_gpu_loftr_scale.py"""
    L0, L1, lazy = hw0[0] * hw0[1], hw1[0] * hw1[1], form == "lazy"
    s0, s1 = (specs_2d(hw0, B, False), specs_2d(hw1, B, True)) if masked else (None, None)
    f0, f1, m0, m1 = planted_2d(B, hw0, hw1, s0, s1, seed=L0 + B)
    nfloats = hip.load().ophip_coarse_workspace_floats(B, L0, L1)

    def run(arena, ws):
        d0, d1, dp = arena.put(f0, name="feat0"), arena.put(f1, name="feat1"), arena.put(pts0(L0, hw0[1]), name="points0")
        dm = [arena.put(m.flatten(1).view(U8), name=f"mask{k}") for k, m in enumerate((m0, m1))] if masked else []
        o = coarse_buffers(arena, B, L0, L1, lazy)
        matchcall.coarse_match_2d(d0, d1, dp, w0c=hw0[1], w1c=hw1[1], temperature=tls.TEMP, thr=tls.THR, border_rm=tls.BD, scale=8.0,
                                  masks=dm or None, **coarse_outputs(o, ws(4 * nfloats)))
        return o

    def bar(out):
        ref = tls._dual_ref(dev, f0, f1, hw0, hw1, m0, m1)
        got = lists_2d(out)
        assert got["lazy_tie"] in ((0,) if lazy else (0, -1))                      # count[1] belongs to the lazy form alone
        K, _ = tls._against_ref(got, ref, f"{hw0} x {hw1} masked={masked} {form}", lambda b, i, j: tls._near_dual(ref["conf_matrix"], b, i, j),
                                conf=not lazy)
        assert K >= 3 * B, "the planted matches must survive: the comparison would be vacuous"
        if masked and not lazy:
            tls._padding_zero(got["conf"], m0, m1, f"{hw0} x {hw1}")

    contract(dev, 16, run, bar)


SKH_GRIDS = tsk.GRIDS[:3]


@rows("ophip_coarse_match_2d_sinkhorn", "ophip_coarse_match_2d_sinkhorn_masked")
@pytest.mark.parametrize("masked", [False, True])
@pytest.mark.parametrize("iters", [0, 3])
@pytest.mark.parametrize("grids", SKH_GRIDS)
def test_coarse_match_2d_sinkhorn(dev, grids, iters, masked):
    """optimal transport at the small grids of tests/test_gpu_loftr_sinkhorn.py; the dual potentials u, v the header promises in the
    workspace on return are outputs of the row like the match lists"""
    (h0, w0), (h1, w1) = grids
    B, L0, L1, prefilter, bin_score = 3, h0 * w0, h1 * w1, 1, 1.0
    lib = hip.load()
    if masked:
        ext = lambda h, w: [("rect", h, w), ("rect", h - 1, w - 2), ("rect", h - 2, w)]
        f0, f1, m0, m1, _ = tls._planted(B, (h0, w0), (h1, w1), ext(h0, w0), ext(h1, w1), n=min(L0, L1) // 2, seed=L0 + iters, amp=4.0, ties=False)
    else:
        f0, f1 = tsk._features(B, L0, L1, seed=h0 * w1 + B + iters)
        m0 = m1 = None
    nfloats, dual_at = lib.ophip_coarse_sinkhorn_workspace_floats(B, L0, L1), lib.ophip_coarse_workspace_floats(B, L0, L1)
    up, vp = (L0 + 4) // 4 * 4, (L1 + 4) // 4 * 4

    def run(arena, ws):
        d0, d1, dp = arena.put(f0, name="feat0"), arena.put(f1, name="feat1"), arena.put(pts0(L0, w0), name="points0")
        dm = [arena.put(m.flatten(1).view(U8), name=f"mask{k}") for k, m in enumerate((m0, m1))] if masked else []
        o = coarse_buffers(arena, B, L0, L1, False)
        wsp = ws(4 * nfloats)
        matchcall.coarse_match_2d(d0, d1, dp, w0c=w0, w1c=w1, sinkhorn=(bin_score, iters, prefilter), thr=tls.THR, border_rm=tls.BD, scale=8.0,
                                  masks=dm or None, **coarse_outputs(o, wsp))
        at = dual_at + (16 - (wsp.data_ptr() // 4 + dual_at) % 16) % 16               # "rounded up to a 64-byte boundary"
        assert 4 * (at + B * (up + vp)) <= wsp.numel()
        duals = wsp.view(F32)[at:at + B * (up + vp)]
        return {**o, "u": duals[:B * up].view(B, up)[:, :L0 + 1], "v": duals[B * up:].view(B, vp)[:, :L1 + 1]}

    def bar(out):
        assert bool(torch.isfinite(out["u"]).all()) and bool(torch.isfinite(out["v"]).all())
        got = lists_2d(out)
        tag = f"{grids} iters={iters} masked={masked}"
        if masked:
            K = tls._check_sinkhorn(got, f0.to(dev).double(), f1.to(dev).double(), (h0, w0), (h1, w1), iters, prefilter, m0.to(dev), m1.to(dev), tag)
        else:
            res = {**got, "conf": got["conf"], "mkpts0": out["mk3"][:got["K"]].cpu()}
            K, _ = tsk._check_stage(res, f0, f1, (h0, w0), (h1, w1), bin_score, iters, prefilter, tag, thr=tls.THR)
        assert K >= 3 * B, "the planted pairs must match: the comparison would be vacuous"

    contract(dev, 16, run, bar)


# ------------------------------------------------------------------------------------------------
# post-optimisation and the coarse-match merge: workspace_bytes is an argument
# ------------------------------------------------------------------------------------------------
@rows("ophip_postopt_refine")
def test_postopt_refine(dev):
    """the smallest seeded case of tests/test_gpu_postopt.py (one step, with residuals); a workspace one byte short, or off its 256-byte
    alignment, is refused before anything is launched: every output still holds its fill"""
    data = make_synthetic_sfm_tracks(0)
    d0, offs, K0, K1, mk0, mk1, li, ri, aa, np_, L, F = postopt._flat_problem(*(data[k].to(dev) for k in tpo.ROW_KEYS))
    table = torch.tensor(postopt.adam_step_table(3e-2, 1), dtype=F64, device=dev)
    nbytes = hip.load().ophip_postopt_workspace_bytes(L, np_, 1)
    assert nbytes > 0

    def enqueue(arena, wsp, declared):
        d = arena.put(d0, name="depth")
        loss, steps, resid = arena.typed((1,), F64, name="loss"), arena.typed((1,), I32, name="steps_run"), arena.typed((L, 2), F64, name="residuals")
        args = (P(d, F64), P(offs, I64), np_, L, P(K0, F64), P(K1, F64), P(mk0, F64), P(mk1, F64), P(li, I64), P(ri, I64), P(aa, F64), F,
                P(table, F64), 1, postopt.ADAM_BETAS[0], postopt.ADAM_BETAS[1], postopt.ADAM_EPS, P(loss, F64), P(steps, I32), P(resid, F64),
                P(wsp, None), ctypes.c_size_t(declared), hip.stream_handle())
        return args, {"depth": d, "loss": loss, "steps": steps, "residuals": resid}

    def run(arena, ws):
        args, out = enqueue(arena, ws(nbytes), nbytes)
        hip.call("ophip_postopt_refine", *args)
        return out

    def bar(out):
        tpo.check_first_evaluation({"residuals": out["residuals"], "steps": int(out["steps"]), "initial_residual": float(out["loss"][0])}, data)

    contract(dev, 256, run, bar)
    for align, shift, declared in [(*b, nbytes - 1) for b in bases(256)] + [(256, 128, nbytes), (256, 16, nbytes)]:      # too small; misaligned
        arena = Arena(dev, 48 << 20)
        args, out = enqueue(arena, arena.region(declared, align, shift, 0xFF, "workspace"), declared)
        with pytest.raises(ValueError):
            hip.call("ophip_postopt_refine", *args)
        torch.cuda.synchronize()
        arena.check()
        assert torch.equal(out["depth"], d0) and bool(torch.isnan(out["loss"]).all()) and bool(torch.isnan(out["residuals"]).all())
        assert int(out["steps"]) == -1


@rows("ophip_sfm_points2d_group", "ophip_sfm_points2d_rank")
def test_sfm_points2d(dev):
    """_group then _rank on one workspace, untouched in between: the hand-worked case of tests/test_gpu_sfm_points2d.py, bit-exact; both
    refuse a workspace one byte short or off its 256-byte alignment before anything is launched"""
    mk0, mk1, conf, off, pim, n_images = hand_case()
    T, n_pairs = len(conf), len(pim)
    t = lambda a: torch.from_numpy(np.ascontiguousarray(a))
    lib = hip.load()
    nbytes = lib.ophip_sfm_points2d_workspace_bytes(T, n_images)
    want = so.oracle_merge(*hand_case())
    U = len(want["scores"])

    def enqueue(arena, wsp, declared):
        d0, d1, dc, do, dp = (arena.put(t(a), name=n) for a, n in ((mk0, "mkpts0"), (mk1, "mkpts1"), (conf, "mconf"), (off, "pair_offsets"),
                                                                   (pim, "pair_images")))
        ucount = arena.typed((1,), I32, name="unique_count")
        out = {"keypoints": arena.typed((U, 2), F32, name="keypoints"), "scores": arena.typed((U,), F32, name="scores"),
               "kpt_offsets": arena.typed((n_images + 1,), I64, name="kpt_offsets"), "match_ids": arena.typed((T, 2), I64, name="match_ids")}
        S = hip.stream_handle()
        group = (P(d0), P(d1), P(do, I64), P(dp, I64), n_pairs, T, n_images, P(wsp, None), declared, P(ucount, I32), S)
        rank = (P(dc), T, n_images, U, P(wsp, None), declared, P(out["keypoints"]), P(out["scores"]), P(out["kpt_offsets"], I64),
                P(out["match_ids"], I64), S)
        return group, rank, ucount, out

    def run(arena, ws):
        group, rank, ucount, out = enqueue(arena, ws(nbytes), nbytes)
        hip.call("ophip_sfm_points2d_group", *group)
        hip.call("ophip_sfm_points2d_rank", *rank)
        return {**out, "unique_count": ucount}

    def bar(out):
        assert int(out["unique_count"]) == U
        tp2.assert_bit_exact({k: out[k].cpu().numpy() for k in want if k in out}, want, "hand case")

    contract(dev, 256, run, bar)
    for align, shift, declared in [(*b, nbytes - 1) for b in bases(256)] + [(256, 128, nbytes), (256, 16, nbytes)]:      # too small; misaligned
        arena = Arena(dev, 48 << 20)
        group, rank, ucount, out = enqueue(arena, arena.region(declared, align, shift, 0xFF, "workspace"), declared)
        for entry, args in (("ophip_sfm_points2d_group", group), ("ophip_sfm_points2d_rank", rank)):
            with pytest.raises(ValueError):
                hip.call(entry, *args)
        torch.cuda.synchronize()
        arena.check()
        assert int(ucount) == -1 and all(bool((v.view(-1).view(U8) == 0xFF).all()) for v in out.values())


# ------------------------------------------------------------------------------------------------
# the frame block
# ------------------------------------------------------------------------------------------------
FRAME_KEYS = ("b_ids", "i_ids", "j_ids", "m_bids", "gt_mask", "mconf", "mkpts_3d_db", "mkpts_query_c", "mkpts_query_f", "expec_f", "conf_matrix")
FRAME_FORMS = ["plain", "query_mask", "object_cache_depth1", "object_cache_depth2", "lazy_conf"]


def frame_model(sd, cfg, dev, **extra):
    c = copy.deepcopy(cfg)
    c.update(extra)
    m = OnePosePlus_model(c).eval()
    m.load_state_dict(sd, strict=True)
    return m.to(dev)


@rows("ophip_frame_enqueue", "ophip_frame_enqueue_padded", "ophip_frame_enqueue_object", "ophip_encoder_object_x3w8")
@pytest.mark.parametrize("form", FRAME_FORMS)
def test_frame_block(sd, cfg, dev, monkeypatch, form):
    """ophip_frame_layout + ophip_frame_enqueue / _padded / _object through ``model.enqueue_features`` on the 128 x 160, 900-point frames of
    tests/test_gpu_parity.py::test_frame_call_equals_the_stage_by_stage_path: the block of ``layout.total`` bytes (and the object cache's
    buffers) come from the arena -- the model's ``torch.empty`` is routed there -- at a 256-byte base that is no multiple of 512, too.  (c):
    every key that test compares equals the stage-by-stage path's, bit for bit."""
    from onepose_st_amd import ops
    if form.startswith("object_cache"):
        monkeypatch.setenv("OPHIP_OBJECT_CACHE_DEPTH", form[-1])
    extra = {"hip_cache_object": True} if form.startswith("object_cache") else ({"hip_conf_matrix": "lazy"} if form == "lazy_conf" else {})
    fast, slow = frame_model(sd, cfg, dev, hip_frame_call=True, **extra), frame_model(sd, cfg, dev, hip_frame_call=False)
    f = make_synthetic_inputs(sd, n_points=900, image_hw=(128, 160), n_plant=350, seed=47, config=cfg, frame=1)
    obj = {k: f[k].to(dev) for k in ("keypoints3d", "descriptors3d_db", "descriptors3d_coarse_db")}
    if form == "query_mask":
        qm = torch.ones(1, 16, 20, dtype=torch.bool)
        qm[:, :, 15:] = False
        obj["query_image_mask"] = qm.to(dev)
    fc, ff = f["feat_c"].to(dev), f["feat_f"].to(dev)
    want = dict(obj)
    slow.forward_features(want, fc, ff, f["image_hw"])
    torch.cuda.synchronize()
    assert len(want["i_ids"]) > 100
    outs = {}
    for align, shift in bases(256):
        for fill in FILLS:
            arena = Arena(dev, 256 << 20)
            fast._obj_cache = None
            calls = ops.CALLS["frame_enqueue"]
            log = []
            with guarded_empty(arena, fill, [model_module, layercall], align, shift, log=log):      # (layercall: the object cache's workspace)
                d = dict(obj)
                fast.enqueue_features(d, fc, ff, f["image_hw"], inputs_ready=True, host_copy=True).finish()
                if form == "lazy_conf":
                    d["conf_matrix"] = d["conf_matrix"].materialize()
                torch.cuda.synchronize()
            assert ops.CALLS["frame_enqueue"] == calls + 1
            block = max((t for t in log if t.dtype == U8 and t.dim() == 1), key=lambda t: t.numel())       # layout.total bytes
            assert block.data_ptr() % align == shift and fast._frame_plans
            assert block.numel() in {int(plan[1].total) for plan in fast._frame_plans.values()}
            lo = block.data_ptr()
            assert all(lo <= d[k].data_ptr() < lo + block.numel() for k in ("mconf", "mkpts_query_f", "expec_f"))      # views of the guarded block
            assert (fast._obj_cache is not None) == form.startswith("object_cache")
            if fast._obj_cache is not None:
                assert (fast._obj_cache["y3d0"] is None) == form.endswith("1")
            arena.check()
            outs[shift, fill] = {k: d[k].clone() for k in FRAME_KEYS}
            fast._obj_cache = None
    for key, out in outs.items():
        for k in FRAME_KEYS:
            assert same_bits(out[k], want[k]), f"{k} at (base shift, fill) = {key} differs from the stage-by-stage path"
