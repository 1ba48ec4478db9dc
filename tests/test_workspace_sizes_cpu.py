"""The host side of the workspace contract (include/onepose_hip.h), on a machine without a GPU: the ``*_workspace_*()`` helpers and
``ophip_frame_layout`` answer without a device (tests/test_cabi_binding.py::test_call_arity_with_the_real_library relies on the same).

* every helper is monotone in each argument and at least the sum of the sub-regions its code carves out, at the LARGEST address shift
  the stated alignment allows (the x3w8 encoder's K^T V block is rounded up to 256 bytes by the pointer's own address, the fragment
  planes and the Sinkhorn potentials to 64: restated here, and for the planes asked of ``ophip_coarse_frag_planes`` itself);
* ``ophip_frame_layout``: regions ordered, disjoint, 256-aligned, the two workspaces at least their helpers' sizes;
* a misaligned workspace is refused before anything is launched, by every entry point that takes one;
* every prototype of the header with a ``workspace`` or ``block`` parameter has a row in tests/test_gpu_workspace_contract.py."""
import ctypes
import itertools

import pytest

from onepose_st_amd import hip
from tests import bf16_faithful as bf
from tests.test_gpu_workspace_contract import ENTRY_ROWS

BS = (1, 2, 3)
LS = (1, 31, 32, 33, 47, 48, 49, 70, 97, 127, 128, 129, 300, 1408)
KV_FLOATS = 8448                      # a K^T V | Ksum slab in f32: 8 heads x (32 x 32 + 32), in all three linear encoders
C = 256


@pytest.fixture(scope="module")
def lib():
    return hip.load()


def three_args(lib, name):
    return lambda B, a, b: getattr(lib, name)(B, a, b)


HELPERS_3 = ("ophip_encoder_workspace_floats", "ophip_encoder_bf16_workspace_bytes", "ophip_encoder_x3w8_workspace_bytes",
             "ophip_encoder_full_workspace_bytes", "ophip_encoder_full_stream_workspace_bytes", "ophip_coarse_workspace_floats",
             "ophip_coarse_sinkhorn_workspace_floats")


@pytest.mark.parametrize("name", HELPERS_3)
def test_helpers_of_three_sizes_are_monotone(lib, name):
    f = three_args(lib, name)
    for B, a, b in itertools.product(BS, LS, LS):
        here = f(B, a, b)
        assert here > 0
        assert f(B + 1, a, b) >= here and f(B, a + 1, b) >= here and f(B, a, b + 1) >= here, (name, B, a, b)
    for k in range(len(LS) - 1):
        assert f(2, LS[k + 1], 45) >= f(2, LS[k], 45) and f(2, 70, LS[k + 1]) >= f(2, 70, LS[k])


def test_postopt_and_points2d_helpers(lib):
    po, p2 = lib.ophip_postopt_workspace_bytes, lib.ophip_sfm_points2d_workspace_bytes
    for L, P, steps in itertools.product((1, 7, 300, 5000), (1, 3, 300), (1, 20, 1000)):
        here = po(L, P, steps)
        assert here % 256 == 0 and here >= 2 * P * 8 + (4 + steps) * 4 + L * 8              # Adam moments, stop flag and counters, >= 1 double per row
        assert po(L + 1, P, steps) >= here and po(L, P + 1, steps) >= here and po(L, P, steps + 1) >= here
    assert po(0, 1, 1) == 0 and po(1, 0, 1) == 0 and po(1, 1, 0) == 0
    for T, I in itertools.product((1, 9, 1000, 70000), (1, 4, 60)):
        here = p2(T, I)
        assert here % 256 == 0 and here >= 2 * T * (8 + 4 + 8 + 4) + I * 4 + 16           # unique keys, ids, scores, ranks of 2T observations
        assert p2(T + 1, I) >= here and p2(T, I + 1) >= here
    assert p2(0, 1) == 0 and p2(1, 0) == 0 and p2(1 << 30, 1) == 0 and p2(1, (1 << 22) + 1) == 0


def test_encoder_helpers_cover_their_sub_regions(lib):
    kvb = lib.ophip_encoder_x3w8_kv_block_bytes()
    assert kvb == bf.KV_BLOCK_BYTES and kvb % 256 == 0
    for B, L3, L2 in itertools.product(BS, LS, LS):
        t32, t48 = (L3 + 31) // 32 + (L2 + 31) // 32, (L3 + 47) // 48 + (L2 + 47) // 48
        # f32: one slab per 32-token tile, then the two summed blocks per batch element; no address-dependent part
        assert lib.ophip_encoder_workspace_floats(B, L3, L2) >= B * t32 * KV_FLOATS + B * 2 * KV_FLOATS
        # full attention: Q, K, V and message planes of both streams / of one query stream and its source
        assert lib.ophip_encoder_full_workspace_bytes(B, L3, L2) >= 4 * B * (L3 + L2) * C * 4
        assert lib.ophip_encoder_full_stream_workspace_bytes(B, L3, L2) >= 2 * B * (L3 + L2) * C * 4
        # plain bf16 (256-byte aligned): two slab sets, the block at the next 256-byte ADDRESS (bf.kv_block_offset mirrors layer_bf16)
        declared = lib.ophip_encoder_bf16_workspace_bytes(B, L3, L2)
        for base in (0, 256):
            assert bf.kv_block_offset(base, B, L3, L2) + B * 2 * bf.KV_BLOCK_BYTES <= declared
        # x3w8 (16-byte aligned): the mirror of layer_x3w8's carve-up at every base residue the alignment allows
        declared = lib.ophip_encoder_x3w8_workspace_bytes(B, L3, L2)
        shifts = set()
        for residue in range(0, 256, 16):
            off = x3w8_kv_block_offset(residue, B, L3, L2)
            shifts.add(off - 2 * B * t48 * KV_FLOATS * 4)
            assert (residue + off) % 256 == 0 and off + B * 2 * kvb <= declared, (B, L3, L2, residue)
        assert max(shifts) == 240 and min(shifts) == 0             # every shift a 16-byte aligned caller can cause


def x3w8_kv_block_offset(base_addr, B, L3, L2):
    """byte offset of the summed K^T V | Ksum blocks ``[B][2][kv_block_bytes]`` inside the x3w8 workspace at address ``base_addr``: behind
    the two slab sets (one slab per 48-token tile), at the next ADDRESS that is a multiple of 256 (csrc/encoder_x3w8.hip, layer_x3w8)"""
    part_floats = B * ((L3 + 47) // 48 + (L2 + 47) // 48) * KV_FLOATS
    off = 2 * part_floats * 4
    return off + (-(base_addr + off)) % 256


def coarse_ws(B, N, M):
    """csrc/coarse_match.hip coarse_ws in floats: -> (offset of the fragment planes, offset of what follows them, total)"""
    ntr, ntc = (N + 127) // 128, (M + 127) // 128
    nspan = max(ntc, (M + 1023) // 1024)
    f = B * ntc * N * 2 + B * ntr * M * 2 + B * N * 2 + B * M * 2          # row / column partials and merged statistics
    f += B * nspan * N * 3 + B * M + B * N + B * M                        # row-best records, column maxima, the two log tables
    f += B * N + (B * N + 255) // 256 + 4                                 # select_decide's choice per point, matches per workgroup
    planes = f
    f += B * (ntr + ntc) * 128 * C + 64                                   # (hi, lo) bf16 fragment planes, rows padded to 128, + the round-up
    return planes, f, f + B * 4 + 64                                      # per-pair border limits, + slack


def test_coarse_helper_equals_its_map_and_the_planes_fit_at_every_residue(lib):
    for B, N, M in itertools.product(BS, LS, LS):
        planes, behind, total = coarse_ws(B, N, M)
        assert lib.ophip_coarse_workspace_floats(B, N, M) == total, (B, N, M)
        ntr, ntc = (N + 127) // 128, (M + 127) // 128
        shifts = set()
        for residue in range(0, 256, 16):
            base = (1 << 40) + residue                                    # an address: ophip_coarse_frag_planes only computes with it
            pa, pb = ctypes.c_void_p(), ctypes.c_void_p()
            hip.call("ophip_coarse_frag_planes", ctypes.c_void_p(base), B, N, M, ctypes.byref(pa), ctypes.byref(pb))
            assert pa.value % 64 == 0 and pa.value - base >= 4 * planes
            shifts.add(pa.value - base - 4 * planes)
            assert pb.value == pa.value + B * ntr * 128 * C * 4
            assert pb.value + B * ntc * 128 * C * 4 <= base + 4 * behind, (B, N, M, residue)          # ends in front of the next sub-region
        assert len(shifts) == 4 and max(shifts) < 64               # the four shifts a 16-byte aligned caller can cause


def test_sinkhorn_helper_covers_the_potentials_at_every_residue(lib):
    for B, L0, L1 in itertools.product(BS, LS, LS):
        coarse, total = lib.ophip_coarse_workspace_floats(B, L0, L1), lib.ophip_coarse_sinkhorn_workspace_floats(B, L0, L1)
        up, vp, nchunk = (L0 + 4) // 4 * 4, (L1 + 4) // 4 * 4, (L0 + 127) // 128
        own = B * up + B * vp + B * nchunk * L1 * 2 + (B * L1 + 3) // 4          # u, v, column partials per 128-row chunk, prefilter bytes
        for residue in range(0, 64, 16):
            start = coarse + (16 - ((residue // 4 + coarse) % 16)) % 16          # the next 64-byte ADDRESS (csrc/coarse_sinkhorn.hip, sinkhorn_impl)
            assert start + own <= total, (B, L0, L1, residue)
    assert lib.ophip_coarse_sinkhorn_workspace_floats(0, 1, 1) == 0


# ------------------------------------------------------------------------------------------------
# ophip_frame_layout
# ------------------------------------------------------------------------------------------------
def frame_desc(B, N, hc, wc, lazy, n_coarse=4, cross_bits=0b1010):
    d = hip.FrameDesc()
    d.B, d.N, d.M, d.hc, d.wc, d.hf, d.wf, d.cf = B, N, hc * wc, hc, wc, 4 * hc, 4 * wc, 128
    d.lazy_conf, d.n_coarse, d.coarse_cross_bits, d.n_fine, d.fine_cross_bits = int(lazy), n_coarse, cross_bits, 2, 0b10
    return d


@pytest.mark.parametrize("lazy", [0, 1])
@pytest.mark.parametrize("external_x3d", [0, 1, 2])
@pytest.mark.parametrize("transpose_fine", [0, 1])
@pytest.mark.parametrize("B,N,hc,wc,n_coarse", [(1, 900, 16, 20, 4), (2, 129, 9, 9, 3), (3, 1, 1, 1, 2), (1, 1408, 24, 32, 8)])
def test_frame_layout(lib, B, N, hc, wc, n_coarse, transpose_fine, external_x3d, lazy):
    d, L = frame_desc(B, N, hc, wc, lazy, n_coarse), hip.FrameLayout()
    hip.call("ophip_frame_layout", ctypes.byref(d), transpose_fine, external_x3d, ctypes.byref(L))
    M, cap = hc * wc, B * N
    rows = 4 * B * N * C
    regions = [("x2d", 4 * B * M * C), ("ffcl", 4 * B * d.hf * d.wf * d.cf if transpose_fine else None), ("x3d", None if external_x3d else rows),
               ("y3d", rows), ("y2d", 4 * B * M * C), ("z3d", rows if external_x3d else None), ("stats", (4 * B + 4) * 4),
               ("enc_ws", lib.ophip_encoder_x3w8_workspace_bytes(B, N, M)), ("conf", None if lazy else 4 * B * N * M),
               ("cws", 4 * lib.ophip_coarse_workspace_floats(B, N, M)), ("result", 16 + 28 * cap), ("i_ids", 8 * cap), ("j_ids", 8 * cap),
               ("m_bids", 8 * cap), ("gt_mask", cap), ("mconf", 4 * cap), ("mkc", 8 * cap), ("expec", 12 * cap)]
    end = 0
    for name, nbytes in regions:
        at = getattr(L, name)
        if nbytes is None:
            assert at == 0, f"{name} is not part of this layout"
            continue
        assert at % 256 == 0 and at >= end, f"{name} at {at} starts before the previous region ends ({end})"
        end = at + nbytes
    assert L.total >= end and L.total % 256 == 0 and L.result_bytes == 16 + 28 * cap
    present = {name: getattr(L, name) for name, nbytes in regions if nbytes is not None}
    assert L.feat3d_out in {present[k] for k in ("x3d", "y3d", "z3d") if k in present}
    assert L.feat2d_out in (present["x2d"], present["y2d"])
    bigger, L2 = frame_desc(B + 1, N, hc, wc, lazy, n_coarse), hip.FrameLayout()
    hip.call("ophip_frame_layout", ctypes.byref(bigger), transpose_fine, external_x3d, ctypes.byref(L2))
    assert L2.total >= L.total


def test_frame_layout_refuses_what_it_cannot_lay_out(lib):
    L = hip.FrameLayout()
    with pytest.raises(ValueError):
        hip.call("ophip_frame_layout", ctypes.byref(frame_desc(1, 10, 3, 3, 0)), 0, 3, ctypes.byref(L))
    with pytest.raises(ValueError):                                      # a cached first layer needs a first layer of kind "self"
        hip.call("ophip_frame_layout", ctypes.byref(frame_desc(1, 10, 3, 3, 0, cross_bits=0b0101)), 0, 2, ctypes.byref(L))
    with pytest.raises(ValueError):
        hip.call("ophip_frame_layout", ctypes.byref(frame_desc(0, 10, 3, 3, 0)), 0, 0, ctypes.byref(L))


# ------------------------------------------------------------------------------------------------
# refusals, and the table of the GPU file against the header
# ------------------------------------------------------------------------------------------------
# stated alignment of each entry's workspace / block (include/onepose_hip.h); the two whose size is an argument check it first and are
# covered where a device is at hand (tests/test_gpu_postopt.py, tests/test_gpu_sfm_points2d.py, tests/test_gpu_workspace_contract.py)
ALIGN_256 = {"ophip_encoder_layer_bf16", "ophip_encoder_layer_bf16_masked", "ophip_frame_enqueue", "ophip_frame_enqueue_padded",
             "ophip_frame_enqueue_object", "ophip_postopt_refine", "ophip_sfm_points2d_group", "ophip_sfm_points2d_rank"}
SIZE_FIRST = {"ophip_postopt_refine", "ophip_sfm_points2d_group", "ophip_sfm_points2d_rank"}


def workspace_entries():
    protos = hip._BINDING.header.prototypes
    return {name: p for name, p in protos.items() if any(n in ("workspace", "block") for _, n in p.params)}


def test_every_workspace_entry_has_a_row_in_the_gpu_table():
    entries = workspace_entries()
    assert len(entries) >= 29 and "ophip_frame_enqueue_object" in entries and "ophip_encoder_kv_first_x3w8" in entries
    missing = sorted(set(entries) - set(ENTRY_ROWS))
    assert not missing, f"no row in tests/test_gpu_workspace_contract.py for {missing}"
    assert not sorted(set(ENTRY_ROWS) - set(entries)), "rows for entry points that take no workspace"


def refusal_args(proto, ws_addr, keep):
    """Arguments that no entry point can launch with -- B (or Bo) is 0, and a frame's layout does not match its inputs -- so that the
    call is refused whatever else happens: the test tells the refusals apart by their message.  Pointers are distinct made-up
    addresses, never dereferenced by a check."""
    args, k = [], 0
    for ctype_, name in proto.params:
        bare = ctype_.replace("const", "").strip()
        if name in ("workspace", "block"):
            args.append(ctypes.c_void_p(ws_addr))
        elif bare == "ophip_frame_desc*":
            keep.append(hip.FrameDesc())
            args.append(ctypes.byref(keep[-1]))
        elif bare == "ophip_frame_layout_t*":
            layout = hip.FrameLayout()
            layout.result_bytes = 16                                   # host_bytes = 16 passes; x3d = 0 says "external" and none is given
            keep.append(layout)
            args.append(ctypes.byref(layout))
        elif bare == "ophip_object_cache*" or name == "x3d_external":
            args.append(None)
        elif bare == "void**":
            keep.append(ctypes.c_void_p())
            args.append(ctypes.byref(keep[-1]))
        elif bare.endswith("*"):
            k += 1
            args.append(ctypes.c_void_p((1 << 41) + 0x10000 * k))
        elif bare == "size_t":
            args.append(16)
        elif bare in ("float", "double"):
            args.append(1.0)
        else:
            args.append(0 if name in ("B", "Bo") and proto.name != "ophip_coarse_frag_planes" else 1)      # (that one launches nothing at all)
    return args


@pytest.mark.parametrize("name", sorted(set(workspace_entries()) - SIZE_FIRST))
def test_misaligned_workspace_is_refused_before_any_launch(lib, name):
    proto = workspace_entries()[name]
    need = 256 if name in ALIGN_256 else 16
    base = 1 << 40
    for off in sorted({4, 8, need // 2, need + need // 2, 256 + need // 2}):
        keep = []
        assert getattr(lib, name)(*refusal_args(proto, base + off, keep)) == -1
        assert "aligned" in lib.ophip_last_error().decode(), (name, off, lib.ophip_last_error().decode())
    for off in (0, need, 256, 512 + need):                           # at the stated alignment the refusal is another one (the sizes)
        keep = []
        rc = getattr(lib, name)(*refusal_args(proto, base + off, keep))
        if name == "ophip_coarse_frag_planes":
            assert rc == 0 and keep[0].value % 64 == 0
            continue
        assert rc == -1 and "aligned" not in lib.ophip_last_error().decode(), (name, off, lib.ophip_last_error().decode())
