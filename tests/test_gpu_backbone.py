"""GPU parity of the hand-written backbone convolutions through the C ABI.

Each convolution is compared with the same op on plain PyTorch fp32 (``F.conv2d`` / ``F.interpolate`` on the device); the
whole backbone is compared with the CPU oracle's ``backbone_8_2`` (reference ``backbone/resnet.py:85-164``) on the same
seeded weights and image.  Tolerances: split-bf16 (``bf16x3``) products carry ~2^-17 relative error per term and f32
accumulation -> 2e-5 of the output scale per layer, 1e-4 over the 22-convolution stack; plain bf16 only has to be close
(2e-2), it is not the parity mode.

Tile shapes.  ``launch_conv`` picks the wave tile (th, nt, wave rows) from the sizes (``conv_tile_shape`` in ``csrc/conv.hip``,
readable through ``ophip_conv_tile_shape``).  ``CASES`` are small maps: they run (1, 1, 1) for 3x3 and (1, 2, 1) for 1x1 only.
``SHAPE_CASES`` put every other shape the rule can give under a direct comparison, at sizes with a ragged second tile column
(Wout = 37), an odd row count (251 / 125: a ragged last row tile for every th * wave rows) and, with 196 output channels, a clamped
eighth channel tile that the epilogue has to drop.  Their reference is float64, built tap by tap on the device (``conv_ref64``), so
it shares no code with the kernel and none with MIOpen; the bounds are the same 2e-5 / 2e-2 of the output's largest magnitude (a
float64 reference adds no error of its own, the fp32 one of ``CASES`` adds ~1e-6).
``test_every_shape_the_product_picks_has_a_parity_case`` closes the loop: whatever shape the backbone's own calls get at 480 x 640
(B = 1 and 4) and 512 x 512 must be one that a case of this file runs.

Measured on the MI355X, max |f32 output - reference| / max |reference| (split bound 2e-5, plain bound 2e-2):

    case  cin->cout  Hin x Win  ks,s  shape      split     plain
    1     128->196   251 x 37   3,1   (2, 2, 2)  4.44e-06  1.08e-03
    2     128->128   251 x 37   3,1   (2, 2, 2)  5.20e-06  1.19e-03      (B = 4)
    3     196->196   125 x 37   3,1   (2, 1, 1)  5.01e-06  1.68e-03
    4     128->196   501 x 73   3,2   (2, 2, 1)  3.75e-06  1.49e-03
    5     128->196   249 x 73   3,2   (1, 2, 1)  4.81e-06  1.70e-03
    6     196->256   251 x 37   1,1   (2, 2, 1)  4.17e-06  1.33e-03
    7     128->196   501 x 73   1,2   (2, 2, 1)  5.95e-06  1.80e-03
    8     256->256   251 x 37   1,1   (2, 2, 1)  3.69e-06  1.33e-03

The planes of the same runs: 5.8e-06 .. 7.6e-06 in split mode (bound 4e-5), 2.6e-03 .. 3.8e-03 in plain mode (bound 2.8e-2).

Plain mode like for like.  The 1e-3 of the plain column is the bf16 rounding of the WEIGHTS, which the reference above does not apply (it
rounds ``x`` and the residual only).  Against the reference that also takes ``bf16_round(w)`` (the packer's hi plane) the plain mode's f32
output meets the split mode's bar: 1.7e-07 .. 2.0e-06 of scale over the eight cases (bound 2e-5), 1.5e-07 .. 7.3e-07 over ``CASES``, and
the hi plane lies within one bf16 rounding of it (|plane - ref| - 2^-8 |ref| <= 9.4e-07 of scale, bound 2e-5).  Both bounds are asserted
beside the 2e-2 ones.

Seeded errors (``OPHIP_CONV_ERR_*`` in ``csrc/conv.hip``; ``EXTRA=-DOPHIP_CONV_ERR_TH tools/build_variant.sh err_th -`` and the file run
with ``OPHIP_LIB`` on that library).  What each one fails:

* ``_TH`` (second accumulator row on the first row's activations): the tile-shape cases 1, 2, 3, 4, 6, 7, 8 in both modes (every
  th = 2 case; case 5 is th = 1 and passes) and ``test_backbone_vs_oracle[1-240-320]``.  Of the tests the file had before, that one
  alone: at 240 x 320 the 196-channel FPN convolutions on the 1/2-resolution map have w22 = 1200, so ``l1out2.0`` / ``l1out2.3`` run
  (2, 1, 1) there, and the 1e-4 bound of the whole stack sees it.  All ``CASES`` pass: none of them has th = 2.
* ``_NT`` (second channel tile on the first tile's weights): the tile-shape cases 1, 2, 4, 5, 6, 7, 8 in both modes (every nt = 2 case;
  case 3 is nt = 1 and passes), ``CASES`` 4, 5, 6 (the 1x1 convolutions: small 1x1 maps run (1, 2, 1), so nt = 2 was compared with a
  reference before, for 1x1 only), both ``test_backbone_vs_oracle``, ``test_backbone_matches_torch_module_and_pe_fusion`` and
  ``test_model_forward_hip_backbone_vs_miopen_backbone``.  New with the tile-shape cases: nt = 2 under a 3x3 kernel (1, 2, 4, 5) and
  together with th = 2 (1, 2, 4, 6, 7, 8).
* ``_WR`` (two wave rows, every stage row from ``acc[t][0]``): the tile-shape cases 1 and 2 in both modes, nothing else: no test the
  file had before runs two wave rows.
* ``_UP`` (bilinear add with ``uy0`` for both rows): tile-shape case 6 and ``CASES`` 5 in both modes, both ``test_backbone_vs_oracle``,
  ``test_backbone_matches_torch_module_and_pe_fusion``.

(``CASES`` counted from 0, as pytest's ids do.)
"""
import ctypes

import pytest
import torch
import torch.nn.functional as F

from onepose_st_amd import hip, packing
from onepose_st_amd.backbone import build_backbone
from onepose_st_amd.backbone_hip import HipBackbone, pack_backbone
from onepose_st_amd.config import default_config
from onepose_st_amd.model import OnePosePlus_model
from onepose_st_amd.synthetic import make_synthetic_inputs
from onepose_st_amd.synthetic import make_synthetic_state_dict
from tests.bf16_faithful import bf16_round

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def dev():
    if not torch.cuda.is_available():
        pytest.skip("needs the MI355X")
    hip.load()
    return torch.device("cuda:0")


def to_planes(x_nchw, cpad):
    """f32 NCHW -> (hi, lo) bf16 channels-last planes with zero channel padding"""
    B, C, H, W = x_nchw.shape
    x = torch.zeros(B, H, W, cpad, device=x_nchw.device)
    x[..., :C] = x_nchw.permute(0, 2, 3, 1)
    hi = x.to(torch.bfloat16)
    lo = (x - hi.float()).to(torch.bfloat16)
    return hi.contiguous(), lo.contiguous()


def from_planes(hi, lo, C):
    return (hi.float() + lo.float())[..., :C].permute(0, 3, 1, 2)


def run_conv(dev, x, w, bias, stride, act, res=None, up=None, table=None, nsplit=3, want_f32=True):
    cout, cin, ks, _ = w.shape
    cip, cop = packing.pad32(cin), packing.pad32(cout)
    B, _, H, W = x.shape
    xh, xl = to_planes(x, cip)
    wp = packing.pack_conv_bf16(w.cpu(), bias.cpu()).to(dev)
    assert wp.numel() == hip.load().ophip_conv_wpack_bytes(cip, cop, ks)
    Ho, Wo = (H + 2 * (ks // 2) - ks) // stride + 1, (W + 2 * (ks // 2) - ks) // stride + 1
    oh = torch.full((B, Ho, Wo, cop), 7.0, dtype=torch.bfloat16, device=dev)
    ol = torch.full((B, Ho, Wo, cop), 7.0, dtype=torch.bfloat16, device=dev)
    # the f32 map is followed by one padded pixel of guard: a store at or above out_c of the last pixel would land there
    o32_buf = torch.full((B * Ho * Wo * cout + cop,), 7.0, device=dev) if want_f32 else None
    o32 = o32_buf[:B * Ho * Wo * cout].view(B, Ho, Wo, cout) if want_f32 else None
    rh = rl = None
    if res is not None:
        rh, rl = to_planes(res, cop)
    upp = None
    if up is not None:
        upp = torch.zeros(B, up.shape[2], up.shape[3], cop, device=dev)
        upp[..., :cout] = up.permute(0, 2, 3, 1)
    tab = None
    if table is not None:
        tab = torch.zeros(Ho, Wo, cop, device=dev)
        tab[..., :cout] = table.permute(1, 2, 0)
    P = hip.ptr
    hip.call("ophip_conv2d_bf16", P(xh, None), P(xl, None), B, H, W, cip, P(wp, None), cop, ks, stride, act,
             P(rh, None), P(rl, None), P(upp), upp.shape[1] if upp is not None else 0, upp.shape[2] if upp is not None else 0, P(tab),
             P(oh, None), P(ol, None), P(o32), cout if want_f32 else 0, nsplit, hip.stream_handle())
    torch.cuda.synchronize()
    got_planes = from_planes(oh, ol if nsplit == 3 else torch.zeros_like(ol), cout)
    if cop > cout:
        assert float(oh[..., cout:].float().abs().max()) == 0.0          # padding channels stay exactly zero
        if nsplit == 3:
            assert float(ol[..., cout:].float().abs().max()) == 0.0
    if want_f32:
        assert bool((o32_buf[B * Ho * Wo * cout:] == 7.0).all())         # nothing written at or above out_c
    return got_planes, (o32.permute(0, 3, 1, 2) if want_f32 else None)


def torch_conv(x, w, bias, stride, act, res=None, up=None, table=None):
    y = F.conv2d(x, w, bias, stride=stride, padding=w.shape[2] // 2)
    if res is not None:
        y = y + res
    if up is not None:
        y = y + F.interpolate(up, size=y.shape[2:], mode="bilinear", align_corners=True)
    if table is not None:
        y = y + table[None]
    return {0: lambda t: t, 1: F.relu, 2: lambda t: F.leaky_relu(t, 0.01)}[act](y)


CASES = [
    # B, cin, cout, H, W, ks, stride, act, res, up, table
    (1, 128, 128, 24, 40, 3, 1, 1, False, False, False),
    (2, 128, 128, 13, 37, 3, 1, 1, True, False, False),      # ragged tile edges + residual
    (1, 128, 196, 24, 40, 3, 2, 1, False, False, False),     # stride 2, 196 -> padded 224 (7 channel tiles: a 1-tile wave)
    (1, 196, 196, 12, 20, 3, 1, 2, False, False, False),     # cin 196 padded, LeakyReLU
    (1, 128, 196, 24, 40, 1, 2, 0, False, False, False),     # 1x1 stride-2 shortcut
    (1, 196, 256, 12, 20, 1, 1, 0, False, True, False),      # 1x1 + bilinear x2 top-down add
    (1, 256, 256, 6, 10, 1, 1, 0, False, False, True),       # 1x1 + positional-encoding table
    (1, 256, 196, 12, 20, 3, 1, 0, False, False, False),
    (2, 196, 128, 9, 33, 3, 1, 0, False, False, False),
]


@pytest.mark.parametrize("nsplit,tol", [(3, 2e-5), (1, 2e-2)])
@pytest.mark.parametrize("case", CASES)
def test_conv_vs_torch(dev, case, nsplit, tol):
    B, cin, cout, H, W, ks, stride, act, use_res, use_up, use_tab = case
    g = torch.Generator().manual_seed(hash(case) % (2 ** 31))
    x = torch.randn(B, cin, H, W, generator=g).to(dev)
    w = (torch.randn(cout, cin, ks, ks, generator=g) / (cin * ks * ks) ** 0.5).to(dev)
    bias = (0.1 * torch.randn(cout, generator=g)).to(dev)
    Ho, Wo = (H + 2 * (ks // 2) - ks) // stride + 1, (W + 2 * (ks // 2) - ks) // stride + 1
    res = torch.randn(B, cout, Ho, Wo, generator=g).to(dev) if use_res else None
    up = torch.randn(B, cout, Ho // 2, Wo // 2, generator=g).to(dev) if use_up else None
    table = torch.randn(cout, Ho, Wo, generator=g).to(dev) if use_tab else None
    if nsplit == 1:      # plain-bf16 mode sees bf16-rounded inputs; compare like with like
        x = x.to(torch.bfloat16).float()
    got_p, got_f = run_conv(dev, x, w, bias, stride, act, res, up, table, nsplit)
    res_ref = res
    if res is not None and nsplit == 1:
        res_ref = res.to(torch.bfloat16).float()
    ref = torch_conv(x, w, bias, stride, act, res_ref, up, table)
    scale = float(ref.abs().max())
    assert float((got_f - ref).abs().max()) <= tol * scale
    # planes hold the same values rounded to hi + lo (16 mantissa bits) / hi only
    assert float((got_p - ref).abs().max()) <= (tol + (2e-5 if nsplit == 3 else 8e-3)) * scale
    if nsplit == 1:
        # like for like: the reference takes the weights the kernel multiplies by (the packer's hi plane) as well.  What is left is f32
        # accumulation order -> the split mode's bar on the f32 output; the hi plane of it adds one bf16 rounding of each element
        ref = torch_conv(x, bf16_round(w), bias, stride, act, res_ref, up, table)
        scale = float(ref.abs().max())
        err_f = float((got_f - ref).abs().max()) / scale
        print(f"conv case {CASES.index(case)} plain bf16 like for like: f32 {err_f:.2e} of scale")
        assert err_f <= 2e-5
        assert bool(((got_p - ref).abs() <= 2.0 ** -8 * ref.abs() + 2e-5 * scale).all())


def conv_ref64(x, w, bias, stride, act, res=None, up=None, table=None):
    """The same operation in float64 on the device, tap by tap: one einsum over the shifted input slice per tap (the zero padding is
    the part of the output a tap does not reach), then residual, bilinear upsampling, table and activation, all in float64."""
    x, w = x.double(), w.double()
    B, cin, H, W = x.shape
    cout, _, ks, _ = w.shape
    pad = ks // 2
    Ho, Wo = (H + 2 * pad - ks) // stride + 1, (W + 2 * pad - ks) // stride + 1
    y = bias.double().view(1, cout, 1, 1).repeat(B, 1, Ho, Wo)

    def span(k, n_in, n_out):          # output indices o with 0 <= o * stride + k - pad < n_in, and the first input index
        o0 = -((k - pad) // stride) if k < pad else 0
        o1 = min(n_out, (n_in - 1 - k + pad) // stride + 1)
        return o0, o1, o0 * stride + k - pad

    for ky in range(ks):
        for kx in range(ks):
            oy0, oy1, iy0 = span(ky, H, Ho)
            ox0, ox1, ix0 = span(kx, W, Wo)
            xs = x[:, :, iy0:iy0 + (oy1 - oy0 - 1) * stride + 1:stride, ix0:ix0 + (ox1 - ox0 - 1) * stride + 1:stride]
            y[:, :, oy0:oy1, ox0:ox1] += torch.einsum("bchw,oc->bohw", xs, w[:, :, ky, kx])
    if res is not None:
        y = y + res.double()
    if up is not None:
        y = y + F.interpolate(up.double(), size=(Ho, Wo), mode="bilinear", align_corners=True)
    if table is not None:
        y = y + table.double()[None]
    return {0: lambda t: t, 1: F.relu, 2: lambda t: F.leaky_relu(t, 0.01)}[act](y)


def tile_shape(B, H, W, cout, ks, stride):
    th, nt, wr = ctypes.c_int(0), ctypes.c_int(0), ctypes.c_int(0)
    hip.call("ophip_conv_tile_shape", B, H, W, packing.pad32(cout), ks, stride, ctypes.byref(th), ctypes.byref(nt), ctypes.byref(wr))
    return th.value, nt.value, wr.value


SHAPE_CASES = [
    # B, cin, cout, H, W, ks, stride, act, res, up, table, (th, nt, wave rows)                    w22
    (2, 128, 196, 251, 37, 3, 1, 1, True, False, False, (2, 2, 2)),       # 1: two wave rows, clamped 8th channel tile    2016
    (4, 128, 128, 251, 37, 3, 1, 1, True, False, False, (2, 2, 2)),       # 2: one channel group, batch 4                 2016
    (2, 196, 196, 125, 37, 3, 1, 2, False, False, False, (2, 1, 1)),      # 3: LeakyReLU                                  1008
    (2, 128, 196, 501, 73, 3, 2, 1, False, False, False, (2, 2, 1)),      # 4: stride 2 -> 251 x 37                       2016
    (2, 128, 196, 249, 73, 3, 2, 1, False, False, False, (1, 2, 1)),      # 5: stride 2 -> 125 x 37                       1008
    (2, 196, 256, 251, 37, 1, 1, 0, False, True, False, (2, 2, 1)),       # 6: bilinear add from 125 x 18                 2016
    (2, 128, 196, 501, 73, 1, 2, 0, False, False, False, (2, 2, 1)),      # 7: stride-2 shortcut                          2016
    (2, 256, 256, 251, 37, 1, 1, 0, False, False, True, (2, 2, 1)),       # 8: per-pixel table                            2016
]


@pytest.mark.parametrize("nsplit,tol", [(3, 2e-5), (1, 2e-2)])
@pytest.mark.parametrize("case", SHAPE_CASES, ids=[str(i + 1) for i in range(len(SHAPE_CASES))])
def test_conv_vs_float64_at_every_tile_shape(dev, case, nsplit, tol):
    B, cin, cout, H, W, ks, stride, act, use_res, use_up, use_tab, shape = case
    assert tile_shape(B, H, W, cout, ks, stride) == shape          # the case runs the kernel it was written for
    g = torch.Generator().manual_seed(1000 + SHAPE_CASES.index(case))
    x = torch.randn(B, cin, H, W, generator=g).to(dev)
    w = (torch.randn(cout, cin, ks, ks, generator=g) / (cin * ks * ks) ** 0.5).to(dev)
    bias = (0.1 * torch.randn(cout, generator=g)).to(dev)
    Ho, Wo = (H + 2 * (ks // 2) - ks) // stride + 1, (W + 2 * (ks // 2) - ks) // stride + 1
    res = torch.randn(B, cout, Ho, Wo, generator=g).to(dev) if use_res else None
    up = torch.randn(B, cout, Ho // 2, Wo // 2, generator=g).to(dev) if use_up else None
    table = torch.randn(cout, Ho, Wo, generator=g).to(dev) if use_tab else None
    if nsplit == 1:      # plain-bf16 mode sees bf16-rounded inputs; compare like with like
        x = x.to(torch.bfloat16).float()
        if res is not None:
            res = res.to(torch.bfloat16).float()
    got_p, got_f = run_conv(dev, x, w, bias, stride, act, res, up, table, nsplit)      # (checks the padding channels and the f32 guard)
    ref = conv_ref64(x, w, bias, stride, act, res, up, table)
    scale = float(ref.abs().max())
    err_f, err_p = float((got_f.double() - ref).abs().max()) / scale, float((got_p.double() - ref).abs().max()) / scale
    print(f"tile-shape case {SHAPE_CASES.index(case) + 1} nsplit {nsplit}: f32 {err_f:.2e}  planes {err_p:.2e}  of scale {scale:.3f}")
    assert err_f <= tol
    # planes hold the same values rounded to hi + lo (16 mantissa bits) / hi only
    assert err_p <= tol + (2e-5 if nsplit == 3 else 8e-3)
    if nsplit == 1:      # like for like in the weights too (see test_conv_vs_torch): the split mode's bar, planes within one bf16 rounding
        ref = conv_ref64(x, bf16_round(w), bias, stride, act, res, up, table)
        scale = float(ref.abs().max())
        err_f = float((got_f.double() - ref).abs().max()) / scale
        excess = float(((got_p.double() - ref).abs() - 2.0 ** -8 * ref.abs()).max()) / scale
        print(f"tile-shape case {SHAPE_CASES.index(case) + 1} plain bf16 like for like: f32 {err_f:.2e}  planes beyond 2^-8 |ref| {excess:.2e}  of scale")
        assert err_f <= 2e-5
        assert excess <= 2e-5


def _case_key(B, H, W, cout, ks, stride):
    return (ks, stride) + tile_shape(B, H, W, cout, ks, stride)


def test_every_shape_the_product_picks_has_a_parity_case(dev, backbone_setup, monkeypatch):
    """A dispatcher change that brings a kernel into the product which no case above compares with a reference fails here."""
    covered = {_case_key(c[0], c[3], c[4], c[2], c[5], c[6]) for c in CASES + SHAPE_CASES}
    cfg, bsd = backbone_setup
    blocks = pack_backbone(bsd, dev)
    calls = []
    real_call = hip.call

    def recording_call(name, *args):
        if name == "ophip_conv2d_bf16":
            calls.append((args[2], args[3], args[4], args[7], args[8], args[9]))          # B, Hin, Win, cout_pad, ks, stride
        return real_call(name, *args)

    monkeypatch.setattr(hip, "call", recording_call)
    for B, H, W in ((1, 480, 640), (4, 480, 640), (1, 512, 512)):
        img = torch.rand(B, 1, H, W, generator=torch.Generator().manual_seed(B + H)).to(dev)
        HipBackbone("bf16x3").forward(blocks, img)
    torch.cuda.synchronize()
    monkeypatch.undo()
    assert len(calls) == 3 * 21          # 21 convolutions behind the stem, three forwards
    seen = {_case_key(B, H, W, cop, ks, stride) for B, H, W, cop, ks, stride in calls}
    assert seen - covered == set(), f"no parity case runs {sorted(seen - covered)} (ks, stride, th, nt, wave rows)"


@pytest.mark.parametrize("nsplit", [3, 1])
@pytest.mark.parametrize("B,H,W", [(2, 40, 72), (1, 8, 8), (3, 42, 130)])      # (1, 8, 8): one partial tile; 42 x 130 -> 21 x 65: a third tile column one pixel wide
def test_stem_vs_torch(dev, B, H, W, nsplit):
    g = torch.Generator().manual_seed(5)
    img = torch.rand(B, 1, H, W, generator=g)
    w = torch.randn(128, 1, 7, 7, generator=g) / 7.0
    bias = 0.1 * torch.randn(128, generator=g)
    wp = packing.pack_stem(w, bias).to(dev)
    Ho, Wo = (H - 1) // 2 + 1, (W - 1) // 2 + 1
    oh = torch.full((B, Ho, Wo, 128), 7.0, dtype=torch.bfloat16, device=dev)
    ol = torch.full_like(oh, 7.0) if nsplit == 3 else None
    imgd = img.to(dev)
    hip.call("ophip_stem_conv7", hip.ptr(imgd), B, H, W, hip.ptr(wp), hip.ptr(oh, None), hip.ptr(ol, None), nsplit, hip.stream_handle())
    torch.cuda.synchronize()
    ref = F.relu(F.conv2d(img.double(), w.double(), bias.double(), stride=2, padding=3))          # float64 on the CPU: one input channel
    assert tuple(ref.shape) == (B, 128, Ho, Wo)
    got = from_planes(oh, ol if nsplit == 3 else torch.zeros_like(oh), 128).double().cpu()
    # exact f32 arithmetic: 2e-5 of the output scale on hi + lo; the hi plane alone adds its bf16 rounding (the 8e-3 of the plane bound above)
    assert float((got - ref).abs().max()) <= (2e-5 if nsplit == 3 else 2e-5 + 8e-3) * float(ref.abs().max())


@pytest.fixture(scope="module")
def backbone_setup(dev):
    cfg = default_config()
    sd = make_synthetic_state_dict(0, cfg)
    bsd = {k[len("backbone."):]: v for k, v in sd.items() if k.startswith("backbone.")}
    g = torch.Generator().manual_seed(11)
    # non-trivial BatchNorm statistics so that the folding is exercised
    for k in list(bsd):
        if k.endswith("running_mean"):
            bsd[k] = 0.1 * torch.randn(bsd[k].shape, generator=g)
        elif k.endswith("running_var"):
            bsd[k] = 0.5 + torch.rand(bsd[k].shape, generator=g)
        elif k.endswith(".bias") and "bn" in k:
            bsd[k] = 0.1 * torch.randn(bsd[k].shape, generator=g)
    return cfg, bsd


@pytest.mark.parametrize("B,H,W", [(1, 240, 320), (2, 64, 104)])
def test_backbone_vs_oracle(dev, backbone_setup, B, H, W):
    from oracle import onepose_oracle as oracle
    cfg, bsd = backbone_setup
    g = torch.Generator().manual_seed(H)
    img = torch.rand(B, 1, H, W, generator=g)
    ref_c, ref_f = oracle.backbone_8_2({"backbone." + k: v for k, v in bsd.items()}, img)
    blocks = pack_backbone(bsd, dev)
    fc, ff = HipBackbone("bf16x3").forward(blocks, img.to(dev))
    torch.cuda.synchronize()
    got_c = fc.view(B, H // 8, W // 8, 256).permute(0, 3, 1, 2).cpu()
    got_f = ff.view(B, H // 2, W // 2, 128).permute(0, 3, 1, 2).cpu()
    for got, ref, name in ((got_c, ref_c, "coarse"), (got_f, ref_f, "fine")):
        err = float((got - ref).abs().max()) / float(ref.abs().max())
        assert err <= 1e-4, f"{name} map: relative max error {err:.2e}"


def test_backbone_matches_torch_module_and_pe_fusion(dev, backbone_setup):
    cfg, bsd = backbone_setup
    bb = build_backbone(cfg["loftr_backbone"])
    bb.load_state_dict(bsd)
    bb = bb.eval().to(dev)
    img = torch.rand(1, 1, 96, 128, generator=torch.Generator().manual_seed(2)).to(dev)
    with torch.no_grad():
        ref_c, ref_f = bb(img)
    blocks = pack_backbone(bsd, dev)
    pe = torch.randn(12 * 16, 256, generator=torch.Generator().manual_seed(3)).to(dev)
    fc, ff = HipBackbone("bf16x3").forward(blocks, img, pe_table=pe)
    torch.cuda.synchronize()
    want_c = ref_c.flatten(2).transpose(1, 2) + pe[None]
    assert float((fc - want_c).abs().max()) <= 1e-4 * float(want_c.abs().max())
    assert float((ff - ref_f.flatten(2).transpose(1, 2)).abs().max()) <= 1e-4 * float(ref_f.abs().max())


def test_model_forward_hip_backbone_vs_miopen_backbone(dev):
    """``model(data)`` with the reference's image input: the HIP backbone (default) against the same model with the
    backbone on PyTorch-ROCm / MIOpen fp32.  A random image gives no matches, so the comparison is on the confidence
    matrix (products of two softmaxes, values ~1e-3: relative 2e-3 covers the exp amplification of 1e-5 feature errors)."""
    cfg = default_config()
    sd = make_synthetic_state_dict(0, cfg)
    img = torch.rand(2, 1, 96, 128, generator=torch.Generator().manual_seed(9)).to(dev)
    obj = make_synthetic_inputs(sd, n_points=300, image_hw=(96, 128), n_plant=0, seed=4, config=cfg)
    outs = []
    for hip_bb in (True, False):
        c = dict(cfg)
        c["hip_backbone"] = hip_bb
        m = OnePosePlus_model(c).eval()
        m.load_state_dict(sd)
        m = m.to(dev)
        assert m.hip_backbone == hip_bb
        data = {"query_image": img, "keypoints3d": obj["keypoints3d"].to(dev).expand(2, -1, -1),
                "descriptors3d_db": obj["descriptors3d_db"].to(dev).expand(2, -1, -1),
                "descriptors3d_coarse_db": obj["descriptors3d_coarse_db"].to(dev).expand(2, -1, -1)}
        assert m(data) is None
        outs.append(data)
    a, b = outs
    assert tuple(a["q_hw_c"]) == (12, 16) and tuple(a["q_hw_f"]) == (48, 64) and a["bs"] == 2
    assert torch.equal(a["i_ids"], b["i_ids"]) and torch.equal(a["j_ids"], b["j_ids"])
    torch.testing.assert_close(a["conf_matrix"], b["conf_matrix"], rtol=2e-3, atol=1e-9)
