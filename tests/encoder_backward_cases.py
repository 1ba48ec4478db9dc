"""The seeded cases of the encoder backward's device test (tests/test_gpu_encoder_backward.py), shared with the CPU test that derives the
precision bars from them (tests/test_encoder_backward_cpu.py): nothing here touches a device.

Every number comes from the splitmix64 stream that tests/train_forward_oracle.py restates (``mix64``), vectorised over uint64 arrays whose
products wrap: no numpy generator, so the values do not depend on the numpy version.  Weights are xavier-uniform (``+-sqrt(6 / (fan_in +
fan_out))``), LayerNorm weights lie around 1 and biases around 0, inputs and upstream gradients are uniform in (-1.7, 1.7) (unit variance).

The ReLU is the layer's only kink, so a case keeps its mask unambiguous: the float32 split-bf16 stand-in's hidden pre-activations have the
signs of the float64 oracle's, and every oracle pre-activation is further from zero than ten times the worst stand-in deviation of any
pre-activation of the case.  :func:`layer_case` redraws the offending rows of ``x`` until that holds (at most ``MAX_SWEEPS`` sweeps; a
random row offends with probability about 20 %: the stand-in's deviation is 5e-5 of a pre-activation's spread, and a row has 512); no
element is ever left out of a comparison."""
import functools

import numpy as np

from onepose_st_amd import encoder_backward
from tests import encoder_backward_oracle as oracle

R, K = encoder_backward.ROW_TILE, encoder_backward.SPLIT_ROWS      # the row tile of the GEMMs and the row-split unit of the sums, from the header
C = encoder_backward.CHANNELS
GOLDEN, MAX_SWEEPS, MARGIN = 0x9E3779B97F4A7C15, 16, 10.0
# The bars of the device test: between two and four times the worst statistic (oracle.worst_error: max |y - y_ref| / max |y_ref| over a
# frame's dx / dsource and over each parameter tensor) of the float32 split-bf16 stand-in over LAYER_CASES, resp. through the six layers of
# chain_case().  Measured on the CPU by tests/test_encoder_backward_cpu.py::test_the_precision_bars, which holds these lines to what it
# measures; nothing comes from a device.
LAYER_BAR = 5.0e-5
CHAIN_BAR = 3.3e-2


def mix64(z):
    """train_forward_oracle.mix64 over a uint64 array (products and sums wrap modulo 2^64)"""
    z = (z ^ (z >> np.uint64(30))) * np.uint64(0xBF58476D1CE4E5B9)
    z = (z ^ (z >> np.uint64(27))) * np.uint64(0x94D049BB133111EB)
    return z ^ (z >> np.uint64(31))


class Stream:
    """draw k of seed s: mix64(s + GOLDEN * (k + 1)), its top 53 bits as a float64 in [0, 1)"""

    def __init__(self, seed):
        self.seed, self.at = np.uint64(seed), 0

    def uniform(self, shape, lo=-1.0, hi=1.0):
        n = int(np.prod(shape))
        k = np.arange(self.at + 1, self.at + n + 1, dtype=np.uint64)
        self.at += n
        with np.errstate(over="ignore"):
            z = mix64(self.seed + np.uint64(GOLDEN) * k)
        u = (z >> np.uint64(11)).astype(np.float64) * 2.0 ** -53
        return (lo + (hi - lo) * u).reshape(shape)


@functools.lru_cache(maxsize=None)
def weights(seed):
    """name -> float32 array of one layer's parameters"""
    draw, P = Stream(seed), {}
    for name, shape in oracle.PARAM_SHAPES.items():
        if len(shape) == 2:
            bound = (6.0 / (shape[0] + shape[1])) ** 0.5
            P[name] = draw.uniform(shape, -bound, bound).astype(np.float32)
        else:
            P[name] = (draw.uniform(shape, -0.2, 0.2) + (1.0 if name.endswith("weight") else 0.0)).astype(np.float32)
    return P


def relu_margin(x, source, P):
    """-> (the offending pre-activations ``[B, L, 512]``, the oracle's pre-activations, the worst stand-in deviation)"""
    want, got = oracle.layer_forward(x, source, P)["pre"], oracle.layer_forward(x, source, P, standin=True)["pre"]
    dev = float(np.abs(got - want).max())
    return (np.abs(want) <= MARGIN * dev) | ((got > 0) != (want > 0)), want, dev


@functools.lru_cache(maxsize=None)
def layer_case(seed, B, L, S, self_layer=False, zero_dy=False):
    """-> dict ``x [B, L, 256]``, ``source [B, S, 256]`` (``x`` itself in a self layer), ``dy`` float32, ``P`` the parameters, ``sweeps``.
    A cross layer redraws the offending rows of ``x``.  In a self layer ``x`` is the source too: a redrawn row moves every row's
    pre-activations, and with about one pre-activation in 2 500 inside the band a draw of 65 rows holds 13 offenders however often it is
    repeated.  There an offending row is moved instead, by the smallest step along its unit's ``mlp.0`` row that takes the pre-activation
    four bands out: a step of 1e-3 that moves the other rows' by 1e-5, so the sweeps converge."""
    assert not self_layer or L == S
    draw, P = Stream(seed), weights(7)
    x = draw.uniform((B, L, C), -1.7, 1.7).astype(np.float32)
    source = x if self_layer else draw.uniform((B, S, C), -1.7, 1.7).astype(np.float32)
    dy = (np.zeros((B, L, C)) if zero_dy else draw.uniform((B, L, C), -1.7, 1.7)).astype(np.float32)
    W0x = P["mlp.0.weight"][:, :C].astype(np.float64)
    for sweep in range(MAX_SWEEPS):
        bad, want, dev = relu_margin(x, source, P)
        if not bad.any():
            return {"x": x, "source": source, "dy": dy, "P": P, "sweeps": sweep}
        if not self_layer:
            rows = bad.any(-1)
            x[rows] = draw.uniform((int(rows.sum()), C), -1.7, 1.7).astype(np.float32)
            continue
        for b, i, j in np.argwhere(bad):
            target = (1.0 if want[b, i, j] >= 0 else -1.0) * 4 * MARGIN * dev
            x[b, i] = (x[b, i] + (target - want[b, i, j]) / (W0x[j] @ W0x[j]) * W0x[j]).astype(np.float32)
    raise AssertionError(f"layer_case{(seed, B, L, S, self_layer)}: the ReLU margin does not hold after {MAX_SWEEPS} sweeps")


# name -> arguments of layer_case.  Cross layers over every tile edge of the row GEMMs (R) against every split edge of the sums over the
# source (K), self layers at one row and one past a tile, each at B = 1 and 2; one call whose rows (2 100 > 16 * 128) make the split rule
# take its second branch (160 rows per split, 14 splits, the last of 20 rows).
LAYER_CASES = {f"cross_b{B}_l{L}_s{S}": dict(seed=10000 * B + 100 * L + S, B=B, L=L, S=S)
               for B in (1, 2) for L in (1, R - 1, R, R + 1, 2 * R + 1) for S in (1, K - 1, K, K + 1)}
LAYER_CASES.update({f"self_b{B}_l{L}": dict(seed=50000 + 1000 * B + L, B=B, L=L, S=L, self_layer=True) for B in (1, 2) for L in (1, R + 1)})
LAYER_CASES["many_splits"] = dict(seed=77, B=1, L=16 * K + 52, S=40)

CHAIN_NAMES = ["self", "cross"] * 3
CHAIN_HW, CHAIN_POINTS, CHAIN_SEED = (32, 40), 64, 3       # the device chain test's small scene (tests/test_gpu_loss_backward.py's)


def chain_inputs(seed, B, N, M):
    """-> (x3 [B, N, 256], x2 [B, M, 256], g3, g2) float32: seeded layer-0 inputs and upstream gradients"""
    draw = Stream(seed)
    return tuple(draw.uniform(s, -1.7, 1.7).astype(np.float32) for s in ((B, N, C), (B, M, C), (B, N, C), (B, M, C)))


@functools.lru_cache(maxsize=None)
def chain_scene():
    """The device chain test's scene, built without a device: the configuration, the synthetic state dict, the two frames, the six layers'
    parameters, and the coarse transformer's inputs ``x3 [2, 64, 256]`` / ``x2 [2, 20, 256]`` as the project's oracle forms them (keypoint
    encoder, position encoding).  The CPU test derives CHAIN_BAR from the stand-in on THESE inputs: over six layers and twelve calls a
    million pre-activations cannot all stay ten deviations from zero, and what a hidden unit at the kink does to a gradient belongs to
    the scene, so the bar has to be measured where the device is."""
    import torch
    from onepose_st_amd.config import default_config
    from onepose_st_amd.synthetic import make_synthetic_inputs, make_synthetic_state_dict
    from oracle import onepose_oracle as orc
    cfg = default_config()
    cfg["coarse_matching"]["border_rm"] = 0
    cfg["coarse_matching"]["train"].update(train_coarse_percent=0.3, train_pad_num_gt_min=4)
    cfg.update(hip_train_forward=True, hip_train_seed=CHAIN_SEED, hip_keep_features=True)
    sd = make_synthetic_state_dict(0, cfg)
    frames = [make_synthetic_inputs(sd, n_points=CHAIN_POINTS, image_hw=CHAIN_HW, n_plant=16, seed=11, config=cfg, frame=f) for f in range(2)]
    with torch.no_grad():
        x2 = orc.pe_add_flatten(torch.cat([f["feat_c"] for f in frames]), orc.position_table(256, tuple(cfg["positional_encoding"]["pos_emb_shape"])))
        d3 = orc.keypoint_encode(sd, orc.normalize_3d_keypoints(frames[0]["keypoints3d"]), frames[0]["descriptors3d_coarse_db"])
    x3 = d3.transpose(1, 2).expand(2, -1, -1).contiguous().numpy()
    params = [{n: sd[f"loftr_coarse.layers.{i}.{n}"].numpy() for n in oracle.PARAM_SHAPES} for i in range(len(CHAIN_NAMES))]
    return {"cfg": cfg, "sd": sd, "frames": frames, "params": params, "x3": x3, "x2": x2.numpy()}
