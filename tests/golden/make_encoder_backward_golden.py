"""Generate ``encoder_backward_small.npz`` FROM THE REFERENCE ITSELF.

Run in the build container only (needs the reference checkout beside the repository; the GPU box never sees it):

    python tests/golden/make_encoder_backward_golden.py

The reference's own ``LoFTREncoderLayer(256, 8, dropout=0.0).double()`` (``src/models/OnePosePlus/loftr_module/transformer.py``, imported by
file path with its package's ``linear_attention``) under float64 autograd, on two seeded cases of tests/encoder_backward_cases.py: a cross
call (B = 2, L = 19, S = 23) and a self call (B = 1, L = S = 13).  The weights are NOT stored: they are ``cases.weights(7)``, and the fixture
keeps per tensor their float64 sum and sum of squares, so a drifted generator is a clear error.  Stored per case: ``x``, ``source`` (the cross case; in the self case it is ``x``), ``dy``
(float32), ``y``, ``dx``, ``dsource`` and the four LayerNorm gradients (float64), and of each of the six weight-matrix gradients two sketches
``dW @ V`` and ``U^T @ dW`` with seeded ``U``, ``V`` of four columns (a full float64 set is 5 MB).  Only data is stored."""
from __future__ import annotations

import importlib.util
import os
import sys
import types

import numpy as np
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
REPO = os.path.abspath(os.path.join(HERE, "..", ".."))
REF = os.environ.get("ONEPOSE_REFERENCE", "/root/reference")
GOLDEN_CASES = {"cross": dict(seed=901, B=2, L=19, S=23), "self": dict(seed=902, B=1, L=13, S=13, self_layer=True)}
SKETCH_SEED, SKETCH_COLUMNS = 903, 4


def sketches(shape):
    """-> (U [out, 4], V [in, 4]) float64, seeded, of a matrix gradient of ``shape``"""
    from tests import encoder_backward_cases as cases
    draw = cases.Stream(SKETCH_SEED + shape[0] + 3 * shape[1])
    return draw.uniform((shape[0], SKETCH_COLUMNS)), draw.uniform((shape[1], SKETCH_COLUMNS))


def weight_sums(P):
    """name -> (sum, sum of squares) in float64"""
    return {n: np.array([np.sum(P[n], dtype=np.float64), np.sum(np.square(P[n], dtype=np.float64))]) for n in P}


def _reference_layer():
    pkg = "ref_loftr_module"
    root = os.path.join(REF, "src", "models", "OnePosePlus", "loftr_module")
    sys.modules[pkg] = types.ModuleType(pkg)
    sys.modules[pkg].__path__ = [root]
    for name in ("linear_attention", "transformer"):
        spec = importlib.util.spec_from_file_location(f"{pkg}.{name}", os.path.join(root, name + ".py"))
        mod = importlib.util.module_from_spec(spec)
        sys.modules[f"{pkg}.{name}"] = mod
        spec.loader.exec_module(mod)
    return sys.modules[f"{pkg}.transformer"].LoFTREncoderLayer


def main():
    from tests import encoder_backward_cases as cases
    from tests import encoder_backward_oracle as oracle
    layer = _reference_layer()(256, 8, dropout=0.0).double()
    P = cases.weights(7)
    layer.load_state_dict({n: torch.tensor(P[n], dtype=torch.float64) for n in P}, strict=True)
    out = {f"weights/{n}": v for n, v in weight_sums(P).items()}
    for tag, args in GOLDEN_CASES.items():
        case = cases.layer_case(**args)
        x = torch.tensor(case["x"], dtype=torch.float64, requires_grad=True)
        # the self case: a second leaf at the same values, so that the reference splits its own gradient into dx and dsource
        source = torch.tensor(case["source"], dtype=torch.float64, requires_grad=True)
        layer.zero_grad()
        y = layer(x, source)
        y.backward(torch.tensor(case["dy"], dtype=torch.float64))
        out.update({f"{tag}/x": case["x"], f"{tag}/dy": case["dy"], f"{tag}/y": y.detach().numpy(), f"{tag}/dx": x.grad.numpy(),
                    f"{tag}/dsource": source.grad.numpy()})
        if not args.get("self_layer"):                              # (in the self case source IS x: not stored twice)
            out[f"{tag}/source"] = case["source"]
        for name, p in layer.named_parameters():
            g = p.grad.numpy()
            if name in oracle.MATRICES:
                U, V = sketches(g.shape)
                out.update({f"{tag}/{name}/right": g @ V, f"{tag}/{name}/left": U.T @ g})
            else:
                out[f"{tag}/{name}"] = g.copy()
    path = os.path.join(HERE, "encoder_backward_small.npz")
    np.savez_compressed(path, **out)
    print(f"wrote {path}: {os.path.getsize(path)} bytes, {len(out)} arrays")


if __name__ == "__main__":                                  # tests/test_encoder_backward_cpu.py imports the helpers: no side effect on import
    sys.dont_write_bytecode = True
    sys.path.insert(0, REPO)
    main()
