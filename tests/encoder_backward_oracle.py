"""The specification of the encoder layer's backward (include/ext/onepose_encoder_backward.h) restated in numpy
float64, one function per entry: the forward of one layer, its backward, and the six-layer chain as ``coarse_backward`` wires it.  The same
code is the float32 split-bf16 STAND-IN (``standin=True``): float32 throughout, and every matrix product the header lists takes both operands
through ``bf16_faithful.split`` and sums ``lo . hi + hi . lo + hi . hi`` -- exactly the header's operand points, nothing else.  The stand-in's
distance from the float64 oracle is what the device test's bar is derived from (tests/test_encoder_backward_cpu.py); nothing here touches a
device.

``faults``: the seeded faults of the CPU test, each a wrong backward somebody could write."""
import numpy as np
import torch

from tests import bf16_faithful

C, H, D, HID = 256, 8, 32, 512
EPS, LN_EPS = 1e-6, 1e-5
PARAM_SHAPES = {"q_proj.weight": (C, C), "k_proj.weight": (C, C), "v_proj.weight": (C, C), "merge.weight": (C, C), "mlp.0.weight": (HID, HID),
                "mlp.2.weight": (C, HID), "norm1.weight": (C,), "norm1.bias": (C,), "norm2.weight": (C,), "norm2.bias": (C,)}
MATRICES = tuple(n for n, s in PARAM_SHAPES.items() if len(s) == 2)


def flat_params(P):
    """name -> array in the header's buffer order, as one vector"""
    return np.concatenate([np.asarray(P[n]).reshape(-1) for n in PARAM_SHAPES])


class _Arith:
    """float64 with plain products, or the float32 stand-in with split operands"""

    def __init__(self, standin):
        self.standin, self.dt = standin, (np.float32 if standin else np.float64)

    def arr(self, a):
        return np.asarray(a, self.dt)

    def mm(self, a, b):
        """``a [.., r, k] @ b [.., k, n]``: the device's split-bf16 product in the stand-in"""
        if not self.standin:
            return a @ b
        (ah, al), (bh, bl) = (bf16_faithful.split(torch.from_numpy(np.ascontiguousarray(t, np.float32))) for t in (a, b))
        return (al @ bh + ah @ bl + ah @ bh).numpy()


def _phi(t):
    return np.where(t > 0, t + 1, np.exp(np.minimum(t, 0)))


def _heads(t):
    """[B, T, 256] -> [B, 8, T, 32]"""
    B, T, _ = t.shape
    return t.reshape(B, T, H, D).transpose(0, 2, 1, 3)


def _unheads(t):
    B, _, T, _ = t.shape
    return t.transpose(0, 2, 1, 3).reshape(B, T, C)


def _ln(z, w, b, dt):
    mean = z.mean(-1, keepdims=True, dtype=dt)
    var = ((z - mean) ** 2).mean(-1, keepdims=True, dtype=dt)
    rstd = (1 / np.sqrt(var + dt(LN_EPS))).astype(dt)
    zhat = (z - mean) * rstd
    return zhat * w + b, zhat, rstd


def _ln_backward(dn, zhat, rstd, w, dt, faults):
    g = dn * w
    if "ln_no_mean_terms" in faults:
        dz = rstd * g
    else:
        dz = rstd * (g - g.mean(-1, keepdims=True, dtype=dt) - zhat * (g * zhat).mean(-1, keepdims=True, dtype=dt))
    return dz, (dn * zhat).reshape(-1, C).sum(0, dtype=dt), dn.reshape(-1, C).sum(0, dtype=dt)


def layer_forward(x, source, P, standin=False):
    """-> dict of the forward's intermediates; ``y`` the layer's output, ``pre`` the hidden pre-activations ``hc W0^T``"""
    A = _Arith(standin)
    dt = A.dt
    x, source = A.arr(x), A.arr(source)
    W = {n: A.arr(P[n]) for n in PARAM_SHAPES}
    S = source.shape[1]
    Q = _phi(A.mm(x, W["q_proj.weight"].T)).astype(dt)
    Wkv = np.concatenate([W["k_proj.weight"], W["v_proj.weight"]])
    kv = A.mm(source, Wkv.T)
    K, vp = _phi(kv[..., :C]).astype(dt), (kv[..., C:] * dt(1.0 / S) if standin else kv[..., C:] / S).astype(dt)
    Qh, Kh, vh = _heads(Q), _heads(K), _heads(vp)
    KV = A.mm(Kh.transpose(0, 1, 3, 2), vh)                           # [B, 8, 32, 32]
    Ks = A.mm(Kh.transpose(0, 1, 3, 2), np.ones((S, 1), dt))[..., 0]  # [B, 8, 32]
    den = np.einsum("bhld,bhd->bhl", Qh, Ks).astype(dt) + dt(EPS)
    Z = (1 / den).astype(dt)
    num = np.einsum("bhld,bhdv->bhlv", Qh, KV).astype(dt)
    m = _unheads(num * (Z * dt(S))[..., None]).astype(dt)
    msg = A.mm(m, W["merge.weight"].T)
    n1, zhat1, rstd1 = _ln(msg, W["norm1.weight"], W["norm1.bias"], dt)
    hc = np.concatenate([x, n1], -1).astype(dt)
    pre = A.mm(hc, W["mlp.0.weight"].T)
    h = np.maximum(pre, 0)
    o = A.mm(h, W["mlp.2.weight"].T)
    n2, zhat2, rstd2 = _ln(o, W["norm2.weight"], W["norm2.bias"], dt)
    return dict(A=A, W=W, Wkv=Wkv, S=S, x=x, source=source, Q=Q, K=K, vp=vp, Qh=Qh, Kh=Kh, vh=vh, KV=KV, Ks=Ks, Z=Z, m=m, zhat1=zhat1, rstd1=rstd1,
                hc=hc, pre=pre, h=h, zhat2=zhat2, rstd2=rstd2, y=(x + n2).astype(dt))


def layer_grads(x, source, dy, P, standin=False, faults=()):
    """One ``openb_layer_grads`` call -> dict ``dx``, ``dsource``, ``dparams`` (name -> array), ``y`` and ``pre``"""
    f = layer_forward(x, source, P, standin)
    A, W, S = f["A"], f["W"], f["S"]
    dt = A.dt
    dy = A.arr(dy)
    rows = lambda t: t.reshape(-1, t.shape[-1])                       # noqa: E731
    do, dg2, db2 = _ln_backward(dy, f["zhat2"], f["rstd2"], W["norm2.weight"], dt, faults)
    dW2 = A.mm(rows(do).T, rows(f["h"]))
    dh = A.mm(do, W["mlp.2.weight"])
    if "relu_mask_ignored" not in faults:
        dh = dh * (f["h"] > 0)
    dW0 = A.mm(rows(dh).T, rows(f["hc"]))
    dhc = A.mm(dh, W["mlp.0.weight"])
    dmsg, dg1, db1 = _ln_backward(dhc[..., C:], f["zhat1"], f["rstd1"], W["norm1.weight"], dt, faults)
    dWm = A.mm(rows(dmsg).T, rows(f["m"]))
    dm = A.mm(dmsg, W["merge.weight"])
    dmh, mh, Z = _heads(dm), _heads(f["m"]), f["Z"]
    dden = (-Z * (dmh * mh).sum(-1, dtype=dt)).astype(dt)             # [B, 8, L]
    dnum = (dmh * (Z * dt(S))[..., None]).astype(dt)
    dQ = np.einsum("bhdv,bhlv->bhld", f["KV"], dnum).astype(dt) + dden[..., None] * f["Ks"][:, :, None, :]
    dKV = A.mm(f["Qh"].transpose(0, 1, 3, 2), dnum)
    dKs = A.mm(f["Qh"].transpose(0, 1, 3, 2), dden[..., None])[..., 0]
    dK = np.einsum("bhdv,bhsv->bhsd", dKV, f["vh"]).astype(dt)
    if "dks_dropped" not in faults:
        dK = dK + dKs[:, :, None, :]
    dv = np.einsum("bhsd,bhdv->bhsv", f["Kh"], dKV).astype(dt)
    if "dv_not_divided" not in faults:
        dv = dv / dt(S)
    dq = _unheads(dQ) * np.minimum(f["Q"], 1)
    dk = _unheads(dK) * np.minimum(f["K"], 1)
    dkv = np.concatenate([dk, _unheads(dv)], -1).astype(dt)
    dWq = A.mm(rows(dq).T, rows(f["x"]))
    dWkv = A.mm(rows(dkv).T, rows(f["source"]))
    dx = A.mm(dq, W["q_proj.weight"])
    if "residual_dropped" not in faults:
        dx = dx + dy
    if "dhc_x_dropped" not in faults:
        dx = dx + dhc[..., :C]
    if "dk_wk_dropped" in faults:
        dsource = A.mm(_unheads(dv), W["v_proj.weight"])
    else:
        dsource = A.mm(dkv, f["Wkv"])
    dparams = {"q_proj.weight": dWq, "k_proj.weight": dWkv[:C], "v_proj.weight": dWkv[C:], "merge.weight": dWm, "mlp.0.weight": dW0,
               "mlp.2.weight": dW2, "norm1.weight": dg1, "norm1.bias": db1, "norm2.weight": dg2, "norm2.bias": db2}
    assert all(v.dtype == dt for v in (dx, dsource, *dparams.values()))
    return {"dx": dx, "dsource": dsource, "dparams": dparams, "y": f["y"], "pre": f["pre"]}


def chain_forward(layer_names, params, x3, x2, standin=False):
    """The coarse transformer (oracle.onepose_oracle.feature_transformer's wiring) -> (the kept ``[(x3, x2)]`` per layer, the outputs)"""
    kept = []
    for name, P in zip(layer_names, params):
        kept.append((x3, x2))
        s3, s2 = (x3, x2) if name == "self" else (x2, x3)
        x2, x3 = layer_forward(x2, s2, P, standin)["y"], layer_forward(x3, s3, P, standin)["y"]
    return kept, (x3, x2)


def chain_grads(layer_names, params, kept, g3, g2, standin=False):
    """``coarse_backward``: from the gradients at the outputs over the kept layer inputs -> (grad at x3, grad at x2, [dparams per layer]).
    The second call of a layer accumulates (in the stand-in: one float32 addition per element)."""
    out = [None] * len(layer_names)
    for i in reversed(range(len(layer_names))):
        x3, x2 = kept[i]
        s3, s2 = (x3, x2) if layer_names[i] == "self" else (x2, x3)
        a = layer_grads(x2, s2, g2, params[i], standin)               # the 2D stream first, as coarse_backward calls it
        b = layer_grads(x3, s3, g3, params[i], standin)
        if layer_names[i] == "self":
            g2, g3 = a["dx"] + a["dsource"], b["dx"] + b["dsource"]
        else:
            g2, g3 = a["dx"] + b["dsource"], b["dx"] + a["dsource"]
        out[i] = {n: a["dparams"][n] + b["dparams"][n] for n in PARAM_SHAPES}
    return g3, g2, out


def frame_error(got, want):
    """The statistic of the bar: ``max |y - y_ref| / max |y_ref|`` over a frame's tensor, worst frame (``dx`` / ``dsource``)"""
    got, want = np.asarray(got, np.float64), np.asarray(want, np.float64)
    return max(tensor_error(got[b], want[b]) for b in range(want.shape[0]))


def tensor_error(got, want):
    """The same over one tensor (a parameter's gradient); an all-zero reference must be met exactly"""
    got, want = np.asarray(got, np.float64), np.asarray(want, np.float64)
    top, err = np.abs(want).max(), np.abs(got - want).max()
    return float((0.0 if err == 0 else np.inf) if top == 0 else err / top)


def call_errors(got, want):
    """name -> statistic of one call (``got`` / ``want`` as :func:`layer_grads` returns them): ``dx`` and ``dsource`` per frame, every
    parameter tensor against its own largest reference value.  One exception, by the layer's arithmetic: with S = 1 the attention returns
    ``m = v (1 - eps / den)`` whatever Q and K are, so the true dWq and dWk are 1e-8 of dWv and ANY float32 result is the rounding of
    terms that cancel; there these two are measured against dWv's largest reference value, the scale of the terms."""
    errs = {"dx": frame_error(got["dx"], want["dx"]), "dsource": frame_error(got["dsource"], want["dsource"])}
    for n in PARAM_SHAPES:
        g, w = np.asarray(got["dparams"][n], np.float64), np.asarray(want["dparams"][n], np.float64)
        if want["dsource"].shape[1] == 1 and n in ("q_proj.weight", "k_proj.weight"):
            errs[n] = float(np.abs(g - w).max() / np.abs(want["dparams"]["v_proj.weight"]).max())
        else:
            errs[n] = tensor_error(g, w)
    return errs


def worst_error(got, want):
    """The worst statistic of one call -> (value, where)"""
    errs = call_errors(got, want)
    where = max(errs, key=errs.get)
    return errs[where], where
