"""Diagnostic: the coarse transformer's backward at working sizes.  HIP events around every step, 5 hot steps, the
median of 20 and its quartile range.  One layer call (the 3D rows updated from the 2D rows) and the whole six-layer ``coarse_backward`` at c2
with B = 4 (N = 7 000, M = 4 800) and at c4 with B = 1 (N = 15 000, M = 4 800), each as ms and as achieved FLOP/s from the algorithmic count
(per row of x 540 672 multiply-adds forward, per row of source 139 264; the backward twice that; the library recomputes the forward, so a
call is three times the forward), beside float32 torch autograd of the reference's layer as the project's oracle restates it
(oracle.onepose_oracle.encoder_layer / feature_transformer) on the same device tensors: forward plus backward (the same work) and backward
alone, and ``torch.cuda.max_memory_allocated`` of both.  ``--kernels``: the library's per-kernel times of one c2 layer call (torch.profiler).
Not part of the product."""
import os
import statistics
import sys
import types

import torch

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), ".."))
from onepose_st_amd import encoder_backward as eb  # noqa: E402
from onepose_st_amd.params import EncoderParams  # noqa: E402
from oracle import onepose_oracle as orc  # noqa: E402

eb.load()
dev = torch.device("cuda:0")
HOT, STEPS = 5, 20
NAMES = ["self", "cross"] * 3


def timed(step):
    """-> (median ms, quartile range ms) of STEPS runs after HOT"""
    for _ in range(HOT):
        step()
    times = []
    for _ in range(STEPS):
        s, e = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        s.record()
        step()
        e.record()
        torch.cuda.synchronize()
        times.append(s.elapsed_time(e))
    q = statistics.quantiles(times, n=4)
    return statistics.median(times), q[2] - q[0]


def peak_mb(step):
    torch.cuda.synchronize()
    torch.cuda.empty_cache()
    base = torch.cuda.memory_allocated()
    torch.cuda.reset_peak_memory_stats()
    keep = step()
    torch.cuda.synchronize()
    peak = (torch.cuda.max_memory_allocated() - base) / 1e6
    del keep
    return peak


def call_flop(rows_x, rows_s):
    return 6.0 * (rows_x * 540672.0 + rows_s * 139264.0)


def torch_backward_alone(forward, grads):
    """-> a step that times the backward of a graph built outside the timed region: (median, quartile range)"""
    for _ in range(HOT):
        torch.autograd.backward(forward(), grads)
    times = []
    for _ in range(STEPS):
        outs = forward()
        s, e = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        s.record()
        torch.autograd.backward(outs, grads)
        e.record()
        torch.cuda.synchronize()
        times.append(s.elapsed_time(e))
    q = statistics.quantiles(times, n=4)
    return statistics.median(times), q[2] - q[0]


def report(name, what, flop, ours, theirs, theirs_bwd, mb, mb_t):
    (ms, iqr), (ms_t, iqr_t), (ms_b, iqr_b) = ours, theirs, theirs_bwd
    print(f"{name} {what}: library          {ms:9.3f} ms (quartile range {iqr:.3f})  {flop / ms / 1e9:7.1f} TFLOP/s algorithmic ({flop / 1e12:.2f} TFLOP)  "
          f"peak {mb:9.1f} MB")
    print(f"{name} {what}: torch fwd + bwd  {ms_t:9.3f} ms (quartile range {iqr_t:.3f})  {flop / ms_t / 1e9:7.1f} TFLOP/s  peak {mb_t:9.1f} MB  "
          f"({ms_t / ms:.2f} x the library)")
    print(f"{name} {what}: torch bwd alone  {ms_b:9.3f} ms (quartile range {iqr_b:.3f})  ({ms_b / ms:.2f} x the library)")
    verdict = "faster" if ms_t - ms > iqr + iqr_t else "NOT faster"
    print(f"{name} {what}: the library is {verdict} than torch's forward plus backward by more than the two quartile ranges together")


def main():
    g = torch.Generator(device=dev).manual_seed(0)
    enc = EncoderParams(NAMES, 256, 8).to(dev)
    for layer in enc.layers:                                     # LayerNorm parameters away from (1, 0), like a trained model's
        for norm in (layer.norm1, layer.norm2):
            norm.weight.data.add_(0.1 * torch.randn(256, device=dev, generator=g))
            norm.bias.data.add_(0.1 * torch.randn(256, device=dev, generator=g))
    model = types.SimpleNamespace(loftr_coarse=enc)
    sd = {"loftr_coarse." + k: v for k, v in enc.state_dict().items()}
    leaves = [v.requires_grad_() for v in sd.values()]
    for name, (B, N, M) in (("c2 x 4", (4, 7000, 4800)), ("c4 x 1", (1, 15000, 4800))):
        x3, x2 = torch.randn(B, N, 256, device=dev, generator=g), torch.randn(B, M, 256, device=dev, generator=g)
        g3, g2 = torch.randn(B, N, 256, device=dev, generator=g), torch.randn(B, M, 256, device=dev, generator=g)
        # ---- one layer call: the 3D rows from the 2D rows --------------------------------------------------------------------------------
        params = eb.pack_params(enc.layers[1])
        workspace = torch.empty(eb.workspace_bytes(B, N, M), dtype=torch.uint8, device=dev)
        out, dparams = (torch.empty_like(x3), torch.empty_like(x2)), torch.empty(eb.PARAM_FLOATS, device=dev)
        step = lambda: eb.layer_backward(x3, x2, g3, params, dparams=dparams, workspace=workspace, out=out)
        a3, a2 = x3.clone().requires_grad_(), x2.clone().requires_grad_()
        fwd = lambda: orc.encoder_layer(sd, "loftr_coarse.layers.1.", a3, a2, 8)

        def ref():
            for t in (a3, a2, *leaves):
                t.grad = None
            fwd().backward(g3)
            return a3.grad
        ours, theirs, theirs_bwd = timed(step), timed(ref), torch_backward_alone(fwd, g3)
        mb = peak_mb(lambda: eb.layer_backward(x3, x2, g3, params))
        report(name, "one layer call ", call_flop(B * N, B * M), ours, theirs, theirs_bwd, mb, peak_mb(ref))
        ref()
        print(f"{name} one layer call : max |dx - torch| / max |torch| {float((out[0] - a3.grad).abs().max() / a3.grad.abs().max()):.1e}, dsource "
              f"{float((out[1] - a2.grad).abs().max() / a2.grad.abs().max()):.1e}")
        if "--kernels" in sys.argv and B == 4:
            try:
                from torch.profiler import ProfilerActivity, profile
                with profile(activities=[ProfilerActivity.CUDA]) as prof:
                    step()
                    torch.cuda.synchronize()
                print(prof.key_averages().table(sort_by="cuda_time_total", row_limit=16, max_name_column_width=60))
            except Exception as err:                             # a diagnostic of a diagnostic
                print(f"per-kernel times: not available ({err})")
        del workspace, out
        # ---- the six layers ----------------------------------------------------------------------------------------------------------------
        data = {"grad_feat_c0": g3, "grad_feat_c1": g2, "layer_inputs_c": [(x3, x2)] * 6}
        chain = lambda: eb.coarse_backward(data, model)
        chain_fwd = lambda: orc.feature_transformer(sd, "loftr_coarse", NAMES, 8, a3.transpose(1, 2), a2)

        def chain_ref():
            for t in (a3, a2, *leaves):
                t.grad = None
            torch.autograd.backward(chain_fwd(), (g3, g2))
            return a3.grad
        flop = 3 * (call_flop(B * N, B * N) + call_flop(B * M, B * M) + call_flop(B * N, B * M) + call_flop(B * M, B * N))
        ours, theirs, theirs_bwd = timed(chain), timed(chain_ref), torch_backward_alone(chain_fwd, (g3, g2))
        report(name, "coarse_backward", flop, ours, theirs, theirs_bwd, peak_mb(chain), peak_mb(chain_ref))
        del x3, x2, g3, g2, a3, a2, data
        torch.cuda.empty_cache()


if __name__ == "__main__":
    main()
