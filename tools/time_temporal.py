"""Time the temporal refinement's stages on the device (HIP events, hot rounds).

    python tools/time_temporal.py [--height 1080] [--width 1440] [--sources 5] [--queries 1000] [--levels 4] [--window 21] [--iters 20]

Frames are the analytic test texture under a small similarity per frame (``tests/temporal_oracle.py``), ``--sources`` + 1 of them; the
queries are random points with a 40 px margin.  Prints one JSON line:
  * ``pyramid_ms``: one ``temporal.build_pyramid`` call (the level-0 conversion and one launch per further level), its read-once /
    write-once bytes (the uint8 frame read, every level written once, every level but the last read once) and ``pyramid_GBps``;
  * ``track_ms``: one ``temporal.track`` launch of ``--queries`` points (forward and backward), ``track_lost``: rows it flagged lost;
  * ``frame_ms``: a refined frame whole -- the frame's pyramid, ``--sources`` track launches, one inject, one ``pnp_device.ransac_pnp``
    on own + carried rows -- without a read-back.
Every figure is the median of ``--iters`` timed rounds after two warm-up rounds.
"""
from __future__ import annotations

import argparse
import json
import os
import statistics
import sys

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

from onepose_st_amd import pnp_device, temporal  # noqa: E402
from tests import temporal_oracle as to  # noqa: E402


def event_ms(fn):
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    torch.cuda.synchronize()
    a.record()
    out = fn()
    b.record()
    b.synchronize()
    return a.elapsed_time(b), out


def median_ms(fn, iters):
    for _ in range(2):
        fn()
    return statistics.median(event_ms(fn)[0] for _ in range(iters))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--height", type=int, default=1080)
    ap.add_argument("--width", type=int, default=1440)
    ap.add_argument("--sources", type=int, default=5)
    ap.add_argument("--queries", type=int, default=1000)
    ap.add_argument("--levels", type=int, default=4)
    ap.add_argument("--window", type=int, default=21)
    ap.add_argument("--iters", type=int, default=20)
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("time_temporal.py needs the GPU: a time taken anywhere else says nothing")
    temporal.load()
    dev = torch.device("cuda:0")
    H, W, n = args.height, args.width, args.sources + 1
    tex = to.Texture(0)
    frames = []
    for t in range(n):                                                  # frame t: the texture moved by t * (1.2 px, -0.8 px) and 0.2 deg
        _, inv = to.similarity(0.2 * t, 1.0, (1.2 * t, -0.8 * t), centre=(W / 2, H / 2))
        frames.append(torch.from_numpy(tex.image(H, W, inv)).to(dev))
    g = np.random.default_rng(0)
    pts = torch.from_numpy(np.stack([g.uniform(40, W - 41, args.queries), g.uniform(40, H - 41, args.queries)], axis=1)).to(dev)
    pyrs = [temporal.build_pyramid(f, args.levels) for f in frames]
    shapes = to.level_shapes(H, W, args.levels)
    pyr_bytes = H * W + sum(4 * h * w for h, w in shapes) + sum(4 * h * w for h, w in shapes[:-1])
    out = {"frame": [H, W], "levels": args.levels, "window": args.window, "sources": args.sources, "queries": args.queries}
    ms = median_ms(lambda: temporal.build_pyramid(frames[-1], args.levels), args.iters)
    out.update(pyramid_ms=round(ms, 4), pyramid_bytes=pyr_bytes, pyramid_GBps=round(pyr_bytes / (ms * 1e-3) / 1e9, 1))
    kw = dict(window=args.window)
    ms = median_ms(lambda: temporal.track(pyrs[0], pyrs[-1], pts, **kw), args.iters)
    tr = temporal.track(pyrs[0], pyrs[-1], pts, **kw)
    out.update(track_ms=round(ms, 4), track_lost=int(((tr.flags & temporal.LOST) != 0).sum()), track_max_iterations=int(tr.iterations.max()))
    # a refined frame: own table of --queries rows and --sources carried tables of --queries rows each (random 3D points: the pose is
    # not the subject, the solver's time on a table of this size is)
    trans = torch.eye(3, dtype=torch.float64, device=dev)
    K = torch.tensor([[1500.0, 0, W / 2], [0, 1500.0, H / 2], [0, 0, 1]], dtype=torch.float64, device=dev)
    p3 = torch.from_numpy(g.normal(size=(args.queries, 3)).astype(np.float32)).to(dev)
    own2 = pts.float()
    count = torch.full((1,), args.queries, dtype=torch.int32, device=dev)
    queries = [temporal.Queries(pts, p3, count) for _ in range(args.sources)]

    def frame():
        pyr = temporal.build_pyramid(frames[-1], args.levels)
        sources = [(q, temporal.track(pyrs[s], pyr, q.pts, count=q.count, **kw)) for s, q in enumerate(queries)]
        p2, p3d, cnt = temporal.inject(own2, p3, count, sources, trans)
        return pnp_device.ransac_pnp(K, p2, p3d, count=cnt, scale=1000, pnp_reprojection_error=7)

    out.update(frame_ms=round(median_ms(frame, args.iters), 4))
    print(json.dumps(out), flush=True)


if __name__ == "__main__":
    main()
