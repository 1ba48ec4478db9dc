"""Time the detector's matcher calls: the view-by-view loop against the batched call in its lazy and its eager form.

    python tools/time_detector.py [--views 15] [--view-size 512 512] [--queries 480x640 1440x1920] [--iters 5] [--warmup 2]
                                  [--budget-gib 4]

``--views`` reference views of ``--view-size`` against one query frame of each of ``--queries``, through
``LocalFeatureObjectDetector.match_worker`` with the LoFTR matcher on seeded random weights and random images.  Random weights give
(almost) no matches, so the numbers are the backbone, the coarse transformer and the coarse matching; the fine stage and the host votes
are next to nothing here (``matches`` says how many there were) and cost the same in every form on real data.  Hot steps only: every
timed call is preceded by ``--warmup`` untimed ones, and the three forms alternate call by call inside one loop.  HIP events around each
call (a call ends with the read-back of its matches, so the host clock would say the same).  One JSON line per query size:

  * ``loop_ms``: ``match_worker(query, batched=False)``, one matcher call and one read-back per view (eager, as the loop always was);
  * ``batched_lazy_ms``: ``match_worker(query)``: chunks of views under ``--budget-gib``, ``conf_matrix="lazy"``;
  * ``batched_eager_ms``: the same chunks by the eager estimate, ``conf_matrix`` stored;
  * ``*_calls``: matcher calls per detection; ``*_peak_bytes``: ``torch.cuda.max_memory_allocated`` over one detection of that form;
  * ``agree``: whether the three forms voted the same boxes.
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

from onepose_st_amd import detector, hip, loftr  # noqa: E402
from onepose_st_amd.synthetic import make_synthetic_loftr_state_dict  # noqa: E402


def stats(ts):
    return {"median": round(statistics.median(ts), 3), "min": round(min(ts), 3), "max": round(max(ts), 3)}


def event_ms(fn):
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    res = fn()
    b.record()
    b.synchronize()
    return res, a.elapsed_time(b)


class Counted:
    """the matcher as the detector sees it, counting calls and matches; ``eager``: the batched call stores conf_matrix (the request for
    the lazy form is dropped and the chunks are planned by the eager estimate)"""

    def __init__(self, matcher, eager=False):
        self.matcher, self.eager, self.config = matcher, eager, matcher.config
        self.calls = self.matches = 0

    def parameters(self):
        return self.matcher.parameters()

    def coarse_batch_bytes(self, V, hw0_c, hw1_c, lazy):
        return self.matcher.coarse_batch_bytes(V, hw0_c, hw1_c, lazy and not self.eager)

    def __call__(self, data, **kw):
        if self.eager:
            kw = {}
        self.calls += 1
        self.matcher(data, **kw)
        self.matches += int(data["b_ids"].shape[0])


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--views", type=int, default=15)
    ap.add_argument("--view-size", type=int, nargs=2, default=(512, 512))
    ap.add_argument("--queries", nargs="+", default=["480x640", "1440x1920"])
    ap.add_argument("--iters", type=int, default=5)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--budget-gib", type=float, default=4.0)
    a = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("time_detector.py measures on the GPU: none found")
    dev = torch.device("cuda:0")
    m = loftr.LoFTR_for_OnePose_Plus().eval()
    m.load_state_dict(make_synthetic_loftr_state_dict(0), strict=True)
    m = m.to(dev)
    g = np.random.default_rng(1)
    views = [g.integers(0, 256, size=tuple(a.view_size), dtype=np.uint8) for _ in range(a.views)]
    budget = int(a.budget_gib * (1 << 30))
    for q in a.queries:
        H, W = (int(v) for v in q.lower().split("x"))
        query = torch.as_tensor(g.random((1, 1, H, W), dtype=np.float32)).to(dev)
        forms = {"loop": (Counted(m), False), "batched_lazy": (Counted(m), True), "batched_eager": (Counted(m, eager=True), True)}
        dets = {k: detector.LocalFeatureObjectDetector(cm, views, batch_budget_bytes=budget) for k, (cm, _) in forms.items()}
        ms = {k: [] for k in forms}
        peak, calls, matches, votes = {}, {}, {}, {}
        for it in range(a.warmup + a.iters):
            for k, (cm, batched) in forms.items():
                cm.calls = cm.matches = 0
                torch.cuda.synchronize()
                torch.cuda.reset_peak_memory_stats()
                votes[k], t = event_ms(lambda: dets[k].match_worker(query, batched=batched))
                torch.cuda.synchronize()
                peak[k], calls[k], matches[k] = torch.cuda.max_memory_allocated(), cm.calls, cm.matches
                if it >= a.warmup:
                    ms[k].append(t)
        same = all(np.array_equal(votes[k][v]["bbox"], votes["loop"][v]["bbox"]) for k in forms for v in range(a.views))
        hw0_c, hw1_c = (a.view_size[0] // 8, a.view_size[1] // 8), (H // 8, W // 8)
        out = {"views": a.views, "view_size": list(a.view_size), "query": [H, W], "budget_bytes": budget, "device": torch.cuda.get_device_name(0),
               "library": hip.build_stamp(), "iters": a.iters, "warmup": a.warmup,
               "estimate_bytes": {"lazy_all_views": m.coarse_batch_bytes(a.views, hw0_c, hw1_c, True),
                                  "eager_all_views": m.coarse_batch_bytes(a.views, hw0_c, hw1_c, False)},
               "agree": bool(same)}
        for k in forms:
            out[f"{k}_ms"], out[f"{k}_calls"], out[f"{k}_peak_bytes"], out[f"{k}_matches"] = stats(ms[k]), calls[k], peak[k], matches[k]
        print(json.dumps(out), flush=True)


if __name__ == "__main__":
    main()
