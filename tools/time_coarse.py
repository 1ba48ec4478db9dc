"""Diagnostic: per-kernel times of the coarse-matching stage at c2 (planted encoder-boundary features).  Not part of the product."""
import os, sys, torch
sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), ".."))
from onepose_st_amd import hip, matchcall
hip.load(); dev = torch.device("cuda:0")
B, N, M, wc = 1, 7000, 4800, 80
g = torch.Generator().manual_seed(0)
f3 = torch.randn(B, N, 256, generator=g) * 2.5
f2 = torch.randn(B, M, 256, generator=g) * 2.5
perm = torch.randperm(M, generator=g)[:3000]
f2[0, perm] = f3[0, :3000] + 0.1 * torch.randn(3000, 256, generator=g)
f3, f2 = f3.to(dev), f2.to(dev)
kp = torch.randn(B, N, 3).to(dev)
ws = torch.empty(hip.load().ophip_coarse_workspace_floats(B, N, M), device=dev)
lists = matchcall.MatchLists.empty(B * N, dev, conf_shape=(B, N, M))
def run():
    matchcall.coarse_match(f3, f2, kp, wc=wc, temperature=0.08, thr=0.1, border_rm=2, scale=8.0, nsplit=3, lists=lists, conf=lists.conf, workspace=ws)
for _ in range(3): run()
torch.cuda.synchronize()
print("matches", int(lists.count[0]))
tot = 0.0
for name in ("frag_planes", "sim_stats", "stat_combine", "conf", "select"):
    hip.timing_select(name)
    for _ in range(20): run()
    torch.cuda.synchronize(); n, ms = hip.timing_read(); hip.timing_select("")
    if n:
        print(f"{name:14s} {ms / 20 * 1e3:7.1f} us per frame ({n // 20} launch(es))"); tot += ms / 20 * 1e3
print(f"sum            {tot:7.1f} us")
s = torch.cuda.Event(enable_timing=True); e = torch.cuda.Event(enable_timing=True)
s.record()
for _ in range(50): run()
e.record(); torch.cuda.synchronize()
print(f"stage wall     {s.elapsed_time(e) / 50 * 1e3:7.1f} us per frame")
