"""Diagnostic: HIP-event time of one kernel family of the coarse-matching stage at c2 (ophip_timing_select)."""
import sys, os, torch
sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), ".."))
from onepose_st_amd import hip, matchcall
dev = torch.device("cuda:0"); hip.load()
N, M, wc = 7000, 4800, 80
g = torch.Generator().manual_seed(0)
f3, f2 = torch.randn(1, N, 256, generator=g).to(dev), torch.randn(1, M, 256, generator=g).to(dev)
kp = torch.zeros(1, N, 3, device=dev)
ws = torch.empty(hip.load().ophip_coarse_workspace_floats(1, N, M), device=dev)
lists = matchcall.MatchLists.empty(N, dev, conf_shape=(1, N, M))
def run():
    matchcall.coarse_match(f3, f2, kp, wc=wc, temperature=0.08, thr=0.1, border_rm=2, scale=8.0, nsplit=3, lists=lists, conf=lists.conf, workspace=ws)
for _ in range(3): run()
for name in sys.argv[1:] or ["sim_stats", "stat_combine", "conf", "select"]:
    torch.cuda.synchronize(); hip.timing_select(name)
    for _ in range(20): run()
    torch.cuda.synchronize(); n, ms = hip.timing_read(); hip.timing_select("")
    print(f"{name:14s} {ms / max(n, 1) * 1e3:8.1f} us  ({n} launches)")
