"""Host cost of a launch of the local-search entry points: wall us per call of rls_maxcut_local_search, _ls_threshold, _ls_propose and
_ls_rounds (4 draws) through torch.ops.rlsolver_hip.* on a launch-bound shape (N = 800, E = 4694, 64 envs), back-to-back calls, one
sync at the end -- what a change to the launchers' host side (csrc/rls_ls_plan.h) is measured with, build against build.

    python tools/timing/ls_launch_host.py [tag] [repeats] [entries, comma-separated: fused,threshold,propose,rounds4]"""
import os
import sys
import time

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__)))))
import torch  # noqa: E402
from rlsolver_amd import graph, ops  # noqa: E402

tag = sys.argv[1] if len(sys.argv) > 1 else ""
reps = int(sys.argv[2]) if len(sys.argv) > 2 else 5
dev = torch.device("cuda:0")


def host_us(fn, n=4000):
    for _ in range(200):
        fn()
    torch.cuda.synchronize()
    t = time.perf_counter()
    for _ in range(n):
        fn()
    dt = time.perf_counter() - t
    torch.cuda.synchronize()
    return dt / n * 1e6


N, B, SPIN, SEED = 800, 64, 5, 11
dg = ops.DeviceGraph(graph.build_csr(graph.generate_gnm(N, 4694, seed=1), num_nodes=N, if_bidirectional=False), dev)
xs = ops.rand_spins(B, N, 1, dev)
obj = ops.maxcut_obj(dg, xs)
ws, ws_std = ops.maxcut_ls_weights(dg, xs, 2, dtype=torch.int8, padded=True)
rd_std = ws_std.to(torch.float32) * 0.3
thresh = ops.maxcut_ls_threshold(dg, ws, rd_std, SEED, SPIN)
scratch = ops.ls_scratch(dg, B, ws, 4)
t = torch.ops.rlsolver_hip      # the ops themselves: no Python wrapper, no allocation in the timed loop
calls = (("fused", lambda: t.maxcut_local_search(dg.handle, xs, ws, rd_std, None, SEED, 0, 8, SPIN, False, obj, False)),
         ("threshold", lambda: t.maxcut_ls_threshold(dg.handle, ws, rd_std, SEED, 0, 0, SPIN, thresh, scratch)),
         ("propose", lambda: t.maxcut_ls_propose(dg.handle, xs, ws, rd_std, thresh, SEED, 0, 1, obj, scratch)),
         ("rounds4", lambda: t.maxcut_ls_rounds(dg.handle, xs, ws, rd_std, thresh, SEED, 0, 1, 4, obj, scratch)))
if len(sys.argv) > 3:
    calls = tuple(c for c in calls if c[0] in sys.argv[3].split(","))
for rep in range(reps):
    print(f"HOST {tag} rep {rep}: " + " ".join(f"{n} {host_us(f):.2f}" for n, f in calls), flush=True)
