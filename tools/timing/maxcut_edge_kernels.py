"""The edge-flip MaxCut gauge + sweep + score kernel (rls_maxcut_edge_local_search), one sweep (num_ls = 1, the kernel's own draws),
at two sizes -- G(2000, 19 990) x 2^16 chains and Barabasi-Albert(10^4, m = 5) x 2^16 chains -- with, for scale, the weighted node
sampler (rls_mcpg_local_search, the same graph and chains) and the score-only launch (num_ls = 0).  HIP events, median of 5 groups
of launches.  A pass reads sum_v deg(v)^2 - 2 E neighbour bits per chain; the line prints that count and the time per read.
`python tools/timing/maxcut_edge_kernels.py [quick]`."""
import os, sys
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__)))))
import numpy as np, torch
from rlsolver_amd import ops_mcpg_tsp as mops
from rlsolver_amd.graph import generate_gnm
from rlsolver_amd.methods import MCPG_maxcut_edge as me
from rlsolver_amd.ops_mcpg_tsp import PackedChains
dev = torch.device("cuda:0")


def t(f, reps):
    f(); torch.cuda.synchronize()
    s = torch.cuda.Event(enable_timing=True); e = torch.cuda.Event(enable_timing=True)
    s.record()
    for _ in range(reps): f()
    e.record(); torch.cuda.synchronize()
    return s.elapsed_time(e) / reps


def ba_edges(n, m, seed):
    rng = np.random.RandomState(seed)
    eu, ev, ends = [], [], list(range(m))
    for v in range(m, n):
        for u in set(rng.choice(ends, m).tolist()):
            eu.append(u), ev.append(v), ends.extend((u, v))
    return np.asarray(eu), np.asarray(ev)


quick = "quick" in sys.argv[1:]
g = np.asarray(generate_gnm(2000, 19990, 5), dtype=np.int64)
C = 1 << (12 if quick else 16)
for name, n, (eu, ev) in (("G(2000, 19990)", 2000, (g[:, 0], g[:, 1])), ("BA(10^4, 5)", 10000, ba_edges(10000, 5, 1))):
    data = me.make_data(n, eu, ev, np.ones(eu.shape[0], np.int64), dev)
    torch.manual_seed(0)
    xf = (torch.rand((n, C), device=dev) < 0.5).float()
    x = PackedChains.pack(xf)
    out = PackedChains.empty(n, C, dev)
    reps = 1 if quick else 3
    ker = [t(lambda: data.local_search(x, 1, None, 7, out=out), reps) for _ in range(5)]
    score = [t(lambda: data.local_search(x, 0, None, 7, out=out), reps) for _ in range(5)]
    try:
        node = "%.3f ms" % np.median([t(lambda: mops.mcpg_local_search(data.graph, xf, data._order_i32, 1, None, 7, visit_stream=data._visit_stream,
                                                                        edge_weights=data._edge_w, gauge_node=data.hub()), reps) for _ in range(5)])
    except RuntimeError:                                     # its batched stream takes rows of up to 253 neighbours
        node = "not covered (a row longer than 253)"
    reads = (data.stream().numel() - 7 * eu.shape[0]) // 2
    k = float(np.median(ker))
    print(f"{name} E={eu.shape[0]} C={C}: edge sweep {k:9.3f} ms (min {min(ker):.3f}, max {max(ker):.3f}; score alone {np.median(score):.3f}); "
          f"{reads} neighbour reads per chain and pass = {k * 1e6 / (reads * C) * 1e3:.2f} ps per (chain, read); weighted node sampler "
          f"{node}", flush=True)
