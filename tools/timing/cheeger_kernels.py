"""The Cheeger-cut sweep + score kernel (rls_cheeger_local_search), one sweep (num_ls = 1), both cuts, at two sizes -- G(2000,
19 990) x 2^16 chains and Barabasi-Albert(10^4, m = 5) x 2^16 chains -- and, at the first size with 2^12 chains, beside the
reference's own op chain per node visit (a gather, a sum, the divisions, min, logical_or and four where) written out as torch ops
on the same device.  HIP events, median of 5 groups of launches; the score-only launch (num_ls = 0) is timed too, so that the
sweep's share can be read off.  `python tools/timing/cheeger_kernels.py [quick]`."""
import os, sys
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__)))))
import numpy as np, torch
from rlsolver_amd.graph import generate_gnm
from rlsolver_amd.methods import MCPG_cheeger as mc
from rlsolver_amd.ops_mcpg_tsp import PackedChains
dev = torch.device("cuda:0")


def t(f, reps):
    f(); torch.cuda.synchronize()
    s = torch.cuda.Event(enable_timing=True); e = torch.cuda.Event(enable_timing=True)
    s.record()
    for _ in range(reps): f()
    e.record(); torch.cuda.synchronize()
    return s.elapsed_time(e) / reps


def torch_sweep(data, rows, samples, normalized):
    """sampling.py:190-207 / :226-243 on device tensors: samples f32 [N, C] of 0 | 1, one pass."""
    n = data.num_nodes
    a, b = data.edge_index
    val = (lambda cut, size: cut * (1 / size + 1 / (n - size))) if normalized else (lambda cut, size: cut / torch.min(size, n - size))
    res_cut = ((2 * samples[a] - 1) * (2 * samples[b] - 1)).sum(dim=0)
    res_cut = (data.edge_weight_sum - res_cut) / 2
    res_node = samples.sum(dim=0)
    h = val(res_cut, res_node)
    for node in data.sorted_degree_nodes.tolist():
        change = torch.sum(samples[rows[node]], dim=0)
        new_cut = res_cut - (2 * samples[node] - 1) * (data.weighted_degree[node] - 2 * change)
        new_node = res_node - (2 * samples[node] - 1)
        new_h = val(new_cut, new_node)
        cond = torch.logical_or(h < new_h, torch.min(new_node, n - new_node) < 0.0000001)
        samples[node] = torch.where(cond, samples[node], 1 - samples[node])
        res_cut = torch.where(cond, res_cut, new_cut)
        res_node = torch.where(cond, res_node, new_node)
        h = torch.where(cond, h, new_h)
    return h


def ba_edges(n, m, seed):
    rng = np.random.RandomState(seed)
    eu, ev, ends = [], [], list(range(m))
    for v in range(m, n):
        for u in set(rng.choice(ends, m).tolist()):
            eu.append(u), ev.append(v), ends.extend((u, v))
    return np.asarray(eu), np.asarray(ev)


quick = "quick" in sys.argv[1:]
g = np.asarray(generate_gnm(2000, 19990, 5), dtype=np.int64)
for name, n, (eu, ev), C, C_torch in (("G(2000, 19990)", 2000, (g[:, 0], g[:, 1]), 1 << 16, 1 << 12), ("BA(10^4, 5)", 10000, ba_edges(10000, 5, 1), 1 << 16, 0)):
    data = mc.make_data(n, eu, ev, np.ones(eu.shape[0], np.int64), dev)
    torch.manual_seed(0)
    x = PackedChains.pack((torch.rand((n, C), device=dev) < 0.5).float())
    out = PackedChains.empty(n, C, dev)
    for normalized in (False, True):
        reps = 3 if quick else 10
        ker = [t(lambda: data.local_search(x, 1, normalized, out=out, want_cut_size=False), reps) for _ in range(5)]
        score = [t(lambda: data.local_search(x, 0, normalized, out=out, want_cut_size=False), reps) for _ in range(5)]
        k = float(np.median(ker))
        line = (f"{name} E={eu.shape[0]} C={C} {'normalised' if normalized else 'ratio':10s}: kernel {k:9.3f} ms (min {min(ker):.3f}, max {max(ker):.3f}; "
                f"score alone {np.median(score):.3f}) = {k * 1e6 / (n * C):.3f} ns per (chain, visit)")
        if C_torch:
            csr = data.graph.csr
            rows = [torch.from_numpy(csr.col[csr.rowptr[i]:csr.rowptr[i + 1]].astype(np.int64)).to(dev) for i in range(n)]
            xt = PackedChains.pack(x.unpack()[:, :C_torch].contiguous())
            kt = float(np.median([t(lambda: data.local_search(xt, 1, normalized, want_cut_size=False), reps) for _ in range(5)]))
            s = xt.unpack()
            ref = float(np.median([t(lambda: torch_sweep(data, rows, s.clone(), normalized), 1) for _ in range(1 if quick else 3)]))
            line += f" | at C={C_torch}: kernel {kt:.3f} ms, torch op chain {ref:.1f} ms, ratio {ref / kt:.0f}"
        print(line, flush=True)
