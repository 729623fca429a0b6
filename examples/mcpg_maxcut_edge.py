#!/usr/bin/env python3
"""MCPG with the edge-flip MaxCut sampler -- the upstream package's flow for Problem.maxcut_edge: Bernoulli start chains, one
epoch-0 call of the reference-shaped sampler for the incumbents, then the sampling loop (metro walk, the edge-sequential sweep
in ONE kernel -- rls_maxcut_edge_local_search --, best of repeats, merge, policy update) through run_mcpg.

    python examples/mcpg_maxcut_edge.py                    # a Barabasi-Albert graph of 100 nodes (m = 4), weights +-1
    python examples/mcpg_maxcut_edge.py --file graph.txt   # "n m" header, then "u v w" lines, 1-based, integer weights

Prints the largest cut found."""
import argparse
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--nodes", type=int, default=100)
    ap.add_argument("--attach", type=int, default=4, help="edges per new node of the Barabasi-Albert graph")
    ap.add_argument("--file", default=None, help="a graph file instead of the generated graph")
    ap.add_argument("--kept", type=int, default=64, help="kept chains (total_mcmc_num), a multiple of 64")
    ap.add_argument("--repeats", type=int, default=8)
    ap.add_argument("--num-ls", type=int, default=2)
    ap.add_argument("--rounds", type=int, default=10)
    ap.add_argument("--seed", type=int, default=0)
    a = ap.parse_args()

    import numpy as np
    import torch
    from rlsolver_amd.methods import MCPG_maxcut_edge as me
    from rlsolver_amd.methods.MCPG import run_mcpg

    dev = torch.device("cuda:0")
    torch.manual_seed(a.seed)
    if a.file:
        data, n = me.maxcut_edge_dataloader(a.file, dev)
    else:
        rng = np.random.RandomState(a.seed)
        n, m = a.nodes, a.attach
        eu, ev, ends = [], [], list(range(m))
        for v in range(m, n):                                       # preferential attachment
            for u in set(rng.choice(ends, m).tolist()):
                eu.append(u), ev.append(v), ends.extend((u, v))
        data = me.make_data(n, np.asarray(eu), np.asarray(ev), rng.choice([-1, 1], len(eu)), dev)
    probs = torch.full((n,), 0.5, device=dev)
    start = torch.bernoulli(probs[:, None].expand(n, a.kept * a.repeats).contiguous())
    vs_init, xs_init, _, _ = me.mcpg_sampling_maxcut_edge(data, start, probs, a.num_ls, max(1, n // 10), a.kept)   # epoch 0: the incumbents
    xs_init = (xs_init > 0.25).float()                               # (a node no edge touches holds -0.5 | 1.5 there)
    value, x, rates = run_mcpg(data, xs_init, vs_init, a.kept, a.repeats, a.num_ls, a.rounds, seed=a.seed)
    print(f"best cut = {value:.1f}  (epoch 0: {float(vs_init.max()):.1f}; {n} nodes, {data.num_graph_edges} edges of weight sum "
          f"{data.edge_weight_sum:.0f}, {a.kept} x {a.repeats} chains, {a.rounds} rounds, median {np.median(rates):.0f} kept chains / s)")
    assert float(data.result(x.float().reshape(-1, 1))[0]) == value
    return 0


if __name__ == "__main__":
    sys.exit(main())
