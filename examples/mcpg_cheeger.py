#!/usr/bin/env python3
"""MCPG on the two Cheeger cuts -- the upstream package's flow for rcheegercut / ncheegercut: sample_initializer's one-hot
start, one epoch-0 call of the reference-shaped sampler for the incumbents, then the sampling loop (metro walk, the
node-sequential sweep in ONE kernel -- rls_cheeger_local_search --, best of repeats, merge, policy update) through run_mcpg.

    python examples/mcpg_cheeger.py                        # a Barabasi-Albert graph of 100 nodes (m = 4), ratio cut
    python examples/mcpg_cheeger.py --normalized           # cut (1 / |S| + 1 / |V \\ S|)
    python examples/mcpg_cheeger.py --file graph.txt       # "n m" header, then "u v w" lines, 1-based

Prints the smallest cut value h found (the samplers return -h: larger is better)."""
import argparse
import os
import sys
import types

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--nodes", type=int, default=100)
    ap.add_argument("--attach", type=int, default=4, help="edges per new node of the Barabasi-Albert graph")
    ap.add_argument("--file", default=None, help="a graph file instead of the generated graph")
    ap.add_argument("--normalized", action="store_true", help="the normalised cut (ncheegercut) instead of the ratio cut")
    ap.add_argument("--kept", type=int, default=64, help="kept chains (total_mcmc_num), a multiple of 64")
    ap.add_argument("--repeats", type=int, default=8)
    ap.add_argument("--num-ls", type=int, default=2)
    ap.add_argument("--rounds", type=int, default=10)
    ap.add_argument("--seed", type=int, default=0)
    a = ap.parse_args()

    import numpy as np
    import torch
    from rlsolver_amd.methods import MCPG_cheeger as mc
    from rlsolver_amd.methods.MCPG import run_mcpg

    dev = torch.device("cuda:0")
    torch.manual_seed(a.seed)
    if a.file:
        data, n = mc.cheeger_dataloader(a.file, dev, normalized=a.normalized)
    else:
        rng = np.random.RandomState(a.seed)
        n, m = a.nodes, a.attach
        eu, ev, ends = [], [], list(range(m))
        for v in range(m, n):                                       # preferential attachment
            for u in set(rng.choice(ends, m).tolist()):
                eu.append(u), ev.append(v), ends.extend((u, v))
        data = mc.make_data(n, np.asarray(eu), np.asarray(ev), np.ones(len(eu), np.int64), dev, normalized=a.normalized)
    problem = "ncheegercut" if a.normalized else "rcheegercut"
    sampler = mc.mcpg_sampling_ncheegercut if a.normalized else mc.mcpg_sampling_rcheegercut
    cfg = types.SimpleNamespace(total_mcmc_num=a.kept, repeat_times=a.repeats)
    probs = torch.full((n,), 0.5, device=dev)
    start = mc.sample_initializer(problem, probs, cfg, dev, data)                       # one-hot chains at the nodes of smallest degree
    vs_init, xs_init, _, _ = sampler(data, start, probs, a.num_ls, 0, a.kept)           # epoch 0: the incumbents
    value, x, rates = run_mcpg(data, xs_init, vs_init, a.kept, a.repeats, a.num_ls, a.rounds, seed=a.seed)
    side = int(x.sum())
    print(f"best {problem} h = {-value:.6f}  (epoch 0: {-float(vs_init.max()):.6f}; {n} nodes, {data.num_graph_edges} edges, side sizes "
          f"{side} / {n - side}, {a.kept} x {a.repeats} chains, {a.rounds} rounds, median {np.median(rates):.0f} kept chains / s)")
    assert float(data.result(x.float().reshape(-1, 1))[0]) == value
    return 0


if __name__ == "__main__":
    sys.exit(main())
