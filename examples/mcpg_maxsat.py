#!/usr/bin/env python3
"""MCPG on MaxSAT -- the sampling loop of the upstream MCPG package (metro walk, node-sequential sweep, best of repeats, merge,
policy update) on a random 3-SAT formula, through run_mcpg: every round is the bit-packed walk, ONE sweep + score kernel
(rls_maxsat_local_search) and the best-merge.

    python examples/mcpg_maxsat.py                          # 200 variables, 840 clauses (ratio 4.2), 64 kept chains x 8 repeats
    python examples/mcpg_maxsat.py --nvar 2000 --kept 512 --rounds 20
    python examples/mcpg_maxsat.py --file instance.cnf      # or .wcnf

Prints the number of satisfied clauses (res = (S + K) / 2 of the reference) of the best assignment found."""
import argparse
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--nvar", type=int, default=200)
    ap.add_argument("--ratio", type=float, default=4.2, help="clauses per variable of the random 3-SAT formula")
    ap.add_argument("--file", default=None, help="a .cnf / .wcnf file instead of the random formula")
    ap.add_argument("--kept", type=int, default=64, help="kept chains (total_mcmc_num), a multiple of 64")
    ap.add_argument("--repeats", type=int, default=8)
    ap.add_argument("--num-ls", type=int, default=2)
    ap.add_argument("--rounds", type=int, default=10)
    ap.add_argument("--seed", type=int, default=0)
    a = ap.parse_args()

    import numpy as np
    import torch
    from rlsolver_amd.methods.MCPG import run_mcpg
    from rlsolver_amd.methods.MCPG_maxsat import make_data, maxsat_dataloader

    dev = torch.device("cuda:0")
    torch.manual_seed(a.seed)
    if a.file:
        data, nvar = maxsat_dataloader(a.file, dev)
    else:
        rng = np.random.RandomState(a.seed)
        nvar = a.nvar
        clauses = [[int(v + 1) * (1 if rng.rand() < 0.5 else -1) for v in rng.choice(nvar, 3, replace=False)]
                   for _ in range(int(a.ratio * nvar))]
        data = make_data(nvar, clauses, device=dev)
    xs_init = (torch.rand((nvar, a.kept), device=dev) < 0.5).float()
    vs_init = data.result(xs_init)                                  # the kernel as a pure scorer (num_ls = 0)
    value, x, rates = run_mcpg(data, xs_init, vs_init, a.kept, a.repeats, a.num_ls, a.rounds, seed=a.seed)
    print(f"best res {value:.1f} of K = {data.num_edges}  (start: {float(vs_init.max()):.1f}; {nvar} variables, "
          f"{data.pdata[1]} clauses, {a.kept} x {a.repeats} chains, {a.rounds} rounds, median {np.median(rates):.0f} kept chains / s)")
    assert float(data.result(x.float().reshape(-1, 1))[0]) == value
    return 0


if __name__ == "__main__":
    sys.exit(main())
