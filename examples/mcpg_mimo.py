#!/usr/bin/env python3
"""MCPG on MIMO detection -- the upstream package's flow for Problem.MIMO: an instance (generated, or read from one of the
package's two file forms), Bernoulli(1/2) start chains, one epoch-0 call of the reference-shaped sampler for the incumbents, then
the sampling loop (metro walk, the coordinate search and the value in ONE kernel -- rls_mimo_local_search --, best of repeats,
merge, policy update) through run_mcpg, and the driver's vote over the best incumbents.

    python examples/mcpg_mimo.py                            # K = N = 90 (180 variables) at SNR 8
    python examples/mcpg_mimo.py --users 180 --snr 12
    python examples/mcpg_mimo.py --file inst.npz            # K, SNR, H, X, v (write_mimo5); or inst.txt (write_mimo3)

Prints the objective -(min_res + sca) = -|Y - H x|^2 of the best chain and the bit error rate of the vote."""
import argparse
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--users", type=int, default=90, help="K: the instance has 2 K variables")
    ap.add_argument("--antennas", type=int, default=None, help="N (default: K)")
    ap.add_argument("--snr", type=float, default=8)
    ap.add_argument("--file", default=None, help="an instance file (.npz or .txt) instead of the generated instance")
    ap.add_argument("--kept", type=int, default=150, help="kept chains (total_mcmc_num); rounded up to a multiple of 64")
    ap.add_argument("--repeats", type=int, default=100)
    ap.add_argument("--num-ls", type=int, default=None, help="sweeps per round (default: the driver's table)")
    ap.add_argument("--rounds", type=int, default=3)
    ap.add_argument("--seed", type=int, default=0)
    a = ap.parse_args()

    import numpy as np
    import torch
    from rlsolver_amd.methods import MCPG_mimo as mm
    from rlsolver_amd.methods.MCPG import run_mcpg

    dev = torch.device("cuda:0")
    torch.manual_seed(a.seed)
    K, N = a.users, a.users if a.antennas is None else a.antennas
    if a.file and a.file.endswith(".npz"):
        with np.load(a.file) as z:
            data = mm.make_data(*mm.instance_arrays(z["H"], z["X"], z["v"], int(z["K"]), float(z["SNR"])), dev)
    elif a.file:
        data = mm.read_data_mimo3(a.file, 1, 0, dev)
    else:
        data = mm.data_from_instance(mm.mimo_instance(K, N, a.snr, a.seed), dev)
    n = data.num_nodes
    num_ls, _, max_range = mm.mimo_parameters(a.snr, N, K)
    num_ls = num_ls if a.num_ls is None else a.num_ls
    M = -(-a.kept // 64) * 64                                    # the round keeps whole 64-chain tiles
    probs = torch.full((n,), 0.5, device=dev)
    start = torch.bernoulli(probs.expand(M * a.repeats, n)).t().contiguous()
    obj0, xs_init, _, _ = mm.mcpg_sampling_mimo(data, start, probs, num_ls, max(1, n // 10), M)      # epoch 0: the incumbents
    value, x, rates, rnd = run_mcpg(data, xs_init, data.result(xs_init), M, a.repeats, num_ls, a.rounds, seed=a.seed, return_round=True)
    vote = mm.mimo_vote(rnd.now_max_res, rnd.now_max_info.unpack(), max_range)
    ber_vote, ber_best = mm.bit_error_rate(vote, data[2]), mm.bit_error_rate(x.float() * 2 - 1, data[2])
    print(f"best objective -(min_res + sca) = {data.objective(value):.4f}  (epoch 0: {float(obj0.max()):.4f}; sent symbols: "
          f"{data.objective(float(data.result((data[2].float().reshape(-1, 1) + 1) / 2)[0])):.4f}); bit error rate of the vote over {min(max_range, M)} "
          f"incumbents {ber_vote:.4f}, of the best chain {ber_best:.4f}  ({n} variables, {M} x {a.repeats} chains, num_ls {num_ls}, "
          f"{a.rounds} rounds, median {np.median(rates):.0f} kept chains / s)")
    assert float(data.result(x.float().reshape(-1, 1))[0]) == value
    return 0


if __name__ == "__main__":
    sys.exit(main())
