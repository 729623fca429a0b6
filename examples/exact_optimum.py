#!/usr/bin/env python3
"""The exact optimum the ECO / S2V papers measure against: `env.calculate_best()` (dqn.py:586, dqn_PECO.py:546 call it for their
"distance from optimum" test score) on the graphs the training generators draw, by enumeration of all 2^N states in one kernel
(rls_spin_exhaustive), and the approximation ratio of one greedy episode of the batched env on the same graphs.

    python examples/exact_optimum.py [--nodes 20,24,28,30] [--envs 8] [--kind BA|ER]

The reference's own calculate_best_energy() raises on every size (tests/golden/spin_exhaustive.npz records how); the one path of it
that runs, a Python loop over the states, takes about ten seconds per graph at 20 spins and three hours at 30."""
import argparse
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--nodes", default="20,24,28,30")
    ap.add_argument("--envs", type=int, default=8)
    ap.add_argument("--kind", default="BA", choices=["BA", "ER"])
    ap.add_argument("--seed", type=int, default=0)
    a = ap.parse_args()

    import torch
    from rlsolver_amd.envs.spinsystem import SpinSystem
    from rlsolver_amd.envs.util_envs_PECO import RandomBAGraphGenerator, RandomERGraphGenerator
    dev = torch.device("cuda:0")
    torch.manual_seed(a.seed)
    for n in (int(v) for v in a.nodes.split(",")):
        gg = (RandomBAGraphGenerator(n_spins=n, m_insertion_edges=4, num_envs=a.envs, device=dev) if a.kind == "BA"
              else RandomERGraphGenerator(n_spins=n, p_connection=0.15, num_envs=a.envs, device=dev))
        env = SpinSystem(None, None, a.envs, max_steps=2 * n, device=dev, graph_generator=gg)
        env.calculate_best()                                          # (the first call also loads the kernel)
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        best_cut, best_spins = env.calculate_best()                   # [B], [B, N]
        torch.cuda.synchronize()
        dt = time.perf_counter() - t0
        assert torch.equal(env.calculate_cut(best_spins), best_cut)   # the env's own cut of the states it was given
        # one greedy episode from the env's random start: flip the spin with the largest immediate cut gain while one is positive
        for _ in range(2 * n):
            gains = env.get_immeditate_rewards_avaialable()
            gain, action = gains.max(dim=1)
            if not bool((gain > 0).any()):
                break
            env.step(action)
        # (the cut of the best state, recomputed: the score a step tracks counts a BA seed clique's self-loops as gains, like the
        # reference's matmul does, and a cut does not)
        reached = env.calculate_cut(env.best_spins)
        ratio = (reached / best_cut.clamp(min=1))[best_cut > 0]       # (a graph of -1 edges alone has optimum 0: left out)
        assert bool((reached <= best_cut).all())                      # nothing beats the optimum
        cuts = [int(c) for c in best_cut.tolist()]
        shown = cuts if len(cuts) <= 8 else f"{min(cuts)} .. {max(cuts)} (mean {sum(cuts) / len(cuts):.1f})"
        print(f"{a.kind}-{n} x {a.envs}: optimum cut {shown}; {a.envs * 2 ** n / dt:.3g} states/s "
              f"({dt * 1e3:.2f} ms with the host work around the kernel); greedy episode reaches {ratio.mean():.3f} of it on average "
              f"(worst {ratio.min():.3f})")
    print("exact_optimum: ok")


if __name__ == "__main__":
    main()
