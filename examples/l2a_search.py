#!/usr/bin/env python3
"""The search loop of L2A's dREINFORCE on one graph (rlsolver/methods/L2A/demo_instance.py:141-165) through
rlsolver_amd.methods.L2A.search_step: per step, candidates around the best solutions (sub_set_sampling, ONE kernel), local
searches on them, the best repeat of every sim, the update of the bests and the evaluator -- no host read inside the step.

The transformer policy is out of scope; a stand-in supplies the probabilities: the best rows' spins pulled toward 0.5 plus the
reference's `randn * 0.02`.

    python examples/l2a_search.py                       # a Barabasi-Albert graph of 300 nodes (m = 4)
    python examples/l2a_search.py --file graph.txt      # "n m" header, then "u v w" lines, 1-based

Prints the reference's `value mean < max < best` line every second step."""
import argparse
import os
import sys
import tempfile

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--nodes", type=int, default=300)
    ap.add_argument("--attach", type=int, default=4, help="edges per new node of the Barabasi-Albert graph")
    ap.add_argument("--file", default=None, help="a graph file instead of the generated graph")
    ap.add_argument("--sims", type=int, default=64, help="num_sims (L2A/config.py: 2 ** 6)")
    ap.add_argument("--repeats", type=int, default=32, help="num_repeats (2 ** 5)")
    ap.add_argument("--searchers", type=int, default=2)
    ap.add_argument("--seq-len", type=int, default=16)
    ap.add_argument("--pull", type=float, default=0.3, help="the stand-in policy: probability 0.5 +- pull by the best row's spin")
    ap.add_argument("--seed", type=int, default=0)
    a = ap.parse_args()

    import torch as th
    from rlsolver_amd.envs.env_L2A import EnvMaxcut
    from rlsolver_amd.graph import generate_ba, read_mygraph
    from rlsolver_amd.methods import L2A
    from rlsolver_amd.methods.util_evaluator import Evaluator

    dev = th.device("cuda:0")
    th.manual_seed(a.seed)
    mygraph = read_mygraph(a.file) if a.file else generate_ba(a.nodes, a.attach, a.seed)
    sim = EnvMaxcut(mygraph=mygraph, device=dev, if_bidirectional=True)
    n = sim.num_nodes
    top_k = n // 4                                                   # L2A/config.py:53
    best_xs = sim.generate_xs_randomly(a.sims)
    best_vs = sim.calculate_obj_values(best_xs)
    evaluator = Evaluator(save_dir=tempfile.mkdtemp(prefix="l2a_search_"), num_bits=n, if_maximize=sim.if_maximize, x=best_xs[0], v=best_vs[0])
    history = [evaluator.best_v]
    for t in range(a.seq_len):
        # the stand-in policy: probability 0.5 +- pull by the best row's spin, plus Gaussian noise of 0.02 as the reference adds
        lean = L2A.convert_solution_to_prob(best_xs)[:, :, 0].t().float()             # [sims, n] of +-1
        probs = 0.5 + a.pull * lean + 0.02 * th.randn(lean.shape, device=dev)
        L2A.search_step(sim, probs, best_xs, best_vs, a.repeats, top_k, a.searchers, evaluator=evaluator, iter_i=t)
        if t % 2 == 1:
            mean_v, max_v, best_v = int(best_vs.float().mean()), int(best_vs.max()), evaluator.best_v
            evaluator.logging_print(show_str=f"step {t:3d}: value {mean_v} < {max_v} < {best_v}")
            history.append(best_v)
    assert all(x <= y for x, y in zip(history, history[1:])), history
    assert th.equal(best_vs, sim.calculate_obj_values(best_xs))
    print(f"best cut = {evaluator.best_v}  ({n} nodes, {sim.num_edges} edges, {a.sims} sims x {a.repeats} repeats, top_k = {top_k}, "
          f"{a.seq_len} steps; best values never decreased: {history})")
    return 0


if __name__ == "__main__":
    sys.exit(main())
