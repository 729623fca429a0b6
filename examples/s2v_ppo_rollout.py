"""The rollout loop of rlsolver/methods/S2V_PPO/train_ddp.py:85-163 on VecEnvMaxcut: 8 envs on Barabasi-Albert graphs of mixed size,
ONE kernel per step for the whole batch, a done env gets a new graph (set_graphs, train_ddp.py:154-160).  The policy is a stand-in --
a masked random choice made on the device -- where the trainer would run its S2V network on (x, edge_index, batch).

    python examples/s2v_ppo_rollout.py [steps]
"""
import os
import sys
import time
import types

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from rlsolver_amd.envs.env_S2V_PPO import VecEnvMaxcut  # noqa: E402


def ba_graph(rng, n, m=4):
    """preferential attachment, m lines per new node; both directions listed, as the reference's loader lists them"""
    targets, repeated, e = list(range(m)), [], []
    for v in range(m, n):
        e += [(v, u) for u in targets]
        repeated += targets + [v] * m
        targets = list({repeated[i] for i in rng.randint(0, len(repeated), size=3 * m)})[:m]
    e = np.array(e, dtype=np.int64).T
    return {"edge_index": torch.from_numpy(np.concatenate([e, e[::-1]], axis=1)), "edge_weight": torch.ones(2 * e.shape[1]), "num_nodes": n}


def policy(state, env):
    """one valid node per env, uniformly: the largest of independent uniforms over the env's valid nodes (all on the device)"""
    score = torch.rand(state["x"].shape[0], device=env.device).masked_fill_(~state["valid_actions_mask"], -1.0)
    top = torch.full((env.num_envs,), -2.0, device=env.device).scatter_reduce_(0, state["batch"], score, "amax")
    node = torch.arange(score.numel(), device=env.device).masked_fill_(score < top[state["batch"]], score.numel())
    first = torch.full((env.num_envs,), score.numel(), dtype=torch.int64, device=env.device).scatter_reduce_(0, state["batch"], node, "amin")
    return first - state["ptr"][:-1]


def main(steps=2000):
    dev = torch.device("cuda:0")
    cfg = types.SimpleNamespace(device=dev, node_feature_dim=5, episode_length_multiplier=2, tabu_tenure=10, stag_punishment=0.01)
    rng = np.random.RandomState(0)
    sizes = [60, 100, 150, 200, 200, 250, 300, 400]
    env = VecEnvMaxcut([ba_graph(rng, n) for n in sizes], cfg, seed=0)
    state = env.reset()
    total, episodes, best = torch.zeros(env.num_envs, dtype=torch.float64, device=dev), 0, []
    torch.cuda.synchronize()
    t0 = time.time()
    for _ in range(steps):
        state, reward, done, info = env.step(policy(state, env))
        total += reward
        ended = done.nonzero().reshape(-1).tolist()          # the loop's one host read (the reference has four per env and step)
        if ended:
            best += [float(info["best_cut"][i]) for i in ended]
            episodes += len(ended)
            state = env.set_graphs(ended, [ba_graph(rng, int(rng.choice(sizes))) for _ in ended])
    torch.cuda.synchronize()
    dt = time.time() - t0
    print(f"{steps * env.num_envs} env-steps in {dt:.2f} s: {steps * env.num_envs / dt:.0f} env-steps/s; {episodes} episodes, "
          f"mean best cut {np.mean(best) if best else float('nan'):.1f}, reward per env-step {float(total.sum()) / (steps * env.num_envs):.4f}")


if __name__ == "__main__":
    main(int(sys.argv[1]) if len(sys.argv) > 1 else 2000)
