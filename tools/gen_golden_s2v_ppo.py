"""Recorder of tests/golden/s2v_ppo.npz: the reference's own EnvMaxcut (rlsolver/methods/S2V_PPO/env.py) run on CPU, start spins,
actions and every per-step output.  torch_scatter is not installed: scatter_add is stood in for by index_add_ (same sums in the same
order on CPU); the fixture says so.  Called by tools/gen_golden.py --only s2v_ppo.  Data only."""
import importlib.util
import json
import os
import sys
import types

import numpy as np
import torch as th

REF_ENV = "/root/reference/rlsolver/methods/S2V_PPO/env.py"


def load_reference_env():
    stub = types.ModuleType("torch_scatter")

    def scatter_add(src, index, dim=0, dim_size=None):
        return th.zeros(dim_size, dtype=src.dtype).index_add_(0, index, src)

    stub.scatter_add = scatter_add
    sys.modules["torch_scatter"] = stub
    spec = importlib.util.spec_from_file_location("s2v_ppo_reference_env", REF_ENV)
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


def _graph(rng, n, m, weights):
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    sys.path.insert(0, os.path.join(root, "tests"))
    try:
        import s2vppo_oracle as orc
    finally:
        sys.path.remove(os.path.join(root, "tests"))
    return orc.random_graph(rng, n, m, weights)


def _actions(rng, n, steps):
    """random nodes; a third of the steps repeat the one before (a revisit: the stag punishment), some three times in a row"""
    acts = []
    while len(acts) < steps:
        a = int(rng.randint(0, n))
        acts += [a] * int(rng.choice([1, 1, 1, 2, 3]))
    return np.array(acts[:steps], dtype=np.int64)


def record(mod, out, name, edge_index, w, n, tenure, coin, rng, fractional=False):
    cfg = types.SimpleNamespace(device=th.device("cpu"), node_feature_dim=5, episode_length_multiplier=2, tabu_tenure=tenure,
                                stag_punishment=0.01)
    gd = {"edge_index": th.from_numpy(edge_index.copy()), "edge_weight": th.from_numpy(w.copy()), "num_nodes": n}
    real = np.random.random
    np.random.random = lambda: coin            # < 0.5: random spins, else greedy from all-ones (env.py:48)
    try:
        env = mod.EnvMaxcut(gd, cfg)
        state = env.reset()
    finally:
        np.random.random = real
    steps = env.max_steps
    acts = _actions(rng, n, steps)
    xs, masks = [state["x"].numpy().copy()], [state["valid_actions_mask"].numpy().copy()]
    deltas = [env.delta_cache.numpy().copy()]
    z0 = env.z.numpy().astype(np.int8)
    rew, done, cut, best = [], [], [env.current_cut], [env.best_cut]
    for a in acts:
        state, r, d, info = env.step(int(a))
        xs.append(state["x"].numpy().copy())
        masks.append(state["valid_actions_mask"].numpy().copy())
        deltas.append(env.delta_cache.numpy().copy())
        rew.append(r)
        done.append(d)
        cut.append(info["cut_value"])
        best.append(info["best_cut"])
    xs = np.stack(xs)
    p = name + "/"
    out[p + "edge_index"], out[p + "edge_weight"] = edge_index.astype(np.int32), w
    out[p + "meta"] = np.array([n, tenure, 2, int(coin >= 0.5)], dtype=np.int64)       # N, tenure, multiplier, greedy start
    out[p + "z0"], out[p + "actions"] = z0, acts.astype(np.int32)
    out[p + "reward"], out[p + "done"] = np.array(rew, dtype=np.float64), np.packbits(np.array(done, dtype=bool))
    out[p + "cut"], out[p + "best"] = np.array(cut, dtype=np.float64), np.array(best, dtype=np.float64)
    out[p + "best_z"] = env.best_z.numpy().astype(np.int8)
    if fractional:
        out[p + "delta"] = np.stack(deltas).astype(np.float32)
        return
    assert np.array_equal(xs[:, :, 0], xs[:, :, 0].astype(np.int8)) and (xs[:, :, 4] == xs[:, :1, 4]).all()
    out[p + "x0"] = xs[:, :, 0].astype(np.int8)
    out[p + "x1"], out[p + "x3"] = xs[:, :, 1].copy(), xs[:, :, 3].copy()
    out[p + "x2"] = np.packbits(xs[:, :, 2] != 0, axis=1)
    assert np.isin(xs[:, :, 2], (0.0, 1.0)).all()
    out[p + "x4"] = xs[:, 0, 4].copy()
    out[p + "mask"] = np.packbits(np.stack(masks), axis=1)


def generate(save):
    mod = load_reference_env()
    rng = np.random.RandomState(20261020)
    out, names = {}, []
    cases = [(1, 0, "unit", 3, 0.9), (5, 6, "unit", 0, 0.1), (5, 7, "pm1", 60, 0.9), (20, 45, "unit", 3, 0.9), (20, 50, "pm1", 10, 0.1),
             (40, 120, "unit", 10, 0.1), (40, 150, "pm1", 0, 0.9), (65, 200, "unit", 60, 0.9), (65, 260, "pm1", 3, 0.1)]
    for n, m, kind, tenure, coin in cases:
        ei, w = _graph(rng, n, m, kind)
        name = f"n{n}_{kind}_t{tenure}"
        record(mod, out, name, ei, w, n, tenure, coin, rng)
        names.append(name)
    # the irregular list: a loop, a pair listed twice with different weights, a negative weight, a one-directional entry
    ei = np.array([[0, 1, 2, 2, 0, 1, 3, 4, 1, 2], [1, 0, 2, 3, 1, 0, 4, 3, 4, 0]], dtype=np.int64)
    w = np.array([1, 1, 2, 1, 3, 3, -2, -2, 1, 1], dtype=np.float32)
    record(mod, out, "irregular", ei, w, 5, 2, 0.1, rng)
    names.append("irregular")
    # a dense graph on which the greedy start stops at its N // 2 cap
    ei, w = _graph(np.random.RandomState(4), 64, int(0.2 * 64 * 63 / 2), "unit")     # (32 flips, a gain of 1 left)
    record(mod, out, "dense64_greedy", ei, w, 64, 10, 0.9, rng)
    names.append("dense64_greedy")
    ei, w = _graph(rng, 40, 120, "fractional")
    record(mod, out, "fractional", ei, w, 40, 10, 0.1, rng, fractional=True)
    out["names"] = np.array(json.dumps(names))
    out["source"] = np.array("recorded from the reference's own EnvMaxcut (rlsolver/methods/S2V_PPO/env.py) on CPU, with a stand-in for "
                             "torch_scatter.scatter_add (zeros(dim_size).index_add_(0, index, src)) and numpy.random.random patched to "
                             "choose the reset branch; row 0 of every per-step array is the reset state; x0 = column 0 as int8, x2 and "
                             "mask as np.packbits(axis=1), x4 = column 4 (one value per step); 'fractional' keeps delta_cache, cut and "
                             "best only")
    save("s2v_ppo", **out)
