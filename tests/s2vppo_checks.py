"""What the GPU tests (tests/test_gpu_s2v_ppo.py) and the fuzzer (tools/fuzz/fuzz_s2v_ppo.py) of the S2V_PPO env share: drive a
VecEnvMaxcut and the numpy oracles (tests/s2vppo_oracle.py) through the same actions, the rollout loop's resets included, and compare
every output of every step bit for bit."""
import types

import numpy as np
import torch

DEV = "cuda:0"


def cfg(tenure=10, multiplier=2, stag=0.01):
    return types.SimpleNamespace(device=torch.device(DEV), node_feature_dim=5, episode_length_multiplier=multiplier, tabu_tenure=tenure,
                                 stag_punishment=stag)


def gd(ei, w, n):
    return {"edge_index": torch.from_numpy(np.ascontiguousarray(ei, dtype=np.int64)), "edge_weight": torch.from_numpy(np.asarray(w, dtype=np.float32)),
            "num_nodes": int(n)}


KEYS = ("x", "mask", "z", "delta", "best_z", "cut", "best", "reward", "done", "steps")


def snap_env(env):
    c = lambda t: t.cpu().numpy().copy()       # noqa: E731
    return dict(x=c(env.x), mask=c(env.valid_mask), z=c(env.z), delta=c(env.delta_cache), best_z=c(env.best_z), cut=c(env.current_cut),
                best=c(env.best_cut), reward=c(env.reward), done=c(env.done), steps=c(env.step_count))


def snap_oracles(os_, last):
    states = [o.state() for o in os_]
    cat = lambda parts, dt: np.concatenate(parts).astype(dt)       # noqa: E731
    return dict(x=np.concatenate([s[0] for s in states]), mask=np.concatenate([s[1] for s in states]), z=cat([o.z for o in os_], np.int8),
                delta=cat([o.delta for o in os_], np.float32), best_z=cat([o.best_z for o in os_], np.int8),
                cut=np.array([o.cut for o in os_]), best=np.array([o.best_cut for o in os_]), reward=last["reward"].copy(),
                done=last["done"].copy(), steps=np.array([o.steps for o in os_], dtype=np.int32))


def drive(env, os_, z0s, acts, steps):
    """Step env (a VecEnvMaxcut) and/or the oracles through cyclic per-env action lists for `steps` steps, resetting a done env to its
    z0 (as the rollout loop does) -> two snapshots per step (before and after the resets) after the one of the first reset."""
    B = len(z0s)
    pos = [0] * B
    last = dict(reward=np.zeros(B), done=np.zeros(B, dtype=bool))
    recs_e, recs_o = [], []
    if env is not None:
        env.reset(z0=z0s)
        env.reward.zero_()
        env.done.zero_()
        recs_e.append(snap_env(env))
    if os_ is not None:
        for o, z in zip(os_, z0s):
            o.reset(z)
        recs_o.append(snap_oracles(os_, last))
    for _ in range(steps):
        a = [int(acts[i][pos[i] % len(acts[i])]) for i in range(B)]
        pos = [p + 1 for p in pos]
        if env is not None:
            env.step(torch.tensor(a, dtype=torch.int64, device=DEV))
            recs_e.append(snap_env(env))
            done = recs_e[-1]["done"]
        if os_ is not None:
            for i, o in enumerate(os_):
                r = o.step(a[i])
                last["reward"][i], last["done"][i] = r["reward"], r["done"]
            recs_o.append(snap_oracles(os_, last))
            done = last["done"]
        ids = np.flatnonzero(done)
        if env is not None:
            if len(ids):
                env.reset(ids=ids, z0=z0s)
            recs_e.append(snap_env(env))
        if os_ is not None:
            for i in ids:
                os_[i].reset(z0s[i])
            recs_o.append(snap_oracles(os_, last))
        for i in ids:
            pos[i] = 0
    return recs_e, recs_o


def bits(a):
    a = np.ascontiguousarray(a)
    return a.view({4: np.uint32, 8: np.uint64}[a.dtype.itemsize]) if a.dtype.kind == "f" else a


def assert_same(ra, rb, tag, lo_a=None, lo_b=None):
    """two records bit-equal; lo_x = (node range, env range) to compare a slice of each"""
    assert len(ra) == len(rb), tag
    for k, (sa, sb) in enumerate(zip(ra, rb)):
        for key in KEYS:
            per_env = key in ("cut", "best", "reward", "done", "steps")
            a, b = sa[key], sb[key]
            if lo_a is not None:
                a = a[slice(*lo_a[1 if per_env else 0])]
            if lo_b is not None:
                b = b[slice(*lo_b[1 if per_env else 0])]
            assert a.shape == b.shape and np.array_equal(bits(a), bits(b)), f"{tag}: snapshot {k} (step {(k + 1) // 2}) {key}"


def actions_for(rng, n, steps):
    acts = []
    while len(acts) < steps:
        acts += [int(rng.randint(0, n))] * int(rng.choice([1, 1, 1, 2, 3]))
    return np.array(acts[:steps], dtype=np.int64)
