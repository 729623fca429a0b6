"""Fuzz of the S2V_PPO env (rls_s2vppo_step / rls_s2vppo_reset through VecEnvMaxcut) against the numpy restatement of
tests/s2vppo_oracle.py: random batches of random edge LISTS -- repeated pairs (also many copies of one pair in one row), loops,
one-directional entries, isolated nodes, integer weights of both signs -- of sizes on both sides of the wave / workgroup thresholds,
any tabu tenure (0, 1, beyond N), start spins recorded or greedy, actions with immediate repeats, envs reset (and re-graphed) as they
end.  Every output of every step must match bit for bit.
`python tools/fuzz/fuzz_s2v_ppo.py [seconds] [seed] [-v]`."""
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)
from tests import s2vppo_oracle as orc  # noqa: E402
from tests import s2vppo_checks as chk  # noqa: E402


def random_list(rng, n):
    kind = rng.choice(["sparse", "dense", "hub", "copies", "empty"])
    m = {"sparse": 2 * n, "dense": min(n * n // 3, 4000), "hub": n, "copies": n + 80, "empty": 0}[kind]
    src, dst = rng.randint(0, n, size=m), rng.randint(0, n, size=m)
    if kind == "hub" and m:                                    # the last node's row is long and ends in loops: in the workgroup form the
        src[: m // 2] = n - 1                                  # loop entries are held by another wave than thread 0
        dst[: 1 + m // 8] = n - 1
    if kind == "copies" and m:
        src[-80:], dst[-80:] = src[0], dst[0]
    if rng.rand() < 0.5 and m:                                 # list the other direction too, as the reference's loader does
        src, dst = np.concatenate([src, dst]), np.concatenate([dst, src])
    w = rng.randint(-3, 4, size=len(src)).astype(np.float32)
    return np.stack([src, dst]).astype(np.int64), w, int(n)


def run(seconds=60.0, seed=0, verbose=False):
    from rlsolver_amd.envs.env_S2V_PPO import VecEnvMaxcut, launch_plan
    rng = np.random.RandomState(seed)
    wave = max(n for n in range(1, 2000) if launch_plan(1, n)["form"] == "wave")
    t_end = time.time() + seconds
    it = 0
    while time.time() < t_end:
        B = int(rng.choice([1, 2, 3, 4, 5, 9]))
        big = int(rng.choice([wave - 1, wave, wave + 1, 400, 700])) if rng.rand() < 0.4 else int(rng.randint(1, 80))
        sizes = [big] + [int(rng.choice([1, 2, 3, 63, 64, 65, int(rng.randint(1, min(big, 120) + 1))])) for _ in range(B - 1)]
        rng.shuffle(sizes)
        tenure = int(rng.choice([0, 1, 2, 10, 200]))
        steps = int(rng.randint(1, 40))
        graphs = [random_list(rng, n) for n in sizes]
        tag = f"it={it} sizes={sizes} tenure={tenure} steps={steps}"
        if verbose:
            print(tag, flush=True)
        env = VecEnvMaxcut([chk.gd(*g) for g in graphs], chk.cfg(tenure), seed=int(rng.randint(1, 1 << 30)))
        os_ = [orc.OracleEnv(ei, w, n, 2, tenure, 0.01) for ei, w, n in graphs]
        if rng.rand() < 0.3:                                   # the greedy start, then on from what it gave
            env.reset(greedy=[True] * B)
            z0s = [o.greedy_start()[0].astype(np.int8) for o in os_]
            assert np.array_equal(env.z.cpu().numpy(), np.concatenate(z0s)), "greedy start " + tag
        else:
            z0s = [rng.choice(np.array([-1, 1], dtype=np.int8), size=n) for n in sizes]
        acts = [chk.actions_for(rng, n, steps) for n in sizes]
        got, want = chk.drive(env, os_, z0s, acts, steps)
        chk.assert_same(got, want, tag)
        if rng.rand() < 0.3:                                   # a new graph for one env, the others go on
            i = int(rng.randint(0, B))
            graphs[i] = random_list(rng, int(rng.randint(1, 90)))
            keep = [j for j in range(B) if j != i]
            before = chk.snap_env(env)
            ptr0 = env.ptr.cpu().numpy()
            env.set_graphs([i], [chk.gd(*graphs[i])])
            after, ptr1 = chk.snap_env(env), env.ptr.cpu().numpy()
            for j in keep:
                for key in ("x", "mask", "z", "delta", "best_z"):
                    assert np.array_equal(chk.bits(before[key][ptr0[j]:ptr0[j + 1]]), chk.bits(after[key][ptr1[j]:ptr1[j + 1]])), f"set_graphs {key} " + tag
            os_[i] = orc.OracleEnv(*graphs[i][:2], graphs[i][2], 2, tenure, 0.01)
            os_[i].reset(after["z"][ptr1[i]:ptr1[i + 1]])
            assert np.array_equal(os_[i].delta.astype(np.float32), after["delta"][ptr1[i]:ptr1[i + 1]]) and os_[i].cut == after["cut"][i], "set_graphs reset " + tag
        it += 1
    return it


if __name__ == "__main__":
    args = [a for a in sys.argv[1:] if a != "-v"]
    n_it = run(float(args[0]) if args else 60.0, int(args[1]) if len(args) > 1 else 0, "-v" in sys.argv)
    print(f"fuzz_s2v_ppo: {n_it} random configurations, no mismatch")
