#!/usr/bin/env python3
"""Record tests/golden/spin_exhaustive.npz from the reference's numpy env (rlsolver/methods/ECO_S2V/src/envs/spinsystem.py) on the
CPU: `_calc_over_range(i0, iMax)` (:615-651), the one path of its brute-force ground-state search that runs, on +-1-weighted
matrices of 5, 11, 12 and 16 spins -- the full range and two unaligned sub-ranges each, with and without a diagonal -- and what
`calculate_best_energy()` (:278-324) itself does at 5 and 12 spins (the type of the exception it raises).  The reference is
IMPORTED (tools/gen_golden.py puts it on sys.path); nothing of it is written but data.

    PYTHONDONTWRITEBYTECODE=1 python tools/gen_golden.py --only spin_exhaustive        (or: python tools/gen_golden_exhaustive.py)

The script also times the reference's loop (states per second on this CPU, stored as `reference_states_per_second`): a figure
to quote beside the kernel's rate, never a target."""
import os
import sys
import time

import numpy as np

TOOLS = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(TOOLS)
for p in (TOOLS, ROOT, os.path.join(ROOT, "tests")):
    if p not in sys.path:
        sys.path.insert(0, p)

KEY = "spin_exhaustive"


def couplings(rng, n, density, diagonal):
    W = np.triu(rng.choice([-1.0, 1.0], size=(n, n)) * (rng.rand(n, n) < density), 1)
    W = W + W.T
    if diagonal:
        W[np.diag_indices(n)] = rng.randint(-2, 3, size=n).astype(np.float64)
    return W


def cases():
    """(tag, W, ranges): every draw from one explicit RandomState"""
    rng = np.random.RandomState(20261021)
    out = []
    for n, density, diagonal in ((5, 0.8, False), (5, 0.6, True), (11, 0.5, False), (11, 0.3, True), (12, 0.5, False), (12, 0.9, True),
                                 (16, 0.4, True)):
        full = 1 << n
        a, b = sorted(int(v) for v in rng.choice(np.arange(1, full - 1), size=2, replace=False))
        out.append((f"n{n}_{'diag' if diagonal else 'plain'}", couplings(rng, n, density, diagonal), [(0, full), (3, full - 5), (a, b + 1)]))
    return out


def reference_env(W, target_name="ENERGY"):
    import gen_golden  # noqa: F401  (its import puts the reference on sys.path)
    from rlsolver.methods.ECO_S2V.src.envs import spinsystem as spc
    from rlsolver.methods.ECO_S2V.src.envs.util_envs import (ECO_PECO_OBSERVABLES, EdgeType, ExtraAction, GraphGenerator, OptimisationTarget,
                                                             RewardSignal, SpinBasis)
    n = W.shape[0]

    class Fixed(GraphGenerator):
        def __init__(self):
            super().__init__(n, EdgeType.DISCRETE, False)

        def get(self, with_padding=False):
            return W.copy()

    env = spc.SpinSystemFactory.get(Fixed(), 2 * n, observables=ECO_PECO_OBSERVABLES, reward_signal=RewardSignal.DENSE,
                                    extra_action=ExtraAction.NONE, optimisation_target=OptimisationTarget[target_name],
                                    spin_basis=SpinBasis.SIGNED, norm_rewards=False, memory_length=None, horizon_length=None,
                                    stag_punishment=None, basin_reward=None, reversible_spins=True, seed=17)
    return env, spc


def generate(save):
    arrays, tags, rate = {}, [], 0.0
    for tag, W, ranges in cases():
        env, _ = reference_env(W)
        assert np.array_equal(env.matrix, W)
        energy, spins = [], []
        for i0, i1 in ranges:
            t0 = time.perf_counter()
            e, s = env._calc_over_range(i0, i1)
            dt = time.perf_counter() - t0
            if i1 - i0 >= 1 << 16:
                rate = (i1 - i0) / dt
            energy.append(float(e))
            spins.append(np.asarray(s, dtype=np.float64))
        tags.append(tag)
        arrays[f"{tag}/W"] = W
        arrays[f"{tag}/ranges"] = np.asarray(ranges, dtype=np.int64)
        arrays[f"{tag}/energy"] = np.asarray(energy, dtype=np.float64)
        arrays[f"{tag}/spins"] = np.stack(spins)
    # what calculate_best_energy() itself does: the exception type (or "none")
    for n in (5, 12):
        W = couplings(np.random.RandomState(n), n, 0.5, False)
        env, spc = reference_env(W, "CUT")
        real = spc.mp.cpu_count
        spc.mp.cpu_count = lambda: 2                       # a pool of 2 is enough to see what happens; the real count only sizes it
        try:
            env.calculate_best_energy()
            what = "none"
        except Exception as e:                             # noqa: BLE001  (the type is the datum)
            what = type(e).__name__ + ": " + str(e)
        finally:
            spc.mp.cpu_count = real
        arrays[f"calculate_best_energy/n{n}"] = np.array(what)
        print(f"calculate_best_energy() at n_spins = {n}: {what}")
    arrays["cases"] = np.array(tags)
    arrays["reference_states_per_second"] = np.float64(rate)
    arrays["source"] = np.array("the reference's numpy env: SpinSystemUnbiased._calc_over_range(i0, i1) -> (energy, signed spins) per range, "
                                "float64; calculate_best_energy/n*: the exception its own calculate_best_energy() raises")
    print(f"the reference's _calc_over_range: {rate:.0f} states / s on this CPU")
    save(KEY, **arrays)


if __name__ == "__main__":
    import gen_golden
    gen_golden._CURRENT["key"] = KEY
    generate(gen_golden.save)
