"""Rates of the exhaustive enumeration kernel (rls_spin_exhaustive) with hipEvents: states / s at N = 24 .. 36 for one graph and
at N = 20 for 256 graphs (one launch each, a range of at most 2^34 states), the duration of a launch of the full default budget
(ops.EXHAUSTIVE_STATES_PER_LAUNCH (graph, state) pairs: it has to stay under 0.1 s) and the pack kernel.  Medians of 5 (min, max).

    python tools/timing/spin_exhaustive.py > profiles/exhaustive_kernels.txt

VALU_PER_STATE below is read from the disassembly (hipcc -S of csrc/rls_exhaustive.hip, the unchecked walk of
k_spin_exhaustive<.., 4>): 41 VALU instructions per block of 16 states; the bound is lanes x clock / that."""
import os
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
for p in (ROOT, os.path.join(ROOT, "tests")):
    if p not in sys.path:
        sys.path.insert(0, p)
import exhaustive_oracle as orc  # noqa: E402
from rlsolver_amd import ops  # noqa: E402

VALU_PER_STATE = 41 / 16
LANES, CLOCK = 256 * 4 * 16, 2.4e9          # CUs x SIMDs x lanes per cycle, Hz (the chip's maximum)
REPS = 5


def timed(fn):
    ms = []
    for _ in range(REPS):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        fn()
        e1.record()
        torch.cuda.synchronize()
        ms.append(e0.elapsed_time(e1))
    ms.sort()
    return ms[len(ms) // 2], ms[0], ms[-1]


def main():
    dev = torch.device("cuda:0")
    rng = np.random.RandomState(1)
    bound = LANES * CLOCK / VALU_PER_STATE
    print(f"# python tools/timing/spin_exhaustive.py  -- medians of {REPS} (min, max); VALU-issue bound {bound / 1e12:.2f} T states/s "
          f"({VALU_PER_STATE:.2f} VALU per state in the walk, {LANES} lanes x {CLOCK / 1e9:.1f} GHz)")
    print("G N states per graph | kernel ms | T (graph, state) pairs / s | fraction of the bound")
    for G, N, states in ((1, 24, 1 << 24), (1, 30, 1 << 30), (1, 32, 1 << 32), (1, 34, 1 << 34), (1, 36, 1 << 34), (1, 48, 1 << 34),
                         (256, 20, 1 << 20), (1, 40, ops.EXHAUSTIVE_STATES_PER_LAUNCH), (256, 40, ops.EXHAUSTIVE_STATES_PER_LAUNCH // 256)):
        Ws = np.stack([orc.random_couplings(rng, N, 0.3) for _ in range(G)])
        pos, neg, flags = ops.spin_exhaustive_pack(torch.from_numpy(Ws).to(dev, torch.float32))
        key = torch.full((G,), ops.EXHAUSTIVE_KEY_EMPTY, dtype=torch.int64, device=dev)
        i0 = (1 << N) - states if N > 24 else 0               # the top of the range: every index bit in play
        run = lambda: torch.ops.rlsolver_hip.spin_exhaustive(pos, neg, i0, i0 + states, key)      # noqa: E731
        run()
        torch.cuda.synchronize()
        med, lo, hi = timed(run)
        rate = G * states / (med * 1e-3)
        print(f"{G} {N} {states} | {med:.3f} ({lo:.3f}, {hi:.3f}) | {rate / 1e12:.2f} | {rate / bound:.2f}")
    m = torch.from_numpy(np.stack([orc.random_couplings(rng, 20, 0.3) for _ in range(256)])).to(dev, torch.float32)
    med, lo, hi = timed(lambda: ops.spin_exhaustive_pack(m))
    print(f"pack 256 x 20 x 20 f32 (with its three allocations) | {med:.3f} ({lo:.3f}, {hi:.3f}) ms")
    W = torch.from_numpy(orc.random_couplings(rng, 30, 0.3)).to(dev)
    med, lo, hi = timed(lambda: ops.spin_exhaustive(W))
    print(f"ops.spin_exhaustive, one graph of 30 spins end to end (pack, flags read, launch, trace) | {med:.3f} ({lo:.3f}, {hi:.3f}) ms")


if __name__ == "__main__":
    main()
