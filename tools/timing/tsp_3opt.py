"""Time of one pass of the reference's 3-opt (rls_tsp_3opt_best, with its reduce kernel where slices > 1) with hipEvents, against
N, slices and B: a lone 52-city tour in exact ranking across slices, a lone 100-city tour in both rankings, 2^12 100-city tours
in delta ranking, and a 700-city tour (matrix read through L2).  Medians of 7 (min, max); outputs allocated once, the op
called directly.  Candidates = 7 trials x (C(N, 3) + C(N - 1, 2)) triples per tour.

    python tools/timing/tsp_3opt.py > profiles/tsp3opt_kernels.txt

The one figure printed beside these is the reference's own time for a 52-city pass as recorded by the fixture's generator
(tests/golden/tsp_3opt.npz: Python on the generator's CPU): where the port starts from, not a target."""
import os
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)
from rlsolver_amd import _abi, ops_mcpg_tsp as mops  # noqa: E402

REPS = 7


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


def candidates(n):
    return 7 * (n * (n - 1) * (n - 2) // 6 + (n - 1) * (n - 2) // 2)


def main():
    dev = torch.device("cuda:0")
    print(f"# python tools/timing/tsp_3opt.py  -- one pass (kernel + reduce), medians of {REPS} (min, max)")
    z = np.load(os.path.join(ROOT, "tests", "golden", "tsp_3opt.npz"), allow_pickle=False)
    print(f"# the reference's own 52-city pass: {float(z['reference_seconds_per_berlin52_pass']):.1f} s (Python, on the CPU that generated the fixture; "
          "not a target)")
    print("N B ranking slices (form) | ms per pass | G candidates / s")
    rows = [(52, 1, True, s) for s in (1, 4, 16, 64, None, 256)] + [(100, 1, True, s) for s in (16, 64, None, 512)]
    rows += [(100, 1, False, s) for s in (1, 16, None, 512)] + [(100, 1 << 12, False, 1), (100, 1 << 12, True, 1), (52, 1 << 12, False, 1)]
    rows += [(700, 1, False, None), (200, 1, True, None)]
    for n, B, exact, slices in rows:
        rng = np.random.RandomState(n)
        c = rng.rand(n, 2) * 100.0
        d = torch.from_numpy(np.sqrt(((c[:, None] - c[None]) ** 2).sum(-1))).to(dev)
        perm = torch.from_numpy(np.stack([rng.permutation(n) for _ in range(B)])).to(dev)
        cur = d[perm, torch.roll(perm, -1, 1)].sum(1) if exact else None
        s = slices if slices is not None else mops.tsp_3opt_default_slices(n, B, exact)
        out = [torch.empty(s * B, dtype=torch.int64, device=dev) for _ in range(4)] + [torch.empty(s * B, dtype=torch.float64, device=dev)]
        run = lambda: torch.ops.rlsolver_hip.tsp_3opt_best(d, perm, cur, *out)      # noqa: E731
        run()
        torch.cuda.synchronize()
        med, lo, hi = timed(run)
        f = _abi.tsp_3opt_launch_form(n, exact)
        form = f"{f.waves} waves, matrix {'in LDS' if f.lds_d else 'through L2'}"
        print(f"{n} {B} {'exact' if exact else 'delta'} {s}{'' if slices is not None else ' (default)'} ({form}) | {med:.3f} ({lo:.3f}, {hi:.3f}) | "
              f"{B * candidates(n) / (med * 1e-3) / 1e9:.2f}")


if __name__ == "__main__":
    main()
