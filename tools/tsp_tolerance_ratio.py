#!/usr/bin/env python3
"""How far is the float32 ISCO_TSP oracle (oracle/oracle_isco.py: tsp_step) from the same restatement run in float64, on exactly
the inputs of the step cases of tests/tsp_cases.py?  Reference against reference, on the CPU, never against the kernel: the
largest |log_acc f32 - log_acc f64| per case is the `gap` column of STEP_CASES (rounded up) and twice it -- or the existing rule
rtol 2e-5 / atol 1e-4 where that is larger -- is the bound tests/test_gpu_tsp_forms.py allows the kernel.  Also prints what the
host test asserts: the share of envs the oracle rejects, that are sure, whose log_acc is negative, whose Gumbel argmax sits
within the bound, and on how many envs the two oracle runs walk different tours.

    PYTHONDONTWRITEBYTECODE=1 python tools/tsp_tolerance_ratio.py [case ...]
"""
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.dont_write_bytecode = True
sys.path.insert(0, ROOT)

import numpy as np

from tests import tsp_cases as tc

print(f"{'case':16s} {'N':>5s} {'T':>8s} {'gap':>10s} {'recorded':>9s} {'bound':>9s} {'|log_acc|':>10s} rejected  sure  neg  undecided  f32!=f64")
for c in tc.STEP_CASES:
    if len(sys.argv) > 1 and c.name not in sys.argv[1:]:
        continue
    r32, r64 = tc.step_oracle(c.name), tc.step_oracle(c.name, True)
    same = (r32["cur_x"] == r64["cur_x"]).all(axis=1)
    gap = np.abs(r32["log_acc"].astype(np.float64) - r64["log_acc"])[same].max()
    sure, decided, rejected = tc.step_gates(c, r32)
    print(f"{c.name:16s} {c.N:5d} {c.T:8.4g} {gap:10.3e} {c.gap:9.2e} {tc.log_acc_tol(c, r32['log_acc']).max():9.2e} "
          f"{np.abs(r32['log_acc']).max():10.4g} {rejected.mean():8.2f} {sure.mean():5.2f} {(r32['log_acc'] < 0).mean():4.2f} "
          f"{(~decided).mean():10.3f} {(~same).sum():4d} / {c.B}")
