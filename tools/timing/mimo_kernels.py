"""The MIMO detection kernel (rls_mimo_local_search) at the reference driver's sizes: n = 2 K = 360 and 2400 variables, C = 19 200
chains (its own batch) and 65 536, num_ls = 4.  HIP events, median of 5 groups of 3 launches, with the groups' min and max.  Per
row: the kernel alone, the whole mcpg_sampling_mimo (walk, pack, kernel, best of repeats, unpack, mean), the share of the float32
matrix peak (157 TFLOP/s) that 2 n^2 C (num_ls + 1) flops in the kernel's time amount to, and K11 (qubo_local_search_value, +-1) on
the same n, C and num_ls -- the same contraction through the float32 node-major surface.
`python tools/timing/mimo_kernels.py [quick] [out.txt]`."""
import os, sys
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__)))))
import numpy as np, torch
from rlsolver_amd import ops_mcpg_tsp as mops
from rlsolver_amd.methods import MCPG_mimo as mm, MCPG_qubo as mq
from rlsolver_amd.ops_mcpg_tsp import PackedChains
dev = torch.device("cuda:0")
PEAK = 157e12


def t(f, reps):
    f(); torch.cuda.synchronize()
    s = torch.cuda.Event(enable_timing=True); e = torch.cuda.Event(enable_timing=True)
    s.record()
    for _ in range(reps): f()
    e.record(); torch.cuda.synchronize()
    return s.elapsed_time(e) / reps


def groups(f, reps):
    g = [t(f, reps) for _ in range(5)]
    return float(np.median(g)), min(g), max(g)


args = [a for a in sys.argv[1:] if a != "quick"]
quick = "quick" in sys.argv[1:]
lines = []
num_ls, M = 4, 64
for n in ((360,) if quick else (360, 2400)):
    data = mm.data_from_instance(mm.mimo_instance(n // 2, n // 2, 8, 5), dev)
    for C in ((4096,) if quick else (19200, 65536)):
        torch.manual_seed(0)
        xf = (torch.rand((n, C), device=dev) < 0.5).float()
        x = PackedChains.pack(xf)
        out = PackedChains.empty(n, C, dev)
        probs = torch.full((n,), 0.5, device=dev)
        _, form = mops.mimo_launch_form(n, C)
        reps = 1 if quick else 3
        k, kmin, kmax = groups(lambda: data.local_search(x, num_ls, out=out), reps)
        s, smin, smax = groups(lambda: mm.mcpg_sampling_mimo(data, xf, probs, num_ls, max(1, n // 10), M), reps)
        q, qmin, qmax = groups(lambda: mq.qubo_local_search_value(data[0], xf, num_ls, False), reps)
        flops = 2.0 * n * n * C * (num_ls + 1)
        lines.append(f"n={n} C={C} num_ls={num_ls} form {form}: kernel {k:8.3f} ms (min {kmin:.3f}, max {kmax:.3f}) = {flops / (k * 1e-3) / 1e12:6.2f} TFLOP/s = "
                     f"{100 * flops / (k * 1e-3) / PEAK:5.1f} % of the f32 matrix peak; mcpg_sampling_mimo {s:8.3f} ms (min {smin:.3f}, max {smax:.3f}); "
                     f"K11 qubo_local_search_value (pm1) {q:8.3f} ms (min {qmin:.3f}, max {qmax:.3f}); kernel / K11 = {k / q:.3f}")
        print(lines[-1], flush=True)
if args:
    with open(args[0], "w") as f:
        f.write("tools/timing/mimo_kernels.py on one MI355X: HIP events, median of 5 groups of 3 launches\n" + "\n".join(lines) + "\n")
