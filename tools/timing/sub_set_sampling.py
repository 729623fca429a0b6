"""sub_set_sampling: the kernel (rls_sub_set_sampling), the same rule as torch ops on the same GPU (ops.sub_set_sampling_torch:
what the wrapper runs past the kernel's node limit, the kernel's own draws restated included) and rand_spins_repeats -- the
write-only kernel of the parent commit -- writing the same [R S, N] bytes; then one L2A search_step at 4096 and 65 536 rows, split
into candidate generation and the rest.  Per shape: warm-up, then 7 interleaved groups of launches per variant, medians (min, max).
    python tools/timing/sub_set_sampling.py [--quick] > profiles/sub_set_sampling_kernels.txt"""
import os, sys
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__)))))
import numpy as np, torch
from rlsolver_amd import ops
from rlsolver_amd.envs.env_L2A import EnvMaxcut
from rlsolver_amd.graph import generate_gnm
from rlsolver_amd.methods import L2A
dev = torch.device("cuda:0")


def t(f, reps):
    s = torch.cuda.Event(enable_timing=True); e = torch.cuda.Event(enable_timing=True)
    s.record()
    for _ in range(reps): f()
    e.record(); torch.cuda.synchronize()
    return s.elapsed_time(e) / reps * 1e3


def groups(fs, reps):
    for f in fs.values():
        t(f, 3)                                                               # warm-up: clocks, code objects, allocator
    rows = {k: [] for k in fs}
    for _ in range(7):                                                        # interleaved, so that drift hits all alike
        for k, f in fs.items():
            rows[k].append(t(f, reps))
    return rows


quick = "--quick" in sys.argv[1:]
fmt = lambda r: f"{np.median(r):9.1f} ({min(r):.1f}, {max(r):.1f})"           # noqa: E731
print("# python tools/timing/sub_set_sampling.py  -- MI355X, medians of 7 interleaved groups (min, max), microseconds")
print("S R N top_k | kernel us (GB/s of its R S N + 9 S N bytes) | torch-op path us (x kernel) | rand_spins_repeats us, same bytes (kernel / it)")
shapes = [(64, 32, 2000, 500), (64, 1024, 2000, 500), (64, 64, 10000, 2500), (64, 32, 800, 200)]
for S, R, N, k in (shapes[:1] + shapes[3:] if quick else shapes):
    torch.manual_seed(S + R + N)
    best = torch.rand((S, N), device=dev) < 0.5
    # the callers' probabilities: a softmax near 0 | 1 pulled toward 0.5, plus the reference's randn * 0.02
    probs = (torch.where(best, 0.8, 0.2) + torch.randn((S, N), device=dev) * 0.02).contiguous()
    out = torch.empty((R * S, N), dtype=torch.bool, device=dev)
    seeds = torch.arange(1, R + 1, dtype=torch.int64, device=dev)
    fs = {"kernel": lambda: ops.sub_set_sampling(probs, best, R, k, seed=7, out=out),
          "torch": lambda: ops.sub_set_sampling_torch(probs, best, R, k, None, 7, 0),
          "spins": lambda: ops.rand_spins_repeats(seeds, S, N, dev, out=out)}
    a, _ = ops.sub_set_sampling(probs, best, R, k, seed=7)
    b, _ = ops.sub_set_sampling_torch(probs, best, R, k, None, 7, 0)
    assert torch.equal(a, b), "the two paths disagree"
    del a, b
    rows = groups(fs, 20 if R * S * N < (1 << 28) else 5)
    med = {key: float(np.median(v)) for key, v in rows.items()}
    assert med["torch"] > med["kernel"], f"the kernel is not faster than the torch-op path at S={S} R={R} N={N}: {med}"
    gbs = (R * S * N + 9 * S * N) / (med["kernel"] * 1e-6) / 1e9
    print(f"{S} {R} {N} {k} | {fmt(rows['kernel'])} ({gbs:.0f} GB/s) | {fmt(rows['torch'])} (x{med['torch'] / med['kernel']:.1f}) | "
          f"{fmt(rows['spins'])} ({med['kernel'] / med['spins']:.2f})", flush=True)

print("# one L2A search_step (2 searchers) on a G22-sized G(n, m) graph, N = 2000, m = 19 990, S = 64, top_k = 500")
print("rows | search_step us | sub_set_sampling us (share) | the rest us")
n, m, S = 2000, 19990, 64
sim = EnvMaxcut(mygraph=generate_gnm(n, m, seed=22), device=dev, if_bidirectional=True, num_nodes=n, seed=1)
for R in ((64,) if quick else (64, 1024)):
    best_xs = sim.generate_xs_randomly(S)
    best_vs = sim.calculate_obj_values(best_xs)
    probs = (torch.where(best_xs, 0.8, 0.2) + torch.randn((S, n), device=dev) * 0.02).contiguous()
    out = torch.empty((R * S, n), dtype=torch.bool, device=dev)
    fs = {"step": lambda: L2A.search_step(sim, probs, best_xs, best_vs, R, n // 4, 2),
          "gen": lambda: ops.sub_set_sampling(probs, best_xs, R, n // 4, seed=7, out=out)}
    rows = groups(fs, 10 if R <= 64 else 3)
    step, gen = float(np.median(rows["step"])), float(np.median(rows["gen"]))
    print(f"{R * S} | {fmt(rows['step'])} | {fmt(rows['gen'])} ({100 * gen / step:.1f} %) | {step - gen:9.1f}", flush=True)
