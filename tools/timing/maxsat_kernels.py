"""The MaxSAT sweep + score kernel (rls_maxsat_local_search) on random 3-SAT at two sizes -- nvar = 2000 / 8400 clauses / 2^16
chains and nvar = 200 / 840 clauses / 2^18 chains, num_ls = 2 -- beside this project's own torch restatement of the per-variable
sweep (two gathers, two segment maxima and a where per variable, as the reference runs it) on the same device and a slice of
the same chains.  Median of 5 groups of launches.  `python tools/timing/maxsat_kernels.py [quick]`."""
import os, sys
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__)))))
import numpy as np, torch
from rlsolver_amd.methods import MCPG_maxsat as ms
from rlsolver_amd.ops_mcpg_tsp import PackedChains
dev = torch.device("cuda:0")


def t(f, reps):
    f(); torch.cuda.synchronize()
    s = torch.cuda.Event(enable_timing=True); e = torch.cuda.Event(enable_timing=True)
    s.record()
    for _ in range(reps): f()
    e.record(); torch.cuda.synchronize()
    return s.elapsed_time(e) / reps


def torch_sweep(data, s, num_ls):
    """The reference's sweep restated on torch ops: s float [C, nvar] of -1 | +1, in place."""
    nvi, nci, nneg, order, _ = data.ndata
    for _ in range(num_ls):
        for i in order.tolist():
            if nvi[i].numel() == 0:
                keep = torch.rand(s.shape[0], device=s.device) < 0.5
                s[:, i] = torch.where(keep, -s[:, i], s[:, i])
                continue
            n = int(nci[i][-1]) + 1
            idx = nci[i].unsqueeze(0).expand(s.shape[0], -1)
            seg = lambda: s.new_zeros((s.shape[0], n)).scatter_reduce(1, idx, s[:, nvi[i]] * nneg[i], "amax", include_self=False).sum(1)   # noqa: E731
            old = seg()
            s[:, i] = -s[:, i]
            new = seg()
            ind = new > old + torch.rand(s.shape[0], device=s.device) - 0.5
            s[:, i] = torch.where(ind, s[:, i], -s[:, i])
    return s


quick = "quick" in sys.argv[1:]
for nvar, C, C_torch in ((2000, 1 << 16, 1 << 12), (200, 1 << 18, 1 << 14)):
    rng = np.random.RandomState(nvar)
    clauses = [[int(v + 1) * (1 if rng.rand() < 0.5 else -1) for v in rng.choice(nvar, 3, replace=False)] for _ in range(int(4.2 * nvar))]
    torch.manual_seed(0)
    data = ms.make_data(nvar, clauses, device=dev)
    lvp = data.schedule()[0].cpu().numpy().view(np.uint32)
    x = PackedChains.pack((torch.rand((nvar, C), device=dev) < 0.5).float())
    out = PackedChains.empty(nvar, C, dev)
    num_ls = 2
    ker = [t(lambda: data.local_search(x, num_ls, seed=1, out=out), 3 if quick else 10) for _ in range(5)]
    score = [t(lambda: data.local_search(x, 0, out=out), 3 if quick else 10) for _ in range(5)]
    s = (x.unpack()[:, :C_torch].t() * 2 - 1).contiguous()
    ref = [t(lambda: torch_sweep(data, s, num_ls), 1) for _ in range(1 if quick else 3)]
    k, r = float(np.median(ker)), float(np.median(ref)) * (C / C_torch)
    print(f"nvar={nvar} clauses={len(clauses)} C={C} num_ls={num_ls}: groups {lvp.size - 1}, levels {int((lvp[:-1] >> 31).sum())} | "
          f"kernel {k:9.3f} ms (min {min(ker):.3f}, max {max(ker):.3f}; score alone {np.median(score):.3f}) | torch sweep on {C_torch} chains "
          f"{np.median(ref):9.1f} ms -> {r:9.1f} ms scaled to C | ratio {r / k:8.1f}", flush=True)
