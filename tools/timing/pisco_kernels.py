"""PISCO_maxcut: the f16 matrix-core product alone (time and share of the f16 MFMA peak), the whole step (product + one
kernel), the same step composed of torch ops on the GPU -- a restatement of env_ISCO.py:384-444 with torch.matmul on f16 and
two products per step, as the reference does -- and ISCO_maxcut.step on the same graph where it is unit-weight.
Per (n, density, B): warm-up, then 7 interleaved groups of launches per variant, medians (min, max).
    python tools/timing/pisco_kernels.py [--quick] > profiles/pisco_kernels.txt"""
import os, sys
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__)))))
import numpy as np, torch
from rlsolver_amd import ops
from rlsolver_amd.envs.env_ISCO import ISCO_maxcut, PISCO_maxcut
dev = torch.device("cuda:0")
PEAK_F16 = 2.5e15            # dense f16 / bf16 matrix rate of the MI355X (datasheet), FLOP / s


def t(f, reps):
    s = torch.cuda.Event(enable_timing=True); e = torch.cuda.Event(enable_timing=True)
    s.record()
    for _ in range(reps): f()
    e.record(); torch.cuda.synchronize()
    return s.elapsed_time(e) / reps * 1e3


def renorm(ll):
    base = ll.max(dim=-1, keepdim=True).values
    p = torch.exp(ll - base)
    d = -torch.abs(torch.log(torch.cumsum(p, dim=-1) - p) + base)
    return torch.clamp(ll - torch.where(d > -0.693, torch.log(-torch.expm1(d)), torch.log1p(-torch.exp(d))), max=0.0)


def torch_step(A, x, pl, T):
    """env_ISCO.py:384-444 as torch ops (closed-form gradient instead of autograd: one op fewer per product, in its favour)."""
    def local(s):
        d = s * 2 - 1
        r = torch.matmul(d, A)
        e = (-0.25 * (r * d).sum(dim=1)).float() / T
        return e, torch.log_softmax((d.float() * r.float()) / (2 * T), dim=-1)
    ll_x, lp = local(x)
    pert = lp - torch.log(-torch.log(torch.rand(lp.shape, device=lp.device)))
    thr = torch.gather(torch.sort(pert).values, 1, (lp.shape[1] - pl).unsqueeze(1))
    mask = (pert >= thr).int()
    order = torch.argsort(-pert, dim=-1)
    ll_sel = torch.zeros_like(lp).scatter_(1, order, renorm(torch.gather(lp, -1, order))) * mask
    y = x * (1 - mask) + mask * (1 - x)
    ll_y, lpy = local(y)
    back = torch.argsort(pert, dim=-1)
    lb = renorm(torch.gather(torch.where(mask.bool(), lpy, torch.full_like(lpy, -1e18)), -1, back))
    ll_y2x = torch.where(torch.gather(mask, -1, back).bool(), lb, torch.zeros_like(lb)).sum(dim=-1)
    log_acc = torch.clamp(ll_y + ll_y2x - ll_x - ll_sel.sum(dim=-1), max=0.0)
    use = torch.log(torch.rand(log_acc.shape, device=lp.device) + 1e-24) < log_acc
    return torch.where(use.unsqueeze(-1), y, x), ll_y * T, log_acc.exp()


quick = "--quick" in sys.argv[1:]
print("n density B | product us (share of f16 peak) | torch.matmul us | step us | torch-op step us | ISCO_maxcut.step us")
for n in ((104, 2000) if quick else (104, 800, 2000, 4000)):
    for density in (0.01, 1.0):
        rng = np.random.RandomState(n)
        U = np.triu(rng.rand(n, n) < density, 1)
        adj = (U | U.T).astype(np.float16)
        iu, ju = np.nonzero(U)
        pd = {"num_nodes": n, "num_edges": len(iu), "edge_from": torch.from_numpy(iu).to(dev), "edge_to": torch.from_numpy(ju).to(dev),
              "adj_matrix": torch.from_numpy(adj).to(dev)}
        for B in ((1, 4096) if quick else (1, 64, 4096)):
            p, q = PISCO_maxcut(pd, batch_size=B, device=dev), ISCO_maxcut(pd, batch_size=B, device=dev)
            torch.manual_seed(0)
            xq = q.random_gen_init_sample()
            x = xq.to(torch.float16)
            pl = torch.full((B,), 10, dtype=torch.int64, device=dev)
            A, out = p.adj_matrix, torch.empty((B, n), dtype=torch.float32, device=dev)
            d = x * 2 - 1
            reps = 100 if B <= 64 else 10
            fs = {"product": lambda: ops.pisco_product(A, x, out), "matmul": lambda: torch.matmul(d, A), "step": lambda: p.step(x, pl, 0.5),
                  "torch": lambda: torch_step(A, x, pl, 0.5), "isco": lambda: q.step(xq, pl, 0.5)}
            for f in fs.values():
                t(f, 3)                                                           # warm-up: clocks, code objects, allocator
            rows = {k: [] for k in fs}
            for _ in range(7):                                                    # interleaved, so that drift hits all alike
                for k, f in fs.items():
                    rows[k].append(t(f, reps))
            m = lambda k: f"{np.median(rows[k]):9.1f} ({min(rows[k]):.1f}, {max(rows[k]):.1f})"
            share = 2.0 * B * n * n / (np.median(rows["product"]) * 1e-6) / PEAK_F16
            print(f"{n} {density} {B} | {m('product')} ({100 * share:.2f} %) | {m('matmul')} | {m('step')} | {m('torch')} | {m('isco')}", flush=True)
