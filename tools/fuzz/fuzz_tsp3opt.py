"""Differential fuzz of the 3-opt pass (rls_tsp_3opt_best, methods/tsp_opt_3.py) against the numpy restatement of
tests/tsp3opt_oracle.py: random N in [3, 40], B, slices, Euclidean / integer (ties everywhere) / asymmetric matrices, both
rankings, a true, an inflated and a zero seed length -- indices and float64 values bit for bit; every third round the whole
local_search_3_opt on one tour.  `python tools/fuzz/fuzz_tsp3opt.py [seconds] [seed]`."""
import sys, time
import numpy as np, torch
sys.path.insert(0, ".")
from tests import tsp3opt_oracle as o3
from rlsolver_amd import ops_mcpg_tsp as mops
from rlsolver_amd.methods import tsp_opt_3 as t3

DEV = torch.device("cuda:0")
budget = float(sys.argv[1]) if len(sys.argv) > 1 else 60.0
rng = np.random.RandomState(int(sys.argv[2]) if len(sys.argv) > 2 else 0)
t_end = time.time() + budget
it = 0
while time.time() < t_end:
    N = int(rng.choice([rng.randint(3, 7), rng.randint(7, 20), rng.randint(20, 41)]))
    kind = rng.choice(["euclid", "integer", "asym"])
    c = rng.rand(N, 2) * 100
    d = np.sqrt(((c[:, None] - c[None]) ** 2).sum(-1))
    if kind == "integer":
        d = np.rint(d / 20.0)
    elif kind == "asym":
        d = d + rng.rand(N, N) * 10
    np.fill_diagonal(d, 0)
    B = int(rng.choice([1, 2, rng.randint(3, 12)]))
    slices = [None, 1, 2, int(rng.randint(3, 40)), int(rng.randint(40, 900))][int(rng.randint(0, 5))]
    perms = np.stack([rng.permutation(N) for _ in range(B)])
    dd, pp = torch.from_numpy(d).to(DEV), torch.from_numpy(perms).to(DEV)
    tag = f"it={it} N={N} kind={kind} B={B} slices={slices}"
    true = np.array([o3.distance_calc(d, [int(v) + 1 for v in p] + [int(p[0]) + 1]) for p in perms])
    scale = float(rng.choice([1.0, 1.0, 1.5, 0.0]))
    cur = true * scale
    got = [o.cpu().numpy() for o in mops.tsp_3opt_best(dd, pp, torch.from_numpy(cur).to(DEV), slices=slices)]
    for b in range(B):
        want = o3.one_pass_exact_grouped(d, perms[b], cur[b])
        if N <= 12:
            assert want == o3.one_pass(d, perms[b], cur[b]), f"the two oracles disagree b={b} " + tag
        assert tuple(int(g[b]) for g in got[:4]) + (float(got[4][b]),) == want, f"exact pass b={b} scale={scale} " + tag
    if kind != "asym":
        got = [o.cpu().numpy() for o in mops.tsp_3opt_best(dd, pp, slices=slices)]
        for b in range(B):
            want = o3.one_pass(d, perms[b], None)
            assert tuple(int(g[b]) for g in got[:4]) + (float(got[4][b]),) == want, f"delta pass b={b} " + tag
    if it % 3 == 0 and N <= 25:
        tour = [int(v) + 1 for v in perms[0]] + [int(perms[0][0]) + 1]
        rs = int(rng.choice([-1, 1, 3]))
        r, dist = o3.local_search(d, tour, true[0], rs)
        r2, dist2 = t3.local_search_3_opt(d, [tour, true[0]], recursive_seeding=rs, verbose=False, device=DEV)
        assert r2 == r and dist2 == dist, f"local_search_3_opt rs={rs} " + tag
    it += 1
print(f"fuzz_tsp3opt: {it} random configurations, no mismatch")
