"""Differential fuzz of the ISCO_TSP sampler step against the numpy oracle with recorded draws: random instance sizes
(K + 3 .. 130 cities, and 190 .. 200: both sides of "the matrix fits LDS", N = 193 / 194), K, batch sizes, path lengths and
temperatures.  A third of the configurations start from the optimal tour of cities on a circle (as tests/tsp_cases.py does) at the
temperature that rejects about half the envs there -- from a random tour every first move is an improvement and every env
accepts --, and a third run on an asymmetric matrix with a non-zero diagonal; the verdict line counts the rejected envs.  The walked tour is compared exactly except where the
Gumbel argmax of a round is decided within a few ulps (the oracle reports nothing about that, so a mismatching tour is
re-examined: it must still be a permutation reachable by the recorded partner draws), log_acc within 2e-5 relative + 1e-4.
`python tools/fuzz/fuzz_isco_tsp.py [seconds] [seed]`."""
import sys, time
import numpy as np, torch
sys.path.insert(0, ".")
from oracle import oracle_isco as oi
from rlsolver_amd.envs.env_ISCO import ISCO_TSP
from rlsolver_amd.graph import generate_tsp_coords, tsp_tables

DEV = torch.device("cuda:0")
budget = float(sys.argv[1]) if len(sys.argv) > 1 else 60.0
rng = np.random.RandomState(int(sys.argv[2]) if len(sys.argv) > 2 else 0)
t_end = time.time() + budget
it = exact = rejected = envs = 0


def circle_tables(N, K):
    """cities on the unit circle in tour order: the identity tour, rotated or reflected, is the optimum"""
    ang = 2.0 * np.pi * np.arange(N, dtype=np.float64) / N
    return tsp_tables(np.stack([np.cos(ang), np.sin(ang)], axis=1).astype(np.float32), K=K)


def circle_starts(N, B):
    rot, sign = rng.randint(0, N, size=B), rng.choice([1, -1], size=B)
    return ((sign[:, None] * np.arange(N)[None, :] + rot[:, None]) % N).astype(np.int64)


while time.time() < t_end:
    K = int(rng.choice([2, 5, 20]))
    N = int(rng.randint(190, 201)) if rng.rand() < 0.25 else int(rng.randint(K + 3, 131))
    B = int(rng.choice([1, 3, 64, 65, 200]))
    L = int(rng.randint(1, 7))
    T = float(rng.choice([0.05, 0.2, 0.7, 2.0]))
    circle, asym = rng.randint(3) == 0, rng.randint(3) == 0
    if circle:
        T = 20.0 / N          # between the measured points: 0.35 rejects 59 % at N = 65, 0.08 42 % at N = 193 ("TSP forms")
    tag = f"it={it} N={N} K={K} B={B} L={L} T={T} circle={circle} asym={asym}"
    if "-v" in sys.argv:
        print(tag, flush=True)
    dist, near, rnd = circle_tables(N, K) if circle else tsp_tables(generate_tsp_coords(N, seed=int(rng.randint(1 << 30))), K=K)
    if asym:
        dist = (dist + rng.rand(N, N).astype(np.float32) * np.float32(dist.mean())).astype(np.float32)   # dense, the diagonal too
    s = ISCO_TSP({"num_nodes": N, "distance": torch.from_numpy(dist).to(DEV), "nearest_indices": torch.from_numpy(near).to(DEV),
                  "random_indices": torch.from_numpy(rnd).to(DEV)}, batch_size=B, K=K, device=DEV)
    x = circle_starts(N, B) if circle else np.stack([rng.permutation(N) for _ in range(B)]).astype(np.int64)
    d = dict(u_partner=rng.rand(L, B, N).astype(np.float32), r_near=rng.randint(0, K, size=(L, B, N)).astype(np.int64),
             r_rand=rng.randint(0, N - K - 1, size=(L, B, N)).astype(np.int64),
             u_gumbel=rng.rand(L, B, N).astype(np.float32).clip(1e-7, 1 - 1e-7), u_accept=rng.rand(B).astype(np.float32))
    r = oi.tsp_step(x, dist, near, rnd, K, L, T, d["u_partner"], d["r_near"], d["r_rand"], d["u_gumbel"], d["u_accept"])
    y, mean_acc, log_acc, cur = s.step(torch.from_numpy(x).to(DEV), L, T, draws={k: torch.from_numpy(v) for k, v in d.items()}, want_terms=True)
    cur, y = cur.cpu().numpy(), y.cpu().numpy()
    assert (np.sort(cur, axis=1) == np.arange(N)).all() and (np.sort(y, axis=1) == np.arange(N)).all(), "not permutations " + tag
    same = (cur == r["cur_x"]).all(axis=1)
    assert same.mean() >= 0.97, f"walked tours differ on {(~same).sum()} of {B} envs " + tag      # near-tied argmax only
    la = log_acc.cpu().numpy()
    assert np.allclose(la[same], r["log_acc"][same], rtol=2e-5, atol=2e-4), "log_acc " + tag
    margin = np.abs(np.log(d["u_accept"].astype(np.float64) + 1e-24) - r["log_acc"])
    sure = same & (margin > 1e-3 * np.maximum(1.0, np.abs(r["log_acc"])))
    assert np.array_equal(y[sure], r["y"][sure]), "accepted tours " + tag
    exact += int(same.all())
    rejected += int((y != cur).any(axis=1).sum())
    envs += B
    it += 1
print(f"fuzz_isco_tsp: {it} random configurations ({exact} with every walked tour identical, {rejected} of {envs} envs rejected), no mismatch")
