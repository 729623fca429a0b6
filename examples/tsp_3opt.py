#!/usr/bin/env python3
"""2-opt, then the reference's 3-opt, on one TSP instance -- the two drop-ins for methods_problem_specific/TSP/opt_2.py and
opt_3.py (rlsolver_amd.methods.tsp_opt_2 / tsp_opt_3), each pass one kernel.

    python examples/tsp_3opt.py --coords berlin52.tsp          # a TSPLIB file, or plain lines of "x y" / "id x y"
    python examples/tsp_3opt.py --cities 100 --seed 3          # a seeded uniform instance in the unit square x 100

From a seeded random tour: local_search_2_opt to convergence, then local_search_3_opt from its result; prints lengths, passes
and seconds.  Both are bit-identical to the reference's functions, which re-sum every candidate tour in Python (a berlin52
pass of its 3-opt: seconds; here: well under a millisecond of kernel time)."""
import argparse
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def read_coords(path):
    import numpy as np
    rows = []
    for line in open(path):
        parts = line.replace(",", " ").split()
        try:
            nums = [float(v) for v in parts]
        except ValueError:
            continue                                         # TSPLIB keywords, EOF
        if len(nums) in (2, 3):
            rows.append(nums[-2:])
    if len(rows) < 3:
        raise SystemExit(f"{path}: fewer than 3 coordinate lines")
    return np.asarray(rows, dtype=np.float64)


def converge(search, d, tour, dev):
    """(route, distance, passes): one pass at a time, so the passes can be counted"""
    passes = 0
    while True:
        route, dist = search(d, tour, recursive_seeding=1, verbose=False, device=dev)
        if dist >= tour[1]:
            return tour[0], tour[1], passes
        tour, passes = [route, dist], passes + 1


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--coords", default=None)
    ap.add_argument("--cities", type=int, default=52)
    ap.add_argument("--seed", type=int, default=0)
    a = ap.parse_args()

    import numpy as np
    import torch
    from rlsolver_amd.methods.tsp_opt_2 import distance_calc, local_search_2_opt
    from rlsolver_amd.methods.tsp_opt_3 import local_search_3_opt, local_search_3_opt_batch
    dev = torch.device("cuda:0")
    rng = np.random.RandomState(a.seed)
    coords = read_coords(a.coords) if a.coords else rng.rand(a.cities, 2) * 100.0
    n = len(coords)
    d = np.sqrt(((coords[:, None, :] - coords[None, :, :]) ** 2).sum(-1))
    perm = rng.permutation(n)
    route = [int(c) + 1 for c in perm] + [int(perm[0]) + 1]
    tour = [route, distance_calc(d, [route, 0.0])]
    print(f"{a.coords or f'uniform-{n} (seed {a.seed})'}: {n} cities, random tour {tour[1]:.2f}")
    local_search_3_opt(d, tour, recursive_seeding=1, verbose=False, device=dev)        # (the first call loads the kernels)
    for name, search in (("2-opt", local_search_2_opt), ("3-opt", local_search_3_opt)):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        r, dist, passes = converge(search, d, tour, dev)
        torch.cuda.synchronize()
        assert dist == distance_calc(d, [r, 0.0]) and sorted(r[:-1]) == list(range(1, n + 1))
        print(f"  {name}: {tour[1]:.2f} -> {dist:.2f} in {passes} improving passes, {time.perf_counter() - t0:.3f} s")
        tour = [r, dist]
    # many tours at once, delta ranking: 256 random starts of the same instance
    perms = torch.from_numpy(np.stack([rng.permutation(n) for _ in range(256)])).to(dev)
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    _, lens = local_search_3_opt_batch(torch.from_numpy(d).to(dev), perms)
    torch.cuda.synchronize()
    print(f"  3-opt alone from 256 random tours (batch form, delta ranking): best {float(lens.min()):.2f}, mean {float(lens.mean()):.2f}, "
          f"{time.perf_counter() - t0:.3f} s")
    print("tsp_3opt: ok")


if __name__ == "__main__":
    main()
