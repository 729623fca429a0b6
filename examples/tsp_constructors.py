#!/usr/bin/env python3
"""The four tour constructors of methods_problem_specific/TSP (nn.py, ins_n.py, ins_f.py, ins_c.py) on one instance -- the
drop-ins rlsolver_amd.methods.tsp_nn / tsp_ins_n / tsp_ins_f / tsp_ins_c.

    python examples/tsp_constructors.py --file berlin52.tsp        # a TSPLIB file, or plain lines of "x y" / "id x y"
    python examples/tsp_constructors.py --cities 100 --seed 3      # seeded uniform points in the unit square x 100

Each function runs from every start (cheapest_insertion has none): the neighbour chains of all starts in one launch, then all
tours grown and 2-opted at every size in one more.  Routes and distances are bit-identical to the reference's functions, which
re-sum every 2-opt candidate of every insertion in Python (farthest_insertion on berlin52: seconds per start)."""
import argparse
import contextlib
import io
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
    if len(rows) < 2:
        raise SystemExit(f"{path}: fewer than 2 coordinate lines")
    return np.asarray(rows, dtype=np.float64)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--file", default=None)
    ap.add_argument("--cities", type=int, default=52)
    ap.add_argument("--seed", type=int, default=0)
    ap.add_argument("--no-cheapest", action="store_true", help="skip cheapest_insertion (N - 2 launches of up to N - 2 rows)")
    a = ap.parse_args()

    import numpy as np
    import torch
    from rlsolver_amd.methods.tsp_ins_c import cheapest_insertion
    from rlsolver_amd.methods.tsp_ins_f import farthest_insertion
    from rlsolver_amd.methods.tsp_ins_n import nearest_insertion
    from rlsolver_amd.methods.tsp_nn import distance_calc, nearest_neighbour
    dev = torch.device("cuda:0")
    coords = read_coords(a.file) if a.file else np.random.RandomState(a.seed).rand(a.cities, 2) * 100.0
    n = len(coords)
    d = np.sqrt(((coords[:, None, :] - coords[None, :, :]) ** 2).sum(-1))
    print(f"{a.file or f'uniform-{n} (seed {a.seed})'}: {n} cities")
    nearest_neighbour(d, 1, True, False, device=dev)                                   # (the first call loads the kernels)
    runs = [("nearest_neighbour, no local search", lambda: nearest_neighbour(d, -1, False, False, device=dev)),
            ("nearest_neighbour", lambda: nearest_neighbour(d, -1, True, False, device=dev)),
            ("nearest_insertion", lambda: nearest_insertion(d, -1, False, device=dev)),
            ("farthest_insertion", lambda: farthest_insertion(d, -1, False, device=dev))]
    if not a.no_cheapest:
        runs.append(("cheapest_insertion", lambda: cheapest_insertion(d, False, device=dev)))
    for name, run in runs:
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        with contextlib.redirect_stdout(io.StringIO()):       # (cheapest_insertion prints its distance, as the reference does)
            route, dist = run()
        torch.cuda.synchronize()
        assert dist == distance_calc(d, [route, 0.0]) and sorted(route[:-1]) == list(range(1, n + 1)) and route[0] == route[-1]
        print(f"  {name}: {dist:.2f} from city {route[0]}, {time.perf_counter() - t0:.3f} s")
    print("tsp_constructors: ok")


if __name__ == "__main__":
    main()
