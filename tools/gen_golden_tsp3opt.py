#!/usr/bin/env python3
"""Record tests/golden/tsp_3opt.npz from the reference's own 3-opt (rlsolver/methods_problem_specific/TSP/opt_3.py:
local_search_3_opt, segments_3_opt, distance_calc), imported by path and run on the CPU.  Only data is written: matrices,
tours, distances, lists of triples.

    PYTHONDONTWRITEBYTECODE=1 python tools/gen_golden.py --only tsp_3opt        (or: python tools/gen_golden_tsp3opt.py)

Cases (every random draw from one explicit RandomState):
  a5, int9 (distances rounded to integers: ties everywhere), uniform12, asym6, asym16: recursive_seeding = 1, 2, .. until
      a pass changes nothing -- so every pass's tour and distance is on record -- and -1;
  uniform30: -1 only;  berlin52: 1, 2, 3 only (a pass of the reference takes seconds there);
  contract cases: a locally optimal 7-city tour handed over with 1.5 x its length, the same with 0.0, three cities with 1e9,
      recursive_seeding = 0;
  segments_3_opt(n) for n = 3, 4, 5, 12; distance_calc of every start tour;
  planted700: 700 points on a circle visited in order with blocks S1 and S2 of a late triple reversed -- the one move that
      restores the optimum, whose key passes 2^31 -- and the (i, j, k, trial, value) the delta ranking must return, computed
      here once by tests/tsp3opt_oracle.py (the matrix is rebuilt from the stored coordinates).
The script also times one berlin52 pass of the reference (`reference_seconds_per_berlin52_pass`): a figure to quote beside
the kernel's, never a target."""
import importlib.util
import os
import sys
import time

import numpy as np

TOOLS = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(TOOLS)
for p in (TOOLS, ROOT, os.path.join(ROOT, "tests")):
    if p not in sys.path:
        sys.path.insert(0, p)

KEY = "tsp_3opt"
PLANTED = (600, 640, 680, 4)          # (i, j, k, trial abC): both blocks 40 cities long


def euclid(coords):
    return np.sqrt(((coords[:, None, :] - coords[None, :, :]) ** 2).sum(-1))


def planted700():
    """(coords, matrix, the tour to hand over: the circle in order with S1 and S2 of PLANTED reversed)"""
    a = 2.0 * np.pi * np.arange(700) / 700.0
    coords = np.stack([1000.0 * np.cos(a), 1000.0 * np.sin(a)], axis=1)
    i, j, k, _ = PLANTED
    tour = np.arange(700)
    tour[i + 1:j + 1] = tour[i + 1:j + 1][::-1].copy()
    tour[j + 1:k + 1] = tour[j + 1:k + 1][::-1].copy()
    return coords, euclid(coords), tour


def generate(save):
    import gen_golden
    import tsp3opt_oracle as o3
    from rlsolver.methods.ISCO import util_TSP
    spec = importlib.util.spec_from_file_location(
        "ref_opt3", os.path.join(gen_golden.REF, "rlsolver", "methods_problem_specific", "TSP", "opt_3.py"))
    opt3 = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(opt3)
    rng = np.random.RandomState(20261021)
    out = {}

    def tsplib(name):
        return euclid(np.asarray(util_TSP.read_tsp_file(os.path.join(gen_golden.DATA, "tsplib", name + ".tsp")), dtype=np.float64))

    def asym(n):
        d = euclid(rng.rand(n, 2) * 100.0) + rng.rand(n, n) * 20.0
        np.fill_diagonal(d, 0.0)
        return d

    matrices = {"a5": tsplib("a5"), "int9": np.rint(euclid(rng.rand(9, 2) * 10.0)), "uniform12": euclid(rng.rand(12, 2) * 100.0),
                "asym6": asym(6), "asym16": asym(16), "uniform30": euclid(rng.rand(30, 2) * 100.0), "berlin52": tsplib("berlin52")}
    names, seconds = [], 0.0
    for name, d64 in matrices.items():
        n = d64.shape[0]
        out[f"{name}/distance_f64"] = d64
        perm = rng.permutation(n)
        tour = [int(c) + 1 for c in perm] + [int(perm[0]) + 1]
        start = [tour, float(opt3.distance_calc(d64, [tour, 0.0]))]
        out[f"{name}/start_tour"] = np.asarray(tour, dtype=np.int64)
        out[f"{name}/start_distance"] = np.float64(start[1])
        if name == "uniform30":
            seedings = [-1]
        elif name == "berlin52":
            seedings = [1, 2, 3]
        else:
            seedings, last, rs = [-1], None, 1
            while True:                                         # until a pass changes nothing
                route, dist = opt3.local_search_3_opt(d64, start, recursive_seeding=rs, verbose=False)
                seedings.append(rs)
                if last is not None and (route, dist) == last:
                    break
                last, rs = (route, dist), rs + 1
        for rs in seedings:
            t0 = time.perf_counter()
            route, dist = opt3.local_search_3_opt(d64, start, recursive_seeding=rs, verbose=False)
            if name == "berlin52" and rs == 1:
                seconds = time.perf_counter() - t0
            out[f"{name}/rs{rs}/tour"] = np.asarray(route, dtype=np.int64)
            out[f"{name}/rs{rs}/distance"] = np.float64(dist)
        out[f"{name}/seedings"] = np.asarray(seedings, dtype=np.int64)
        names.append(name)
        print(f"{name}: n = {n}, recursive_seeding {seedings}")
    out["names"] = np.asarray(names)

    # the contract cases
    d7 = euclid(rng.rand(7, 2) * 100.0)
    perm = rng.permutation(7)
    tour = [int(c) + 1 for c in perm] + [int(perm[0]) + 1]
    opt_route, opt_dist = opt3.local_search_3_opt(d7, [tour, float(opt3.distance_calc(d7, [tour, 0.0]))], recursive_seeding=-1, verbose=False)
    d3 = euclid(rng.rand(3, 2) * 100.0)
    contract = {"inflated": (d7, opt_route, 1.5 * float(opt_dist), -1), "zero": (d7, opt_route, 0.0, -1),
                "zero_start": (d7, tour, 0.0, 2), "three": (d3, [2, 3, 1, 2], 1e9, -1),
                "no_pass": (d7, tour, 123.25, 0)}
    for tag, (d, route_in, cur, rs) in contract.items():
        route, dist = opt3.local_search_3_opt(d, [list(route_in), cur], recursive_seeding=rs, verbose=False)
        out[f"contract/{tag}/distance_f64"] = d
        out[f"contract/{tag}/start_tour"] = np.asarray(route_in, dtype=np.int64)
        out[f"contract/{tag}/start_distance"] = np.float64(cur)
        out[f"contract/{tag}/seeding"] = np.int64(rs)
        out[f"contract/{tag}/tour"] = np.asarray(route, dtype=np.int64)
        out[f"contract/{tag}/distance"] = np.float64(dist)
    assert list(out["contract/inflated/tour"]) == list(opt_route) and out["contract/inflated/distance"] == opt_dist
    assert list(out["contract/zero/tour"]) == list(opt_route) and out["contract/zero/distance"] == 0.0
    out["contract_cases"] = np.asarray(list(contract))

    for n in (3, 4, 5, 12):
        out[f"segments/n{n}"] = np.asarray(opt3.segments_3_opt(n), dtype=np.int64)

    coords, d700, tour700 = planted700()
    t0 = time.perf_counter()
    i, j, k, r, v = o3.one_pass(d700, tour700, None)
    print(f"planted700: oracle (delta ranking) {(i, j, k, r, v)} in {time.perf_counter() - t0:.0f} s")
    assert (i, j, k, r) == PLANTED and v < 0
    assert np.array_equal(o3.apply_move(tour700, i, j, k, r), np.arange(700))
    out["planted700/coords"] = coords
    out["planted700/tour"] = tour700.astype(np.int64)
    out["planted700/answer"] = np.asarray([i, j, k, r], dtype=np.int64)
    out["planted700/value"] = np.float64(v)
    out["reference_seconds_per_berlin52_pass"] = np.float64(seconds)
    out["source"] = np.array("the reference's opt_3.py on the CPU: <case>/rs<k>/{tour, distance} = local_search_3_opt(distance_f64, [start_tour, "
                             "start_distance], recursive_seeding=k); contract/<case> likewise with its `seeding`; segments/n<k> = "
                             "segments_3_opt(k); planted700/{answer, value} by tests/tsp3opt_oracle.py")
    print(f"the reference's berlin52 pass: {seconds:.1f} s on this CPU")
    save(KEY, **out)


if __name__ == "__main__":
    import gen_golden
    gen_golden._CURRENT["key"] = KEY
    generate(gen_golden.save)
