#!/usr/bin/env python3
"""Record tests/golden/tsp_construct.npz from the reference's own tour constructors (rlsolver/methods_problem_specific/TSP/nn.py,
ins_n.py, ins_f.py, ins_c.py), imported by path and run on the CPU.  Only data is written: matrices, routes, distances, and the
public names and parameter names of the four files.

    PYTHONDONTWRITEBYTECODE=1 python tools/gen_golden.py --only tsp_construct        (or: python tools/gen_golden_tsp_construct.py)

Cases (every random draw from one explicit RandomState); fn = nn (nearest_neighbour with its local search), nn0 (without), ins_n,
ins_f (initial_location = -1 and every single start where `starts` says all), ins_c:
  sym2 .. sym6, asym2 .. asym6: entries in {1, 2, 3}, ties everywhere -- all starts, all functions;
  uniform12: 12 seeded Euclidean points -- all starts, all functions;
  berlin16: the first 16 cities of berlin52 -- all starts, the chain-based functions;
  berlin52: initial_location = 1 only, the chain-based functions (seconds each in the reference);
  berlin20: cheapest_insertion on the first 20 cities;
  gon12: a regular 12-gon, whose rotated and reflected tours tie in exact arithmetic and differ only in rounding -- all starts, all
      functions.
The script also times the reference's single-start calls on berlin52 (`reference_seconds/<fn>`): figures to quote beside the
kernels', never targets."""
import contextlib
import importlib.util
import inspect
import io
import os
import sys
import time

import numpy as np

TOOLS = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(TOOLS)
for p in (TOOLS, ROOT, os.path.join(ROOT, "tests")):
    if p not in sys.path:
        sys.path.insert(0, p)

KEY = "tsp_construct"
FILES = {"nn": "nn.py", "ins_n": "ins_n.py", "ins_f": "ins_f.py", "ins_c": "ins_c.py"}


def euclid(coords):
    return np.sqrt(((coords[:, None, :] - coords[None, :, :]) ** 2).sum(-1))


def generate(save):
    import gen_golden
    from rlsolver.methods.ISCO import util_TSP
    mods = {}
    for tag, fname in FILES.items():
        spec = importlib.util.spec_from_file_location("ref_" + tag, os.path.join(gen_golden.REF, "rlsolver", "methods_problem_specific", "TSP", fname))
        mods[tag] = importlib.util.module_from_spec(spec)
        spec.loader.exec_module(mods[tag])
    rng = np.random.RandomState(20261022)
    out = {}

    def quiet(fn, *a, **k):
        with contextlib.redirect_stdout(io.StringIO()):       # (cheapest_insertion prints its distance whatever `verbose` says)
            t0 = time.perf_counter()
            route, dist = fn(*a, **k)
        return np.asarray(route, dtype=np.int64), np.float64(dist), time.perf_counter() - t0

    calls = {"nn": lambda d, loc: quiet(mods["nn"].nearest_neighbour, d, loc, True, False),
             "nn0": lambda d, loc: quiet(mods["nn"].nearest_neighbour, d, loc, False, False),
             "ins_n": lambda d, loc: quiet(mods["ins_n"].nearest_insertion, d, loc, False),
             "ins_f": lambda d, loc: quiet(mods["ins_f"].farthest_insertion, d, loc, False)}

    def small(n, symmetric):
        d = rng.randint(1, 4, size=(n, n)).astype(np.float64)
        if symmetric:
            d = np.triu(d, 1) + np.triu(d, 1).T
        np.fill_diagonal(d, 0.0)
        return d

    berlin = euclid(np.asarray(util_TSP.read_tsp_file(os.path.join(gen_golden.DATA, "tsplib", "berlin52.tsp")), dtype=np.float64))
    a = 2.0 * np.pi * np.arange(12) / 12.0
    cases = {}
    for n in range(2, 7):
        cases[f"sym{n}"] = (small(n, True), "all", True)
        cases[f"asym{n}"] = (small(n, False), "all", True)
    cases["uniform12"] = (euclid(rng.rand(12, 2) * 100.0), "all", True)
    cases["gon12"] = (euclid(np.stack([100.0 * np.cos(a), 100.0 * np.sin(a)], axis=1)), "all", True)
    cases["berlin16"] = (np.ascontiguousarray(berlin[:16, :16]), "all", False)
    cases["berlin52"] = (berlin, "one", False)
    cases["berlin20"] = (np.ascontiguousarray(berlin[:20, :20]), "none", True)
    seconds = {}
    for name, (d, starts, cheapest) in cases.items():
        n = d.shape[0]
        out[f"{name}/distance_f64"] = d
        locs = {"all": [-1] + list(range(1, n + 1)), "one": [1], "none": []}[starts]
        out[f"{name}/locations"] = np.asarray(locs, dtype=np.int64)
        for fn, call in calls.items():
            got = [call(d, loc) for loc in locs]
            if locs:                                            # row k: initial_location = locations[k]
                out[f"{name}/{fn}/routes"] = np.stack([g[0] for g in got])
                out[f"{name}/{fn}/distances"] = np.asarray([g[1] for g in got], dtype=np.float64)
            if name == "berlin52":
                seconds[fn] = got[0][2]
        if cheapest:
            route, dist, sec = quiet(mods["ins_c"].cheapest_insertion, d, False)
            out[f"{name}/ins_c/route"] = route
            out[f"{name}/ins_c/distance"] = dist
            if name == "berlin20":
                seconds["ins_c_berlin20"] = sec
        out[f"{name}/cheapest"] = np.int64(cheapest)
        print(f"{name}: n = {n}, starts {starts}, cheapest {cheapest}")
    out["names"] = np.asarray(list(cases))
    for fn, sec in seconds.items():
        out[f"reference_seconds/{fn}"] = np.float64(sec)
        print(f"the reference's {fn} (berlin52, one start unless named otherwise): {sec:.2f} s on this CPU")
    # the public surface of the four files, as data: the functions each defines and their parameter names
    for tag, mod in mods.items():
        fns = [f for f, obj in vars(mod).items() if inspect.isfunction(obj) and obj.__module__ == mod.__name__]
        out[f"surface/{tag}/functions"] = np.asarray(fns)
        for f in fns:
            out[f"surface/{tag}/{f}/parameters"] = np.asarray(list(inspect.signature(getattr(mod, f)).parameters))
    out["source"] = np.array("the reference's nn.py / ins_n.py / ins_f.py / ins_c.py on the CPU: <case>/<fn>/{routes, distances}[k] = fn(distance_f64, "
                             "initial_location=locations[k]) (nn0: local_search=False); <case>/ins_c/{route, distance} = cheapest_insertion(distance_f64); "
                             "surface/<file>: its functions and their parameter names")
    save(KEY, **out)


if __name__ == "__main__":
    import gen_golden
    gen_golden._CURRENT["key"] = KEY
    generate(gen_golden.save)
