"""Times of the tour constructors (rls_tsp_neighbour_chain, rls_tsp_grow_2opt; methods/tsp_nn.py, tsp_ins_n.py, tsp_ins_f.py,
tsp_ins_c.py), medians of 7 (min, max):

  1. each public function from all starts on berlin52 (its coordinates given with --file; skipped without) and on 100 uniform
     points, wall clock with a device synchronisation on both sides (a call is two launches and the host reads between and after
     them), beside the reference's own single-start seconds as recorded by the fixture's generator (tests/golden/tsp_construct.npz:
     Python on the generator's CPU, berlin52 from city 1; x N for all starts -- an extrapolation, said so in the output);
  2. full tours (m_seed = first_m = m_end = N): ONE on-device convergence (hipEvents around the launch) beside the host loop of
     local_search_2_opt_batch(exact=True) -- a launch, a gather and a host read per pass (wall clock) -- on the nearest-neighbour
     tours of every start and on 4096 random 100-city tours;
  3. the two kernels alone (hipEvents): the chains of all starts, and grow-and-converge from them.

    python tools/timing/tsp_constructors.py [--file berlin52.tsp] > profiles/tsp_construct_kernels.txt"""
import argparse
import contextlib
import io
import os
import sys
import time

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)
from rlsolver_amd import _abi, ops_mcpg_tsp as mops  # noqa: E402
from rlsolver_amd.methods import tsp_construct as tc, tsp_ins_c, tsp_ins_f, tsp_ins_n, tsp_nn, tsp_opt_2  # noqa: E402

REPS = 7
DEV = torch.device("cuda:0")


def timed(fn, events=True):
    ms = []
    for _ in range(REPS):
        torch.cuda.synchronize()
        if events:
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record()
            fn()
            e1.record()
            torch.cuda.synchronize()
            ms.append(e0.elapsed_time(e1))
        else:
            t0 = time.perf_counter()
            fn()
            torch.cuda.synchronize()
            ms.append((time.perf_counter() - t0) * 1e3)
    ms.sort()
    return f"{ms[len(ms) // 2]:.3f} ({ms[0]:.3f}, {ms[-1]:.3f})"


def quiet(fn):
    def run():
        with contextlib.redirect_stdout(io.StringIO()):
            return fn()
    return run


def euclid(c):
    return np.sqrt(((c[:, None, :] - c[None, :, :]) ** 2).sum(-1))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--file", default=None, help="coordinates of berlin52 (TSPLIB or plain lines of x y)")
    a = ap.parse_args()
    print(f"# python tools/timing/tsp_constructors.py  -- ms, medians of {REPS} (min, max)")
    z = np.load(os.path.join(ROOT, "tests", "golden", "tsp_construct.npz"), allow_pickle=False)
    ref = {k: float(z[f"reference_seconds/{k}"]) for k in ("nn", "ins_n", "ins_f")}
    print("# the reference on berlin52 from city 1 (Python, on the CPU that generated the fixture; not a target): "
          + ", ".join(f"{k} {v:.2f} s" for k, v in ref.items()) + f"; cheapest_insertion on its first 20 cities {float(z['reference_seconds/ins_c_berlin20']):.2f} s")
    instances = {}
    if a.file:
        sys.path.insert(0, os.path.join(ROOT, "examples"))
        from tsp_constructors import read_coords
        instances["berlin52"] = euclid(read_coords(a.file))
    else:
        instances["berlin52 (the fixture's matrix)"] = z["berlin52/distance_f64"]
    instances["uniform100"] = euclid(np.random.RandomState(100).rand(100, 2) * 100.0)

    print("\n## 1. the public functions, all starts, wall clock")
    print("instance function | ms | the reference, single start x N (extrapolated)")
    for name, d in instances.items():
        n = d.shape[0]
        dd = torch.from_numpy(np.ascontiguousarray(d)).to(DEV)
        runs = [("nearest_neighbour", lambda: tsp_nn.nearest_neighbour(dd, -1, True, False, device=DEV), "nn"),
                ("nearest_insertion", lambda: tsp_ins_n.nearest_insertion(dd, -1, False, device=DEV), "ins_n"),
                ("farthest_insertion", lambda: tsp_ins_f.farthest_insertion(dd, -1, False, device=DEV), "ins_f"),
                ("cheapest_insertion", quiet(lambda: tsp_ins_c.cheapest_insertion(dd, False, device=DEV)), None)]
        for fn, run, key in runs:
            run()
            beside = f"{ref[key] * n:.0f} s" if key and n == 52 else "-"
            print(f"{name} {fn} | {timed(run, events=False)} | {beside}")

    print("\n## 2. full tours: one on-device convergence beside the host loop of one launch per pass")
    print("tours | passes (max over rows) | rls_tsp_grow_2opt, one launch | local_search_2_opt_batch(exact=True), wall clock")
    cases = []
    for name, d in instances.items():
        dd = torch.from_numpy(np.ascontiguousarray(d)).to(DEV)
        n = d.shape[0]
        cases.append((f"{name}: {n} nearest-neighbour tours", dd, tc.neighbour_chains(dd, torch.arange(n, device=DEV))))
    d100 = torch.from_numpy(instances["uniform100"]).to(DEV)
    cases.append(("uniform100: 4096 random tours", d100, mops.rand_perms(4096, 100, 7, DEV)))
    for what, dd, perms in cases:
        n = dd.shape[0]
        out = [torch.zeros_like(perms), torch.zeros(len(perms), dtype=torch.float64, device=DEV), torch.zeros(len(perms), dtype=torch.int64, device=DEV),
               torch.zeros(len(perms), dtype=torch.int32, device=DEV)]
        grow = lambda: torch.ops.rlsolver_hip.tsp_grow_2opt(dd, perms, n, n, n, n * n, *out)      # noqa: E731
        grow()
        host = lambda: tsp_opt_2.local_search_2_opt_batch(dd, perms, exact=True)      # noqa: E731
        hp, hl = host()
        assert torch.equal(hp, out[0]) and torch.equal(hl, out[1])
        print(f"{what} | {int(out[2].max())} | {timed(grow)} | {timed(host, events=False)}")

    print("\n## 3. the kernels alone, all starts")
    print("instance | chains nearest | chains farthest | grow 2..N converged from 3 (nearest chains) | (farthest chains) | form")
    for name, d in instances.items():
        dd = torch.from_numpy(np.ascontiguousarray(d)).to(DEV)
        n = d.shape[0]
        starts = torch.arange(n, device=DEV)
        chain, st = torch.zeros((n, n), dtype=torch.int64, device=DEV), torch.zeros(n, dtype=torch.int32, device=DEV)
        cols = []
        for far in (0, 1):
            run = lambda: torch.ops.rlsolver_hip.tsp_neighbour_chain(dd, starts, far, chain, st)      # noqa: E731
            run()
            cols.append(timed(run))
        for far in (False, True):
            order = tc.neighbour_chains(dd, starts, far)
            out = [torch.zeros_like(order), torch.zeros(n, dtype=torch.float64, device=DEV), torch.zeros(n, dtype=torch.int64, device=DEV),
                   torch.zeros(n, dtype=torch.int32, device=DEV)]
            run = lambda: torch.ops.rlsolver_hip.tsp_grow_2opt(dd, order, 2, n, 3, n * n, *out)      # noqa: E731
            run()
            cols.append(timed(run) + f" [{int(out[2].sum())} passes in all]")
        f = _abi.tsp_grow_launch_form(n)
        print(f"{name} | " + " | ".join(cols) + f" | {f.waves} waves, matrix {'in LDS' if f.lds_d else 'through L2'}, {f.lds_bytes} B")


if __name__ == "__main__":
    main()
