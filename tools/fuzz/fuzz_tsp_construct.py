"""Differential fuzz of the tour constructors (rls_tsp_neighbour_chain, rls_tsp_grow_2opt, methods/tsp_nn.py / tsp_ins_n.py /
tsp_ins_f.py / tsp_ins_c.py) against the numpy restatement of tests/tsp_construct_oracle.py: random N in [2, 40], Euclidean /
integer (ties everywhere) / asymmetric matrices, random starts, random (m_seed, m_end, first_m), now and then a max_passes the
row runs into -- chains, tours, float64 lengths, pass counts and status bit for bit; every third round one of the four public
functions.  `python tools/fuzz/fuzz_tsp_construct.py [seconds] [seed]`."""
import sys, time
import numpy as np, torch
sys.path.insert(0, ".")
from tests import tsp_construct_oracle as oc
from rlsolver_amd import ops_mcpg_tsp as mops
from rlsolver_amd.methods import tsp_ins_c, tsp_ins_f, tsp_ins_n, tsp_nn

DEV = torch.device("cuda:0")
budget = float(sys.argv[1]) if len(sys.argv) > 1 else 60.0
rng = np.random.RandomState(int(sys.argv[2]) if len(sys.argv) > 2 else 0)
t_end = time.time() + budget
it = 0
while time.time() < t_end:
    N = int(rng.choice([rng.randint(2, 7), rng.randint(7, 20), rng.randint(20, 41)]))
    kind = rng.choice(["euclid", "integer", "asym"])
    c = rng.rand(N, 2) * 100
    d = np.sqrt(((c[:, None] - c[None]) ** 2).sum(-1))
    if kind == "integer":
        d = np.rint(d / 20.0)
    elif kind == "asym":
        d = d + rng.rand(N, N) * 10
    np.fill_diagonal(d, 0)
    dd = torch.from_numpy(d).to(DEV)
    S = int(rng.choice([1, 2, rng.randint(3, 9)]))
    far = bool(rng.randint(0, 2))
    starts = rng.randint(0, N, size=S)
    tag = f"it={it} N={N} kind={kind} S={S} far={far}"
    chains, st = mops.tsp_neighbour_chain(dd, torch.from_numpy(starts).to(DEV), far)
    chains = chains.cpu().numpy()
    assert not st.cpu().numpy().any(), "chain status " + tag
    for s in range(S):
        assert np.array_equal(chains[s], oc.neighbour_chain(d, starts[s], far)), f"chain s={s} " + tag
    order = chains if rng.randint(0, 2) else np.stack([rng.permutation(N) for _ in range(S)])
    m_seed = int(rng.randint(2, N + 1))
    m_end = int(rng.randint(m_seed, N + 1))
    first_m = int(rng.randint(2, m_end + 2))
    max_passes = int(rng.choice([N * N, N * N, 1, 2]))
    tag += f" m_seed={m_seed} m_end={m_end} first_m={first_m} max_passes={max_passes}"
    tours, length, passes, st = (o.cpu().numpy() for o in mops.tsp_grow_2opt(dd, torch.from_numpy(order).to(DEV), m_seed, m_end, first_m, max_passes))
    for s in range(S):
        wt, wl, wp, ws = oc.grow(d, order[s], m_seed, m_end, first_m, max_passes)
        assert int(st[s]) == ws and int(passes[s]) == wp, f"passes / status s={s}: {int(passes[s])}, {int(st[s])} != {wp}, {ws} " + tag
        assert np.array_equal(tours[s], wt) and float(length[s]) == wl, f"tour / length s={s} " + tag
    if it % 3 == 0 and N <= 25:
        loc = int(rng.choice([-1, rng.randint(1, N + 1)]))
        which = int(rng.randint(0, 5))
        if which == 0:
            ls = bool(rng.randint(0, 2))
            got, want = tsp_nn.nearest_neighbour(d, loc, ls, False, device=DEV), oc.nearest_neighbour(d, loc, ls)
        elif which == 1:
            got, want = tsp_ins_n.nearest_insertion(d, loc, False, device=DEV), oc.nearest_insertion(d, loc)
        elif which == 2:
            got, want = tsp_ins_f.farthest_insertion(dd, loc, False, device=DEV), oc.farthest_insertion(d, loc)
        elif N <= 14 and np.argmax(d) // N != np.argmax(d) % N:
            import contextlib, io
            with contextlib.redirect_stdout(io.StringIO()):
                got = tsp_ins_c.cheapest_insertion(d, False, device=DEV)
            want = oc.cheapest_insertion(d)
        else:
            got = want = None
        assert got == want, f"public function {which} loc={loc} " + tag
    it += 1
print(f"fuzz_tsp_construct: {it} random configurations, no mismatch")
