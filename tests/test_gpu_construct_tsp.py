"""The reference's tour constructors on the device (rls_tsp_neighbour_chain, rls_tsp_grow_2opt, methods/tsp_construct.py and the
four modules over it) against the reference's own runs (tests/golden/tsp_construct.npz) and the numpy restatement of
tests/tsp_construct_oracle.py.  Every comparison is exact: int64 routes, pass counts and float64 bits, no tolerance.

Sizes: 2 to 5 cities with entries in {1, 2, 3} (ties everywhere, the smallest tours a pass exists for); 63 .. 66 cities (the chain's
lanes one city short of, at, and past a full wave; a pass's candidates past one round of the workgroup's 1024 threads); the largest N
whose matrix is staged in LDS and the first that reads it through L2, both asked of rls_tsp_grow_launch_form; 100 cities.

At import this file also registers the two ops' valid calls with tests/op_contract.py, so that the completeness test and the
refusal sweep of tests/test_gpu_op_contract.py cover them unchanged -- the mechanism of tests/test_gpu_3opt_tsp.py: pytest imports
test modules in name order while it collects, and this name sorts before that one.  The 5-second slice of
tools/fuzz/fuzz_tsp_construct.py runs in tests/test_gpu_fuzzers.py, which takes up every fuzzer of that folder."""
import contextlib
import functools
import io

import numpy as np
import pytest
import torch

from tests import op_contract as oc
from tests import tsp_construct_oracle as orc

gpu = pytest.mark.gpu
DEV = oc.DEV


def _mops():
    from rlsolver_amd import ops_mcpg_tsp
    return ops_mcpg_tsp


def _tc():
    from rlsolver_amd.methods import tsp_construct
    return tsp_construct


# ---------------------------------------------------------------------------------------------------------------- contract rows
@oc.row("tsp_neighbour_chain", outs=("chain", "status"))
def _():
    d64 = oc.tsp_env().distance.to(torch.float64)
    starts = oc.t(np.array([0, 5, oc.N - 1, 33, 7], dtype=np.int64))
    return oc.taken("tsp_neighbour_chain", lambda: _mops().tsp_neighbour_chain(d64, starts, True))


@oc.row("tsp_grow_2opt", outs=("tours", "length", "passes", "status"))
def _():
    d64 = oc.tsp_env().distance.to(torch.float64)
    return oc.taken("tsp_grow_2opt", lambda: _mops().tsp_grow_2opt(d64, oc.tours(), m_seed=5, first_m=oc.N - 1))


# ---------------------------------------------------------------------------------------------------------------- helpers
@functools.lru_cache(maxsize=None)
def matrix(n, kind, seed=0):
    """read-only float64 [n, n]: 'sym' Euclidean, 'asym' every oriented entry its own number, 'const' all ones"""
    r = oc.rng(1000 * n + seed)
    c = r.rand(n, 2) * 100.0
    d = np.sqrt(((c[:, None] - c[None]) ** 2).sum(-1))
    if kind == "asym":
        d = d + r.rand(n, n) * 20.0
    elif kind == "const":
        d = np.ones((n, n))
    np.fill_diagonal(d, 0.0)
    d.setflags(write=False)
    return d


def small_matrix(r, n, symmetric):
    d = r.randint(1, 4, size=(n, n)).astype(np.float64)
    if symmetric:
        d = np.triu(d, 1) + np.triu(d, 1).T
    np.fill_diagonal(d, 0.0)
    return d


def chains(d, starts, farthest=False):
    got, status = _mops().tsp_neighbour_chain(oc.t(np.array(d)), oc.t(np.asarray(starts, dtype=np.int64)), farthest)
    assert got.dtype == torch.int64 and status.dtype == torch.int32 and not bool(status.any())
    return got.cpu().numpy()


def grow(d, order, **kw):
    """-> (tours, lengths, passes, status) as numpy"""
    out = _mops().tsp_grow_2opt(oc.t(np.array(d)), oc.t(np.array(order, dtype=np.int64)), **kw)
    assert [o.dtype for o in out] == [torch.int64, torch.float64, torch.int64, torch.int32]
    return [o.cpu().numpy() for o in out]


def assert_rows(got, d, order, what, **kw):
    """every row of a grow launch against the oracle: tour, length bits, passes, status"""
    for s, row in enumerate(np.asarray(order)):
        wt, wl, wp, ws = orc.grow(np.asarray(d), row, **kw)
        assert int(got[3][s]) == ws and int(got[2][s]) == wp, (what, s, int(got[2][s]), wp, int(got[3][s]), ws)
        assert np.array_equal(got[0][s], wt), (what, s)
        assert np.float64(got[1][s]).tobytes() == np.float64(wl).tobytes(), (what, s)


@functools.lru_cache(maxsize=None)
def oracle_chains(n, kind, farthest, starts):
    d = matrix(n, kind)
    c = np.stack([orc.neighbour_chain(d, s, farthest) for s in starts])
    c.setflags(write=False)
    return c


def quiet(fn, *a, **k):
    with contextlib.redirect_stdout(io.StringIO()):
        return fn(*a, **k)


def public():
    from rlsolver_amd.methods import tsp_ins_c, tsp_ins_f, tsp_ins_n, tsp_nn
    return {"nn": lambda d, loc: tsp_nn.nearest_neighbour(d, loc, True, False, device=DEV),
            "nn0": lambda d, loc: tsp_nn.nearest_neighbour(d, loc, False, False, device=DEV),
            "ins_n": lambda d, loc: tsp_ins_n.nearest_insertion(d, loc, False, device=DEV),
            "ins_f": lambda d, loc: tsp_ins_f.farthest_insertion(d, loc, False, device=DEV),
            "ins_c": lambda d: quiet(tsp_ins_c.cheapest_insertion, d, False, device=DEV)}


def same(got, route, distance, what):
    assert got[0] == [int(c) for c in route], what
    assert isinstance(got[1], float) and np.float64(got[1]).tobytes() == np.float64(distance).tobytes(), what


def staged_edge():
    """(the largest N whose matrix is staged in LDS, the first that is not): the launcher's own answer"""
    from rlsolver_amd import _abi
    last = max(n for n in range(2, 400) if _abi.tsp_grow_launch_form(n).lds_d)
    assert not _abi.tsp_grow_launch_form(last + 1).lds_d and _abi.tsp_grow_launch_form(last + 1).supported
    return last, last + 1


# ---------------------------------------------------------------------------------------------------------------- 1. the reference's runs
GOLDEN = [f"{k}{n}" for n in range(2, 7) for k in ("sym", "asym")] + ["uniform12", "gon12", "berlin16", "berlin52", "berlin20"]


@gpu
@pytest.mark.parametrize("name", GOLDEN)
def test_every_golden_through_the_public_functions(golden, name):
    z = golden("tsp_construct")
    d = z[f"{name}/distance_f64"]
    fns = public()
    for fn in ("nn", "nn0", "ins_n", "ins_f"):
        for k, loc in enumerate(int(v) for v in z[f"{name}/locations"]):
            same(fns[fn](d, loc), z[f"{name}/{fn}/routes"][k], z[f"{name}/{fn}/distances"][k], (name, fn, loc))
    if int(z[f"{name}/cheapest"]):
        same(fns["ins_c"](d), z[f"{name}/ins_c/route"], z[f"{name}/ins_c/distance"], (name, "ins_c"))


@gpu
def test_the_12_gon_and_the_printed_lines(golden, capsys):
    """rotated and reflected tours of the regular 12-gon tie in exact arithmetic and differ only in rounding: every start's tour,
    length bits and pass count, not only the winner's; and `verbose` prints what the reference prints"""
    from rlsolver_amd.methods import tsp_ins_c, tsp_ins_f, tsp_nn
    d = golden("tsp_construct")["gon12/distance_f64"]
    for far in (False, True):
        ch = chains(d, range(12), far)
        assert np.array_equal(ch, np.stack([orc.neighbour_chain(d, s, far) for s in range(12)]))
        assert_rows(grow(d, ch), d, ch, ("gon12", far))
        assert_rows(grow(d, ch, m_seed=12, first_m=12), d, ch, ("gon12 full", far), m_seed=12, first_m=12)
    capsys.readouterr()
    route, dist = tsp_ins_f.farthest_insertion(d, 3, device=DEV)
    assert capsys.readouterr().out == f"Iteration =  2 Distance =  {round(dist, 2)}\n"
    tsp_nn.nearest_neighbour(d, device=DEV)
    lines = capsys.readouterr().out.splitlines()
    assert len(lines) == 12 and [ln.split()[2] for ln in lines] == [str(i) for i in range(12)]
    route, dist = tsp_ins_c.cheapest_insertion(d[:5, :5], device=DEV)
    assert capsys.readouterr().out == "Iteration =  0\nIteration =  1\nIteration =  2\n" + f"distance:  {dist}\n"


# ---------------------------------------------------------------------------------------------------------------- 2. the smallest sizes
@gpu
@pytest.mark.parametrize("symmetric", [True, False])
@pytest.mark.parametrize("n", [2, 3, 4, 5])
def test_200_small_integer_matrices_all_starts_all_constructors(n, symmetric):
    r = oc.rng(31 * n + symmetric)
    fns = public()
    ofn = {"nn": lambda d, loc: orc.nearest_neighbour(d, loc, True), "nn0": lambda d, loc: orc.nearest_neighbour(d, loc, False),
           "ins_n": orc.nearest_insertion, "ins_f": orc.farthest_insertion}
    for k in range(200):
        d = small_matrix(r, n, symmetric)
        for far in (False, True):
            ch = chains(d, range(n), far)
            assert np.array_equal(ch, np.stack([orc.neighbour_chain(d, s, far) for s in range(n)])), (k, far)
            assert_rows(grow(d, ch), d, ch, (k, far, "insertion"))
        assert_rows(grow(d, ch, m_seed=n, first_m=n), d, ch, (k, "full"), m_seed=n, first_m=n)
        loc = [-1] + list(range(1, n + 1))
        for fn in ofn:
            got, want = fns[fn](d, loc[k % len(loc)]), ofn[fn](d, loc[k % len(loc)])
            assert got == want and isinstance(got[1], float), (k, fn)
        assert fns["ins_c"](d) == orc.cheapest_insertion(d), k


# ---------------------------------------------------------------------------------------------------------------- 3. around a wave
@gpu
@pytest.mark.parametrize("kind", ["sym", "asym"])
@pytest.mark.parametrize("n", [63, 64, 65, 66])
def test_chains_from_all_starts_and_grow_from_four_around_64_cities(n, kind):
    d = matrix(n, kind)
    for far in (False, True):
        assert np.array_equal(chains(d, range(n), far), oracle_chains(n, kind, far, tuple(range(n)))), far
    order = oracle_chains(n, kind, kind == "asym", tuple(range(n)))[[0, 1, n // 2, n - 1]]
    assert_rows(grow(d, order, first_m=n - 2), d, order, (n, kind), first_m=n - 2)


# ---------------------------------------------------------------------------------------------------------------- 4. the staging edge
@gpu
@pytest.mark.parametrize("which", [0, 1])
def test_the_largest_staged_and_the_first_unstaged_size(which):
    n = staged_edge()[which]
    d = matrix(n, "sym")
    order = oracle_chains(n, "sym", False, (0, n - 1))
    assert_rows(grow(d, order, first_m=n - 1), d, order, n, first_m=n - 1)


@gpu
@pytest.mark.parametrize("which", [0, 1, 2])
def test_a_full_tour_equals_the_host_loop_of_2opt_passes(which):
    """m_seed = first_m = m_end = N: one on-device convergence against local_search_2_opt_batch(exact=True), a launch and a host
    read per pass, bit for bit"""
    from rlsolver_amd.methods import tsp_opt_2
    n = (staged_edge() + (100,))[which]
    d = oc.t(np.array(matrix(n, "asym" if which == 2 else "sym")))
    perms = oc.t(np.stack([oc.rng(n + b).permutation(n) for b in range(3)]).astype(np.int64))
    want_p, want_l = tsp_opt_2.local_search_2_opt_batch(d, perms, exact=True)
    tours, lengths, passes = _tc().grow_2opt(d, perms, m_seed=n, first_m=n)
    assert torch.equal(tours, want_p) and torch.equal(lengths.view(torch.int64), want_l.view(torch.int64))
    assert bool((passes >= 2).all())


# ---------------------------------------------------------------------------------------------------------------- 5. the forms of a launch
@gpu
def test_a_partial_end_keeps_the_tail_of_order_and_measures_the_partial_tour():
    n, m_end = 30, 17
    d = matrix(n, "asym")
    order = np.stack([oc.rng(b).permutation(n) for b in range(3)])
    got = grow(d, order, m_seed=4, m_end=m_end, first_m=6)
    assert_rows(got, d, order, "partial", m_seed=4, m_end=m_end, first_m=6)
    for s in range(3):
        assert np.array_equal(got[0][s, m_end:], order[s, m_end:]) and sorted(got[0][s]) == list(range(n))
        assert got[1][s] == orc.seq_length(d, got[0][s, :m_end])


@gpu
def test_the_single_append_of_cheapest_insertion():
    """a converged m-city tour, every absent city in turn at its end, converged once: a row per absent city"""
    n, m = 24, 9
    d = matrix(n, "sym")
    base = orc.grow(d, np.arange(n), m_end=m)[0][:m]
    absent = [c for c in range(n) if c not in set(base.tolist())]
    order = np.stack([np.concatenate([base, [c], [a for a in absent if a != c]]) for c in absent])
    got = grow(d, order, m_seed=m, m_end=m + 1, first_m=m + 1)
    assert_rows(got, d, order, "append", m_seed=m, m_end=m + 1, first_m=m + 1)
    assert len(set(got[1].tolist())) > 1                      # the rows do differ: the first minimum is a choice


@gpu
def test_a_constant_matrix_takes_one_pass_per_convergence_and_moves_nothing():
    n = 40
    d = matrix(n, "const")
    order = np.stack([oc.rng(b).permutation(n) for b in range(2)])
    tours, lengths, passes, status = grow(d, order)
    assert np.array_equal(tours, order) and not status.any()
    assert passes.tolist() == [n - 2, n - 2] and lengths.tolist() == [float(n), float(n)]


@gpu
def test_rows_are_independent():
    n = 33
    d = matrix(n, "sym")
    ch = chains(d, range(n), True)
    whole = grow(d, ch)
    assert np.array_equal(np.concatenate([chains(d, range(0, 7), True), chains(d, range(7, n), True)]), ch)
    a, b = grow(d, ch[:7]), grow(d, ch[7:])
    for k in range(4):
        assert np.array_equal(np.concatenate([a[k], b[k]]), whole[k]), k
    assert_rows(whole, d, ch, "rows")


# ---------------------------------------------------------------------------------------------------------------- 6. status
@gpu
def test_max_passes_is_reported_and_leaves_the_state_after_that_many_passes():
    n = 20
    d = matrix(n, "sym")
    order = np.stack([oc.rng(50 + b).permutation(n) for b in range(2)] + [orc.grow(d, np.arange(n), m_seed=n, first_m=n)[0]])
    assert [orc.grow(d, o, m_seed=n, first_m=n)[2] >= 2 for o in order] == [True, True, False]      # the last row is converged: one pass
    got = grow(d, order, m_seed=n, first_m=n, max_passes=1)
    assert got[3].tolist() == [1, 1, 0] and got[2].tolist() == [1, 1, 1]
    for s in range(2):
        after_one = orc.one_pass(d, order[s], orc.seq_length(d, order[s]))
        assert np.array_equal(got[0][s], after_one[0]) and got[1][s] == after_one[1]
    assert_rows(got, d, order, "max_passes", m_seed=n, first_m=n, max_passes=1)
    # while growing: the row stops at the size that ran into the guard, the rest of order behind it
    got = grow(d, order[:2], first_m=n - 3, max_passes=1)
    assert_rows(got, d, order[:2], "max_passes growing", first_m=n - 3, max_passes=1)
    assert got[3].tolist() == [1, 1]
    with pytest.raises(RuntimeError, match="max_passes"):
        _tc().grow_2opt(oc.t(np.array(d)), oc.t(order), m_seed=n, first_m=n, max_passes=1)


@gpu
@pytest.mark.parametrize("bad", [None, -1])
def test_an_order_entry_outside_the_matrix_is_reported_and_its_row_left_alone(bad):
    n = 12
    d = matrix(n, "sym")
    bad = n if bad is None else bad
    order = np.stack([oc.rng(b).permutation(n) for b in range(4)])
    order[1, 9] = bad                                          # behind m_end too: the tail is copied, so it is checked
    order[3, 0] = bad
    dev_out = (torch.full((4, n), -7, dtype=torch.int64, device=DEV), torch.full((4,), -7.0, dtype=torch.float64, device=DEV),
               torch.full((4,), -7, dtype=torch.int64, device=DEV), torch.full((4,), -7, dtype=torch.int32, device=DEV))
    tours, lengths, passes, status = (o.cpu().numpy() for o in _mops().tsp_grow_2opt(oc.t(np.array(d)), oc.t(order), m_end=8, out=dev_out))
    assert status.tolist() == [0, 2, 0, 2]
    for s in (1, 3):
        assert (tours[s] == -7).all() and lengths[s] == -7.0 and passes[s] == -7
    for s in (0, 2):
        wt, wl, wp, _ = orc.grow(d, order[s], m_end=8)
        assert np.array_equal(tours[s], wt) and lengths[s] == wl and passes[s] == wp
    with pytest.raises(ValueError, match="cities"):
        _tc().grow_2opt(oc.t(np.array(d)), oc.t(order))
    # the chain: a start outside leaves its row untouched
    chain = torch.full((3, n), -7, dtype=torch.int64, device=DEV)
    st = torch.full((3,), -7, dtype=torch.int32, device=DEV)
    torch.ops.rlsolver_hip.tsp_neighbour_chain(oc.t(np.array(d)), oc.t(np.array([2, bad, 5], dtype=np.int64)), 0, chain, st)
    assert st.tolist() == [0, 2, 0] and bool((chain[1] == -7).all())
    assert np.array_equal(chain[[0, 2]].cpu().numpy(), np.stack([orc.neighbour_chain(d, 2), orc.neighbour_chain(d, 5)]))
    with pytest.raises(ValueError, match="starts"):
        _tc().neighbour_chains(oc.t(np.array(d)), oc.t(np.array([2, bad], dtype=np.int64)))
