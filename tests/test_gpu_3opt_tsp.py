"""The reference's 3-opt as one kernel per pass (rls_tsp_3opt_best, ops_mcpg_tsp.tsp_3opt_best, methods/tsp_opt_3.py) against
the reference's own runs (tests/golden/tsp_3opt.npz) and the numpy restatement of tests/tsp3opt_oracle.py.  Every comparison is
exact: routes, indices and float64 values bit for bit.

Sizes: every tour of 3, 4 and 5 cities (empty S2 and C, k = N, a lone ragged chunk per i); 63 .. 66 cities (delta ranking: the lanes
of a wave stride over k, one k-trip short of, at, and past a full wave; exact ranking: the (j, k) of one i go to the lanes in chunks of
64; both with 1, 2 and 300 tours and 1 to default slices); the first N whose matrix is no longer staged in LDS; 700 cities for a key past 2^31.

At import this file also registers the op's valid calls with tests/op_contract.py, so that the completeness test and the refusal
sweep of tests/test_gpu_op_contract.py cover it unchanged -- the mechanism of tests/test_gpu_exhaustive.py: pytest imports test
modules in name order while it collects, and this name sorts before that one.  Running tests/test_gpu_op_contract.py on its own
does not see these rows (its completeness test then names the op): run it together with this file."""
import functools
import itertools

import numpy as np
import pytest
import torch

from tests import op_contract as oc
from tests import tsp3opt_oracle as o3

gpu = pytest.mark.gpu
DEV = oc.DEV


def _mops():
    from rlsolver_amd import ops_mcpg_tsp
    return ops_mcpg_tsp


def _t3():
    from rlsolver_amd.methods import tsp_opt_3
    return tsp_opt_3


# ---------------------------------------------------------------------------------------------------------------- contract rows
def _contract_inputs():
    d64 = oc.tsp_env().distance.to(torch.float64)
    return d64, oc.tours()


@oc.row("tsp_3opt_best", outs=("best_i", "best_value"))      # (of best_j / best_k / best_trial only the first B entries are written when slices > 1)
def _():
    d64, p = _contract_inputs()
    return oc.taken("tsp_3opt_best", lambda: _mops().tsp_3opt_best(d64, p, slices=2))


@oc.row("tsp_3opt_best", outs=("best_i", "best_j", "best_k", "best_trial", "best_value"), variant="exact")
def _():
    d64, p = _contract_inputs()
    cur = _mops().tsp_tour_length(oc.tsp_env().distance, p).to(torch.float64)
    return oc.taken("tsp_3opt_best", lambda: _mops().tsp_3opt_best(d64, p, cur, slices=1))


# ---------------------------------------------------------------------------------------------------------------- helpers
@functools.lru_cache(maxsize=None)
def matrix(n, kind, seed=0):
    """read-only float64 [n, n]: 'sym' Euclidean, 'int' symmetric small integers (ties everywhere), 'asym' every oriented entry
    its own number"""
    r = oc.rng(1000 * n + seed)
    c = r.rand(n, 2) * 100.0
    d = np.sqrt(((c[:, None] - c[None]) ** 2).sum(-1))
    if kind == "int":
        d = np.rint(d / 12.0)
    elif kind == "asym":
        d = d + r.rand(n, n) * 20.0
    np.fill_diagonal(d, 0.0)
    d.setflags(write=False)
    return d


def lengths(d, perms):
    """distance_calc of every row: sequential float64, the closing edge last"""
    v = np.zeros(len(perms))
    n = perms.shape[1]
    for p in range(n):
        v = v + d[perms[:, p], perms[:, (p + 1) % n]]
    return v


@functools.lru_cache(maxsize=None)
def random_tour(n, seed):
    p = oc.rng(77 * n + seed).permutation(n).astype(np.int64)
    p.setflags(write=False)
    return p


@functools.lru_cache(maxsize=None)
def want_random(n, kind, seed, exact):
    d, p = matrix(n, kind), random_tour(n, seed)
    # (exact ranking at these sizes: the grouped form of the oracle, which tests/test_tsp3opt_oracle.py holds against the plain one)
    return o3.one_pass_exact_grouped(d, p, lengths(d, p[None])[0]) if exact else o3.one_pass(d, p, None)


def run(d, perms, cur=None, slices=None):
    out = _mops().tsp_3opt_best(oc.t(np.array(d)), oc.t(np.array(perms)), None if cur is None else oc.t(np.array(cur, dtype=np.float64)), slices=slices)
    assert [o.dtype for o in out] == [torch.int64] * 4 + [torch.float64] and all(o.shape == (len(perms),) for o in out)
    return [o.cpu().numpy() for o in out]


def rows(out):
    return [tuple(int(out[c][b]) for c in range(4)) + (float(out[4][b]),) for b in range(len(out[0]))]


# ---------------------------------------------------------------------------------------------------------------- 1. the whole tour space
@gpu
@pytest.mark.parametrize("kind", ["sym", "int", "asym"])
@pytest.mark.parametrize("n", [3, 4, 5])
def test_every_tour_of_the_smallest_sizes(n, kind):
    d = matrix(n, kind)
    perms = np.array(list(itertools.permutations(range(n))), dtype=np.int64)
    true = lengths(d, perms)
    cases = [("exact", true), ("inflated", true * 1.5), ("zero", np.zeros(len(perms)))] + ([("delta", None)] if kind != "asym" else [])
    for what, cur in cases:
        want = [o3.one_pass(d, p, None if cur is None else cur[b]) for b, p in enumerate(perms)]
        for slices in (1, 3):
            assert rows(run(d, perms, cur, slices)) == want, (what, slices)
        if what == "inflated":                               # the seed tour is itself a candidate: its true length replaces the inflated one
            assert all(w[0] >= 0 and w[4] <= true[b] for b, w in enumerate(want))
        if what == "zero":
            assert all(w == (-1, -1, -1, -1, 0.0) for w in want)
    assert len(o3.segments(n)) == o3.count_segments(n)


# ---------------------------------------------------------------------------------------------------------------- 2. goldens
def _golden_cases(z):
    for name in z["names"]:
        for rs in z[f"{name}/seedings"]:
            yield f"{name}/rs{int(rs)}", f"{name}", int(rs)
    for tag in z["contract_cases"]:
        yield f"contract/{tag}", f"contract/{tag}", int(z[f"contract/{tag}/seeding"])


@gpu
def test_local_search_3_opt_reproduces_the_reference(golden, capsys):
    z = golden("tsp_3opt")
    t3 = _t3()
    seen = set()
    for out, src, rs in _golden_cases(z):
        d, start = z[f"{src}/distance_f64"], [[int(c) for c in z[f"{src}/start_tour"]], float(z[f"{src}/start_distance"])]
        route, dist = t3.local_search_3_opt(d, start, recursive_seeding=rs, verbose=False, device=DEV)
        assert route == [int(c) for c in z[f"{out}/tour"]] and dist == float(z[f"{out}/distance"]), out
        seen.add(rs)
        # the batch form in exact ranking: the same tour and distance for the same number of passes
        perm = oc.t(np.asarray(start[0][:-1], dtype=np.int64)[None] - 1)
        perms, lens = t3.local_search_3_opt_batch(oc.t(d), perm, max_passes=rs, exact=True, lengths=oc.t(np.array([start[1]])))
        assert [int(c) + 1 for c in perms[0].tolist()] == route[:-1] and float(lens[0]) == dist, out
    assert {0, 2, -1} <= seen
    assert float(z["contract/inflated/distance"]) < float(z["contract/inflated/start_distance"])
    assert float(z["contract/zero/distance"]) == 0.0 and float(z["contract/three/distance"]) < 1e9
    # verbose prints the reference's line
    t3.local_search_3_opt(z["a5/distance_f64"], [[int(c) for c in z["a5/start_tour"]], float(z["a5/start_distance"])], recursive_seeding=1, device=DEV)
    assert capsys.readouterr().out.startswith("Iteration =  0 Distance = ")


# ---------------------------------------------------------------------------------------------------------------- 3. wave and workgroup edges
EDGE = [(n, exact, "asym" if exact else "sym") for n in (63, 64, 65, 66) for exact in (True, False)] + [(65, True, "int"), (65, False, "int")]


@gpu
@pytest.mark.parametrize("n,exact,kind", EDGE)
def test_wave_and_workgroup_edges(n, exact, kind):
    d = matrix(n, kind)
    distinct = np.stack([random_tour(n, s) for s in range(3)])
    want3 = [want_random(n, kind, s, exact) for s in range(3)]
    assert any(w[0] >= 0 for w in want3)
    for B in (1, 2, 300):
        perms = distinct[np.arange(B) % 3]
        cur = lengths(d, perms) if exact else None
        want = [want3[b % 3] for b in range(B)]
        for slices in (1, 2, 7, None):
            assert rows(run(d, perms, cur, slices)) == want, (B, slices)


def first_unstaged(exact):
    from rlsolver_amd import _abi
    n = 3
    while _abi.tsp_3opt_launch_form(n, exact).lds_d:
        n += 1
    return n


@gpu
def test_the_first_size_past_the_staged_matrix():
    from rlsolver_amd import _abi
    n = first_unstaged(True)
    assert _abi.tsp_3opt_launch_form(n - 1, True).lds_d == 1 and _abi.tsp_3opt_launch_form(n, True).supported == 1
    d, p = matrix(n, "sym"), random_tour(n, 0)
    cur = lengths(d, p[None])
    want = o3.one_pass_exact_grouped(d, p, cur[0])
    assert want[0] >= 0
    assert rows(run(d, p[None], cur)) == [want]
    assert rows(run(d, p[None], cur, slices=3)) == [want]
    assert rows(run(matrix(n - 1, "sym"), random_tour(n - 1, 0)[None])) == [o3.one_pass(matrix(n - 1, "sym"), random_tour(n - 1, 0), None)]


# ---------------------------------------------------------------------------------------------------------------- 4. slices
def circle(n):
    a = 2.0 * np.pi * np.arange(n) / n
    c = np.stack([100.0 * np.cos(a), 100.0 * np.sin(a)], axis=1)
    return np.sqrt(((c[:, None] - c[None]) ** 2).sum(-1))


def planted(n, i, j, k):
    """the circle in order with S1 and S2 of (i, j, k) reversed: trial abC of that triple restores the optimum"""
    t = np.arange(n)
    t[i + 1:j + 1] = t[i + 1:j + 1][::-1].copy()
    t[j + 1:k + 1] = t[j + 1:k + 1][::-1].copy()
    return t


@gpu
@pytest.mark.parametrize("exact", [True, False])
def test_results_do_not_depend_on_slices(exact):
    from rlsolver_amd import _abi
    n, (i, j, k) = 40, (30, 34, 38)
    d = circle(n)
    perms = np.stack([planted(n, i, j, k), random_tour(n, 5)])
    cur = lengths(d, perms) if exact else None
    want = [o3.one_pass(d, p, None if cur is None else cur[b]) for b, p in enumerate(perms)]
    assert want[0][:4] == (i, j, k, 4)
    # item q of the kernel's work list goes to wave q mod (s waves) of the s slices, that is to slice (q mod (s waves)) / waves.
    # exact ranking: the (j, k) of one i are cut into chunks of 64 and the items are the chunks of all i; delta ranking: the items
    # are the (i, j) pairs.  The slices that put the planted winner's item into the LAST slice:
    waves = _abi.tsp_3opt_launch_form(n, exact).waves
    if exact:
        row_chunks = [(len(o3.pairs_of(n, a)[0]) + 63) // 64 for a in range(n - 1)]
        js, ks = o3.pairs_of(n, i)
        q, items = sum(row_chunks[:i]) + int(np.flatnonzero((js == j) & (ks == k))[0]) // 64, sum(row_chunks)
    else:
        q, items = i * (2 * n - i - 1) // 2 + (j - i - 1), n * (n - 1) // 2
    last = [s for s in range(2, 64) if (q % (s * waves)) // waves == s - 1]
    assert last
    # past items / waves slices some workgroups have no item at all: rows of (-1, start value)
    for slices in [1, 2, 3, 5, 16, last[0], last[-1], items // waves + 3, items + 1, 1000, None]:
        assert rows(run(d, perms, cur, slices)) == want, slices


# ---------------------------------------------------------------------------------------------------------------- 5. key width
@gpu
def test_a_winner_whose_key_passes_2_to_the_31(golden):
    z = golden("tsp_3opt")
    c = z["planted700/coords"]
    d = np.sqrt(((c[:, None, :] - c[None, :, :]) ** 2).sum(-1))
    i, j, k, r = (int(v) for v in z["planted700/answer"])
    assert ((i * 700 + j) * 701 + k) * 8 + r > 1 << 31 and o3.TRIALS[r] == "abC" and j - i >= 2 and k - j >= 2 and i >= 590
    out = run(d, z["planted700/tour"][None])
    assert rows(out) == [(i, j, k, r, float(z["planted700/value"]))]
    moved = _t3()._apply_moves(oc.t(z["planted700/tour"][None]), *(oc.t(o) for o in out[:4]))
    assert moved[0].tolist() == list(range(700))


# ---------------------------------------------------------------------------------------------------------------- 6. delta == exact on integers
@gpu
@pytest.mark.parametrize("n", [12, 30])
def test_both_rankings_agree_pass_by_pass_on_integer_matrices(n):
    t3 = _t3()
    d = oc.t(np.array(matrix(n, "int")))
    perms = oc.t(np.stack([random_tour(n, s) for s in range(6)]))
    prev = None
    for passes in range(1, 40):
        a, la = t3.local_search_3_opt_batch(d, perms, max_passes=passes, exact=True)
        b, lb = t3.local_search_3_opt_batch(d, perms, max_passes=passes)
        assert torch.equal(a, b) and torch.equal(la, lb), passes
        if prev is not None and torch.equal(a, prev):
            break
        prev = a
    else:
        raise AssertionError("no convergence in 40 passes")
    assert passes > 2
    # a converged batch: one more pass names no move
    for cur in (la, None):
        out = _mops().tsp_3opt_best(d, a, cur)
        assert all(bool((o == -1).all()) for o in out[:4])
        assert torch.equal(out[4], la if cur is not None else torch.zeros_like(la))


# ---------------------------------------------------------------------------------------------------------------- 7. refusals
@gpu
def test_refusals():
    mops, t3 = _mops(), _t3()
    d3, p3 = oc.t(np.array(matrix(3, "sym"))), oc.t(np.array([[0, 1, 2]], dtype=np.int64))
    d2, p2 = oc.t(np.array(matrix(2, "sym"))), oc.t(np.array([[0, 1]], dtype=np.int64))
    i64 = lambda m: torch.full((m,), 7, dtype=torch.int64, device=DEV)       # noqa: E731
    f64 = lambda m: torch.full((m,), 7.0, dtype=torch.float64, device=DEV)   # noqa: E731
    with pytest.raises(ValueError, match="N >= 3"):
        mops.tsp_3opt_best(d2, p2)
    outs = [i64(1), i64(1), i64(1), i64(1), f64(1)]
    with pytest.raises(RuntimeError):
        torch.ops.rlsolver_hip.tsp_3opt_best(d2, p2, None, *outs)
    with pytest.raises(ValueError):
        t3.local_search_3_opt(np.array(matrix(2, "sym")), [[1, 2, 1], 10.0], verbose=False, device=DEV)
    for slices in (0, 65536, -1):
        with pytest.raises(ValueError, match="slices"):
            mops.tsp_3opt_best(d3, p3, slices=slices)
    big = [i64(65536), i64(65536), i64(65536), i64(65536), f64(65536)]
    with pytest.raises(RuntimeError, match="slices"):
        torch.ops.rlsolver_hip.tsp_3opt_best(d3, p3, None, *big)
    torch.cuda.synchronize()
    assert all(bool((o == 7).all()) for o in outs + big)
    with pytest.raises(ValueError, match="symmetric"):
        t3.local_search_3_opt_batch(np.array(matrix(5, "asym")), oc.t(random_tour(5, 0)[None].copy()))
    perms, lens = t3.local_search_3_opt_batch(np.array(matrix(5, "asym")), oc.t(random_tour(5, 0)[None].copy()), exact=True)
    assert sorted(perms[0].tolist()) == list(range(5)) and float(lens[0]) == lengths(matrix(5, "asym"), perms.cpu().numpy())[0]
    with pytest.raises(ValueError, match="permutations"):
        t3.local_search_3_opt_batch(np.array(matrix(5, "sym")), oc.t(np.array([[0, 1, 2, 3, 3]], dtype=np.int64)))
    empty = mops.tsp_3opt_best(d3, torch.empty((0, 3), dtype=torch.int64, device=DEV))
    assert all(o.shape == (0,) for o in empty)
    empty = mops.tsp_3opt_best(d3, torch.empty((0, 3), dtype=torch.int64, device=DEV), torch.empty(0, dtype=torch.float64, device=DEV))
    assert all(o.shape == (0,) for o in empty)
