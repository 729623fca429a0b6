"""tests/tsp3opt_oracle.py against the reference's own runs of opt_3.py (tests/golden/tsp_3opt.npz): the restatement the GPU tests
compare the kernel with reproduces every recorded pass, route and float64 distance bit for bit.  No GPU."""
import numpy as np
import pytest

from tests import tsp3opt_oracle as o3


def _start(z, src):
    return [int(c) for c in z[f"{src}/start_tour"]], float(z[f"{src}/start_distance"])


@pytest.mark.parametrize("name", ["a5", "int9", "uniform12", "asym6", "asym16", "uniform30", "berlin52"])
def test_oracle_reproduces_every_recorded_pass(golden, name):
    z = golden("tsp_3opt")
    assert name in z["names"]
    d = z[f"{name}/distance_f64"]
    tour, cur = _start(z, name)
    assert o3.distance_calc(d, tour) == cur
    for rs in z[f"{name}/seedings"]:
        route, dist = o3.local_search(d, tour, cur, int(rs))
        assert route == [int(c) for c in z[f"{name}/rs{int(rs)}/tour"]] and dist == float(z[f"{name}/rs{int(rs)}/distance"]), rs


def test_oracle_reproduces_the_contract_cases(golden):
    z = golden("tsp_3opt")
    assert set(z["contract_cases"]) == {"inflated", "zero", "zero_start", "three", "no_pass"}
    for tag in z["contract_cases"]:
        src = f"contract/{tag}"
        tour, cur = _start(z, src)
        route, dist = o3.local_search(z[f"{src}/distance_f64"], tour, cur, int(z[f"{src}/seeding"]))
        assert route == [int(c) for c in z[f"{src}/tour"]] and dist == float(z[f"{src}/distance"]), tag
    # what the cases are there to show
    tour, cur = _start(z, "contract/inflated")
    assert [int(c) for c in z["contract/inflated/tour"]] == tour                       # a local optimum comes back unchanged ...
    assert float(z["contract/inflated/distance"]) == o3.distance_calc(z["contract/inflated/distance_f64"], tour) < cur    # ... with its true length
    assert float(z["contract/zero/distance"]) == 0.0 and float(z["contract/zero_start/distance"]) == 0.0
    assert [int(c) for c in z["contract/zero_start/tour"]] == _start(z, "contract/zero_start")[0]
    assert float(z["contract/three/distance"]) == o3.distance_calc(z["contract/three/distance_f64"], [2, 3, 1, 2])
    assert float(z["contract/no_pass/distance"]) == 123.25


def test_segments_and_their_count(golden):
    z = golden("tsp_3opt")
    for n in (3, 4, 5, 12):
        assert o3.segments(n) == [tuple(int(v) for v in row) for row in z[f"segments/n{n}"]]
        assert o3.count_segments(n) == len(o3.segments(n))
    assert o3.segments(3) == [(0, 1, 2), (1, 2, 3)] and len(o3.segments(4)) == 7
    assert o3.count_segments(52) == 23375 and o3.count_segments(100) == 166551
    for n in (3, 4, 7):                                        # pairs_of lists the same triples
        assert [(i, int(j), int(k)) for i in range(n - 1) for j, k in zip(*o3.pairs_of(n, i))] == o3.segments(n)


def test_delta_ranking_is_exact_ranking_in_integer_arithmetic(golden):
    """int9: every entry an integer, so both rankings are exact arithmetic and name the same move with values that differ by the seed's length"""
    z = golden("tsp_3opt")
    d = z["int9/distance_f64"]
    tour, cur = _start(z, "int9")
    t = np.asarray(tour[:-1]) - 1
    for _ in range(10):
        a, b = o3.one_pass(d, t, cur), o3.one_pass(d, t, None)
        assert a[:4] == b[:4] and (a[0] < 0 or a[4] - cur == b[4])
        if a[0] < 0:
            break
        t, cur = o3.apply_move(t, *a[:4]), a[4]
    else:
        raise AssertionError("no convergence")


@pytest.mark.parametrize("kind", ["sym", "int", "asym"])
def test_the_grouped_exact_pass_is_the_plain_one(kind):
    """one_pass_exact_grouped shares partial sums between candidates; it must name the same move with the same bits as one_pass
    on every kind of matrix, with a true, an inflated and a zero seed length, from 3 cities up"""
    for n in (3, 4, 5, 6, 7, 9, 13, 16, 24):
        for seed in range(2):
            r = np.random.RandomState(100 * n + seed)
            c = r.rand(n, 2) * 100.0
            d = np.sqrt(((c[:, None] - c[None]) ** 2).sum(-1))
            if kind == "int":
                d = np.rint(d / 12.0)
            elif kind == "asym":
                d = d + r.rand(n, n) * 20.0
            np.fill_diagonal(d, 0.0)
            p = r.permutation(n)
            true = o3.distance_calc(d, [int(x) + 1 for x in p] + [int(p[0]) + 1])
            for cur in (true, true * 1.5, 0.0):
                assert o3.one_pass_exact_grouped(d, p, cur) == o3.one_pass(d, p, cur), (n, seed, cur)


def test_the_grouped_exact_pass_reproduces_the_recorded_first_passes(golden):
    z = golden("tsp_3opt")
    for name in ("uniform12", "asym16", "berlin52"):
        d = z[f"{name}/distance_f64"]
        tour, cur = _start(z, name)
        t = np.asarray(tour[:-1]) - 1
        i, j, k, r, v = o3.one_pass_exact_grouped(d, t, cur)
        assert v == float(z[f"{name}/rs1/distance"])
        assert [int(c) + 1 for c in o3.apply_move(t, i, j, k, r)] == [int(c) for c in z[f"{name}/rs1/tour"]][:-1]


def test_planted700_answer_restores_the_circle(golden):
    z = golden("tsp_3opt")
    i, j, k, r = (int(v) for v in z["planted700/answer"])
    assert np.array_equal(o3.apply_move(z["planted700/tour"], i, j, k, r), np.arange(700))
    assert float(z["planted700/value"]) < 0
