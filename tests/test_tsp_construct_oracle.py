"""tests/tsp_construct_oracle.py against the reference's recorded runs (tests/golden/tsp_construct.npz, written by
tools/gen_golden_tsp_construct.py from nn.py, ins_n.py, ins_f.py and ins_c.py on the CPU): the same routes and the same float64
distances, bit for bit -- small matrices full of ties, Euclidean points, berlin52 and its first 16 / 20 cities, and a regular
12-gon whose rotated and reflected tours differ only in rounding."""
import numpy as np
import pytest

from tests import tsp_construct_oracle as oc

FNS = {"nn": lambda d, loc: oc.nearest_neighbour(d, loc, True), "nn0": lambda d, loc: oc.nearest_neighbour(d, loc, False),
       "ins_n": oc.nearest_insertion, "ins_f": oc.farthest_insertion}
NAMES = [f"{k}{n}" for n in range(2, 7) for k in ("sym", "asym")] + ["uniform12", "gon12", "berlin16", "berlin52", "berlin20"]


def same(got, route, distance, what):
    assert got[0] == [int(c) for c in route], what
    assert isinstance(got[1], float) and np.float64(got[1]).tobytes() == np.float64(distance).tobytes(), what


def test_the_golden_holds_the_cases_this_file_names(golden):
    z = golden("tsp_construct")
    assert list(z["names"]) == NAMES
    assert [int(v) for v in z["berlin52/locations"]] == [1] and len(z["berlin20/locations"]) == 0
    assert [int(v) for v in z["sym5/locations"]] == [-1, 1, 2, 3, 4, 5]
    assert z["berlin52/distance_f64"].shape == (52, 52) and z["gon12/distance_f64"].shape == (12, 12)


@pytest.mark.parametrize("name", NAMES)
def test_oracle_equals_the_reference(golden, name):
    z = golden("tsp_construct")
    d = z[f"{name}/distance_f64"]
    for fn, call in FNS.items():
        for k, loc in enumerate(int(v) for v in z[f"{name}/locations"]):
            same(call(d, loc), z[f"{name}/{fn}/routes"][k], z[f"{name}/{fn}/distances"][k], (name, fn, loc))
    if int(z[f"{name}/cheapest"]):
        same(oc.cheapest_insertion(d), z[f"{name}/ins_c/route"], z[f"{name}/ins_c/distance"], (name, "ins_c"))


def test_the_chain_prefers_the_lowest_city_among_equals_and_ignores_the_diagonal():
    d = np.ones((6, 6))
    np.fill_diagonal(d, -5.0)                                   # the diagonal would win both ways if it were looked at
    assert list(oc.neighbour_chain(d, 3)) == [3, 0, 1, 2, 4, 5]
    np.fill_diagonal(d, 9.0)
    assert list(oc.neighbour_chain(d, 3, farthest=True)) == [3, 0, 1, 2, 4, 5]


def test_a_pass_is_the_double_loop_of_the_reference_restated_plainly():
    """the vectorised pass against the loop it restates: every reversal, python sums, the first strict minimum kept"""
    r = np.random.RandomState(5)
    for n, kind in ((5, "int"), (7, "real"), (9, "asym")):
        d = r.randint(1, 4, size=(n, n)).astype(np.float64) if kind == "int" else r.rand(n, n) * 10.0
        if kind != "asym":
            d = np.triu(d, 1) + np.triu(d, 1).T
        for _ in range(5):
            t = r.permutation(n)
            cur = oc.seq_length(d, t)
            best, bt, bij = cur, t, (-1, -1)
            for i in range(n - 1):
                for j in range(i + 1, n):
                    c = t.copy()
                    c[i:j + 1] = c[i:j + 1][::-1]
                    v = 0
                    for k in range(n):
                        v = v + d[c[k], c[(k + 1) % n]]
                    if best > v:
                        best, bt, bij = v, c, (i, j)
            got = oc.one_pass(d, t, cur)
            assert list(got[0]) == list(bt) and got[1] == best and got[2:] == bij


def test_passes_and_the_guard_are_counted_as_the_kernel_counts_them():
    r = np.random.RandomState(11)
    d = r.rand(9, 9) * 10.0
    order = r.permutation(9)
    t, v, p, st = oc.grow(d, order, m_seed=9, first_m=9)
    assert st == 0 and p >= 2 and v == oc.seq_length(d, t[:9])
    t1, v1, p1, st1 = oc.grow(d, order, m_seed=9, first_m=9, max_passes=1)
    assert st1 == 1 and p1 == 1 and list(t1) == list(oc.one_pass(d, order, oc.seq_length(d, order))[0])
    const = np.ones((6, 6))
    t, v, p, st = oc.grow(const, np.arange(6))
    assert list(t) == list(range(6)) and p == 4 and st == 0 and v == 6.0       # one fruitless pass at each of m = 3, 4, 5, 6
    t, v, p, st = oc.grow(d, order, m_end=5)
    assert list(t[5:]) == list(order[5:]) and v == oc.seq_length(d, t[:5])
    assert oc.grow(d, np.array([0, 1, 9, 3, 4, 5, 6, 7, 8]))[3] == 2 and oc.grow(d, np.array([0, -1, 2, 3, 4, 5, 6, 7, 8]))[3] == 2
