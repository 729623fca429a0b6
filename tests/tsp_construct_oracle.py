"""Numpy restatement of the reference's tour constructors (rlsolver/methods_problem_specific/TSP/nn.py, ins_n.py, ins_f.py,
ins_c.py) and of the two device entries under them (rls_tsp_neighbour_chain, rls_tsp_grow_2opt): the same routes and the same
float64 distances, bit for bit (tests/test_tsp_construct_oracle.py holds it against the reference's recorded runs).

What the reference does, restated:
  * the order in which nn.py / ins_n.py / ins_f.py take up cities does not depend on the 2-opt: the next city is the argmin
    (ins_f.py: argmax) of the row of the city taken last, over the cities not yet taken, the lowest index among equals;
  * a tour grows by one city at its end and is then 2-opted until a pass brings nothing; a pass (opt_2.py's double loop) values
    every reversal [i..j] of the pass's seed by distance_calc -- float64, edge after edge from the candidate's first city, the closing
    edge last -- and keeps the first strict minimum in (i, j) order;
  * cheapest_insertion tries every absent city at the end of the tour, converges each, and keeps the first shortest.
Sums are np.add.accumulate along the edges (sequential; never np.sum, which adds pairwise).  A pass is vectorised over its
m (m - 1) / 2 candidates, so 150 cities stay in seconds.  Passes are counted as the kernel counts them: every evaluated pass, the
fruitless one that ends a convergence included."""
import functools

import numpy as np


def seq_length(d, tour):
    """distance_calc of the closed tour over the open `tour`: 0 + e_0 + e_1 + .. left to right, the closing edge last"""
    t = np.asarray(tour, dtype=np.int64)
    e = d[t, np.roll(t, -1)]
    return float(np.add.accumulate(np.concatenate([[0.0], e]))[-1])


def neighbour_chain(d, start, farthest=False):
    """c_0 = start, c_{k+1} = argmin (farthest: argmax) of d[c_k, :] over the cities not yet in the chain, first among equals"""
    n = d.shape[0]
    fill = -np.inf if farthest else np.inf
    free = np.ones(n, dtype=bool)
    chain = [int(start)]
    free[start] = False
    for _ in range(n - 1):
        row = np.where(free, d[chain[-1]], fill)
        nxt = int(row.argmax() if farthest else row.argmin())
        chain.append(nxt)
        free[nxt] = False
    return np.asarray(chain, dtype=np.int64)


@functools.lru_cache(maxsize=None)
def _candidates(m):
    """(I, J, P): the reversals [i..j], 0 <= i < j <= m - 1, in (i, j) order, and P [M, m]: candidate c holds seed position P[c, k]
    at position k"""
    I, J = np.triu_indices(m, 1)
    k = np.arange(m)[None, :]
    inside = (k >= I[:, None]) & (k <= J[:, None])
    P = np.where(inside, I[:, None] + J[:, None] - k, k)
    for a in (I, J, P):
        a.setflags(write=False)
    return I, J, P


def one_pass(d, tour, cur):
    """-> (tour', value, i, j): the first strict minimum below `cur` in (i, j) order applied, or (tour, cur, -1, -1)"""
    t = np.asarray(tour, dtype=np.int64)
    m = len(t)
    I, J, P = _candidates(m)
    C = t[P]
    E = d[C, np.roll(C, -1, axis=1)]
    V = np.add.accumulate(np.concatenate([np.zeros((len(C), 1)), E], axis=1), axis=1)[:, -1]
    lo = V.min()
    if not lo < cur:
        return t, cur, -1, -1
    c = int(np.flatnonzero(V == lo)[0])
    return C[c].copy(), float(lo), int(I[c]), int(J[c])


def converge(d, tour, max_passes=None):
    """-> (tour, length, passes, status): passes until one brings nothing; status 1 once `max_passes` passes have improved"""
    t = np.asarray(tour, dtype=np.int64)
    cur, passes = seq_length(d, t), 0
    while True:
        t, cur, i, _ = one_pass(d, t, cur)
        passes += 1
        if i < 0:
            return t, cur, passes, 0
        if max_passes is not None and passes == max_passes:
            return t, cur, passes, 1


def grow(d, order, m_seed=2, m_end=None, first_m=3, max_passes=None):
    """rls_tsp_grow_2opt for one row -> (tours [N], length, passes, status)"""
    order = np.asarray(order, dtype=np.int64)
    n = len(order)
    m_end = n if m_end is None else m_end
    if ((order < 0) | (order >= d.shape[0])).any():
        return None, None, None, 2
    t, passes, status = order[:m_seed].copy(), 0, 0
    for m in range(m_seed, m_end + 1):
        if m > m_seed:
            t = np.concatenate([t, order[m - 1:m]])
        if m >= first_m:
            t, _, p, status = converge(d, t, max_passes)
            passes += p
            if status:
                break
    return np.concatenate([t, order[len(t):]]), seq_length(d, t), passes, status


def _route(t):
    return [int(c) + 1 for c in t] + [int(t[0]) + 1]


def _starts(n, initial_location):
    return list(range(n)) if initial_location == -1 else [initial_location - 1]


def _best_start(results):
    """the first start whose length is strictly smallest -> (route, distance)"""
    best = None
    for t, v in results:
        if best is None or v < best[1]:
            best = (t, v)
    return _route(best[0]), float(best[1])


def nearest_neighbour(d, initial_location=-1, local_search=True):
    d = np.asarray(d, dtype=np.float64)
    n, out = d.shape[0], []
    for s in _starts(n, initial_location):
        chain = neighbour_chain(d, s)
        t, v, _, _ = grow(d, chain, m_seed=n, first_m=n if local_search else n + 1)
        out.append((t, v))
    return _best_start(out)


def _insertion(d, initial_location, farthest):
    d = np.asarray(d, dtype=np.float64)
    out = []
    for s in _starts(d.shape[0], initial_location):
        t, v, _, _ = grow(d, neighbour_chain(d, s, farthest))
        out.append((t, v))
    return _best_start(out)


def nearest_insertion(d, initial_location=-1):
    return _insertion(d, initial_location, False)


def farthest_insertion(d, initial_location=-1):
    return _insertion(d, initial_location, True)


def cheapest_insertion(d):
    d = np.asarray(d, dtype=np.float64)
    n = d.shape[0]
    i, j = np.unravel_index(np.argmax(d, axis=None), d.shape)
    t = np.asarray([i, j], dtype=np.int64)
    while len(t) < n:
        best = None
        for c in (c for c in range(n) if c not in set(t.tolist())):           # ascending; the first minimum stays
            order = np.concatenate([t, [c], np.zeros(n - len(t) - 1, dtype=np.int64)])
            tt, v, _, _ = grow(d, order, m_seed=len(t), m_end=len(t) + 1, first_m=len(t) + 1)
            if best is None or v < best[1]:
                best = (tt[:len(t) + 1], v)
        t = best[0]
    return _route(t), seq_length(d, t)
