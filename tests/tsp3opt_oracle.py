"""numpy restatement of one pass of the reference's 3-opt (methods_problem_specific/TSP/opt_3.py:42-105) in both rankings of
rls_tsp_3opt_best, and of the search around it.  Vectorised over the candidates of one `i` at a time (bounded memory),
sequential over tour positions, so every float64 sum is made of the same additions in the same order as the reference's
distance_calc (exact ranking) or as include/rlsolver_hip.h states them (delta ranking).  Imports nothing from rlsolver_amd."""
import numpy as np

# trial -> is S1 / S2 / C reversed: aBC AbC ABc Abc abC aBc abc
REV = np.array([[1, 0, 0, 0, 1, 1, 1], [0, 1, 0, 1, 1, 0, 1], [0, 0, 1, 1, 0, 1, 1]], dtype=bool)
TRIALS = ("aBC", "AbC", "ABc", "Abc", "abC", "aBc", "abc")


def segments(n):
    return [(i, j, k) for i in range(n) for j in range(i + 1, n) for k in range(j + 1, n + (i > 0))]


def count_segments(n):
    return n * (n - 1) * (n - 2) // 6 + (n - 1) * (n - 2) // 2


def distance_calc(D, closed_1based):
    total = 0
    for a, b in zip(closed_1based[:-1], closed_1based[1:]):
        total = total + D[a - 1, b - 1]
    return total


def pairs_of(n, i):
    """(j, k) of every triple that starts with i, in order"""
    top = n + (i > 0)
    js = np.repeat(np.arange(i + 1, n), [top - (j + 1) for j in range(i + 1, n)])
    ks = np.concatenate([np.arange(j + 1, top) for j in range(i + 1, n)]) if len(js) else np.zeros(0, dtype=np.int64)
    return js.astype(np.int64), ks.astype(np.int64)


def source_positions(n, i, js, ks, trial):
    """[M, n]: the seed position each position of the candidate takes its city from"""
    p = np.arange(n)[None, :]
    J, KE = js[:, None], np.minimum(ks, n - 1)[:, None]
    src = np.where((p > i) & (p <= J) & REV[0, trial], i + 1 + J - p, p)
    src = np.where((p > J) & (p <= KE) & REV[1, trial], J + 1 + KE - p, src)
    return np.where((p > KE) & REV[2, trial], KE + n - p, src)


def apply_move(tour, i, j, k, trial):
    t = np.asarray(tour)
    return t[source_positions(len(t), i, np.array([j]), np.array([k]), trial)[0]]


def _values_exact(D, t, i, js, ks):
    n = len(t)
    out = np.empty((len(js), 7))
    for r in range(7):
        tours = t[source_positions(n, i, js, ks, r)]
        v = np.zeros(len(js))
        for p in range(n):
            v = v + D[tours[:, p], tours[:, (p + 1) % n]]
        out[:, r] = v
    return out


def _values_delta(D, t, i, js, ks):
    n = len(t)
    ke = np.minimum(ks, n - 1)
    has2, hasc = js + 1 <= ke, ke + 1 <= n - 1
    f2, l2 = t[np.minimum(js + 1, n - 1)], t[ke]
    fc, lc = t[np.minimum(ke + 1, n - 1)], t[n - 1]
    ci, f1, l1 = t[i], t[i + 1], t[js]
    out = np.empty((len(js), 7))
    old = D[ci, f1] + np.zeros(len(js))
    po = l1
    old = np.where(has2, old + D[po, f2], old)
    po = np.where(has2, l2, po)
    old = np.where(hasc, old + D[po, fc], old)
    po = np.where(hasc, lc, po)
    old = old + D[po, t[0]]
    for r in range(7):
        new = D[ci, l1 if REV[0, r] else f1] + np.zeros(len(js))
        pc = (f1 + np.zeros(len(js), dtype=np.int64)) if REV[0, r] else l1
        new = np.where(has2, new + D[pc, l2 if REV[1, r] else f2], new)
        pc = np.where(has2, f2 if REV[1, r] else l2, pc)
        new = np.where(hasc, new + D[pc, lc if REV[2, r] else fc], new)
        pc = np.where(hasc, fc if REV[2, r] else lc, pc)
        out[:, r] = (new + D[pc, t[0]]) - old
    return out


def one_pass(D, tour, cur=None):
    """tour: open, 0-based.  cur given: exact ranking against cur; None: delta ranking against 0.
    -> (i, j, k, trial, value), or (-1, -1, -1, -1, cur or 0.0) when nothing is strictly better"""
    D = np.asarray(D, dtype=np.float64)
    t = np.asarray(tour, dtype=np.int64)
    n = len(t)
    best = np.float64(0.0 if cur is None else cur)
    win = (-1, -1, -1, -1)
    for i in range(n - 1):
        js, ks = pairs_of(n, i)
        if not len(js):
            continue
        vals = (_values_delta if cur is None else _values_exact)(D, t, i, js, ks).reshape(-1)
        a = int(np.argmin(vals))                                   # the first of equals
        if vals[a] < best:
            best, win = vals[a], (i, int(js[a // 7]), int(ks[a // 7]), a % 7)
    return win + (float(best),)


def one_pass_exact_grouped(D, tour, cur):
    """one_pass(D, tour, cur) -- the same candidates, the same additions in the same order for each, the same answer -- in a
    fraction of the time: candidates that share the beginning of their walk share its partial sum.  A candidate's sum runs
    through H and S1 (it then depends on (i, j) and whether S1 is reversed), through S2 (then also on ke = min(k, n - 1) and
    whether S2 is reversed), through C and the closing edge.  All candidates with one ke walk the SAME edges after S2, only from
    different partial sums: a scalar added to an array per position, no gather.  Arrays are indexed [j, i] (i < j valid).
    tests/test_tsp3opt_oracle.py holds this function against one_pass; the GPU tests use it where one_pass takes too long."""
    D = np.asarray(D, dtype=np.float64)
    t = np.asarray(tour, dtype=np.int64)
    n = len(t)
    fwd, bwd = D[t[:-1], t[1:]], D[t[1:], t[:-1]]               # the edge between positions p and p + 1, walked up / walked down
    S = np.zeros(n)
    for p in range(n - 1):
        S[p + 1] = S[p] + fwd[p]
    jj, ii = np.meshgrid(np.arange(n), np.arange(n), indexing="ij")
    valid = ii < jj
    base = (ii * n + jj) * (n + 1) * 8
    state = {"best": np.float64(cur), "key": -1}

    def consider(vals, keys, ok):
        vals = np.where(ok, vals, np.inf)
        m = vals.min()
        if m < state["best"] or (m == state["best"] and state["key"] >= 0):
            k = int(keys[vals == m].min())
            if m < state["best"] or k < state["key"]:
                state["best"], state["key"] = m, k

    # after S1: A[r1][j, i] and the city the walk stands on
    A = np.zeros((2, n, n))
    pcA = np.zeros((2, n, n), dtype=np.int64)
    A[0] = S[:, None]
    pcA[0] = t[:, None]
    pcA[1, :, :n - 1] = t[None, 1:]                             # t[i + 1]
    for j in range(1, n):
        v = S[:j] + D[t[:j], t[j]]
        for s in range(1, j):
            v[:j - s] += bwd[j - s]
        A[1, j, :j] = v
    R1, R2, R3 = REV.astype(int)
    run0 = np.zeros((2, n, n))                                  # S2 straight: grows by one edge per ke
    for ke in range(1, n):
        if ke >= 2:
            run0[:, :ke - 1] += fwd[ke - 1]
        run0[:, ke - 1] = A[:, ke - 1] + D[pcA[:, ke - 1], t[ke]]
        run1 = A[:, :ke] + D[pcA[:, :ke], t[ke]]               # S2 reversed: from t[ke] down to t[j + 1]
        for s in range(1, ke):
            run1[:, :ke - s] += bwd[ke - s]
        start = np.stack([run0[:, :ke], run1])                  # [r2, r1, j, i]
        pc = np.stack([np.full((2, ke, n), t[ke]), np.broadcast_to(t[1:ke + 1][None, :, None], (2, ke, n))])
        if ke < n - 1:
            up = start + D[pc, t[ke + 1]]
            for p in range(ke + 1, n - 1):
                up += fwd[p]
            up += D[t[n - 1], t[0]]
            down = start + D[pc, t[n - 1]]
            for p in range(n - 2, ke, -1):
                down += bwd[p]
            down += D[t[ke + 1], t[0]]
            final, ks = np.stack([up, down]), [ke]              # [r3, r2, r1, j, i]
        else:
            final, ks = np.stack([start + D[pc, t[0]]] * 2), [n - 1, n]
        for k in ks:
            ok = valid[:ke] & ((ii[:ke] > 0) | (k < n))
            for r in range(7):
                consider(final[R3[r], R2[r], R1[r]], base[:ke] + k * 8 + r, ok)
    # S2 and C empty: (i, n - 1, n), i > 0
    last = A[:, n - 1] + D[pcA[:, n - 1], t[0]]
    for r in range(7):
        consider(last[R1[r]], base[n - 1] + n * 8 + r, valid[n - 1] & (ii[n - 1] > 0))
    key = state["key"]
    if key < 0:
        return (-1, -1, -1, -1, float(cur))
    q = key >> 3
    return (q // (n + 1) // n, q // (n + 1) % n, q % (n + 1), key & 7, float(state["best"]))


def local_search(D, closed_1based, cur, recursive_seeding=-1):
    """the reference's outer loop in exact ranking -> (closed 1-based route, distance)"""
    t = np.asarray(closed_1based[:-1], dtype=np.int64) - 1
    done = 0
    while recursive_seeding < 0 or done < recursive_seeding:
        i, j, k, r, v = one_pass(D, t, cur)
        done += 1
        if i < 0:
            if recursive_seeding < 0:
                break
            continue
        t, cur = apply_move(t, i, j, k, r), v
    route = [int(c) + 1 for c in t]
    return route + [route[0]], cur
