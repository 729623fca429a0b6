"""The reference's tour constructors on the device -- the shared implementation behind methods/tsp_nn.py, tsp_ins_n.py,
tsp_ins_f.py and tsp_ins_c.py (rlsolver/methods_problem_specific/TSP/nn.py, ins_n.py, ins_f.py, ins_c.py).

All four are deterministic, and restated they are two steps:

  * the ORDER in which nn.py / ins_n.py / ins_f.py take up cities does not depend on the 2-opt in between: the next city is the
    nearest (ins_f.py: farthest) to the one taken last among the cities not yet taken, the lowest index among equals --
    ``neighbour_chains`` (rls_tsp_neighbour_chain, a wave per start);
  * a tour takes the next city at its END and is then 2-opted until a pass brings nothing, size after size -- ``grow_2opt``
    (rls_tsp_grow_2opt, a persistent workgroup per start: the partial tour, its running sums and the float64 matrix stay in LDS
    and passes repeat without a launch or a host read).  A pass ranks candidates as the reference does (the exact ranking of
    tsp_opt_2), so routes AND distances are bit-identical to the reference's, ties and rounding included, for any matrix.

nearest_neighbour is the chain as the tour and one convergence at full size; the insertions converge at every size from three
cities on; cheapest_insertion is a host loop of N - 2 launches, each trying every absent city at the end of the tour.  The
reference re-sums every candidate of every pass of every insertion in Python: seconds per start at 52 cities.

Two batch forms for callers that hold many starts:

    neighbour_chains(d, starts, farthest=False) -> chains int64 [S, N]
    grow_2opt(d, order, m_seed=2, m_end=None, first_m=3, max_passes=None) -> (tours int64 [S, N], lengths f64 [S], passes int64 [S])

The reference's 2-opt stops after one pass when it is handed a tour of length <= 0 (its `distance * 2 > distance` test); with
distances >= 0 that changes nothing, and negative matrices are outside what this file reproduces.  There is no CPU path."""
from __future__ import annotations

import numpy as np
import torch

from .. import ops_mcpg_tsp as mops
from .tsp_opt_2 import distance_calc  # noqa: F401


def checked_matrix(distance_matrix):
    """-> float64 tensor [N, N] (where it lives), refused with ValueError unless square, N >= 2 and finite"""
    d = distance_matrix if torch.is_tensor(distance_matrix) else torch.as_tensor(np.asarray(distance_matrix, dtype=np.float64))
    d = d.detach().to(torch.float64)
    if d.dim() != 2 or d.shape[0] != d.shape[1]:
        raise ValueError(f"distance_matrix must be square, got {tuple(d.shape)}")
    if d.shape[0] < 2:
        raise ValueError(f"distance_matrix must hold N >= 2 cities, got {d.shape[0]}")
    if not bool(torch.isfinite(d).all()):
        raise ValueError("distance_matrix must hold finite entries")
    return d.contiguous()


def hip_device(device, what):
    device = torch.device(device) if device is not None else torch.device("cuda:0")
    if device.type != "cuda":
        raise TypeError(f"{what} needs a HIP device; there is no CPU path")
    return device


def checked_starts(n, initial_location):
    """the 0-based starts of `initial_location` (-1: all N), refused with ValueError when it names no city"""
    loc = int(initial_location)
    if loc == -1:
        return list(range(n))
    if not 1 <= loc <= n:
        raise ValueError(f"initial_location must be -1 or a city in 1..{n}, got {initial_location}")
    return [loc - 1]


def neighbour_chains(d, starts, farthest: bool = False):
    """chains[s] = starts[s], then again and again the nearest (``farthest``: farthest) city to the last one among those not yet in
    the chain, the lowest index among equals: the order in which nn.py / ins_n.py (ins_f.py) take up cities.  ``starts`` int64 [S]
    on a HIP device, ``d`` float64 [N, N].  -> int64 [S, N]."""
    if not torch.is_tensor(starts) or starts.device.type != "cuda":
        raise TypeError("neighbour_chains needs starts on a HIP device; there is no CPU path")
    d = checked_matrix(d).to(starts.device)
    starts = starts.to(torch.int64).contiguous()
    if starts.dim() != 1 or bool(((starts < 0) | (starts >= d.shape[0])).any()):
        raise ValueError(f"starts must be [S] cities in 0..{d.shape[0] - 1}")
    chains, status = mops.tsp_neighbour_chain(d, starts, farthest)
    if bool((status != 0).any()):
        raise ValueError("a start lies outside the matrix")
    return chains


def grow_2opt(d, order, m_seed: int = 2, m_end=None, first_m: int = 3, max_passes=None):
    """Row s starts as order[s, :m_seed]; for m = m_seed .. m_end it takes order[s, m - 1] at its end (m > m_seed) and, from m =
    first_m on, is 2-opted on the closed m-city tour until a pass finds nothing strictly shorter -- the reference's ranking, bit for
    bit.  ``order`` int64 [S, N] on a HIP device (rows: permutations of 0..N-1), ``d`` float64 [N, N]; m_end defaults to N.
    -> (tours int64 [S, N]: the tour in [:m_end], order's tail behind it; lengths float64 [S]: the sequential float64 sum of the
    closed tour; passes int64 [S]: evaluated passes, the fruitless last one of every convergence included).
    ``max_passes`` (default N^2) bounds one convergence -- a guard that guarantees the kernel returns, not a tuning value: reaching
    it raises RuntimeError."""
    if not torch.is_tensor(order) or order.device.type != "cuda":
        raise TypeError("grow_2opt needs order on a HIP device; there is no CPU path")
    d = checked_matrix(d).to(order.device)
    order = order.to(torch.int64).contiguous()
    tours, lengths, passes, status = mops.tsp_grow_2opt(d, order, m_seed, m_end, first_m, max_passes)
    status = status.cpu()
    if bool((status == 2).any()):
        raise ValueError(f"order must hold cities in 0..{d.shape[0] - 1}")
    if bool((status == 1).any()):
        raise RuntimeError(f"2-opt did not converge within max_passes = {d.shape[0] ** 2 if max_passes is None else max_passes} passes "
                           f"(rows {torch.nonzero(status == 1).flatten().tolist()[:8]})")
    return tours, lengths, passes


def first_minimum(values):
    """index of the first strictly smallest entry, as the reference's `if val < minimum` keeps it"""
    best = 0
    for k, v in enumerate(values):
        if v < values[best]:
            best = k
    return best


def closed_route(tour):
    route = [int(c) + 1 for c in tour]
    return route + [route[0]]


def construct(distance_matrix, initial_location, farthest, insertion, local_search, verbose, device, what):
    """the body of nearest_neighbour / nearest_insertion / farthest_insertion: one chain launch and one grow launch for all starts.
    ``insertion``: converge at every size from three cities on; else the chain is the tour, converged once (``local_search``) or
    only measured."""
    d = checked_matrix(distance_matrix)
    n = d.shape[0]
    starts = checked_starts(n, initial_location)
    device = hip_device(device, what)
    d = d.to(device)
    chains = neighbour_chains(d, torch.tensor(starts, dtype=torch.int64, device=device), farthest)
    if insertion:
        tours, lengths, _ = grow_2opt(d, chains, m_seed=2, first_m=3)
    else:
        tours, lengths, _ = grow_2opt(d, chains, m_seed=n, first_m=n if local_search else n + 1)
    lengths = lengths.tolist()
    if verbose:
        best = float('+inf')
        for i1, val in zip(starts, lengths):
            best = min(best, val)
            print('Iteration = ', i1, 'Distance = ', round(best, 2))
    k = first_minimum(lengths)
    return closed_route(tours[k].tolist()), lengths[k]


def best_insertion(distance_matrix, temp, device=None):
    """ins_n.py:61-68: the open 0-based (partial) tour ``temp`` 2-opted until a pass brings nothing -> the 0-based tour"""
    d = checked_matrix(distance_matrix)
    n = d.shape[0]
    temp = [int(c) for c in temp]
    if len(set(temp)) != len(temp) or any(not 0 <= c < n for c in temp):
        raise ValueError(f"temp must hold different cities in 0..{n - 1}")
    if len(temp) < 2:
        return temp
    device = hip_device(device, "best_insertion")
    rest = [c for c in range(n) if c not in set(temp)]
    order = torch.tensor([temp + rest], dtype=torch.int64, device=device)
    tours, _, _ = grow_2opt(d.to(device), order, m_seed=len(temp), m_end=len(temp), first_m=len(temp))
    return tours[0, :len(temp)].tolist()


def cheapest_insertion(distance_matrix, verbose=True, device=None):
    """ins_c.py:60-95: from the two cities of the largest entry, N - 2 times: every absent city in turn at the end of the tour,
    2-opted until a pass brings nothing (one launch, a row per absent city), the first shortest kept.  Prints what the reference
    prints (its `distance:` line whatever ``verbose`` says)."""
    d = checked_matrix(distance_matrix)
    n = d.shape[0]
    host = d.cpu().numpy()
    i, idx = (int(v) for v in np.unravel_index(np.argmax(host, axis=None), host.shape))
    if i == idx:
        raise ValueError("the largest entry of distance_matrix lies on the diagonal: the reference would start from a repeated city")
    device = hip_device(device, "cheapest_insertion")
    d = d.to(device)
    temp, count = [i, idx], 0
    distance = float(distance_calc(host, [closed_route(temp), 1]))
    while len(temp) < n:
        m = len(temp)
        absent = [c for c in range(n) if c not in set(temp)]
        order = torch.tensor([temp + [c] + [a for a in absent if a != c] for c in absent], dtype=torch.int64, device=device)
        tours, lengths, _ = grow_2opt(d, order, m_seed=m, m_end=m + 1, first_m=m + 1)
        lengths = lengths.tolist()
        k = first_minimum(lengths)
        temp, distance = tours[k, :m + 1].tolist(), lengths[k]
        if verbose:
            print('Iteration = ', count)
        count = count + 1
    route = closed_route(temp)
    print("distance: ", distance)
    return route, distance
