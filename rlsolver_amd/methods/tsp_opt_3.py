"""The reference's 3-opt local search -- drop-in for rlsolver/methods_problem_specific/TSP/opt_3.py:17-105.

    distance_calc(distance_matrix, city_tour) -> float                 (the reference's sequential float64 sum)
    segments_3_opt(n) -> [(i, j, k), ...]                               (the reference's list of triples, in its order)
    local_search_3_opt(distance_matrix, city_tour, recursive_seeding=-1, verbose=True) -> (route, distance)
    local_search_3_opt_batch(distance_matrix, perms, max_passes=-1) -> (perms, lengths)      many tours at once

``city_tour = [route, distance]`` with ``route`` the closed tour as 1-based city numbers (first city repeated at the end),
as in the reference.  The reference's move reverses blocks in place and moves none: a triple (i, j, k) cuts the open tour
into H = t[:i+1], S1 = t[i+1:j+1], S2 = t[j+1:k+1], C = t[k+1:], and the seven trials aBC AbC ABc Abc abC aBc abc (a
lower-case letter: that block reversed) are compared by the length of the whole closed tour, re-summed in Python for each of
the 7 (C(n, 3) + C(n - 1, 2)) candidates of a pass.  Here a pass is ONE kernel (rls_tsp_3opt_best, the (i, j) pairs of a
tour dealt to the waves of its workgroups) and a gather.  Two rankings of the candidates:

  exact (local_search_3_opt, and the batch form with exact=True): each candidate's whole length, summed in float64 edge
        after edge as distance_calc does -- the reference's own comparison values, so routes AND distances are
        bit-identical to the reference's, ties, rounding and its degenerate trials included, for any matrix;
  delta (batch form, default): new minus old junction edges in float64, O(1) per candidate, symmetric matrices only;
        candidates whose lengths agree to rounding may rank differently than under the reference's re-summation.

What the reference does with the distance it is handed is kept: the seed tour is itself among the candidates, so a
``city_tour[1]`` larger than the tour's true length is replaced by that length, and ``city_tour[1] = 0.0`` lets nothing win.
"""
from __future__ import annotations

import numpy as np
import torch

from .. import ops_mcpg_tsp as mops
from .tsp_opt_2 import _device_matrix, _lengths, distance_calc  # noqa: F401  (distance_calc: opt_3.py:17-22 is opt_2.py's)

# trial -> is S1 / S2 / C reversed (aBC AbC ABc Abc abC aBc abc)
_REV = ((1, 0, 0, 0, 1, 1, 1), (0, 1, 0, 1, 1, 0, 1), (0, 0, 1, 1, 0, 1, 1))


def segments_3_opt(n):
    """opt_3.py:27-37: (i, j, k) with 0 <= i < j < n and j < k < n + (i > 0), in the reference's order."""
    return [(i, j, k) for i in range(n) for j in range(i + 1, n) for k in range(j + 1, n + (i > 0))]


def _apply_moves(perms, bi, bj, bk, bt):
    """perms[b] with S1 = [i+1..j], S2 = [j+1..min(k, N-1)] and C = the rest reversed in place as trial bt[b] says, where
    bi[b] >= 0 (one gather)."""
    B, N = perms.shape
    dev = perms.device
    p = torch.arange(N, device=dev).unsqueeze(0)
    won = (bi >= 0).unsqueeze(1)
    i, j = bi.unsqueeze(1), bj.unsqueeze(1)
    ke = torch.clamp(bk, max=N - 1).unsqueeze(1)
    rev = torch.tensor(_REV, dtype=torch.bool, device=dev)[:, torch.clamp(bt, min=0)]          # [3, B]
    in1, in2, in3 = (p > i) & (p <= j), (p > j) & (p <= ke), p > ke
    src = torch.where(in1 & rev[0].unsqueeze(1), i + 1 + j - p, p)
    src = torch.where(in2 & rev[1].unsqueeze(1), j + 1 + ke - p, src)
    src = torch.where(in3 & rev[2].unsqueeze(1), ke + N - p, src)
    return torch.gather(perms, 1, torch.where(won, src, p))


def local_search_3_opt_batch(distance_matrix, perms, max_passes: int = -1, exact: bool = False, lengths=None):
    """Best-improvement passes of the reference's 3-opt over a batch of open 0-based tours int64 [B, N] on a HIP device until
    no tour improves (max_passes < 0) or for max_passes passes.  -> (perms, float64 lengths [B]).  ``exact``: rank candidates
    as the reference does (see the module docstring); ``lengths`` then seeds the comparison (default: computed here).
    Without ``exact`` the matrix must be symmetric."""
    if perms.device.type != "cuda":
        raise TypeError("local_search_3_opt_batch needs a HIP device; there is no CPU path")
    d = _device_matrix(distance_matrix, perms.device, symmetric=not exact)
    perms = perms.to(torch.int64).contiguous().clone()
    if perms.dim() != 2 or perms.shape[1] != d.shape[0] or not bool((perms.sort(dim=1).values == torch.arange(d.shape[0], device=perms.device)).all()):
        raise ValueError("perms must be [B, N] permutations of 0..N-1")
    if exact:
        cur = (_lengths(d, perms) if lengths is None else lengths.to(torch.float64)).contiguous().clone()
    done = 0
    while max_passes < 0 or done < max_passes:
        bi, bj, bk, bt, bv = mops.tsp_3opt_best(d, perms, cur if exact else None)
        if not bool((bi >= 0).any()):         # the host decides when to stop, as the reference's while loop does
            break
        perms = _apply_moves(perms, bi, bj, bk, bt)
        if exact:
            cur = bv
        done += 1
    return perms, (cur if exact else _lengths(d, perms))


def local_search_3_opt(distance_matrix, city_tour, recursive_seeding: int = -1, verbose: bool = True, device=None):
    """opt_3.py:42-105: (route, distance) after best-improvement passes -- until a pass brings nothing when
    ``recursive_seeding < 0``, else exactly ``recursive_seeding`` passes.  Bit-identical to the reference."""
    route = [int(c) for c in city_tour[0]]
    n = len(route) - 1
    if n < 1 or route[0] != route[-1] or sorted(route[:-1]) != list(range(1, n + 1)):
        raise ValueError("city_tour[0] must be a closed tour over cities 1..N (first city repeated at the end)")
    if tuple(distance_matrix.shape if hasattr(distance_matrix, "shape") else np.shape(distance_matrix)) != (n, n):
        raise ValueError(f"city_tour[0] must be a closed tour over the {n} cities of a [{n}, {n}] distance_matrix")
    device = torch.device(device) if device is not None else torch.device("cuda:0")
    if device.type != "cuda":
        raise TypeError("local_search_3_opt needs a HIP device; there is no CPU path")
    d = _device_matrix(distance_matrix, device, symmetric=False)
    perm = torch.tensor([[c - 1 for c in route[:-1]]], dtype=torch.int64, device=device)
    distance = city_tour[1]
    cur = torch.tensor([float(distance)], dtype=torch.float64, device=device)
    iteration = 0
    while recursive_seeding < 0 or iteration < recursive_seeding:
        if verbose:
            print('Iteration = ', iteration, 'Distance = ', round(float(distance), 2))
        bi, bj, bk, bt, bv = mops.tsp_3opt_best(d, perm, cur)
        iteration += 1
        if int(bi[0]) < 0:                    # nothing shorter than the pass's seed
            if recursive_seeding < 0:
                break
            continue
        perm = _apply_moves(perm, bi, bj, bk, bt)
        cur = bv
        distance = float(bv[0])
    if iteration:
        route = [int(c) + 1 for c in perm[0].tolist()]
        route.append(route[0])
    return route, distance
