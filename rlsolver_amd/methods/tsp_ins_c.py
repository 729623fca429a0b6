"""Cheapest insertion -- drop-in for rlsolver/methods_problem_specific/TSP/ins_c.py.

    distance_calc(distance_matrix, city_tour) -> float
    local_search_2_opt(distance_matrix, city_tour, recursive_seeding=-1, verbose=True) -> (route, distance)
    cheapest_insertion(distance_matrix, verbose=True) -> (route, distance)

From the two cities of the largest entry: every absent city in turn joins the end of the tour, which is 2-opted until a pass brings
nothing, and the first shortest result is kept -- N - 2 launches, a row per absent city (methods/tsp_construct.py).  Routes
(closed, 1-based) and distances (Python floats) are bit-identical to the reference's."""
from __future__ import annotations

from . import tsp_construct as _c
from .tsp_opt_2 import distance_calc, local_search_2_opt  # noqa: F401


def cheapest_insertion(distance_matrix, verbose=True, *, device=None):
    """ins_c.py:60-95"""
    return _c.cheapest_insertion(distance_matrix, verbose, device)
