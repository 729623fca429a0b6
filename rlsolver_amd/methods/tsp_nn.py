"""Nearest neighbour -- drop-in for rlsolver/methods_problem_specific/TSP/nn.py.

    distance_calc(distance_matrix, city_tour) -> float
    local_search_2_opt(distance_matrix, city_tour, recursive_seeding=-1, verbose=True) -> (route, distance)
    nearest_neighbour(distance_matrix, initial_location=-1, local_search=True, verbose=True) -> (route, distance)

From every start (``initial_location = -1``) or from city ``initial_location`` (1-based): always on to the nearest city not yet
visited, the lowest index among equals, then (``local_search``) 2-opt until a pass brings nothing; the first start whose tour is
strictly shortest wins.  All starts run in one chain launch and one convergence launch (methods/tsp_construct.py); routes (closed,
1-based) and distances (Python floats) are bit-identical to the reference's."""
from __future__ import annotations

from . import tsp_construct as _c
from .tsp_opt_2 import distance_calc, local_search_2_opt  # noqa: F401


def nearest_neighbour(distance_matrix, initial_location=-1, local_search=True, verbose=True, *, device=None):
    """nn.py:58-97"""
    return _c.construct(distance_matrix, initial_location, False, False, bool(local_search), verbose, device, "nearest_neighbour")
