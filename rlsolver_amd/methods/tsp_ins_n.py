"""Nearest insertion -- drop-in for rlsolver/methods_problem_specific/TSP/ins_n.py.

    distance_calc(distance_matrix, city_tour) -> float
    local_search_2_opt(distance_matrix, city_tour, recursive_seeding=-1, verbose=True) -> (route, distance)
    best_insertion(distance_matrix, temp) -> temp
    nearest_insertion(distance_matrix, initial_location=-1, verbose=True) -> (route, distance)

From every start (``initial_location = -1``) or from city ``initial_location`` (1-based): the nearest city not yet visited to the
one taken last joins the END of the tour, which is then 2-opted until a pass brings nothing (best_insertion), size after size; the
first start whose tour is strictly shortest wins.  All starts run in one chain launch and one grow launch
(methods/tsp_construct.py); routes (closed, 1-based) and distances (Python floats) are bit-identical to the reference's."""
from __future__ import annotations

from . import tsp_construct as _c
from .tsp_opt_2 import distance_calc, local_search_2_opt  # noqa: F401


def best_insertion(distance_matrix, temp, *, device=None):
    """ins_n.py:61-68"""
    return _c.best_insertion(distance_matrix, temp, device=device)


def nearest_insertion(distance_matrix, initial_location=-1, verbose=True, *, device=None):
    """ins_n.py:73-108"""
    return _c.construct(distance_matrix, initial_location, False, True, True, verbose, device, "nearest_insertion")
