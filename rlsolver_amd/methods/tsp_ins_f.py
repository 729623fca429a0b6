"""Farthest insertion -- drop-in for rlsolver/methods_problem_specific/TSP/ins_f.py.

    distance_calc(distance_matrix, city_tour) -> float
    local_search_2_opt(distance_matrix, city_tour, recursive_seeding=-1, verbose=True) -> (route, distance)
    best_insertion(distance_matrix, temp) -> temp
    farthest_insertion(distance_matrix, initial_location=-1, verbose=True) -> (route, distance)

As methods/tsp_ins_n.py with the FARTHEST city not yet visited from the one taken last.  All starts run in one chain launch and
one grow launch (methods/tsp_construct.py); routes (closed, 1-based) and distances (Python floats) are bit-identical to the
reference's."""
from __future__ import annotations

from . import tsp_construct as _c
from .tsp_opt_2 import distance_calc, local_search_2_opt  # noqa: F401


def best_insertion(distance_matrix, temp, *, device=None):
    """ins_f.py:61-68"""
    return _c.best_insertion(distance_matrix, temp, device=device)


def farthest_insertion(distance_matrix, initial_location=-1, verbose=True, *, device=None):
    """ins_f.py:73-108"""
    return _c.construct(distance_matrix, initial_location, True, True, True, verbose, device, "farthest_insertion")
