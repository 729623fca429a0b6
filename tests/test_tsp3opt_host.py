"""What of the 3-opt path runs without a GPU: the C ABI's two new entries and their ctypes rows, the launch form of
rls_tsp_3opt_best (csrc/rls_tsp3_plan.h) against the formula include/rlsolver_hip.h documents, the host functions of
rlsolver_amd.methods.tsp_opt_3 against the reference's recorded results, and the refusals that come before any device work."""
import numpy as np
import pytest
import torch

from tests.test_abi import declared_functions

LDS = 160 * 1024           # the LDS of a compute unit: what a workgroup may ask for
WAVES_STAGED, WAVES_GLOBAL = 16, 4


def lds_bytes(n, exact, waves, staged):
    """include/rlsolver_hip.h, rls_tsp_3opt_launch_form: lds_d * 8 N^2 + exact * 8 (N + 1) + 16 waves + 4 N"""
    return staged * 8 * n * n + exact * 8 * (n + 1) + 16 * waves + 4 * n


def test_abi_lists_both_entries_with_the_header_s_argument_counts():
    from rlsolver_amd import _abi, torch_ops
    fns = declared_functions()
    assert fns["rls_tsp_3opt_best"] == 12 and fns["rls_tsp_3opt_launch_form"] == 3
    assert len(_abi.SIGNATURES["rls_tsp_3opt_best"]) == 12 and len(_abi.SIGNATURES["rls_tsp_3opt_launch_form"]) == 3
    assert "tsp_3opt_best" in torch_ops.DEVICE_ENTRY_POINTS and "tsp_3opt_launch_form" in torch_ops.HOST_ENTRY_POINTS
    assert _abi.version() == 12
    names = [a.name for a in torch.ops.rlsolver_hip.tsp_3opt_best.default._schema.arguments]
    assert names == ["dist", "perm", "cur_length", "best_i", "best_j", "best_k", "best_trial", "best_value"]


@pytest.mark.parametrize("exact", [0, 1])
def test_launch_form_follows_the_documented_formula(exact):
    from rlsolver_amd import _abi
    form = lambda n: _abi.tsp_3opt_launch_form(n, exact)      # noqa: E731
    fields = lambda f: (f.lds_d, f.tab8, f.block, f.waves, f.lds_bytes, f.kernel, f.supported)      # noqa: E731
    last_staged = max(n for n in range(3, 400) if lds_bytes(n, exact, WAVES_STAGED, 1) <= LDS)
    first_refused = min(n for n in range(3, 50000) if lds_bytes(n, exact, WAVES_GLOBAL, 0) > LDS)
    assert last_staged == 142 and first_refused == (13648 if exact else 40945)
    for n in (3, 52, 100, last_staged):
        assert fields(form(n)) == (1, 0, 64 * WAVES_STAGED, WAVES_STAGED, lds_bytes(n, exact, WAVES_STAGED, 1), _abi.TSP_KERNEL_ONLY, 1), n
    for n in (last_staged + 1, 700, first_refused - 1):
        assert fields(form(n)) == (0, 0, 64 * WAVES_GLOBAL, WAVES_GLOBAL, lds_bytes(n, exact, WAVES_GLOBAL, 0), _abi.TSP_KERNEL_ONLY, 1), n
    for n in (first_refused, first_refused + 1000):
        assert fields(form(n)) == (0, 0, 0, 0, 0, 0, 0), n
    for n in (2, 0, -1):
        with pytest.raises(_abi.RlsError) as e:
            form(n)
        assert e.value.code == -1
    with pytest.raises(_abi.RlsError):
        _abi.call("rls_tsp_3opt_launch_form", 10, exact, None)


def test_the_entry_point_refuses_bad_sizes_before_any_device_work():
    from rlsolver_amd import _abi
    ok_args = lambda n, b, s: ("rls_tsp_3opt_best", None, n, None, b, None, s, None, None, None, None, None, None)      # noqa: E731
    for n, b, s in ((2, 1, 1), (10, -1, 1), (10, 1, 0), (10, 1, 65536), (10, 1, 1)):           # the last: NULL pointers
        with pytest.raises(_abi.RlsError) as e:
            _abi.call(*ok_args(n, b, s))
        assert e.value.code == -1, (n, b, s)
    _abi.call(*ok_args(10, 0, 1))                              # no tours: nothing to do
    # rls_tsp_launch_form keeps its six values: the 3-opt form has an entry of its own
    with pytest.raises(_abi.RlsError):
        _abi.tsp_launch_form(6, 10)


def test_segments_and_distance_calc_are_the_reference_s(golden):
    from rlsolver_amd.methods import tsp_opt_3 as t3
    z = golden("tsp_3opt")
    for n in (3, 4, 5, 12):
        got = t3.segments_3_opt(n)
        assert isinstance(got, list) and all(isinstance(s, tuple) for s in got)
        assert got == [tuple(int(v) for v in row) for row in z[f"segments/n{n}"]]
    for name in z["names"]:
        d = z[f"{name}/distance_f64"]
        tour = [int(c) for c in z[f"{name}/start_tour"]]
        assert t3.distance_calc(d, [tour, 0.0]) == float(z[f"{name}/start_distance"]), name
        assert t3.distance_calc(torch.from_numpy(d), [tour, 1]) == float(z[f"{name}/start_distance"]), name
        if f"{name}/rs1/tour" in z.files:
            assert t3.distance_calc(d, [[int(c) for c in z[f"{name}/rs1/tour"]], 0]) == float(z[f"{name}/rs1/distance"]), name


def test_malformed_tours_and_host_devices_are_refused(golden):
    from rlsolver_amd.methods import tsp_opt_3 as t3
    z = golden("tsp_3opt")
    d = z["a5/distance_f64"]
    for route in ([1, 2, 3, 4, 5], [1, 2, 3, 4, 5, 2], [1, 2, 2, 4, 5, 1], [1, 2, 3, 4, 6, 1], [0, 1, 2, 3, 4, 0], [1, 2, 3, 4, 1], []):
        for device in ("cpu", None):                           # the tour is checked before the device
            with pytest.raises(ValueError, match="closed tour"):
                t3.local_search_3_opt(d, [route, 10.0], verbose=False, device=device)
    good = [int(c) for c in z["a5/start_tour"]]
    with pytest.raises(TypeError, match="HIP device"):
        t3.local_search_3_opt(d, [good, float(z["a5/start_distance"])], verbose=False, device="cpu")
    with pytest.raises(TypeError, match="HIP device"):
        t3.local_search_3_opt_batch(d, torch.tensor([[0, 1, 2, 3, 4]]))
    from rlsolver_amd import ops_mcpg_tsp as mops
    with pytest.raises(TypeError):
        mops.tsp_3opt_best(torch.from_numpy(d), torch.tensor([[0, 1, 2, 3, 4]]))
    with pytest.raises(NotImplementedError):
        torch.ops.rlsolver_hip.tsp_3opt_best(torch.from_numpy(d), torch.tensor([[0, 1, 2, 3, 4]]), None, *[torch.zeros(1, dtype=torch.int64)] * 4,
                                             torch.zeros(1, dtype=torch.float64))


def test_apply_moves_is_the_oracle_s_move():
    """the gather that applies a winner, on the host: every trial of every triple of 6 cities, and -1 leaves a tour alone"""
    from rlsolver_amd.methods import tsp_opt_3 as t3
    from tests import tsp3opt_oracle as o3
    n = 6
    tour = np.array([3, 0, 5, 1, 4, 2])
    moves = [(i, j, k, r) for (i, j, k) in o3.segments(n) for r in range(7)] + [(-1, -1, -1, -1)]
    cols = [torch.tensor(c, dtype=torch.int64) for c in zip(*moves)]
    got = t3._apply_moves(torch.from_numpy(np.tile(tour, (len(moves), 1))), *cols).numpy()
    for row, (i, j, k, r) in zip(got, moves):
        assert np.array_equal(row, tour if i < 0 else o3.apply_move(tour, i, j, k, r)), (i, j, k, r)
