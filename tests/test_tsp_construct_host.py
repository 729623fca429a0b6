"""What of the tour constructors runs without a GPU: the C ABI's three new entries and their ctypes rows, the launch form of
rls_tsp_grow_2opt (csrc/rls_tsp_grow_plan.h) against the formula include/rlsolver_hip.h documents, the refusals that come before
any device work, and the public surface of the four modules against the reference's, recorded as data in
tests/golden/tsp_construct.npz."""
import inspect

import numpy as np
import pytest
import torch

from tests.test_abi import declared_functions

LDS = 160 * 1024           # the LDS of a compute unit: what a workgroup may ask for
WAVES = 16


def lds_bytes(n, staged):
    """include/rlsolver_hip.h, rls_tsp_grow_launch_form: lds_d * 8 N^2 + 8 (N + 1) + 16 waves + 8 N"""
    return staged * 8 * n * n + 8 * (n + 1) + 16 * WAVES + 8 * n


def test_abi_lists_the_three_entries_with_the_header_s_argument_counts():
    from rlsolver_amd import _abi, build, torch_ops
    fns = declared_functions()
    want = {"rls_tsp_neighbour_chain": 8, "rls_tsp_grow_2opt": 13, "rls_tsp_grow_launch_form": 2}
    for name, argc in want.items():
        assert fns[name] == argc and len(_abi.SIGNATURES[name]) == argc, name
    assert "tsp_neighbour_chain" in torch_ops.DEVICE_ENTRY_POINTS and "tsp_grow_2opt" in torch_ops.DEVICE_ENTRY_POINTS
    assert "tsp_grow_launch_form" in torch_ops.HOST_ENTRY_POINTS
    assert "rls_tsp_grow.hip" in build.SOURCES
    assert _abi.version() == 12
    names = lambda op: [a.name for a in getattr(torch.ops.rlsolver_hip, op).default._schema.arguments]      # noqa: E731
    assert names("tsp_neighbour_chain") == ["dist", "start", "farthest", "chain", "status"]
    assert names("tsp_grow_2opt") == ["dist", "order", "m_seed", "m_end", "first_m", "max_passes", "tours", "length", "passes", "status"]
    for op in ("tsp_neighbour_chain", "tsp_grow_2opt"):
        assert torch._C._dispatch_has_kernel_for_dispatch_key(f"rlsolver_hip::{op}", "CUDA")
        assert not torch._C._dispatch_has_kernel_for_dispatch_key(f"rlsolver_hip::{op}", "CPU")


def test_launch_form_follows_the_documented_formula():
    from rlsolver_amd import _abi
    form = _abi.tsp_grow_launch_form
    fields = lambda f: (f.lds_d, f.tab8, f.block, f.waves, f.lds_bytes, f.kernel, f.supported)      # noqa: E731
    last_staged = max(n for n in range(2, 400) if lds_bytes(n, 1) <= LDS)
    first_refused = min(n for n in range(2, 50000) if lds_bytes(n, 0) > LDS)
    assert last_staged == 141 and first_refused == 10224          # the sizes the header names
    for n in (2, 3, 52, 100, last_staged):
        assert fields(form(n)) == (1, 0, 64 * WAVES, WAVES, lds_bytes(n, 1), _abi.TSP_KERNEL_ONLY, 1), n
    for n in (last_staged + 1, 700, first_refused - 1):
        assert fields(form(n)) == (0, 0, 64 * WAVES, WAVES, lds_bytes(n, 0), _abi.TSP_KERNEL_ONLY, 1), n
    for n in (first_refused, first_refused + 1000):
        assert fields(form(n)) == (0, 0, 0, 0, 0, 0, 0), n
    for n in (1, 0, -1, 1 << 20):
        with pytest.raises(_abi.RlsError) as e:
            form(n)
        assert e.value.code == -1
    with pytest.raises(_abi.RlsError):
        _abi.call("rls_tsp_grow_launch_form", 10, None)


def test_the_entry_points_refuse_bad_sizes_before_any_device_work():
    from rlsolver_amd import _abi
    grow = lambda n, s, m0, m1, mp: ("rls_tsp_grow_2opt", None, n, None, s, m0, m1, 3, mp, None, None, None, None, None)      # noqa: E731
    for args in ((1, 1, 2, 2, 1), (10, -1, 2, 10, 1), (10, 1, 1, 10, 1), (10, 1, 5, 4, 1), (10, 1, 2, 11, 1), (10, 1, 2, 10, 0),
                 (10, 1, 2, 10, 1)):                           # the last: NULL pointers
        with pytest.raises(_abi.RlsError) as e:
            _abi.call(*grow(*args))
        assert e.value.code == -1, args
    _abi.call(*grow(10, 0, 2, 10, 1))                          # no rows: nothing to do
    chain = lambda n, s, far: ("rls_tsp_neighbour_chain", None, n, None, s, far, None, None, None)      # noqa: E731
    for args in ((1, 1, 0), (10, -1, 0), (10, 1, 2), (10, 1, -1), (10, 1, 0)):
        with pytest.raises(_abi.RlsError) as e:
            _abi.call(*chain(*args))
        assert e.value.code == -1, args
    _abi.call(*chain(10, 0, 1))


D4 = np.array([[0, 1, 2, 3], [1, 0, 1, 2], [2, 1, 0, 1], [3, 2, 1, 0]], dtype=np.float64)


def _public_calls():
    from rlsolver_amd.methods import tsp_ins_c, tsp_ins_f, tsp_ins_n, tsp_nn
    return {"nearest_neighbour": lambda d, **k: tsp_nn.nearest_neighbour(d, k.pop("loc", -1), True, False, **k),
            "nearest_insertion": lambda d, **k: tsp_ins_n.nearest_insertion(d, k.pop("loc", -1), False, **k),
            "farthest_insertion": lambda d, **k: tsp_ins_f.farthest_insertion(d, k.pop("loc", -1), False, **k),
            "cheapest_insertion": lambda d, **k: tsp_ins_c.cheapest_insertion(d, False, **k)}


@pytest.mark.parametrize("device", ["cpu", None])
def test_bad_matrices_and_starts_are_refused_before_any_launch(device):
    """ValueError comes before the device is looked at: with device='cpu' as with the default device"""
    bad = {"not square": np.zeros((3, 4)), "one city": np.zeros((1, 1)), "empty": np.zeros((0, 0)), "a vector": np.zeros(4),
           "inf": np.where(np.eye(4) > 0, 0.0, np.inf), "nan": D4 + np.where(np.arange(16).reshape(4, 4) == 7, np.nan, 0.0),
           "-inf": D4 - np.where(np.arange(16).reshape(4, 4) == 2, np.inf, 0.0)}
    for fn, call in _public_calls().items():
        for what, d in bad.items():
            with pytest.raises(ValueError):
                call(d, device=device)
            with pytest.raises(ValueError):
                call(torch.from_numpy(d), device=device)
        if fn != "cheapest_insertion":
            for loc in (0, 5, 6, -2, 100):
                with pytest.raises(ValueError, match="initial_location"):
                    call(D4, loc=loc, device=device)
    diag = D4.copy()
    diag[2, 2] = 9.0                                            # the largest entry on the diagonal: the reference starts from [2, 2]
    with pytest.raises(ValueError, match="diagonal"):
        _public_calls()["cheapest_insertion"](diag, device=device)


def test_host_devices_and_host_tensors_are_refused_with_type_error():
    from rlsolver_amd import ops_mcpg_tsp as mops
    from rlsolver_amd.methods import tsp_construct as tc, tsp_ins_n
    for fn, call in _public_calls().items():
        with pytest.raises(TypeError, match="HIP device"):
            call(D4, device="cpu")
    with pytest.raises(TypeError, match="HIP device"):
        tsp_ins_n.best_insertion(D4, [0, 2, 1], device="cpu")
    with pytest.raises(ValueError):
        tsp_ins_n.best_insertion(D4, [0, 2, 2], device="cpu")
    with pytest.raises(ValueError):
        tsp_ins_n.best_insertion(D4, [0, 4], device="cpu")
    assert tsp_ins_n.best_insertion(D4, [3], device="cpu") == [3]          # one city: nothing to do, as in the reference
    d = torch.from_numpy(D4)
    with pytest.raises(TypeError):
        tc.neighbour_chains(d, torch.tensor([0, 1]))
    with pytest.raises(TypeError):
        tc.grow_2opt(d, torch.tensor([[0, 1, 2, 3]]))
    with pytest.raises(TypeError):
        mops.tsp_neighbour_chain(d, torch.tensor([0, 1]))
    with pytest.raises(TypeError):
        mops.tsp_grow_2opt(d, torch.tensor([[0, 1, 2, 3]]))
    with pytest.raises(NotImplementedError):
        torch.ops.rlsolver_hip.tsp_neighbour_chain(d, torch.tensor([0]), 0, torch.zeros((1, 4), dtype=torch.int64), torch.zeros(1, dtype=torch.int32))
    with pytest.raises(NotImplementedError):
        torch.ops.rlsolver_hip.tsp_grow_2opt(d, torch.tensor([[0, 1, 2, 3]]), 2, 4, 3, 16, torch.zeros((1, 4), dtype=torch.int64),
                                             torch.zeros(1, dtype=torch.float64), torch.zeros(1, dtype=torch.int64), torch.zeros(1, dtype=torch.int32))


def test_the_four_modules_export_the_reference_s_names_with_its_leading_parameters(golden):
    import importlib
    z = golden("tsp_construct")
    for tag in ("nn", "ins_n", "ins_f", "ins_c"):
        mod = importlib.import_module(f"rlsolver_amd.methods.tsp_{tag}")
        fns = [str(f) for f in z[f"surface/{tag}/functions"]]
        assert len(fns) >= 3
        for f in fns:
            want = [str(p) for p in z[f"surface/{tag}/{f}/parameters"]]
            params = inspect.signature(getattr(mod, f)).parameters
            assert list(params)[:len(want)] == want, (tag, f)
            for extra in list(params)[len(want):]:                  # what this package adds never shifts a positional argument
                assert extra == "device" and params[extra].default is None, (tag, f, extra)
            if f in ("nearest_neighbour", "nearest_insertion", "farthest_insertion", "cheapest_insertion", "best_insertion"):
                assert params["device"].kind is inspect.Parameter.KEYWORD_ONLY, (tag, f)
    from rlsolver_amd.methods import tsp_nn, tsp_opt_2
    assert tsp_nn.distance_calc is tsp_opt_2.distance_calc and tsp_nn.local_search_2_opt is tsp_opt_2.local_search_2_opt
    d = inspect.signature(tsp_nn.nearest_neighbour).parameters
    assert (d["initial_location"].default, d["local_search"].default, d["verbose"].default) == (-1, True, True)
