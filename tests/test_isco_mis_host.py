"""ISCO_MIS without a GPU: the numpy oracle (tests/mis_oracle.py) against the traces captured from the reference
(tests/golden/isco_mis.npz), the public surface of the class against the reference's, and the argument checks of
rls_isco_mis_step that come before any device work."""
import ctypes as C
import inspect
import json
import os

import numpy as np
import pytest

from tests import mis_oracle as mo
from tests.isco_tol import RTOL, assert_ll_close, ll_atol

GRAPHS = ["BA_100_ID0", "PL_20_ID0", "loader_13"]


@pytest.mark.parametrize("gname", GRAPHS)
def test_mis_local_dist_oracle_golden(golden, gname):
    z = golden("isco_mis")
    g = z[f"{gname}/graph"]
    assert str(z[f"{gname}/x_dtype"]) == "torch.float32"
    for T in (1.0, 0.37):
        energy, logp = mo.mis_local_dist(z[f"{gname}/x"], g[:, 0], g[:, 1], float(z["lam"]), T)
        np.testing.assert_allclose(energy, z[f"{gname}/T{T}/energy"], rtol=1e-6)
        np.testing.assert_allclose(logp, z[f"{gname}/T{T}/log_prob"], rtol=1e-5, atol=1e-5)


def test_loader_graph_ends_in_loops_on_node_0(golden):
    """The reference's loader keeps num_edges entries while networkx merges repeated and reversed lines: the rest are (0, 0)."""
    g = golden("isco_mis")["loader_13/graph"]
    loops = g[:, 0] == g[:, 1]
    assert loops.sum() >= 5 and not g[loops, 0].any() and loops[-int(loops.sum()):].all()


@pytest.mark.parametrize("gname", GRAPHS)
def test_mis_step_oracle_golden(golden, gname):
    z = golden("isco_mis")
    g = z[f"{gname}/graph"]
    n = int(z[f"{gname}/x"].shape[1])
    for k in range(3):
        t = f"{gname}/step{k}"
        pl = z[f"{t}/path_length"]
        r = mo.mis_step(z[f"{t}/x"], g[:, 0], g[:, 1], float(z["lam"]), pl, float(z[f"{t}/temperature"]),
                        z[f"{t}/rand_gumbel"], z[f"{t}/rand_accept"])
        assert np.array_equal(r["mask"], z[f"{t}/mask"]), t
        assert int(r["mask"][0].sum()) == 1 and int(r["mask"][1].sum()) == n
        assert np.array_equal(r["y_prop"], z[f"{t}/y_prop"])
        for key in ("ll_x", "ll_y", "energy"):           # no renormalisation involved: tight
            np.testing.assert_allclose(r[key], z[f"{t}/{key}"], rtol=RTOL, atol=1e-5, err_msg=f"{t}/{key}")
        checked = [assert_ll_close(r[key], z[f"{t}/{key}"], r["remaining_mass"], f"{t}/{key}", pl)
                   for key in ("ll_x2y", "ll_y2x", "log_acc")]
        # all but the path_length = N env carry information (on the 13-node graph the drawn lengths reach N as well)
        assert min(checked) >= (10 if n > 13 else 8)
        sure = r["accept_margin"] > 2 * (ll_atol(r["remaining_mass"], pl) + RTOL * np.abs(r["log_acc"]))
        assert sure.sum() >= 8 and np.array_equal(r["y"][sure], z[f"{t}/y"][sure])


def test_tolerance_factor_follows_the_measured_ratio():
    assert mo.K_TOL == int(np.ceil(2 * mo.MEASURED_RATIO)) == 2


# pieces of a step() that is ONE kernel here, as for ISCO_maxcut (tests/test_api_surface.py)
INSIDE_THE_KERNEL = {"ISCO_MIS.proposal": "inside rls_isco_mis_step", "ISCO_MIS.ll_y2x": "inside rls_isco_mis_step",
                     "ISCO_MIS.select_sample": "inside rls_isco_mis_step"}


def test_isco_mis_surface_matches_the_reference():
    """Every public name of the reference's ISCO_MIS exists on rlsolver_amd.envs.env_ISCO.ISCO_MIS with the same leading
    positional parameters (this supersedes the out-of-scope row of tests/test_api_surface.py)."""
    gold = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "api_surface.npz")
    names = json.loads(str(np.load(gold)["surface"]))["rlsolver/envs/env_ISCO.py"]
    mine = {k: v for k, v in names.items() if k.split(".")[0] == "ISCO_MIS"}
    assert {"ISCO_MIS", "ISCO_MIS.__init__", "ISCO_MIS.step", "ISCO_MIS.get_local_dist", "ISCO_MIS.model",
            "ISCO_MIS.random_gen_init_sample"} <= set(mine) and set(INSIDE_THE_KERNEL) <= set(mine)
    from rlsolver_amd.envs import env_ISCO
    cls = env_ISCO.ISCO_MIS
    for name, ref in mine.items():
        if name in INSIDE_THE_KERNEL or ref.get("class"):
            continue
        obj = getattr(cls, name.split(".")[1])
        want, have = list(ref["args"]), list(inspect.signature(obj).parameters)
        assert have[:len(want)] == want, f"{name}: reference {want} here {have}"
    assert all(not hasattr(cls, k.split(".")[1]) for k in INSIDE_THE_KERNEL)
    p = inspect.signature(cls.__init__).parameters
    assert p["lam"].default == 1.001 and p["chain_length"].default == 20000 and p["final_temperature"].default == 0.0
    with pytest.raises(TypeError, match="HIP device"):
        import torch
        cls({"num_nodes": 3, "num_edges": 1, "edge_from": torch.tensor([0]), "edge_to": torch.tensor([1])})


def _call(**over):
    """rls_isco_mis_step on a 64-node graph whose pointers are never followed: every call here must fail in the checks"""
    from rlsolver_amd import _abi
    fake = lambda k: C.c_void_p(0x1000 * k)
    g = _abi.RlsGraph(num_nodes=64, num_stored_edges=0, nnz=0, rowptr=0x1000, erowptr=0x2000)
    a = dict(g=C.byref(g), x=fake(3), y_out=fake(4), B=2, path_length=fake(5), temperature=1.0, lam=1.001, u_gumbel=None,
             u_accept=None, seed=1, env_offset=0, energy_out=None, acc_out=None, terms_out=None, mask_out=None, scratch=None,
             scratch_bytes=0, stream=None)
    a.update(over)
    _abi.call("rls_isco_mis_step", *a.values())


@pytest.mark.parametrize("over,msg", [
    (dict(g=None), "graph is NULL"),
    (dict(temperature=0.0), "temperature must be > 0"),
    (dict(temperature=-1.0), "temperature must be > 0"),
    (dict(lam=float("inf")), "lam must be finite"),
    (dict(lam=float("nan")), "lam must be finite"),
    (dict(u_gumbel=C.c_void_p(0x6000)), "both be given or both be NULL"),
    (dict(u_accept=C.c_void_p(0x6000)), "both be given or both be NULL"),
    (dict(y_out=C.c_void_p(0x3000)), "must not alias x"),
    (dict(x=None), "NULL pointer"),
])
def test_rls_isco_mis_step_rejects_before_device_work(over, msg):
    from rlsolver_amd import _abi
    with pytest.raises(_abi.RlsError, match=msg) as e:
        _call(**over)
    assert "EINVAL" in str(e.value)


def test_isco_mis_op_has_a_hip_kernel_only():
    import torch
    from rlsolver_amd import torch_ops
    assert "isco_mis_step" in torch_ops.DEVICE_ENTRY_POINTS
    assert torch._C._dispatch_has_kernel_for_dispatch_key("rlsolver_hip::isco_mis_step", "CUDA")
    assert not torch._C._dispatch_has_kernel_for_dispatch_key("rlsolver_hip::isco_mis_step", "CPU")
    schema = torch.ops.rlsolver_hip.isco_mis_step.default._schema
    assert [a.name for a in schema.arguments][:6] == ["graph", "x", "y_out", "path_length", "temperature", "lam"]
