"""The S2V_PPO env without a GPU: the numpy oracle (tests/s2vppo_oracle.py) against the traces recorded from the reference
(tests/golden/s2v_ppo.npz), the host-side batch builder, the launch plan (csrc/rls_s2vppo_plan.h through rls_s2vppo_launch_plan) and
the checks that come before any device work."""
import json
import os
import types

import numpy as np
import pytest
import torch

from tests import s2vppo_oracle as orc


def names(z):
    return json.loads(str(z["names"]))


def test_fixture_covers_the_sizes_tenures_and_both_reset_branches(golden):
    z = golden("s2v_ppo")
    cs = [orc.golden_case(z, n) for n in names(z)]
    assert {c["n"] for c in cs} >= {1, 5, 20, 40, 64, 65} and {c["tenure"] for c in cs} >= {0, 3, 10, 60}
    assert {c["greedy"] for c in cs} == {True, False} and "index_add_" in str(z["source"])
    assert os.path.getsize(os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "s2v_ppo.npz")) < 532175
    assert all(len(c["actions"]) == 2 * c["n"] and c["done"][-1] and not c["done"][:-1].any() for c in cs)
    assert sum(int((c["reward"] < 0).sum()) for c in cs) > 100                      # steps that carry a stag punishment


def test_oracle_reproduces_the_reference_exactly(golden):
    z = golden("s2v_ppo")
    steps = 0
    for name in names(z):
        c = orc.golden_case(z, name)
        o = orc.oracle_for(c)
        if c["greedy"]:
            assert np.array_equal(o.greedy_start()[0].astype(np.int8), c["z0"]), name
        x, mask = o.reset(c["z0"])
        assert np.array_equal(x.view(np.uint32), c["x"][0].view(np.uint32)) and np.array_equal(mask, c["mask"][0]), name
        assert o.cut == c["cut"][0] and o.best_cut == c["best"][0]
        for k, a in enumerate(c["actions"]):
            r = o.step(a)
            assert r["reward"] == c["reward"][k] and r["done"] == c["done"][k], (name, k)
            assert r["cut"] == c["cut"][k + 1] and r["best"] == c["best"][k + 1], (name, k)
            assert np.array_equal(r["x"].view(np.uint32), c["x"][k + 1].view(np.uint32)), (name, k)
            assert np.array_equal(r["mask"], c["mask"][k + 1]), (name, k)
            steps += 1
        assert np.array_equal(o.best_z.astype(np.int8), c["best_z"]), name
    assert steps == 660


def test_greedy_cap_binds_on_the_dense_fixture_graph(golden):
    c = orc.golden_case(golden("s2v_ppo"), "dense64_greedy")
    o = orc.oracle_for(c)
    z, flips = o.greedy_start()
    assert flips == 32 and o.all_deltas(z).max() > 0


def test_fractional_trace_measures_the_reference_float32_deviation(golden):
    """what tests/test_gpu_s2v_ppo.py allows the kernel four times of"""
    c = orc.golden_case(golden("s2v_ppo"), "fractional")
    o = orc.oracle_for(c)
    o.reset(c["z0"])
    dd, dc = [np.abs(o.delta - c["delta"][0]).max()], [abs(o.cut - c["cut"][0])]
    for k, a in enumerate(c["actions"]):
        o.step(a)
        dd.append(np.abs(o.delta - c["delta"][k + 1]).max())
        dc.append(max(abs(o.cut - c["cut"][k + 1]), abs(o.best_cut - c["best"][k + 1])))
    assert 2.2e-07 < max(dd) < 2.3e-07 and 2.43e-06 < max(dc) < 2.44e-06
    assert (c["edge_weight"] >= 0.1).all() and (c["edge_weight"] <= 1).all() and len(np.unique(c["edge_weight"])) > 50


# ---- the batch builder --------------------------------------------------------------------------------------------------------------
def _gd(ei, w, n):
    return {"edge_index": torch.tensor(ei, dtype=torch.int64).reshape(2, -1), "edge_weight": torch.tensor(w, dtype=torch.float32), "num_nodes": n}


def test_batch_csr_keeps_the_list_as_given():
    from rlsolver_amd.envs.env_S2V_PPO import build_batch_csr
    a = _gd([[0, 1, 2, 2, 0, 1, 2], [1, 0, 2, 0, 1, 0, 2]], [1, 1, 5, 2, 3, 3, 7], 3)     # (0, 1) twice, a loop on 2 twice, (2, 0) one way
    empty = _gd([[], []], [], 4)
    b = _gd([[1, 0], [0, 1]], [-2, -2], 2)
    h = build_batch_csr([a, empty, b])
    assert h["ptr"].tolist() == [0, 3, 7, 9] and h["num_nodes"].tolist() == [3, 4, 2]
    assert h["rowptr"].tolist() == [0, 2, 4, 7, 7, 7, 7, 7, 8, 9]
    assert h["col"].tolist() == [1, 1, 0, 0, 0, 2, 2, 8, 7] and h["col"].dtype == np.int32
    assert h["w"].tolist() == [1, 3, 1, 3, 2, 5, 7, -2, -2]                             # equal pairs stay in list order
    assert np.array_equal(h["edge_index"], np.array([[0, 1, 2, 2, 0, 1, 2, 8, 7], [1, 0, 2, 0, 1, 0, 2, 7, 8]]))
    assert h["edge_weight"].tolist() == [1, 1, 5, 2, 3, 3, 7, -2, -2]
    assert h["wtot"][:, 0].tolist() == [11.0, 0.0, -2.0] and h["wtot"][1, 1] == np.float32(1e-8) and h["wtot"][0, 1] == 11.0
    assert h["degrees"].tolist() == [4, 4, 14, 0, 0, 0, 0, -2, -2]
    assert h["wtot"][:, 2].tolist() == [0.0, 1.0, 1.0]                                  # (2, 0) has no (0, 2): not its own transpose
    sym = build_batch_csr([_gd([[0, 1, 0, 1, 2], [1, 0, 1, 0, 2]], [1, 3, 3, 1, 5], 3), _gd([[0, 1], [1, 0]], [1, 2], 2)])
    assert sym["wtot"][:, 2].tolist() == [1.0, 0.0]                                     # a pair twice with swapped weights; unequal weights
    none = build_batch_csr([])
    assert none["ptr"].tolist() == [0] and none["rowptr"].tolist() == [0] and none["edge_index"].shape == (2, 0)
    zero = build_batch_csr([_gd([[], []], [], 0), b])
    assert zero["ptr"].tolist() == [0, 0, 2] and zero["col"].tolist() == [1, 0]
    with pytest.raises(ValueError, match="outside"):
        build_batch_csr([_gd([[0], [3]], [1], 3)])
    with pytest.raises(ValueError, match="entries"):
        build_batch_csr([_gd([[0], [1]], [1, 2], 3)])


def test_batch_csr_rows_match_the_oracle_rows():
    from rlsolver_amd.envs.env_S2V_PPO import build_batch_csr
    rng = np.random.RandomState(1)
    gs = []
    for n in (1, 7, 30):
        m = 4 * n
        gs.append((rng.randint(0, n, size=(2, m)), rng.randint(-2, 3, size=m).astype(np.float32), n))
    h = build_batch_csr([dict(edge_index=ei, edge_weight=w, num_nodes=n) for ei, w, n in gs])
    for i, (ei, w, n) in enumerate(gs):
        o = orc.OracleEnv(ei, w, n)
        for v in range(n):
            lo, hi = h["rowptr"][h["ptr"][i] + v], h["rowptr"][h["ptr"][i] + v + 1]
            rows = o.rows[v][np.argsort(ei[1][o.rows[v]], kind="stable")]
            assert np.array_equal(h["col"][lo:hi] - h["ptr"][i], ei[1][rows]) and np.array_equal(h["w"][lo:hi], w[rows])


# ---- the launch plan ------------------------------------------------------------------------------------------------------------------
def test_launch_plan_at_every_edge():
    from rlsolver_amd.envs.env_S2V_PPO import launch_plan
    for n in (1, 64, 65, 255, 256):
        assert launch_plan(130, n) == dict(form="wave", block=256, envs_per_workgroup=4, grid=33), n
    assert launch_plan(1, 256)["grid"] == 1 and launch_plan(4, 256)["grid"] == 1 and launch_plan(5, 256)["grid"] == 2
    for n in (257, 4095, 4096):
        assert launch_plan(130, n) == dict(form="workgroup", block=256, envs_per_workgroup=1, grid=130), n
    for n in (4097, 10_000, 2 ** 31 - 1):
        assert launch_plan(64, n) == dict(form="workgroup", block=1024, envs_per_workgroup=1, grid=64), n
    assert launch_plan(0, 10)["grid"] == 0
    from rlsolver_amd import _abi
    for B, n in ((-1, 5), (5, -1), (5, 2 ** 31), (2 ** 31, 5)):
        with pytest.raises(_abi.RlsError, match="2\\^31"):
            launch_plan(B, n)


# ---- before any device work -------------------------------------------------------------------------------------------------------------
def test_entry_points_reject_before_device_work():
    from rlsolver_amd import _abi
    with pytest.raises(_abi.RlsError, match="env is NULL"):
        _abi.call("rls_s2vppo_step", None, None, 0.01, None, None, None)
    with pytest.raises(_abi.RlsError, match="env is NULL"):
        _abi.call("rls_s2vppo_reset", None, None, 0, None, None, 0, 0, None)
    with pytest.raises(_abi.RlsError, match="out is NULL"):
        _abi.call("rls_s2vppo_launch_plan", 1, 1, None)


def test_ops_are_hip_only_and_the_env_needs_a_device():
    from rlsolver_amd import torch_ops
    from rlsolver_amd.envs.env_S2V_PPO import EnvMaxcut, VecEnvMaxcut
    for name in ("s2vppo_step", "s2vppo_reset"):
        assert name in torch_ops.DEVICE_ENTRY_POINTS
        assert torch._C._dispatch_has_kernel_for_dispatch_key(f"rlsolver_hip::{name}", "CUDA")
        assert not torch._C._dispatch_has_kernel_for_dispatch_key(f"rlsolver_hip::{name}", "CPU")
    assert "s2vppo_launch_plan" in torch_ops.HOST_ENTRY_POINTS
    cfg = types.SimpleNamespace(device=torch.device("cpu"), node_feature_dim=5, episode_length_multiplier=2, tabu_tenure=10, stag_punishment=0.01)
    g = _gd([[0, 1], [1, 0]], [1, 1], 2)
    with pytest.raises(TypeError, match="HIP device"):
        VecEnvMaxcut([g], cfg)
    with pytest.raises(TypeError, match="HIP device"):
        EnvMaxcut(g, cfg)

