"""PISCO_maxcut without a GPU: the loader against the rules read off the reference's networkx loader, the constructor's checks,
the public surface of the class against the reference's, and the argument checks of the three C entry points that come before
any device work."""
import ctypes as C
import inspect
import json
import os

import numpy as np
import pytest
import torch


def test_loader_comment_repeat_reverse_loop(tmp_path):
    """util_maxcut.py:7-46: `//` lines are comments, ids are 1-based, a repeated or reversed line REPLACES the weight
    (Graph.add_edge overwrites), a loop sets the diagonal, the matrix is symmetric and padded to 8, the edge arrays hold the
    distinct edges as Graph.edges() lists them, zero-filled up to the header's num_edges."""
    from rlsolver_amd.envs.env_PISCO_maxcut import load_data
    f = tmp_path / "g.txt"
    f.write_text("5 7\n// a comment line 9 9 9\n1 2 3\n2 3 -4\n1 2 5\n3 2 7\n4 4 2\n5 1 -1\n2 5 6\n")
    d = load_data(str(f), "cpu")
    A = d["adj_matrix"]
    assert d["num_nodes"] == 5 and d["num_edges"] == 7 and A.dtype == torch.float16 and tuple(A.shape) == (8, 8)
    want = np.zeros((8, 8))
    for u, v, w in ((0, 1, 5), (1, 2, 7), (3, 3, 2), (0, 4, -1), (1, 4, 6)):
        want[u, v] = want[v, u] = w
    assert np.array_equal(A.numpy().astype(np.float64), want) and torch.equal(A, A.t())
    # node 0: neighbours 1, 4 in first-seen order; node 1: 2, 4; node 3: its loop; then zeros up to num_edges
    assert d["edge_from"].tolist() == [0, 0, 1, 1, 3, 0, 0] and d["edge_to"].tolist() == [1, 4, 2, 4, 3, 0, 0]
    assert d["edge_from"].dtype == torch.int64
    f.write_text("3 1\n1 2 1\n2 3 1\n")              # more distinct edges than the header says: the reference's IndexError
    with pytest.raises(IndexError):
        load_data(str(f), "cpu")


def test_record_keeps_the_best_on_the_device_side():
    from rlsolver_amd.envs.env_PISCO_maxcut import record
    best, sample = torch.tensor(0.0), torch.zeros(4, dtype=torch.float16)
    new = torch.tensor([[1, 0, 0, 0], [0, 1, 0, 0]], dtype=torch.float16)
    best, sample = record(best, sample, torch.tensor([-1.0, 2.5]), new)
    assert float(best) == 2.5 and sample.tolist() == [0, 1, 0, 0]
    best, sample = record(best, sample, torch.tensor([2.0, 2.5]), 1 - new)
    assert float(best) == 2.5 and sample.tolist() == [0, 1, 0, 0]


def test_record_takes_the_reference_drivers_shapes():
    """main_PISCO_maxcut.py:28 starts from best_sample = zeros(num_nodes) (100 entries on the default BA_100_ID0) while the
    samples are padded to Np = 104 columns: the reference assigns, here the kept sample has the samples' width from the first
    call on, whether or not a row was better."""
    from rlsolver_amd.envs.env_PISCO_maxcut import record
    n, Np = 100, 104
    new = torch.zeros((3, Np), dtype=torch.float16)
    new[1, 5] = new[1, 103] = 1
    best, sample = record(torch.tensor(0.0), torch.zeros(n, dtype=torch.float16), torch.tensor([-3.0, -1.0, -2.0]), new)
    assert float(best) == 0.0 and tuple(sample.shape) == (Np,) and not sample.any()        # nothing better: zeros, padded
    best, sample = record(torch.tensor(0.0), torch.zeros(n, dtype=torch.float16), torch.tensor([-3.0, 4.0, -2.0]), new)
    assert float(best) == 4.0 and tuple(sample.shape) == (Np,) and torch.equal(sample, new[1]) and sample.dtype == torch.float16
    best, sample = record(best, sample, torch.tensor([1.0, 2.0, 3.0]), 1 - new)
    assert float(best) == 4.0 and torch.equal(sample, new[1])
    keep = torch.ones(Np + 8, dtype=torch.float16)                                          # a longer incumbent is cut
    assert tuple(record(torch.tensor(9.0), keep, torch.tensor([1.0, 2.0, 3.0]), new)[1].shape) == (Np,)


def _params(A):
    return {"num_nodes": A.shape[0], "num_edges": 0, "edge_from": torch.zeros(0, dtype=torch.int64),
            "edge_to": torch.zeros(0, dtype=torch.int64), "adj_matrix": A}


def test_constructor_rejects_bad_matrices_and_a_cpu_device():
    from rlsolver_amd.envs.env_ISCO import PISCO_maxcut
    from rlsolver_amd.envs import env_PISCO_maxcut
    assert PISCO_maxcut is env_PISCO_maxcut.PISCO_maxcut
    sym = torch.zeros((8, 8), dtype=torch.float16)
    with pytest.raises(TypeError, match="HIP device"):
        PISCO_maxcut(_params(sym))
    with pytest.raises(TypeError, match="HIP device"):
        PISCO_maxcut(_params(sym), device="cpu")
    # the matrix checks do not depend on the device: name one, the tensors stay where they are
    with pytest.raises(TypeError, match="float16"):
        PISCO_maxcut(_params(sym.float()), device="cuda:0")
    with pytest.raises(ValueError, match="multiple of 8"):
        PISCO_maxcut(_params(torch.zeros((12, 12), dtype=torch.float16)), device="cuda:0")
    with pytest.raises(ValueError, match="multiple of 8"):
        PISCO_maxcut(_params(torch.zeros((8, 16), dtype=torch.float16)), device="cuda:0")
    bad = sym.clone()
    bad[1, 2] = 1
    with pytest.raises(ValueError, match="symmetric"):
        PISCO_maxcut(_params(bad), device="cuda:0")


def test_pisco_surface_matches_the_reference():
    """Every public name of the reference's PISCO_maxcut exists on rlsolver_amd.envs.env_ISCO.PISCO_maxcut with the same
    leading positional parameters (this supersedes the out-of-scope row of tests/test_api_surface.py, which stays)."""
    gold = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "api_surface.npz")
    names = json.loads(str(np.load(gold)["surface"]))["rlsolver/envs/env_ISCO.py"]
    mine = {k: v for k, v in names.items() if k.split(".")[0] == "PISCO_maxcut"}
    assert {"PISCO_maxcut", "PISCO_maxcut.__init__", "PISCO_maxcut.step", "PISCO_maxcut.get_local_dist", "PISCO_maxcut.proposal",
            "PISCO_maxcut.tensor_core_energy", "PISCO_maxcut.random_gen_init_sample", "PISCO_maxcut.check_tensor"} <= set(mine)
    from rlsolver_amd.envs import env_ISCO
    cls = env_ISCO.PISCO_maxcut
    for name, ref in mine.items():
        if ref.get("class"):
            continue
        obj = getattr(cls, name.split(".")[1])
        want, have = list(ref["args"]), list(inspect.signature(obj).parameters)
        assert have[:len(want)] == want, f"{name}: reference {want} here {have}"
    p = inspect.signature(cls.__init__).parameters
    assert p["half_rounding"].default is True and {"batch_size", "device", "chain_length", "init_temperature", "final_temperature",
                                                   "env_offset", "seed"} <= set(p)
    with pytest.raises(ValueError, match="inf"):
        cls.check_tensor(None, torch.tensor([1.0, float("inf")]))
    cls.check_tensor(None, torch.tensor([1.0]))


fake = lambda k: C.c_void_p(0x1000 * k)


def _step(**over):
    """rls_pisco_step with pointers that are never followed: every call here must fail in the checks."""
    from rlsolver_amd import _abi
    a = dict(adj=fake(1), Np=64, x=fake(3), y_out=fake(4), B=2, path_length=fake(5), temperature=1.0, half_rounding=1,
             u_gumbel=None, u_accept=None, seed=1, env_offset=0, energy_out=None, acc_out=None, terms_out=None, mask_out=None,
             scratch=fake(9), scratch_bytes=2 * 64 * 8, stream=None)
    a.update(over)
    _abi.call("rls_pisco_step", *a.values())


@pytest.mark.parametrize("over,code,msg", [
    (dict(Np=12), "EINVAL", "multiple of 8"),
    (dict(Np=0), "EINVAL", "multiple of 8"),
    (dict(B=-1), "EINVAL", "B < 0"),
    (dict(temperature=0.0), "EINVAL", "temperature must be > 0"),
    (dict(y_out=fake(3)), "EINVAL", "must not alias x"),
    (dict(scratch_bytes=2 * 64 * 8 - 1), "EINVAL", "of scratch"),
    (dict(scratch=None), "EINVAL", "of scratch"),
    (dict(u_gumbel=fake(6)), "EINVAL", "both be given or both be NULL"),
    (dict(adj=None), "EINVAL", "NULL pointer"),
    # the LDS limit is a size check: it comes before the pointer and scratch checks, so tiny dummy buffers reach it
    (dict(Np=20000, scratch_bytes=16), "EUNSUPPORTED", "B of LDS"),
])
def test_rls_pisco_step_rejects_before_device_work(over, code, msg):
    from rlsolver_amd import _abi
    with pytest.raises(_abi.RlsError, match=msg) as e:
        _step(**over)
    assert code in str(e.value)


def test_pisco_no_op_scratch_query_and_product_checks():
    from rlsolver_amd import _abi
    _step(B=0, adj=None, x=None, y_out=None, scratch=None, scratch_bytes=0)           # B = 0: nothing is read, nothing launched
    _abi.call("rls_pisco_product", None, 64, None, 0, None, None)
    lib = _abi.lib()
    assert lib.rls_pisco_scratch_bytes(104, 12) == 12 * 104 * 8 and lib.rls_pisco_scratch_bytes(2000, 4096) == 4096 * 2000 * 8
    assert lib.rls_pisco_scratch_bytes(12, 5) == 0 and lib.rls_pisco_scratch_bytes(64, 0) == 0 and lib.rls_pisco_scratch_bytes(0, 5) == 0
    for args, msg in (((fake(1), 12, fake(2), 1, fake(3), None), "multiple of 8"), ((None, 8, fake(2), 1, fake(3), None), "NULL pointer"),
                      ((C.c_void_p(0x1008), 8, fake(2), 1, fake(3), None), "16-byte aligned")):
        with pytest.raises(_abi.RlsError, match=msg):
            _abi.call("rls_pisco_product", *args)


def test_pisco_ops_have_a_hip_kernel_only():
    from rlsolver_amd import torch_ops
    for name in ("pisco_product", "pisco_step"):
        assert name in torch_ops.DEVICE_ENTRY_POINTS
        assert torch._C._dispatch_has_kernel_for_dispatch_key(f"rlsolver_hip::{name}", "CUDA")
        assert not torch._C._dispatch_has_kernel_for_dispatch_key(f"rlsolver_hip::{name}", "CPU")
    assert "pisco_scratch_bytes" in torch_ops.HOST_ENTRY_POINTS
    schema = torch.ops.rlsolver_hip.pisco_step.default._schema
    assert [a.name for a in schema.arguments][:6] == ["adj", "x", "y_out", "path_length", "temperature", "half_rounding"]
    with pytest.raises(NotImplementedError):
        torch.ops.rlsolver_hip.pisco_product(torch.zeros((8, 8), dtype=torch.float16), torch.zeros((1, 8), dtype=torch.float16),
                                             torch.zeros((1, 8)))
