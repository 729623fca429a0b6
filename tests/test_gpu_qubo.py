"""QUBO samplers vs golden vectors captured from rlsolver/methods/MCPG/sampling.py."""
import numpy as np
import pytest
import torch

from oracle import oracle_np as onp
from rlsolver_amd.methods import MCPG_qubo as q
from tests.gpu_util import DEV

pytestmark = pytest.mark.gpu


def dev(a, dtype=None):
    t = torch.from_numpy(np.ascontiguousarray(a)).to(DEV)
    return t.to(dtype) if dtype is not None else t


@pytest.mark.parametrize("name", ["nbiq_5", "rand_24"])
@pytest.mark.parametrize("mode", ["pm1", "bin"])
def test_qubo_golden(golden, name, mode):
    _check_golden(golden("qubo"), name, mode)


@pytest.mark.parametrize("name", ["upper_30", "asym_32", "frac_20"])
@pytest.mark.parametrize("mode", ["pm1", "bin"])
def test_qubo_asym_golden(golden, name, mode):
    """An upper-triangular Q, an asymmetric one and one in quarters with a fractional diagonal: the reference takes Q as given.
    The sampler picks its kernel by itself; every kernel path on such matrices: test_gpu_qubo_general.py."""
    _check_golden(golden("qubo_asym"), name, mode)


def _check_golden(z, name, mode):
    data = {"Q": dev(z[f"{name}/Q"]), "nvar": z[f"{name}/Q"].shape[0]}
    fn = q.mcpg_sampling_qubo if mode == "pm1" else q.mcpg_sampling_qubo_bin
    max_res, best, raw, value = fn(data, dev(z[f"{name}/start"], torch.float32), dev(z[f"{name}/probs"]),
                                   int(z[f"{name}/num_ls"]), int(z[f"{name}/change_times"]), int(z[f"{name}/M"]),
                                   DEV, index=dev(z[f"{name}/{mode}/index"]), u=dev(z[f"{name}/{mode}/u"]))
    assert np.array_equal(raw.cpu().numpy().astype(np.uint8), z[f"{name}/{mode}/raw"])
    assert np.array_equal(max_res.cpu().numpy(), z[f"{name}/{mode}/max_res"])
    assert np.array_equal(best.cpu().numpy(), z[f"{name}/{mode}/best"])
    np.testing.assert_allclose(value.cpu().numpy(), z[f"{name}/{mode}/value"], rtol=1e-6, atol=1e-3)


def test_qubo_value_is_quadratic_form_and_sweep_is_monotone():
    rng = np.random.RandomState(3)
    n, C = 150, 130
    Qn = rng.randint(-50, 51, size=(n, n)).astype(np.float32)
    Qn = Qn + Qn.T
    x0 = rng.randint(0, 2, size=(n, C)).astype(np.float32)
    Q = dev(Qn)
    for binary in (False, True):
        x1, v1 = q.qubo_local_search_value(Q, dev(x0), 0, binary)       # no sweeps: pure value
        s = x0 if binary else 2 * x0 - 1
        assert np.array_equal(x1.cpu().numpy(), x0)
        assert np.array_equal(v1.cpu().numpy(), np.einsum("ic,ij,jc->c", s, Qn, s).astype(np.float32))
        x2, v2 = q.qubo_local_search_value(Q, dev(x0), 3, binary)
        s2 = x2.cpu().numpy() if binary else 2 * x2.cpu().numpy() - 1
        assert np.array_equal(v2.cpu().numpy(), np.einsum("ic,ij,jc->c", s2, Qn, s2).astype(np.float32))
        want_x, want_v = onp.qubo_local_search_value(Qn, x0, 3, binary)
        assert np.array_equal(x2.cpu().numpy(), want_x) and np.array_equal(v2.cpu().numpy(), want_v.astype(np.float32))
        assert (v2 >= v1).all()                                          # symmetric Q: coordinate ascent never loses


@pytest.mark.parametrize("n,C,density", [(150, 130, 0.05), (1000, 70, 0.01), (64, 64, 0.5), (333, 200, 0.2)])
def test_qubo_sparse_equals_dense_and_block_sweep_equals_sequential(n, C, density):
    """(1) The block Gauss-Seidel kernel (8 variables per block, in-block corrections) gives exactly the variable-by-
    variable sweep of MCPG/sampling.py:332-337 / :357-362 -- checked against a numpy restatement of that loop;
    (2) the CSR kernel gives exactly what the dense kernel gives (integer Q: every sum is order independent)."""
    rng = np.random.RandomState(n)
    Qn = (rng.randint(-30, 31, size=(n, n)) * (rng.rand(n, n) < density)).astype(np.float32)
    Qn = np.triu(Qn) + np.triu(Qn, 1).T
    x0 = rng.randint(0, 2, size=(n, C)).astype(np.float32)
    Q = dev(Qn)
    csr = q.qubo_to_csr(Q)
    assert int(csr[0][-1]) == int((Qn != 0).sum())
    for binary in (False, True):
        want_x, want_v = onp.qubo_local_search_value(Qn, x0, 2, binary)       # the reference's loop, sampling.py:332-337
        want_v = want_v.astype(np.float32)
        xd, vd = q.qubo_local_search_value(Q, dev(x0), 2, binary)
        xs_, vs_ = q.qubo_sparse_local_search_value(csr, dev(x0), 2, binary)            # by levels: the waves of a workgroup side by side
        xq_, vq_ = q.qubo_sparse_local_search_value(csr[:3], dev(x0), 2, binary)        # one wave walking the rows in order
        assert np.array_equal(xd.cpu().numpy(), want_x) and np.array_equal(vd.cpu().numpy(), want_v)
        assert torch.equal(xd, xs_) and torch.equal(vd, vs_) and torch.equal(xd, xq_) and torch.equal(vd, vq_)
    # the level schedule itself: every row once, ascending within a level, no entry between two rows of a level, and every
    # neighbour below a row in an earlier level
    lv_ptr, lv_rows = csr[3].cpu().numpy(), csr[4].cpu().numpy()
    assert sorted(lv_rows.tolist()) == list(range(n)) and lv_ptr[0] == 0 and lv_ptr[-1] == n
    level = np.empty(n, dtype=np.int64)
    for lv in range(lv_ptr.size - 1):
        rows = lv_rows[lv_ptr[lv]:lv_ptr[lv + 1]]
        assert (np.diff(rows) > 0).all()
        level[rows] = lv
    ii, jj = np.nonzero(Qn)
    off = ii != jj
    assert (level[ii[off]] != level[jj[off]]).all() and (level[jj[off & (jj < ii)]] < level[ii[off & (jj < ii)]]).all()


def test_qubo_sampler_picks_the_kernel_by_cost_and_both_agree():
    """n = 1500 at 0.3 % fill over 2^15 chains: the CSR kernel's level sweep beats 2 n^2 C flops (qubo_prefers_sparse);
    a 30 %-filled matrix goes dense.  Either way the sampler returns what the other kernel returns."""
    rng = np.random.RandomState(5)
    n, M, R = 1500, 256, 128
    Qn = (rng.randint(-9, 10, size=(n, n)) * (rng.rand(n, n) < 0.003)).astype(np.float32)
    Qn = np.triu(Qn) + np.triu(Qn, 1).T
    start = dev(rng.randint(0, 2, size=(n, M * R)).astype(np.float32))
    probs = dev((rng.rand(n) * 0.6 + 0.2).astype(np.float32))
    T = 8
    index = torch.randint(0, n, (5 * T, M * R), device=DEV)
    u = torch.rand(5 * T, M * R, device=DEV)
    auto = {"Q": dev(Qn), "nvar": n}
    dense = {"Q": dev(Qn), "nvar": n, "csr": None}
    a = q.mcpg_sampling_qubo(auto, start, probs, 2, T, M, DEV, index=index, u=u)
    b = q.mcpg_sampling_qubo(dense, start, probs, 2, T, M, DEV, index=index, u=u)
    assert auto["csr"] is not None and dense["csr"] is None
    assert all(torch.equal(x, y) for x, y in zip(a, b))
    # a 30 %-filled matrix goes dense at any chain count (the CSR kernel's entry count has caught up)
    Qd = (rng.randint(-9, 10, size=(n, n)) * (rng.rand(n, n) < 0.3)).astype(np.float32)
    few = {"Q": dev(np.triu(Qd) + np.triu(Qd, 1).T), "nvar": n}
    q.mcpg_sampling_qubo(few, start[:, :64].contiguous(), probs, 1, T, 16, DEV, index=index[:, :64].contiguous(),
                         u=u[:, :64].contiguous())
    assert few["csr"] is None


@pytest.mark.parametrize("n,C", [(70, 32768 + 37), (45, 20000), (129, 100), (31, 64), (257, 33)])
def test_qubo_dense_kernel_variants_equal_the_sequential_sweep(n, C):
    """The launcher picks 64-chain workgroups from 2^15 chains on and 4 instead of 8 waves once the grid exceeds two
    workgroups per CU; n is chosen off every alignment the kernel likes (rows not 16-byte aligned, ragged last block,
    ragged last batch, ragged chain tile).  Integer Q: bit-exact against the variable-by-variable loop of
    MCPG/sampling.py:332-337 / :357-362 and against x^T Q x."""
    rng = np.random.RandomState(n + C)
    Qn = rng.randint(-40, 41, size=(n, n)).astype(np.float32)
    Qn = np.triu(Qn) + np.triu(Qn, 1).T
    x0 = rng.randint(0, 2, size=(n, C)).astype(np.float32)
    Q = dev(Qn)
    for binary in (False, True):
        want_x, want_v = onp.qubo_local_search_value(Qn, x0, 2, binary)
        want_v = want_v.astype(np.float32)
        xd, vd = q.qubo_local_search_value(Q, dev(x0), 2, binary)
        assert np.array_equal(xd.cpu().numpy(), want_x)
        assert np.array_equal(vd.cpu().numpy(), want_v)
