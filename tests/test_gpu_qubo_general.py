"""K11 (dense MFMA) and K11s (CSR, sequential and by levels) on the matrices the reference accepts and the symmetric tests never
reach: triangular and asymmetric Q, empty matrices and rows, rows around the CSR chunk length, exact ties at the threshold,
fractional values, and n at every kernel's LDS limit.  Every path bit for bit against oracle_np.qubo_local_search_value (the
reference's loop, MCPG/sampling.py:332-337 / :357-362, in float64): the values are integers or multiples of 1/4 with every
partial sum far below 2^22, so every float32 sum is exact in any order."""
import contextlib

import numpy as np
import pytest
import torch

from oracle import oracle_np as onp
from rlsolver_amd import _abi
from rlsolver_amd.methods import MCPG_qubo as q
from tests.gpu_util import DEV

pytestmark = pytest.mark.gpu

RLS_EUNSUPPORTED = -2


def dev(a):
    return torch.from_numpy(np.ascontiguousarray(a)).to(DEV)


@contextlib.contextmanager
def level_waves(value):
    """RLS_QUBO_LEVELS: 4 / 8 / 16 forces the level kernel's waves per tile, 0 the sequential kernel."""
    _abi.tuning_set("RLS_QUBO_LEVELS", value)
    try:
        yield
    finally:
        _abi.tuning_unset("RLS_QUBO_LEVELS")


def _ints(rng, shape, lo, hi):
    """Nonzero integers in +-[lo, hi]."""
    return rng.randint(lo, hi + 1, size=shape) * (2 * rng.randint(0, 2, size=shape) - 1)


def make_q(kind, seed):
    rng = np.random.RandomState(seed)
    if kind in ("upper", "lower", "asym"):
        n = 150
        A = _ints(rng, (n, n), 1, 30) * (rng.rand(n, n) < 0.15)
        if kind == "upper":
            return np.triu(A).astype(np.float32)
        if kind == "lower":
            return np.tril(A).astype(np.float32)
        drop = rng.rand(n, n) < 0.5                                   # Q_ij != 0 with Q_ji == 0, in both triangles
        return np.where(drop & ~drop.T & ~np.eye(n, dtype=bool), 0, A).astype(np.float32)
    if kind == "zero":
        return np.zeros((40, 40), np.float32)
    if kind == "diag":
        return np.diag(_ints(rng, 50, 1, 20) * (rng.rand(50) < 0.8)).astype(np.float32)
    if kind == "empty_rows":                                          # a third of the rows and a third of the columns empty
        n = 100
        A = _ints(rng, (n, n), 1, 30) * (rng.rand(n, n) < 0.05)
        A[rng.choice(n, n // 3, replace=False)] = 0
        A[:, rng.choice(n, n // 3, replace=False)] = 0
        return A.astype(np.float32)
    if kind == "n1":
        return np.array([[-3.0]], np.float32)
    if kind == "n1_zero":
        return np.zeros((1, 1), np.float32)
    if kind == "degrees":                                             # the CSR kernels' 64-entry chunks: 0, 1, 63, 64, 65, > 128
        n = 300
        Q = np.zeros((n, n), np.float32)
        degs = [0, 1, 63, 64, 65, 129, 200, 128, 127]
        for i in range(n):
            d = degs[i % len(degs)] if i < 5 * len(degs) else int(rng.randint(0, 6))
            cols = rng.choice(n, d, replace=False)
            Q[i, cols] = _ints(rng, d, 1, 9)
        return Q
    if kind == "ties":                                                # {-1, 0, 1} and even diagonals: res hits thr exactly
        n = 80
        Q = rng.randint(-1, 2, size=(n, n)).astype(np.float32)
        np.fill_diagonal(Q, 2.0 * rng.randint(-1, 2, size=n))
        return Q
    if kind == "quarters":                                            # multiples of 1/4, odd quarters on the diagonal
        n = 64
        Q = (rng.randint(-40, 41, size=(n, n)) * (rng.rand(n, n) < 0.3) / 4.0).astype(np.float32)
        np.fill_diagonal(Q, (2 * rng.randint(-20, 21, size=n) + 1) / 4.0)
        return Q
    if kind in ("upper_sparse", "asym_sparse", "zero_600"):             # sparse enough for the sampler's cost model to pick CSR
        n = 600
        if kind == "zero_600":
            return np.zeros((n, n), np.float32)
        A = _ints(rng, (n, n), 1, 30) * (rng.rand(n, n) < 0.01)
        if kind == "upper_sparse":
            return np.triu(A).astype(np.float32)
        drop = rng.rand(n, n) < 0.5
        return np.where(drop & ~drop.T & ~np.eye(n, dtype=bool), 0, A).astype(np.float32)
    raise ValueError(kind)


KINDS = ["upper", "lower", "asym", "zero", "diag", "empty_rows", "n1", "n1_zero", "degrees", "ties", "quarters"]


def every_path(Qn, x0, num_ls, binary):
    """(name, x, value) of every K11 path on the same input."""
    Q, xs = dev(Qn), dev(x0)
    csr = q.qubo_to_csr(Q)
    out = [("dense",) + q.qubo_local_search_value(Q, xs, num_ls, binary),
           ("csr",) + q.qubo_sparse_local_search_value(csr[:3], xs, num_ls, binary),
           ("levels auto",) + q.qubo_sparse_local_search_value(csr, xs, num_ls, binary)]
    for w in (0, 16, 8, 4):
        with level_waves(w):
            out.append((f"levels knob {w}",) + q.qubo_sparse_local_search_value(csr, xs, num_ls, binary))
    return out


@pytest.mark.parametrize("C", [1, 63, 64, 65, 200])
@pytest.mark.parametrize("kind", KINDS)
def test_every_kernel_path_equals_the_oracle(kind, C):
    """The dense kernel, the sequential CSR kernel, and the level kernel (auto, and forced to W = 16 / 8 / 4 and off) return the
    reference loop's x and x^T Q x bit for bit.  For an asymmetric Q the level schedule must separate Q_ij from Q_ji: with
    levels over row i's own entries only, an upper-triangular Q was one level and its rows raced."""
    Qn = make_q(kind, 7 + C)
    n = Qn.shape[0]
    rng = np.random.RandomState(1000 * n + C)
    x0 = rng.randint(0, 2, size=(n, C)).astype(np.float32)
    for num_ls in (0, 3):
        for binary in (False, True):
            stats = {}
            want_x, want_v = onp.qubo_local_search_value(Qn, x0, num_ls, binary, stats)
            assert np.array_equal(want_v.astype(np.float32).astype(np.float64), want_v)
            if kind == "ties" and num_ls and C >= 63:                 # the strict '>' is really exercised, in both modes
                assert stats["ties"] > 0, binary
            for name, x, v in every_path(Qn, x0, num_ls, binary):
                tag = (kind, C, num_ls, binary, name)
                assert np.array_equal(x.cpu().numpy(), want_x), tag
                assert np.array_equal(v.cpu().numpy(), want_v.astype(np.float32)), tag


@pytest.mark.parametrize("kind", ["upper", "asym", "zero", "degrees", "ties", "quarters", "n1", "upper_sparse", "asym_sparse",
                                  "zero_600"])
@pytest.mark.parametrize("M,R", [(16, 4), (13, 5)])
@pytest.mark.parametrize("mode", ["pm1", "bin"])
def test_sampler_auto_dispatch_equals_the_oracle(kind, M, R, mode):
    """mcpg_sampling_qubo(_bin) with the kernel picked by the sampler (the sparse ones go to the CSR kernel by levels, where
    a triangular or asymmetric Q raced and the zero matrix arrived with NULL entry pointers and was refused): the best samples, their values and the centred values are the oracle's sweep on the
    sampler's own metro output."""
    Qn = make_q(kind, 11)
    n, C, T = Qn.shape[0], M * R, 3
    g = torch.Generator(device=DEV).manual_seed(n + C)
    start = torch.randint(0, 2, (n, C), device=DEV, generator=g).float()
    probs = torch.rand(n, device=DEV, generator=g) * 0.6 + 0.2
    index = torch.randint(0, n, (5 * T, C), device=DEV, generator=g)
    u = torch.rand(5 * T, C, device=DEV, generator=g)
    fn = q.mcpg_sampling_qubo if mode == "pm1" else q.mcpg_sampling_qubo_bin
    data = {"Q": dev(Qn), "nvar": n}
    max_res, best, raw, value = fn(data, start, probs, 2, T, M, DEV, index=index, u=u)
    if kind in ("upper_sparse", "asym_sparse", "zero_600"):
        assert data["csr"] is not None                                # the CSR kernel by levels
    assert torch.equal(raw, q.metro_sampling(probs, start, T, DEV, index=index, u=u))      # (the metro walk: test_gpu_qubo.py)
    x, v = onp.qubo_local_search_value(Qn, raw.cpu().numpy(), 2, mode == "bin")
    idx = np.arange(M) + v.reshape(-1, M).argmax(axis=0) * M
    assert np.array_equal(max_res.cpu().numpy(), v[idx].astype(np.float32))
    assert np.array_equal(best.cpu().numpy(), x[:, idx])
    np.testing.assert_allclose(value.cpu().numpy(), -(v - v.mean()), rtol=1e-6, atol=1e-3)


# ------------------------------------------------------------------------------------------------ LDS limits

def _num_cus():
    return torch.cuda.get_device_properties(DEV).multi_processor_count


def sparse_csr(n, seed):
    """An asymmetric sparse Q in CSR form (numpy): three off-diagonal entries per row, a diagonal entry on every other row,
    integers in +-[1, 9]."""
    rng = np.random.RandomState(seed)
    rows, cols = [], []
    for i in range(n):
        c = np.unique(np.concatenate([rng.randint(0, n, 3), [i] if i % 2 else []]).astype(np.int64))
        rows.append(np.full(c.size, i, np.int64))
        cols.append(c)
    r, c = np.concatenate(rows), np.concatenate(cols)
    rowptr = np.zeros(n + 1, np.int64)
    rowptr[1:] = np.cumsum(np.bincount(r, minlength=n))
    return rowptr, c, _ints(rng, c.size, 1, 9).astype(np.float64)


def dense_from_csr(n, csr):
    rowptr, col, val = csr
    Q = torch.zeros((n, n), dtype=torch.float32, device=DEV)
    Q[torch.from_numpy(np.repeat(np.arange(n), np.diff(rowptr))).to(DEV), torch.from_numpy(col).to(DEV)] = \
        torch.from_numpy(val.astype(np.float32)).to(DEV)
    return Q


def csr_on_device(csr, levels):
    rowptr, col, val = (dev(csr[0].astype(np.int32)), dev(csr[1].astype(np.int32)), dev(csr[2].astype(np.float32)))
    return (rowptr, col, val) + (q.qubo_levels(rowptr, col) if levels else ())


def _chain_sample(C):
    """The chains compared against the oracle: the chains are independent, so the first and the last tiles stand for all."""
    return np.unique(np.r_[0:min(C, 64), max(0, C - 65):C])


def _check_chains(csr, xs, x, v, num_ls, binary):
    cols = torch.from_numpy(_chain_sample(xs.shape[1])).to(DEV)
    want_x, want_v = onp.qubo_local_search_value(csr, xs[:, cols].cpu().numpy(), num_ls, binary)
    assert np.array_equal(x[:, cols].cpu().numpy(), want_x)
    assert np.array_equal(v[cols].cpu().numpy(), want_v.astype(np.float32))


def _refused(fn):
    with pytest.raises(_abi.RlsError) as e:
        fn()
    assert e.value.code == RLS_EUNSUPPORTED, str(e.value)


# (form, level-kernel waves forced or None, chains, largest n); LDS of 160 KB:
#   sequential CSR  12 n + 4                     -> 13 653
#   CSR by levels   8 n + 256 W                  -> 19 968 / 20 224 / 20 352 at W = 16 / 8 / 4
#   dense           4 n_pad + 40 960 (8 waves, n_pad a multiple of 256)             -> 30 720 while ceil(C / 32) <= 2 CUs
#                   4 n_pad + 20 480 (4 waves, n_pad a multiple of 128)             -> 35 840 up to C < 128 CUs
#                   8 n_pad + 36 864 (64-chain workgroups, n_pad a multiple of 128) -> 15 872 from C = 128 CUs on
# Chain counts in CUs are resolved in the test (no device query at collection).
LDS_CASES = [("csr", None, 64, 13653), ("levels", 16, 64, 19968), ("levels", 8, 64, 20224), ("levels", 4, 64, 20352),
             ("levels", None, 65, 19968),
             ("dense", None, 33, 30720), ("dense", None, "64 CUs + 1", 35840), ("dense", None, "128 CUs", 15872)]


def _chains(C):
    return {"64 CUs + 1": 64 * _num_cus() + 1, "128 CUs": 128 * _num_cus()}.get(C, C)


@pytest.mark.parametrize("form,waves,C,n_max", LDS_CASES)
def test_kernels_at_their_lds_limits(form, waves, C, n_max):
    """n = the largest size a kernel's LDS holds: the oracle's result; n + 1: RLS_EUNSUPPORTED before any launch (the outputs
    untouched), and rls_qubo_local_search_supported says so in both cases."""
    binary = bool(n_max % 2)
    C = _chains(C)
    ctx = level_waves(waves) if waves else contextlib.nullcontext()
    with ctx:
        for n in (n_max, n_max + 1):
            ok = n == n_max
            csr_np = sparse_csr(n, n)
            g = torch.Generator(device=DEV).manual_seed(n)
            xs = torch.randint(0, 2, (n, C), device=DEV, generator=g).float()
            out = torch.full_like(xs, float("nan"))
            value = torch.full((C,), float("nan"), device=DEV)
            assert q.qubo_supported(n, C, form) == ok, (form, waves, C, n)
            if form == "dense":
                Q = dense_from_csr(n, csr_np)
                call = lambda: _abi.call("rls_qubo_local_search_value", Q.data_ptr(), n, xs.data_ptr(), out.data_ptr(), C, 1,
                                         int(binary), value.data_ptr(), None)
            else:
                csr = csr_on_device(csr_np, form == "levels")
                lv = (csr[3].data_ptr(), csr[4].data_ptr(), csr[3].numel() - 1) if form == "levels" else (None, None, 0)
                call = lambda: _abi.call("rls_qubo_sparse_local_search_value", csr[0].data_ptr(), csr[1].data_ptr(),
                                         csr[2].data_ptr(), n, *lv, xs.data_ptr(), out.data_ptr(), C, 1, int(binary),
                                         value.data_ptr(), None)
            if ok:
                call()
                torch.cuda.synchronize()
                _check_chains(csr_np, xs, out, value, 1, binary)
            else:
                _refused(call)
                torch.cuda.synchronize()
                assert bool(out.isnan().all()) and bool(value.isnan().all())
                with pytest.raises(RuntimeError, match=r"\(-2\)"):          # the same through the torch op
                    if form == "dense":
                        q.qubo_local_search_value(Q, xs, 1, binary)
                    else:
                        q.qubo_sparse_local_search_value(csr, xs, 1, binary)
            del xs, out, value, call
            Q = csr = None
            torch.cuda.empty_cache()


def _sample_and_check(Qdev, csr_np, n, M, R, binary):
    C, T = M * R, 2
    g = torch.Generator(device=DEV).manual_seed(n)
    start = torch.randint(0, 2, (n, C), device=DEV, generator=g).float()
    probs = torch.rand(n, device=DEV, generator=g) * 0.6 + 0.2
    index = torch.randint(0, n, (5 * T, C), device=DEV, generator=g)
    u = torch.rand(5 * T, C, device=DEV, generator=g)
    data = {"Q": Qdev, "nvar": n}
    fn = q.mcpg_sampling_qubo_bin if binary else q.mcpg_sampling_qubo
    max_res, best, raw, value = fn(data, start, probs, 1, T, M, DEV, index=index, u=u)
    x, v = onp.qubo_local_search_value(csr_np, raw.cpu().numpy(), 1, binary)
    idx = np.arange(M) + v.reshape(-1, M).argmax(axis=0) * M
    assert np.array_equal(max_res.cpu().numpy(), v[idx].astype(np.float32))
    assert np.array_equal(best.cpu().numpy(), x[:, idx])
    np.testing.assert_allclose(value.cpu().numpy(), -(v - v.mean()), rtol=1e-6, atol=1e-2)
    return data


def test_sampler_takes_the_kernel_that_fits():
    """Shapes only one kernel runs.  n = 20 400 at 64 chains (16 waves per tile; the metro walk still fits): past both CSR
    kernels' LDS, the dense kernel's fits -- a sparse Q, which the cost model sends to the CSR kernel, must still come back
    from the dense one.  n = 14 000 with the level
    kernel switched off (RLS_QUBO_LEVELS = 0): the sequential CSR kernel refuses it, the dense one runs it.  n = 15 873 from
    128 chains per CU on: the dense kernel's 64-chain workgroups refuse it, the level kernel runs it."""
    n = 20400
    csr_np = sparse_csr(n, 3)
    assert not q.qubo_supported(n, 64, "levels") and q.qubo_supported(n, 64, "dense")
    assert q.qubo_prefers_sparse(n, csr_np[1].size, 64)
    data = _sample_and_check(dense_from_csr(n, csr_np), csr_np, n, 16, 4, False)
    assert data["csr"] is None
    del data
    torch.cuda.empty_cache()
    n = 14000
    csr_np = sparse_csr(n, 4)
    with level_waves(0):
        assert not q.qubo_supported(n, 64, "levels") and q.qubo_supported(n, 64, "dense")
        data = _sample_and_check(dense_from_csr(n, csr_np), csr_np, n, 32, 2, True)
        assert data["csr"] is None
    del data
    torch.cuda.empty_cache()
    n, C = 15873, 128 * _num_cus()
    csr_np = sparse_csr(n, 5)
    assert not q.qubo_supported(n, C, "dense") and q.qubo_supported(n, C, "levels")
    Qd = dense_from_csr(n, csr_np)
    g = torch.Generator(device=DEV).manual_seed(n)
    start = torch.randint(0, 2, (n, C), device=DEV, generator=g).float()
    probs = torch.rand(n, device=DEV, generator=g) * 0.6 + 0.2
    index = torch.randint(0, n, (10, C), device=DEV, generator=g)
    u = torch.rand(10, C, device=DEV, generator=g)
    for data in ({"Q": Qd, "nvar": n}, {"Q": Qd, "nvar": n, "csr": None}):    # the cost model's pick, and a forced dense one
        max_res, best, raw, value = q.mcpg_sampling_qubo(data, start, probs, 1, 2, C // 64, DEV, index=index, u=u)
        x, v = q.qubo_sparse_local_search_value(csr_on_device(csr_np, True), raw, 1, False)
        _check_chains(csr_np, raw, x, v, 1, False)
        assert torch.equal(-(v - v.mean()), value)
    del Qd, start, raw, x
    torch.cuda.empty_cache()
