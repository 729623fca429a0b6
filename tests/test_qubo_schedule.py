"""The level schedule of the CSR QUBO kernel (MCPG_qubo.qubo_levels): host work, no GPU."""
import numpy as np
import pytest
import torch

from rlsolver_amd.methods import MCPG_qubo as q


def _levels(Qn):
    csr = q.qubo_to_csr(torch.from_numpy(np.ascontiguousarray(Qn, dtype=np.float32)))
    lv_ptr, lv_rows = csr[3].numpy(), csr[4].numpy()
    n = Qn.shape[0]
    assert sorted(lv_rows.tolist()) == list(range(n)) and lv_ptr[0] == 0 and lv_ptr[-1] == n
    level = np.empty(n, dtype=np.int64)
    for lv in range(lv_ptr.size - 1):
        rows = lv_rows[lv_ptr[lv]:lv_ptr[lv + 1]]
        assert rows.size and (np.diff(rows) > 0).all()
        level[rows] = lv
    return lv_ptr, lv_rows, level


def _rowwise_levels(Qn):
    """The round-6 rule over row i's own entries, level(i) = 1 + max(level(j): j < i, Q_ij != 0) -- the schedule whose timings
    DESIGN.md records; for a symmetric pattern the symmetrised rule must reproduce it exactly."""
    n = Qn.shape[0]
    level = np.zeros(n, dtype=np.int64)
    for i in range(n):
        nb = np.nonzero(Qn[i, :i])[0]
        if nb.size:
            level[i] = level[nb].max() + 1
    order = np.lexsort((np.arange(n), level))
    L = int(level.max()) + 1 if n else 1
    lv_ptr = np.zeros(L + 1, dtype=np.int32)
    lv_ptr[1:] = np.cumsum(np.bincount(level, minlength=L))
    return lv_ptr, order.astype(np.int32)


def _patterns(n, seed):
    rng = np.random.RandomState(seed)
    A = (rng.randint(-3, 4, size=(n, n)) * (rng.rand(n, n) < 0.08)).astype(np.float32)
    asym = A.copy()
    asym[np.triu(np.ones((n, n), bool), 1) & (rng.rand(n, n) < 0.5)] = 0          # Q_ij != 0 with Q_ji == 0 in both triangles
    asym[np.tril(np.ones((n, n), bool), -1) & (rng.rand(n, n) < 0.5)] = 0
    return {"upper": np.triu(A), "lower": np.tril(A), "asym": asym, "strict_upper": np.triu(A, 1),
            "chain_upper": np.diag(np.ones(n - 1, np.float32), 1)}


@pytest.mark.parametrize("n", [2, 7, 64, 150])
@pytest.mark.parametrize("kind", ["upper", "lower", "asym", "strict_upper", "chain_upper"])
def test_levels_separate_every_entry_of_an_asymmetric_pattern(n, kind):
    """Row i reads word j whenever Q_ij != 0: the rows of one level may hold no entry between them in EITHER direction, and
    every neighbour j < i (through Q_ij or Q_ji) must sit in an earlier level -- otherwise the level kernel's waves race on
    word j.  With the rule over row i's own entries only, an upper-triangular Q put every row in level 0."""
    Qn = _patterns(n, n)[kind]
    _, _, level = _levels(Qn)
    ii, jj = np.nonzero(Qn)
    off = ii != jj
    ii, jj = ii[off], jj[off]
    assert (level[ii] != level[jj]).all(), kind
    lo, hi = np.minimum(ii, jj), np.maximum(ii, jj)
    assert (level[lo] < level[hi]).all(), kind
    if kind == "chain_upper":                                # Q_{i,i+1} only: a strict chain, one row per level
        assert (level == np.arange(n)).all()


@pytest.mark.parametrize("n,density,seed", [(150, 0.05, 0), (1000, 0.02, 1), (333, 0.2, 2), (64, 0.5, 3), (1500, 0.003, 4)])
def test_levels_of_a_symmetric_pattern_are_the_round6_schedule(n, density, seed):
    rng = np.random.RandomState(seed)
    A = (rng.randint(-30, 31, size=(n, n)) * (rng.rand(n, n) < density)).astype(np.float32)
    Qn = np.triu(A) + np.triu(A, 1).T
    lv_ptr, lv_rows, _ = _levels(Qn)
    want_ptr, want_rows = _rowwise_levels(Qn)
    assert np.array_equal(lv_ptr, want_ptr) and np.array_equal(lv_rows, want_rows)


def test_levels_of_empty_and_diagonal_patterns():
    for Qn in (np.zeros((5, 5), np.float32), np.diag(np.arange(1, 6, dtype=np.float32)), np.zeros((1, 1), np.float32)):
        lv_ptr, lv_rows, level = _levels(Qn)
        assert lv_ptr.tolist() == [0, Qn.shape[0]] and (level == 0).all()
    csr = q.qubo_to_csr(torch.zeros((4, 4)))
    assert csr[1].numel() == 0 and csr[2].numel() == 0 and csr[0].tolist() == [0] * 5
