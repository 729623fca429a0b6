"""MaxSAT family, host side (no GPU): the loader against hand-computed lists, the numpy oracle against the fixture recorded
from the reference, the host library's level schedule replayed in plain Python against the sequential oracle, the limits
and the errors."""
import os

import numpy as np
import pytest
import torch

import maxsat_oracle as orc

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "maxsat.npz")


@pytest.fixture(scope="module")
def fx():
    return np.load(GOLDEN)


def ms():
    from rlsolver_amd.methods import MCPG_maxsat
    return MCPG_maxsat


def case_names(fx):
    return [str(n) for n in fx["names"]]


def write(tmp_path, name, text):
    p = tmp_path / name
    p.write_text(text)
    return str(p)


def test_loader_cnf_by_hand(tmp_path):
    # clause 0: x1 v -x2; clause 1: x2 v x2 v -x3 (a duplicate literal: listed twice for x2); clause 2: empty; header count 5
    path = write(tmp_path, "a.cnf", "c comment\np cnf 4 5\n1 -2 0\n2 2 -3 0\n0\n")
    data, nvar = ms().maxsat_dataloader(path, "cpu", sorted_nodes=[1, 0, 2, 3])
    assert nvar == 4 and data.pdata[:2] == [4, 5] and len(data.pdata) == 5
    assert data.pdata[2] == [0, 1, 1, 1, 2]
    assert data.pdata[3].tolist() == [0, 0, 1, 1, 1] and data.pdata[4].tolist() == [1, -1, 1, 1, -1]
    nvi, nci, nneg, order, degree = data.ndata
    assert [t.tolist() for t in nvi] == [[0, 1], [0, 1, 1, 1, 2, 1, 1, 2], [1, 1, 2], []]
    assert [t.tolist() for t in nci] == [[0, 0], [0, 0, 1, 1, 1, 2, 2, 2], [0, 0, 0], []]
    assert [t.tolist() for t in nneg] == [[1, -1], [1, -1, 1, 1, -1, 1, 1, -1], [1, 1, -1], []]
    assert degree.tolist() == [1, 3, 1, 0] and order.tolist() == [1, 0, 2, 3]
    assert (data.num_nodes, data.num_edges) == (4, 5)


def test_loader_wcnf_by_hand(tmp_path):
    path = write(tmp_path, "a.wcnf", "p wcnf 3 3 9\n9 1 -2 0\n3 2 0\n1 -3 -1 0\n")
    data, nvar = ms().maxsat_dataloader(path, "cpu", sorted_nodes=[0, 1, 2])
    assert data.pdata[:2] == [3, 3] and data.pdata[5:] == [9, 1]
    assert data.pdata[2] == [0, 1, 1, 2, 0] and data.pdata[4].tolist() == [9, -9, 3, -1, -1]
    assert [t.tolist() for t in data.ndata[2]] == [[9, -9, -1, -1], [9, -9, 3], [-1, -1]]
    assert data.num_edges == 3 - 1 + 9 * 1                     # K = nclause - nhard + top * nhard
    with pytest.raises(Exception, match="Unrecognized file type"):
        ms().maxsat_dataloader(write(tmp_path, "a.txt", "p cnf 1 0\n"), "cpu")


def test_sort_node_orders_by_degree_with_a_bounded_tie_break():
    data = ms().make_data(6, [[1, 2], [1, 3], [1, -4], [2, 5]], device="cpu")
    order = data.ndata[3].tolist()
    assert order[0] == 0 and order[1] == 1 and order[-1] == 5 and sorted(order) == list(range(6))
    nd = ms().sort_node(list(data.ndata))
    assert sorted(nd[3].tolist()) == list(range(6)) and nd[3][0] == 0


def _instance(fx, name):
    return orc.parse(str(fx[f"{name}/text"]), str(fx[f"{name}/ext"]))


def test_oracle_and_product_loader_match_the_reference_lists(fx):
    assert "reference" in str(fx["source"])
    for name in case_names(fx):
        inst = _instance(fx, name)
        cat = lambda rows: np.asarray([v for r in rows for v in r], dtype=np.int64)      # noqa: E731
        assert np.array_equal(inst.vi, fx[f"{name}/variable_index"]) and np.array_equal(inst.ci, fx[f"{name}/clause_index"])
        assert np.array_equal(inst.neg, fx[f"{name}/neg_index"]) and np.array_equal(inst.degree, fx[f"{name}/degree"])
        assert [len(r) for r in inst.nvi] == fx[f"{name}/nvi_len"].tolist()
        for got, key in ((inst.nvi, "nvi"), (inst.nci, "nci"), (inst.nneg, "nneg")):
            assert np.array_equal(cat(got), fx[f"{name}/{key}"]), (name, key)
        extra = [] if inst.weights is None else [inst.top, inst.nhard]
        assert extra == fx[f"{name}/extra"].tolist()
        data = ms().make_data(inst.nvar, inst.clauses, inst.weights, inst.top, inst.nclause, "cpu", sorted_nodes=fx[f"{name}/order"])
        assert data.pdata[2] == inst.vi.tolist() and data.pdata[5:] == extra and data.num_edges == inst.K
        for got, key in ((data.ndata[0], "nvi"), (data.ndata[1], "nci"), (data.ndata[2], "nneg")):
            assert np.array_equal(torch.cat(got).numpy(), fx[f"{name}/{key}"]), (name, key)


def test_oracle_reproduces_the_reference_sampler(fx):
    for name in case_names(fx):
        inst = _instance(fx, name)
        M, R, num_ls, T = fx[f"{name}/params"].tolist()
        got = orc.sampling(inst, fx[f"{name}/order"], fx[f"{name}/start"].astype(np.float32), fx[f"{name}/probs"], num_ls, T, M,
                           fx[f"{name}/index"].astype(np.int64), fx[f"{name}/u"], fx[f"{name}/uniforms"])
        assert np.array_equal(got[0], fx[f"{name}/max_res"]), name
        assert np.array_equal(got[1], fx[f"{name}/best"].astype(np.float32)), name
        assert np.array_equal(got[2], fx[f"{name}/raw"].astype(np.float32)), name
        assert np.array_equal(got[3], fx[f"{name}/value"]), name


def _words(x01):
    """0|1 [nvar, C <= 64] -> one python int per variable."""
    return [int(sum(int(b) << c for c, b in enumerate(row))) for row in x01]


def test_level_schedule_replay_equals_the_sequential_sweep(fx):
    """Deciding a level's variables from the pre-level state, on the table the host library builds, is the sequential sweep."""
    for name in case_names(fx):
        inst = _instance(fx, name)
        M, R, num_ls, _ = fx[f"{name}/params"].tolist()
        order = fx[f"{name}/order"]
        data = ms().make_data(inst.nvar, inst.clauses, inst.weights, inst.top, inst.nclause, "cpu", sorted_nodes=order)
        lvp, lvd = data.schedule()
        raw = fx[f"{name}/raw"].astype(np.float32)
        uni = orc.prepare_uniforms(fx[f"{name}/uniforms"])
        s = (raw.T * 2 - 1).astype(np.float32)
        assert orc.coin_rule_agrees(inst, s, order, num_ls, uni), name
        want = (orc.sweep(inst, s.copy(), order, num_ls, uni).T + 1) / 2
        coins = [[_words([uni[cnt, pos] < 0.5])[0] for pos in range(inst.nvar)] for cnt in range(num_ls)]
        got = orc.replay_schedule(lvp.numpy(), lvd.numpy(), inst.nvar, _words(raw), num_ls, coins)
        live = (1 << raw.shape[1]) - 1                  # the replay carries 64 chains per word; the fixture fills the low ones
        assert [g & live for g in got] == _words(want), name


def test_schedule_levels_of_a_chain_and_of_disjoint_clauses():
    n = 9
    chain = ms().make_data(n, [[i + 1, i + 2] for i in range(n - 1)], device="cpu", sorted_nodes=list(range(n)))
    lvp = chain.schedule()[0].numpy().view(np.uint32)
    assert lvp.size - 1 == n and all(int(v) >> 31 for v in lvp[:-1])            # every variable its own level
    flat = ms().make_data(n, [[i + 1] for i in range(n)], device="cpu", sorted_nodes=list(range(n)))
    lvp = flat.schedule()[0].numpy().view(np.uint32)
    assert lvp.size - 1 == 1 and int(lvp[0]) >> 31 == 1                          # one level, one group
    flat.ndata[3] = torch.arange(n - 1, -1, -1)                                  # a replaced order rebuilds the schedule
    assert flat.schedule()[1].numpy()[1] == 0 and flat._schedule[0][0] == n - 1


def test_supported_limits_and_errors():
    from rlsolver_amd import _abi
    max_nvar, max_w = ms().supported_limits()
    assert max_nvar == (160 * 1024 - 272) // 8 - 1 and max_w == (1 << 24) - 1
    lib = _abi.lib()
    assert lib.rls_maxsat_local_search_supported(max_nvar, max_w, None, None) == 1
    assert lib.rls_maxsat_local_search_supported(max_nvar + 1, 0, None, None) == 0
    assert lib.rls_maxsat_local_search_supported(1, max_w + 1, None, None) == 0
    assert lib.rls_maxsat_local_search_supported(0, 0, None, None) == 0
    ms().make_data(max_nvar, [[1, -max_nvar]], device="cpu")
    with pytest.raises(_abi.RlsError, match=f"RLS_EUNSUPPORTED.*{max_nvar}"):
        ms().make_data(max_nvar + 1, [[1]], device="cpu")
    with pytest.raises(_abi.RlsError, match=f"RLS_EUNSUPPORTED.*{max_w}"):
        ms().make_data(2, [[1], [2]], weights=[1 << 23, 1 << 23], top=1 << 23, device="cpu")
    with pytest.raises(_abi.RlsError, match=f"RLS_EUNSUPPORTED.*variable 0.*{max_w}"):       # one clause listed three times for x1
        ms().make_data(2, [[1, 1, 1, 2]], weights=[6_000_000], top=7_000_000, device="cpu")
    for bad in ([[0, 1]], [[1, 3]], [[-3]]):
        with pytest.raises(ValueError, match="literal"):
            ms().make_data(2, bad, device="cpu")
    # the host builder itself refuses what the Python layer checks first
    cp, order = np.array([0, 1], dtype=np.int32), np.array([0, 1], dtype=np.int32)
    for l in (0, 3, -3):
        with pytest.raises(_abi.RlsError, match="RLS_EINVAL.*literal"):
            ms().build_visit_levels(cp, np.array([l], dtype=np.int32), None, 2, order)
    with pytest.raises(_abi.RlsError, match="RLS_EINVAL.*weight"):
        ms().build_visit_levels(cp, np.array([1], dtype=np.int32), np.array([0], dtype=np.int32), 2, order)
    with pytest.raises(_abi.RlsError, match="RLS_EINVAL.*permutation"):
        ms().build_visit_levels(cp, np.array([1], dtype=np.int32), None, 2, np.array([0, 0], dtype=np.int32))
