"""Cheeger-cut family, host side (no GPU): the numpy oracle against the fixture recorded from the reference, the visit-stream
builder decoded back into order / degrees / weighted degrees / neighbour rows, sample_initializer's one-hot layout, the limits."""
import types

import numpy as np
import pytest
import torch

import cheeger_oracle as orc


def mc():
    from rlsolver_amd.methods import MCPG_cheeger
    return MCPG_cheeger


ENTRIES = list(orc.fixture_entries())


def test_fixture_covers_the_recipe():
    names = {e["name"] for e in ENTRIES}
    assert len(names) == len(ENTRIES) == 5 * 2 * 2 * 2 * 2
    for g in ("BA_5_ID0", "PL_20_ID0", "BA_100_ID0", "ER_100_ID0", "gset_14_stub"):
        for cfg in ("5x3", "64x2"):
            for kind in ("onehot", "bernoulli"):
                for fn in ("rcheegercut", "ncheegercut"):
                    for ls in (1, 2):
                        assert f"{g}/{cfg}/{kind}/{fn}/ls{ls}" in names


@pytest.mark.parametrize("e", ENTRIES, ids=[e["name"] for e in ENTRIES])
def test_oracle_equals_fixture(e):
    neg_h, best, value, h, _ = orc.sampler(e["n"], e["eu"], e["ev"], e["w"], e["order"], e["raw"], e["num_ls"], e["M"], e["normalized"])
    assert not np.isnan(h).any()                          # NaN exists only where nothing has been swept
    assert orc.same_bits(neg_h, e["neg_h"])
    assert np.array_equal(best, e["best"])
    assert orc.same_bits(value, e["value"])
    if e["kind"] == "onehot":                             # change_times = 0: the walk returns its start
        assert np.array_equal(e["raw"], e["start"]) and e["index"].shape[0] == 0


def test_fixture_onehot_start_is_sample_initializer():
    for e in ENTRIES:
        if e["kind"] != "onehot" or e["num_ls"] != 1 or e["normalized"]:
            continue
        data = types.SimpleNamespace(num_nodes=e["n"], sorted_degree_nodes=torch.from_numpy(e["order"]))
        cfg = types.SimpleNamespace(total_mcmc_num=e["M"], repeat_times=e["R"])
        for problem in ("rcheegercut", types.SimpleNamespace(value="ncheegercut")):
            got = mc().sample_initializer(problem, torch.from_numpy(e["probs"]), cfg, device="cpu", data=data)
            assert got.dtype == torch.float32 and np.array_equal(got.numpy(), e["start"])


@pytest.mark.parametrize("n,M", [(12, 5), (5, 12), (7, 7)])
def test_sample_initializer_onehot_layout(n, M):
    R = 3
    order = torch.from_numpy(np.random.RandomState(n).permutation(n))
    data = types.SimpleNamespace(num_nodes=n, sorted_degree_nodes=order)
    cfg = types.SimpleNamespace(total_mcmc_num=M, repeat_times=R)
    x = mc().sample_initializer("rcheegercut", torch.full((n,), 0.5), cfg, device="cpu", data=data).numpy()
    assert x.shape == (n, M * R)
    tail = order.numpy()[-M:]                              # M > n: all n nodes, chains n .. M - 1 stay empty
    for c in range(M * R):
        i = c % M
        want = np.zeros(n, np.float32)
        if i < len(tail):
            want[tail[i]] = 1
        assert np.array_equal(x[:, c], want)


def test_sample_initializer_other_problems_draw_bernoulli():
    cfg = types.SimpleNamespace(total_mcmc_num=4, repeat_times=3)
    probs = torch.tensor([0.0, 1.0, 0.5, 0.25])
    torch.manual_seed(5)
    got = mc().sample_initializer(types.SimpleNamespace(value="maxcut"), probs, cfg, device="cpu")
    torch.manual_seed(5)
    want = torch.distributions.bernoulli.Bernoulli(probs).sample([12]).t()
    assert got.shape == (4, 12) and torch.equal(got, want)
    assert (got[0] == 0).all() and (got[1] == 1).all()


def stream_case(name):
    rng = np.random.RandomState(3)
    if name == "hub300":
        n, eu, ev = 301, np.zeros(300, np.int64), np.arange(1, 301)
    elif name == "isolated":
        n, eu, ev = 9, np.array([0, 2, 2]), np.array([2, 5, 8])          # nodes 1, 3, 4, 6, 7 have no edge
    elif name == "loops_dups":
        n, eu, ev = 6, np.array([0, 1, 1, 2, 3, 3, 4, 1]), np.array([1, 1, 2, 1, 3, 4, 3, 0])
    elif name == "empty":
        n, eu, ev = 0, np.zeros(0, np.int64), np.zeros(0, np.int64)
    else:
        n = 40
        eu, ev = rng.randint(0, n, 120), rng.randint(0, n, 120)
    w = rng.randint(-3, 4, size=eu.shape[0])
    return n, eu.astype(np.int64), ev.astype(np.int64), w.astype(np.int64), rng.permutation(n)


@pytest.mark.parametrize("name", ["hub300", "isolated", "loops_dups", "empty", "random"])
def test_stream_round_trips(name):
    from rlsolver_amd.graph import build_csr
    from rlsolver_amd.methods.MCPG import build_cheeger_stream
    n, eu, ev, w, order = stream_case(name)
    csr = build_csr((eu, ev, w), num_nodes=n, if_bidirectional=False, keep_loops=True) if n else types.SimpleNamespace(
        num_nodes=0, rowptr=np.zeros(1, np.int32), col=np.zeros(0, np.int32), wgt=np.zeros(0, np.int32))
    stream = build_cheeger_stream(csr, order)
    assert stream.dtype == np.int32 and stream.shape == (3 * n + 2 * eu.shape[0],)
    o, deg, wdeg, rows = orc.decode_stream(stream, n)
    want_rows, want_wdeg = orc.neighbor_rows(n, eu, ev), orc.weighted_degrees(n, eu, ev, w)
    assert np.array_equal(o, order)
    for k, node in enumerate(order.tolist()):
        assert deg[k] == want_rows[node].size and wdeg[k] == want_wdeg[node]
        assert np.array_equal(np.sort(rows[k]), np.sort(want_rows[node]))          # the same multiset: the sum over a row has no order
    if name == "loops_dups":
        assert np.count_nonzero(rows[list(order).index(1)] == 1) == 2               # the loop (1, 1) lists node 1 twice
        assert np.count_nonzero(rows[list(order).index(1)] == 0) == 2               # (0, 1) and (1, 0): a duplicate, kept
    if name == "isolated":
        assert deg[list(order).index(4)] == 0


def test_stream_refuses_a_non_permutation():
    from rlsolver_amd.graph import build_csr
    from rlsolver_amd.methods.MCPG import build_cheeger_stream
    csr = build_csr((np.array([0, 1]), np.array([1, 2]), np.array([1, 1])), num_nodes=3, keep_loops=True)
    with pytest.raises(ValueError):
        build_cheeger_stream(csr, np.array([0, 1, 1]))
    with pytest.raises(ValueError):
        build_cheeger_stream(csr, np.array([0, 1]))


def test_limits():
    import ctypes as C
    from rlsolver_amd import _abi
    lib, mx = _abi.lib(), C.c_int64(0)
    assert lib.rls_cheeger_local_search_supported(1, 0, 0, C.byref(mx)) == 1
    N = int(mx.value)
    assert N == mc().supported_limit() == 160 * 1024 // 8
    assert lib.rls_cheeger_local_search_supported(N, 0, 0, None) == 1 and lib.rls_cheeger_local_search_supported(N + 1, 0, 0, None) == 0
    assert lib.rls_cheeger_local_search_supported(0, 0, 0, None) == 0
    E = 1000
    assert lib.rls_cheeger_local_search_supported(10, E, (1 << 24) - 2 * E - 1, None) == 1
    assert lib.rls_cheeger_local_search_supported(10, E, (1 << 24) - 2 * E, None) == 0
    with pytest.raises(ValueError, match="20480"):          # refused by name before anything touches a device
        mc().make_data(N + 1, np.array([0]), np.array([1]), np.array([1]), "cpu")
    with pytest.raises(ValueError, match="2\\^24"):
        mc().make_data(4, np.array([0]), np.array([1]), np.array([1 << 24]), "cpu")


def test_oracle_keeps_inf_and_nan_rules():
    # an all-0 and an all-1 chain: 0 / 0 before any visit, and the first visit always flips (n >= 2)
    n, eu, ev, w = 4, np.array([0, 1, 2]), np.array([1, 2, 3]), np.array([1, 1, 1])
    x = np.array([[0, 1], [0, 1], [0, 1], [0, 1]])
    for nrm in (False, True):
        _, h0, _, _ = orc.local_search(n, eu, ev, w, np.arange(n), x, 0, nrm)
        assert np.isnan(h0).all()
        xs, h1, cut, size = orc.local_search(n, eu, ev, w, np.arange(n), x, 1, nrm)
        assert not np.isnan(h1).any() and (size > 0).all() and (size < n).all()
    # signed weights: a negative cut on an empty side gives -inf, and -inf < nh keeps it through the sweep
    w = np.array([-2, 0, 0])
    _, h, _, _ = orc.local_search(n, eu, ev, w, np.arange(n), x[:, :1], 2, False)
    assert np.isneginf(h).all()
