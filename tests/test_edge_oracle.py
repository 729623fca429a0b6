"""Edge-flip MaxCut family, host side (no GPU): the numpy oracle against the fixture recorded from the reference, the loader's
tables and edge order, the visit-stream builder against a direct recount, the kernel's integer path emulated on random graphs,
the production draws restated, the limits."""
import ctypes as C

import numpy as np
import pytest

import edge_oracle as orc
from oracle import oracle_np as onp

CASES = orc.fixture_cases()
GRAPHS = [orc.fixture_graph(g) for g in orc.fixture()["names"].tolist()]


def me():
    from rlsolver_amd.methods import MCPG_maxcut_edge
    return MCPG_maxcut_edge


def test_fixture_covers_the_recipe():
    names = {c["case"] for c in CASES}
    assert len(names) == len(CASES)
    for g, cfgs in (("BA_5_ID0", ("5x3", "64x2")), ("PL_20_ID0", ("5x3",)), ("BA_100_ID0", ("5x3",)), ("gset_14_stub", ("5x3", "64x2")),
                    ("signed_12", ("5x3", "64x2")), ("one_edge", ("5x3", "64x2"))):
        for cfg in cfgs:
            for ls in (1, 2):
                assert f"{g}/{cfg}/ls{ls}" in names
    s = orc.fixture_graph("signed_12")
    n, eu, ev, w = orc.parse_text(s["text"])
    assert n == s["n"] and np.array_equal(eu, s["eu"]) and np.array_equal(ev, s["ev"]) and np.array_equal(w, s["w"])
    pairs = list(zip(eu.tolist(), ev.tolist(), w.tolist()))
    assert any(a == c and b == d and x != y for i, (a, b, x) in enumerate(pairs) for (c, d, y) in pairs[i + 1:])     # parallel, other weight
    assert any(a == d and b == c and a != b for i, (a, b, _) in enumerate(pairs) for (c, d, _) in pairs[i + 1:])    # reversed duplicate
    assert (w < 0).any() and (w > 0).any() and (eu == ev).any()                                                       # signed, a loop
    assert np.setdiff1d(np.arange(n), np.concatenate([eu, ev])).size >= 1                                             # an isolated node
    one = orc.fixture_graph("one_edge")
    assert one["n"] == 2 and one["eu"].tolist() == [0] and one["ev"].tolist() == [1]
    for c in CASES:                                       # the mean of `expected` is exact in any order
        assert c["M"] * c["R"] * int(np.abs(c["w"]).sum()) < 2 ** 24


@pytest.mark.parametrize("c", CASES, ids=[c["case"] for c in CASES])
def test_oracle_equals_fixture(c):
    raw, _ = onp.metro_sampling(c["probs"], c["start"], c["change_times"], c["index"], c["u"])
    assert np.array_equal(raw.astype(np.uint8), c["raw"])
    v, expected = orc.sweep(c["n"], c["eu"], c["ev"], c["w"], c["order_edges"], c["add"], c["raw"], int(c["order_nodes"][0]), c["num_ls"],
                            c["uniforms"])
    res, best, value = orc.returns(v, expected, c["M"], c["edge_weight_sum"])
    assert orc.same_bits(res, c["res"])
    assert orc.same_bits(best, c["best"])
    assert orc.same_bits(value, c["value"])
    iso = np.setdiff1d(np.arange(c["n"]), np.concatenate([c["eu"], c["ev"]]))
    assert np.isin(c["best"][iso], (-0.5, 1.5)).all()     # a node no edge touches keeps the unwritten value
    rest = np.setdiff1d(np.arange(c["n"]), iso)
    assert np.isin(c["best"][rest], (0.0, 1.0)).all()


@pytest.mark.parametrize("g", GRAPHS, ids=[g["name"] for g in GRAPHS])
def test_loader_tables_equal_the_reference(g):
    add, order, key, max_a, wsum = me().edge_tables(g["n"], g["eu"], g["ev"], g["w"])
    assert add.dtype == np.float32 and orc.same_bits(add, g["add"])
    o_add, o_key, _, adeg = orc.loader(g["n"], g["eu"], g["ev"], g["w"])
    assert orc.same_bits(o_add, g["add"]) and np.array_equal(key, o_key)
    assert max_a == int(adeg.max()) and wsum == int(np.abs(g["w"]).sum())
    assert np.array_equal(order, orc.stable_order(key))
    assert (np.diff(key[order]) <= 0).all()                                 # non-increasing in the key
    assert (np.diff(key[g["order_edges"]]) <= 0).all()                      # and so is the recorded (unstable) one
    distinct = np.isin(key, [k for k, cnt in zip(*np.unique(key, return_counts=True)) if cnt == 1])
    pos_here, pos_ref = np.argsort(order), np.argsort(g["order_edges"])
    assert np.array_equal(pos_here[distinct], pos_ref[distinct])            # an edge whose key is unique sits where the reference put it
    _, given, _, _, _ = me().edge_tables(g["n"], g["eu"], g["ev"], g["w"], g["order_edges"])
    assert np.array_equal(given, g["order_edges"])                          # a caller's order is kept


def stream_cases():
    rng = np.random.RandomState(11)
    out = [("path_from_far_end", 5, np.array([0, 1, 2, 3]), np.array([1, 2, 3, 4]), np.array([1, 1, 1, 1]), np.array([3, 2, 1, 0])),
           ("parallel", 3, np.array([0, 1, 0, 1]), np.array([1, 0, 1, 2]), np.array([5, -2, 3, 1]), np.array([2, 0, 1, 3])),
           ("loops", 4, np.array([0, 1, 1, 2, 3]), np.array([0, 1, 2, 2, 0]), np.array([2, -1, 3, 1, 1]), np.array([4, 3, 2, 1, 0])),
           ("one_edge", 2, np.array([0]), np.array([1]), np.array([1]), np.array([0]))]
    for k in range(4):
        n, E = int(rng.randint(3, 30)), int(rng.randint(1, 80))
        eu, ev, w = orc.random_graph(rng, n, E, 5, hub=bool(k & 1))
        out.append((f"random{k}", n, eu, ev, w, rng.permutation(E)))
    g = orc.fixture_graph("signed_12")
    out.append(("signed_12", g["n"], g["eu"], g["ev"], g["w"], g["order_edges"]))
    return out


@pytest.mark.parametrize("name,n,eu,ev,w,order", stream_cases(), ids=[c[0] for c in stream_cases()])
def test_stream_against_a_direct_recount(name, n, eu, ev, w, order):
    from rlsolver_amd.methods.MCPG import build_edge_stream
    add, _, _, _, _ = me().edge_tables(n, eu, ev, w)
    stream = build_edge_stream(n, eu, ev, w, order, add)
    E = eu.shape[0]
    assert stream.dtype == np.int32 and stream.shape[0] == me().stream_words(n, eu, ev)
    recs = orc.decode_stream(stream, E)
    rows = orc.neighbor_rows(n, eu, ev, w)
    first = {}
    for i, e in enumerate(order.tolist()):
        first.setdefault(int(eu[e]), i)
        first.setdefault(int(ev[e]), i)
    for i, (e, (r, c, a3, row_r, row_c)) in enumerate(zip(order.tolist(), recs)):
        assert (r, c) == (int(eu[e]), int(ev[e])) and orc.same_bits(a3, add[:, e])
        for node, other, (nb, fr, wt) in ((r, c, row_r), (c, r, row_c)):
            want, k = orc.row_less_first(rows[node], other)
            assert nb.shape[0] == len(rows[node]) - 1                       # len_r, len_c
            assert nb.tolist() == [v for v, _ in want] and wt.tolist() == [x for _, x in want]   # the removed entry and its weight
            assert rows[node][k][0] == other and all(v != other for v, _ in rows[node][:k])
            assert fr.tolist() == [int(first[v] >= i) for v, _ in want]     # fresh = not an endpoint of an earlier position
    if name == "parallel":
        # position 0 visits edge 2 = (0, 1, w 3): what leaves row(0) is its FIRST entry 1, edge 0's weight 5 -- not the visited edge's 3
        r, c, _, row_r, row_c = recs[0]
        assert (r, c) == (0, 1) and row_r[2].tolist() == [-2, 3] and row_c[2].tolist() == [-2, 3, 1]
    if name == "path_from_far_end":
        assert recs[0][3][1].tolist() == [1] and recs[0][4][1].tolist() == []      # edge (3, 4) first: neighbour 2 still fresh
        assert recs[1][4][1].tolist() == [0]                                       # edge (2, 3): neighbour 4 of node 3 written by now


def test_stream_refuses_bad_arguments():
    from rlsolver_amd.methods.MCPG import build_edge_stream
    eu, ev, w = np.array([0, 1]), np.array([1, 2]), np.array([1, 1])
    add = np.zeros((3, 2), np.float32)
    with pytest.raises(ValueError, match="permutation"):
        build_edge_stream(3, eu, ev, w, np.array([0, 0]), add)
    with pytest.raises(ValueError, match="permutation"):
        build_edge_stream(3, eu, ev, w, np.array([0]), add)
    with pytest.raises(ValueError, match="add"):
        build_edge_stream(3, eu, ev, w, np.array([0, 1]), add[:2])


def test_integer_path_equals_the_oracle_on_random_graphs():
    """The kernel's arithmetic (integer 2 t from the stream, fresh flags in pass 0 only, bits + written mask) against the float32
    oracle: 300 random multigraphs with signed weights up to the exactness limit, hubs, loops and parallel edges."""
    from rlsolver_amd.methods.MCPG import build_edge_stream
    rng = np.random.RandomState(2024)
    for k in range(300):
        n, E, Cc = int(rng.randint(2, 14)), int(rng.randint(1, 30)), 6
        big = k % 5 == 0
        eu, ev, w = orc.random_graph(rng, n, E, 4, loops=True, hub=bool(k % 3 == 0))
        if big:                                            # one hub whose |weighted degree| sits just under 2^24 / 3
            ev[0] = (eu[0] + 1) % n                        # (not a loop: a loop counts twice at its node)
            w[0] = ((2 ** 24 - 1) // 3 - 2 * int(np.abs(w).sum()) - 1) * rng.choice([-1, 1])
        add, order, _, max_a, wsum = me().edge_tables(n, eu, ev, w)
        assert 3 * max_a < 2 ** 24 and wsum < 2 ** 24
        order = order if k % 2 else rng.permutation(E)
        stream = build_edge_stream(n, eu, ev, w, order, add)
        raw = rng.randint(0, 2, (n, Cc)).astype(np.uint8)
        num_ls = int(rng.randint(1, 4))
        uni = rng.rand(num_ls, E, 3, Cc).astype(np.float32)
        uni[rng.rand(*uni.shape) < 0.2] = 0.0              # ties between the four rows
        hub = int(rng.randint(-1, n))
        v, expected = orc.sweep(n, eu, ev, w, order, add, raw, hub, num_ls, uni)
        x, written = orc.emulate_kernel(n, stream, E, raw, hub, num_ls, uni)
        assert orc.same_bits(orc.as_float_output(x, written), v), k
        assert np.array_equal(orc.score(eu, ev, w, x), expected)
        assert np.array_equal(written, np.isin(np.arange(n), np.concatenate([eu, ev])))


def test_production_draws_restated():
    u = orc.production_uniforms(7, np.arange(4), 2, 3)
    assert u.shape == (2, 3, 3, 4) and u.dtype == np.float32
    assert ((u >= 0) & (u < 1)).all()
    assert (u * 16777216.0 == np.round(u * 16777216.0)).all()               # 24 bits
    # known values: murmur3's finaliser on its published vectors, and draw (pass 0, position 0, which 0) of chain 0 by hand
    assert int(orc.fmix32(0)) == 0 and int(orc.fmix32(1)) == 0x514E28B7 and int(orc.fmix32(0xFFFFFFFF)) == 0x81F16F39
    ck = int(orc.fmix32(7 ^ int(orc.fmix32(0 ^ int(orc.fmix32(0))))))
    k = ck ^ 0 ^ 0x165667B1
    assert u[0, 0, 0, 0] == np.float32((int(orc.fmix32((k + 0x27D4EB2F) & 0xFFFFFFFF)) >> 8) / 16777216.0)
    big = orc.production_uniforms(123456789012345, np.arange(200) + (1 << 33), 2, 20)
    assert ((big >= 0) & (big < 1)).all()
    assert (big[:, :, 0] != big[:, :, 1]).all() and (big[:, :, 1] != big[:, :, 2]).all() and (big[:, :, 0] != big[:, :, 2]).all()
    assert abs(float(big.mean()) - 0.5) < 0.01
    assert not np.array_equal(orc.production_uniforms(8, np.arange(4), 2, 3), u)
    assert np.array_equal(orc.production_uniforms(7, np.arange(2, 4), 2, 3), u[..., 2:])     # keyed by the global id


def test_limits():
    from rlsolver_amd import _abi
    lib, mx = _abi.lib(), C.c_int64(0)
    sup = lib.rls_maxcut_edge_local_search_supported
    assert sup(1, 0, 0, 0, 0, C.byref(mx)) == 1
    N = int(mx.value)
    lds = lambda n: ((8 * n + 15) & ~15) + 4 * ((n + 31) // 32)             # noqa: E731  the tile and the written-node bitmap
    assert N == me().supported_limit() == 20164 and lds(N) <= 160 * 1024 < lds(N + 1)
    assert sup(N, 0, 0, 0, 0, None) == 1 and sup(N + 1, 0, 0, 0, 0, None) == 0 and sup(0, 0, 0, 0, 0, None) == 0
    top = (1 << 24) - 1
    assert sup(10, 5, top // 3, 0, 0, None) == 1 and sup(10, 5, top // 3 + 1, 0, 0, None) == 0           # 3 max A_v < 2^24
    assert sup(10, 5, 0, top, 0, None) == 1 and sup(10, 5, 0, top + 1, 0, None) == 0                       # sum |w| < 2^24
    assert sup(10, 5, 0, 0, (1 << 31) - 1, None) == 1 and sup(10, 5, 0, 0, 1 << 31, None) == 0             # stream_len < 2^31
    assert sup(10, -1, 0, 0, 0, None) == 0 and sup(10, 0, -1, 0, 0, None) == 0 and sup(10, 0, 0, -1, 0, None) == 0
    with pytest.raises(ValueError, match="20164"):          # refused by name before anything touches a device
        me().make_data(N + 1, np.array([0]), np.array([1]), np.array([1]), "cpu")
    with pytest.raises(ValueError, match="2\\^24"):
        me().make_data(4, np.array([0]), np.array([1]), np.array([1 << 23]), "cpu")
    with pytest.raises(ValueError, match="integer"):
        me().make_data(4, np.array([0]), np.array([1]), np.array([0.5]), "cpu")
