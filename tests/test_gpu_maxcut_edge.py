"""Edge-flip MaxCut family on the GPU: the gauge + sweep + score kernel, the reference-shaped sampler, the packed sampler, MCPGRound
(whole and in two shards) and run_mcpg against the numpy oracle (tests/edge_oracle.py) and the fixture recorded from the
reference.  Every comparison is exact, bit for bit."""
import importlib.util
import os

import numpy as np
import pytest
import torch

import edge_oracle as orc

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
F = np.float32


def dev():
    return torch.device("cuda:0")


def me():
    from rlsolver_amd.methods import MCPG_maxcut_edge
    return MCPG_maxcut_edge


def packed():
    from rlsolver_amd.ops_mcpg_tsp import PackedChains
    return PackedChains


def t(a, dt=torch.float32):
    return torch.from_numpy(np.array(a, order="C")).to(dev(), dt)        # (a copy: the shared oracle arrays are read-only)


# ---------------------------------------------------------------------------------------------------------------- cases
def graph_case(name):
    """(n, eu, ev, w, node order, edge order or None = the loader's) of the named graph."""
    rng = np.random.RandomState(sum(map(ord, name)))
    order_e = None
    if name == "n2_edge":
        n, eu, ev, w = 2, [0], [1], [1]
    elif name == "path_far_end":                          # visited from its far end: a neighbour is still fresh at a visit
        n, eu, ev, w = 7, list(range(6)), list(range(1, 7)), [1] * 6
        order_e = np.arange(5, -1, -1)
    elif name == "parallel":                              # the removed entry's weight is not the visited edge's
        n, eu, ev, w = 4, [0, 1, 0, 1, 2], [1, 0, 1, 2, 3], [5, -2, 3, 1, 2]
        order_e = np.array([2, 0, 1, 3, 4])
    elif name == "loops_isolated":                        # loops (one at an otherwise bare node), duplicates, nodes 7 and 9 bare
        n, eu, ev, w = 10, [0, 1, 1, 2, 3, 3, 4, 1, 5, 5, 8], [1, 1, 2, 1, 3, 4, 3, 0, 6, 6, 8], [1, 2, -1, 3, 1, -2, 1, 1, 2, 2, -3]
    elif name == "star70":
        n, eu, ev, w = 71, [0] * 70, list(range(1, 71)), rng.choice([-2, -1, 1, 3], 70).tolist()
    elif name == "signed30":
        n = 30
        eu, ev = rng.randint(0, n, 90).tolist(), rng.randint(0, n, 90).tolist()
        w = rng.choice([-3, -2, -1, 1, 2], 90).tolist()
    else:
        raise KeyError(name)
    eu, ev, w = (np.asarray(a, dtype=np.int64) for a in (eu, ev, w))
    return n, eu, ev, w, rng.permutation(n), order_e


NAMED = ["n2_edge", "path_far_end", "parallel", "loops_isolated", "star70", "signed30"]
FIXED = [g for g in orc.fixture()["names"].tolist()]
_DATA = {}


def data_of(name):
    """The data object of a named or a fixture graph, built once: (data, (n, eu, ev, w, add, node order, edge order))."""
    if name not in _DATA:
        if name in NAMED:
            n, eu, ev, w, order_n, order_e = graph_case(name)
        else:
            g = orc.fixture_graph(name)
            n, eu, ev, w, order_n, order_e = g["n"], g["eu"], g["ev"], g["w"], g["order_nodes"], g["order_edges"]
        data = me().make_data(n, eu, ev, w, dev(), sorted_degree_nodes=order_n, sorted_degree_edges=order_e)
        add, _, _, _ = orc.loader(n, eu, ev, w)
        assert orc.same_bits(data.add.cpu().numpy(), add)
        _DATA[name] = (data, (n, eu, ev, w, add, np.asarray(order_n), data.sorted_degree_edges.numpy().copy()))
    return _DATA[name]


def start_chains(n, c, seed):
    """Chains drawn at p = 0.05 / 0.5 / 0.95 by column, with an all-0 and an all-1 chain planted in columns 0 and 1."""
    rng = np.random.RandomState(seed)
    x = (rng.rand(n, c) < np.asarray([0.05, 0.5, 0.95])[np.arange(c) % 3][None, :]).astype(F)
    for col in range(min(c, 2)):
        x[:, col] = float(col)
    return x


def draws(num_ls, E, c, seed):
    """Uniforms with a fifth of them 0: ties between the four rows are frequent."""
    rng = np.random.RandomState(1000 + seed)
    u = rng.rand(num_ls, E, 3, c).astype(F)
    u[rng.rand(*u.shape) < 0.2] = 0.0
    return u


_WANT = {}


def oracle_of(name, C, c_in, num_ls, seed, gauge):
    """(start, uniforms, v f32 [n, C], expected) of a configuration, computed once and shared."""
    key = (name, C, c_in, num_ls, seed, gauge)
    if key not in _WANT:
        _, (n, eu, ev, w, add, order_n, order_e) = data_of(name)
        start = start_chains(n, c_in, seed)
        uni = draws(num_ls, eu.shape[0], C, seed)
        v, expected = orc.sweep(n, eu, ev, w, order_e, add, start[:, np.arange(C) % c_in], int(order_n[0]) if gauge else -1, num_ls, uni)
        for a in (start, uni, v, expected):
            a.setflags(write=False)
        _WANT[key] = (start, uni, v, expected)
    return _WANT[key]


def check_kernel(name, C, num_ls, c_in=None, form="packed", seed=0, gauge=True):
    """Gauge + sweep + score of `C` chains (started from `c_in` of them, broadcast) in one output form: chains and expected equal
    the oracle's; the bits of chains past C are zero.  Returns the kernel's outputs."""
    data, (n, eu, ev, w, add, order_n, order_e) = data_of(name)
    c_in = C if c_in is None else c_in
    start, uni, want_v, want_e = oracle_of(name, C, c_in, num_ls, seed, gauge)
    xin = packed().pack(t(start))
    out = {"packed": packed().empty(n, C, dev()), "inplace": xin, "f32": None}[form]
    if form == "packed":
        out.words.fill_(-1)
    xs, expected = data.local_search(xin, num_ls, t(uni), out=out, num_chains=C, gauge=gauge)
    assert form != "inplace" or xs is xin
    tag = (name, C, num_ls, form, gauge)
    if form == "f32":
        assert xs.shape == (n, C) and orc.same_bits(xs.cpu().numpy(), want_v), tag             # -0.5 | 1.5 where never written
    else:
        assert np.array_equal(xs.unpack().cpu().numpy(), (want_v > 0.25).astype(F)), tag       # a bit-packed result holds the bit
        if C % 64:
            last = xs.words[-1].cpu().numpy().view(np.uint64)
            assert not (last >> np.uint64(C % 64)).any()
    assert expected.dtype == torch.float32 and expected.shape == (C,) and orc.same_bits(expected.cpu().numpy(), want_e), tag
    return xs, expected


# ---------------------------------------------------------------------------------------------------------------- kernel
@pytest.mark.parametrize("name", NAMED + FIXED)
def test_kernel_equals_oracle(name):
    for num_ls in (0, 1, 2, 3):
        a = check_kernel(name, 70, num_ls, form="packed", seed=num_ls)
        b = check_kernel(name, 70, num_ls, form="inplace", seed=num_ls)
        c = check_kernel(name, 70, num_ls, form="f32", seed=num_ls)
        assert torch.equal(a[0].words, b[0].words) and torch.equal(a[0].unpack(), (c[0] > 0.25).float())
        assert torch.equal(a[1], b[1]) and torch.equal(a[1], c[1])


def test_tie_takes_the_first_maximum():
    """One edge, N = 2, w = 1, every uniform 0: add = (-0.5 + 1 - 0.05, the same, 1.05), the empty rows give t = 0, so the four
    rows are (0.45 + 0.45 - 1.05, 0.45, 0.45, 0) = (-0.15, 0.45, 0.45, 0) and the first maximum is k = 1: (r, c) = (0, 1)."""
    data, (n, eu, ev, w, add, _, _) = data_of("n2_edge")
    a, b = F(add[0, 0]), F(add[1, 0])
    z = F(F(a + b) - add[2, 0])
    assert a == b and abs(float(a) - 0.45) < 1e-6 and abs(float(z) + 0.15) < 1e-6 and z < 0 < a     # (z, a, b, 0): a and b tie, a first
    for start in (np.zeros((2, 64), F), np.ones((2, 64), F), start_chains(2, 64, 3)):
        xs, expected = data.local_search(packed().pack(t(start)), 1, torch.zeros((1, 1, 3, 64), device=dev()))
        assert bool((xs[0] == 0).all()) and bool((xs[1] == 1).all()) and bool((expected == -1).all())


def test_fresh_rule():
    # a path visited from its far end: at position 0 the neighbour 4 of node 5 has not been written; the stream says so
    data, (n, eu, ev, w, add, order_n, order_e) = data_of("path_far_end")
    recs = orc.decode_stream(data.stream().cpu().numpy(), eu.shape[0])
    assert recs[0][:2] == (5, 6) and recs[0][3][1].tolist() == [1] and all(r[3][1].tolist() == [1] for r in recs[:-1])
    assert recs[-1][3][0].size == 0                       # node 0 has no other neighbour
    check_kernel("path_far_end", 64, 1, seed=21)
    # a second pass reads no fresh entry: two passes equal one pass followed by one pass on a stream whose flags are all clear
    start, uni, want_v, want_e = oracle_of("path_far_end", 64, 64, 2, 22, False)
    one, _ = data.local_search(packed().pack(t(start)), 1, t(uni[:1]), out=packed().empty(n, 64, dev()), gauge=False)
    from rlsolver_amd import ops_mcpg_tsp as mops
    clear = data.stream().cpu().numpy().copy()
    p = 0
    for _ in range(eu.shape[0]):
        k = int(clear[p + 2] + clear[p + 3])
        clear[p + 7:p + 7 + 2 * k:2] &= 0x7fffffff
        p += 7 + 2 * k
    two, e2 = mops.mcpg_maxcut_edge_local_search(data.graph, data._edge_w, one, t(clear, torch.int32), data.max_abs_degree, data.weight_abs_sum,
                                                 1, -1, t(uni[1:]), out=packed().empty(n, 64, dev()))
    assert np.array_equal(two.unpack().cpu().numpy(), (want_v > 0.25).astype(F)) and orc.same_bits(e2.cpu().numpy(), want_e)
    # an isolated node in float32 output keeps -0.5 | 1.5, a bit-packed one its gauge-fixed bit
    xs, _ = check_kernel("loops_isolated", 65, 2, form="f32", seed=23)
    got = xs.cpu().numpy()
    assert np.isin(got[[7, 9]], (-0.5, 1.5)).all() and np.isin(np.delete(got, [7, 9], axis=0), (0.0, 1.0)).all()
    assert (got[[7, 9]] == -0.5).any() and (got[[7, 9]] == 1.5).any()


def test_parallel_edges_remove_the_first_entry():
    data, (n, eu, ev, w, add, order_n, order_e) = data_of("parallel")
    recs = orc.decode_stream(data.stream().cpu().numpy(), eu.shape[0])
    assert recs[0][:2] == (0, 1) and recs[0][3][2].tolist() == [-2, 3]       # edge (0, 1, 3) visited: weight 5 left the row, 3 stayed
    for num_ls in (1, 2):
        check_kernel("parallel", 128, num_ls, seed=30 + num_ls)


@pytest.mark.parametrize("C", [1, 63, 64, 65, 129])
def test_chain_counts(C):
    for form in ("packed", "f32"):
        check_kernel("loops_isolated", C, 2, form=form, seed=C)
        check_kernel("signed30", C, 1, form=form, seed=C)


def test_outputs_past_C_are_not_written():
    data, (n, eu, ev, w, add, order_n, order_e) = data_of("signed30")
    op = torch.ops.rlsolver_hip.maxcut_edge_local_search
    for C in (1, 63, 65, 129):
        start, uni, want_v, want_e = oracle_of("signed30", C, C, 2, C, True)
        xin = packed().pack(t(start))
        tiles = (C + 63) // 64
        big_e = torch.full((C + 64,), -7.0, device=dev())
        big_w = torch.full((tiles + 1, n), 0x5A5A5A5A5A5A5A5A, dtype=torch.int64, device=dev())
        op(data.graph.handle, data._edge_w, xin.words, C, big_w[:tiles], C, data.stream(), data.max_abs_degree, data.weight_abs_sum,
           int(order_n[0]), 2, t(uni), 0, big_e[:C])
        assert orc.same_bits(big_e[:C].cpu().numpy(), want_e) and bool((big_e[C:] == -7.0).all())
        assert np.array_equal(packed()(big_w[:tiles], C).unpack().cpu().numpy(), (want_v > 0.25).astype(F))
        assert bool((big_w[tiles] == 0x5A5A5A5A5A5A5A5A).all())
        big_f = torch.full((n + 1, C), -7.0, device=dev())                      # float32 [N, C]: one canary row behind
        op(data.graph.handle, data._edge_w, xin.words, C, big_f[:n], C, data.stream(), data.max_abs_degree, data.weight_abs_sum,
           int(order_n[0]), 2, t(uni), 0, big_e[:C])
        assert orc.same_bits(big_f[:n].cpu().numpy(), want_v) and bool((big_f[n] == -7.0).all())


def test_broadcast_start():
    check_kernel("signed30", 192, 2, c_in=64, seed=4)
    check_kernel("loops_isolated", 192, 1, c_in=64, form="f32", seed=5)
    check_kernel("star70", 256, 2, c_in=128, seed=6)


def test_without_gauge():
    for name in ("signed30", "loops_isolated"):
        a, _ = check_kernel(name, 70, 2, seed=8, gauge=False)
        b, _ = check_kernel(name, 70, 2, seed=8, gauge=True)
        assert not torch.equal(a.words, b.words)


def test_two_edge_orders():
    data, (n, eu, ev, w, add, order_n, order_e) = data_of("signed30")
    other = np.random.RandomState(77).permutation(eu.shape[0])
    start, uni = start_chains(n, 64, 3), draws(1, eu.shape[0], 64, 3)
    got = []
    try:
        for o in (order_e, other):
            data.sorted_degree_edges = torch.from_numpy(o)                   # replaced: the stream is rebuilt
            xs, expected = data.local_search(packed().pack(t(start)), 1, t(uni))
            want_v, want_e = orc.sweep(n, eu, ev, w, o, add, start, int(order_n[0]), 1, uni)
            recs = orc.decode_stream(data.stream().cpu().numpy(), eu.shape[0])
            assert [(r[0], r[1]) for r in recs] == [(int(eu[e]), int(ev[e])) for e in o]
            assert orc.same_bits(xs.cpu().numpy(), want_v) and orc.same_bits(expected.cpu().numpy(), want_e)
            got.append(xs)
    finally:
        data.sorted_degree_edges = torch.from_numpy(order_e)
    assert not torch.equal(got[0], got[1])


def test_expected_is_a_recount():
    for name in ("signed30", "star70", "BA_100_ID0"):
        data, (n, eu, ev, w, *_r) = data_of(name)
        xs, expected = check_kernel(name, 129, 2, form="f32", seed=6)
        s = 2 * (xs > 0.25).double() - 1
        again = (t(w, torch.float64)[:, None] * s[t(eu, torch.int64)] * s[t(ev, torch.int64)]).sum(dim=0)
        assert torch.equal(expected.double(), again)


def test_largest_supported_num_nodes():
    from rlsolver_amd import ops_mcpg_tsp as mops
    from rlsolver_amd.methods import MCPG_maxcut
    nmax = me().supported_limit()
    eu = np.array([nmax - 1, nmax - 2, nmax - 1, 0, nmax - 3, nmax - 1])
    ev = np.array([nmax - 2, nmax - 3, 0, 1, nmax - 1, nmax - 1])
    w = np.array([2, -1, 3, 1, 1, -2])
    data = me().make_data(nmax, eu, ev, w, dev())
    add, _, _, _ = orc.loader(nmax, eu, ev, w)
    start = (np.random.RandomState(2).rand(nmax, 64) < 0.5).astype(F)
    uni = draws(1, 6, 64, 2)
    hub = data.hub()
    want_v, want_e = orc.sweep(nmax, eu, ev, w, data.sorted_degree_edges.numpy(), add, start, hub, 1, uni)
    xs, expected = data.local_search(packed().pack(t(start)), 1, t(uni))
    assert orc.same_bits(xs.cpu().numpy(), want_v) and orc.same_bits(expected.cpu().numpy(), want_e)
    with pytest.raises(ValueError, match=f"{nmax}"):                         # the Python layer names the limit
        me().make_data(nmax + 1, eu, ev, w, dev())
    big = MCPG_maxcut.make_data(nmax + 1, eu, ev, w, dev())
    x = packed().empty(nmax + 1, 64, dev())
    with pytest.raises(RuntimeError, match=f"\\(-2\\).*{nmax}"):              # RLS_EUNSUPPORTED from the entry point itself
        mops.mcpg_maxcut_edge_local_search(big.graph, big._edge_w, x, data.stream(), 6, 10, 0, out=x)


def test_weight_sum_at_the_exactness_limit():
    """3 max |weighted degree| = 2^24 - 1 - (2^24 - 1) % 3 < 2^24: the largest the kernel takes; 2 t reaches +-(2^24 - 4) and the
    score +-(2^24 - 1) / 3 and more, all exact."""
    from rlsolver_amd import ops_mcpg_tsp as mops
    top = ((1 << 24) - 1) // 3
    n = 6
    eu, ev = np.array([0, 0, 0, 1, 2, 0]), np.array([1, 2, 3, 2, 3, 4])
    w = np.array([top - 7, 3, -2, 1, 1, 2])                 # node 0: the sum of |w| is top
    data = me().make_data(n, eu, ev, w, dev())
    assert data.max_abs_degree == top and 3 * top < 1 << 24
    add, _, _, _ = orc.loader(n, eu, ev, w)
    start, uni = start_chains(n, 64, 9), draws(2, 6, 64, 9)
    want_v, want_e = orc.sweep(n, eu, ev, w, data.sorted_degree_edges.numpy(), add, start, data.hub(), 2, uni)
    xs, expected = data.local_search(packed().pack(t(start)), 2, t(uni))
    assert orc.same_bits(xs.cpu().numpy(), want_v) and orc.same_bits(expected.cpu().numpy(), want_e)
    assert np.abs(want_e).max() > top - 20
    with pytest.raises(ValueError, match="2\\^24"):
        me().make_data(n, eu, ev, w + np.array([1, 0, 0, 0, 0, 0]), dev())
    x = packed().pack(t(start))
    with pytest.raises(RuntimeError, match="\\(-2\\).*2\\^24"):
        mops.mcpg_maxcut_edge_local_search(data.graph, data._edge_w, x, data.stream(), top + 1, data.weight_abs_sum, 1)
    with pytest.raises(RuntimeError, match="\\(-2\\).*2\\^24"):
        mops.mcpg_maxcut_edge_local_search(data.graph, data._edge_w, x, data.stream(), top, 1 << 24, 1)


# ------------------------------------------------------------------------------------------------------ production draws
def test_production_draws():
    data, (n, eu, ev, w, add, order_n, order_e) = data_of("signed30")
    E, C, hub = eu.shape[0], 128, int(order_n[0])
    start = start_chains(n, C, 41)
    seed = 0x1234567890ABCDEF
    xs, expected = data.local_search(packed().pack(t(start)), 2, None, seed)
    uni = orc.production_uniforms(seed, np.arange(C), 2, E)
    want_v, want_e = orc.sweep(n, eu, ev, w, order_e, add, start, hub, 2, uni)
    assert orc.same_bits(xs.cpu().numpy(), want_v) and orc.same_bits(expected.cpu().numpy(), want_e)
    # two half-batches with chain_ids offsets equal the whole
    halves = [data.local_search(packed().pack(t(start[:, lo:lo + 64])), 2, None, seed, chain_ids=(lo, 0, 0)) for lo in (0, 64)]
    assert torch.equal(torch.cat([h[0] for h in halves], dim=1), xs) and torch.equal(torch.cat([h[1] for h in halves]), expected)
    # ... and repeats of a kept shard: local chain c = repeat c // 64 of kept chain 64 + c % 64, the repeats 128 apart
    start4 = start_chains(n, 256, 42)
    whole, e_whole = data.local_search(packed().pack(t(start4)), 1, None, seed)
    part, e_part = data.local_search(packed().pack(t(start4[:, [64 + k for k in range(64)] + [192 + k for k in range(64)]])), 1, None, seed,
                                     chain_ids=(64, 64, 64))
    cols = torch.tensor([64 + k for k in range(64)] + [192 + k for k in range(64)], device=dev())
    assert torch.equal(part, whole[:, cols]) and torch.equal(e_part, e_whole[cols])
    other, e_other = data.local_search(packed().pack(t(start)), 2, None, seed + 1)
    assert not torch.equal(other, xs)


# -------------------------------------------------------------------------------------------------------------- samplers
CASES = orc.fixture_cases()


@pytest.mark.parametrize("gname", FIXED)
def test_sampler_against_the_reference_fixture(gname):
    """mcpg_sampling_maxcut_edge with the reference's recorded walk and draws, on the reference's own node and edge order: its four
    returns; the packed sampler on the same raw samples."""
    seen = 0
    data, _ = data_of(gname)
    for c in CASES:
        if not c["case"].startswith(gname + "/"):
            continue
        seen += 1
        uni = t(c["uniforms"][:c["num_ls"]])
        got = me().mcpg_sampling_maxcut_edge(data, t(c["start"]), t(c["probs"]), c["num_ls"], c["change_times"], c["M"],
                                             index=t(c["index"], torch.int64), u=t(c["u"]), uniforms=uni)
        want = (c["res"], c["best"], c["raw"].astype(F), c["value"])
        for g, wnt, what in zip(got, want, ("res", "best", "raw", "value")):
            assert g.dtype == torch.float32 and g.device.type == "cuda" and orc.same_bits(g.cpu().numpy(), wnt), (c["case"], what)
        best_val, best, value, xs = me().sampler_maxcut_edge_packed(data, packed().pack(got[2]), c["num_ls"], c["M"], c["R"], uniforms=uni,
                                                                    in_place=False)
        assert torch.equal(best_val, got[0]) and torch.equal(best.unpack(), (got[1] > 0.25).float())
        assert orc.same_bits(value.cpu().numpy(), c["value"])
    assert seen in (2, 4)


def test_sampler_num_ls_zero_runs_one_pass():
    """The reference tests num_ls after the loop body: num_ls = 0 is one pass."""
    c = next(c for c in CASES if c["case"] == "signed_12/5x3/ls1")
    data, _ = data_of("signed_12")
    got = me().mcpg_sampling_maxcut_edge(data, t(c["start"]), t(c["probs"]), 0, c["change_times"], c["M"], index=t(c["index"], torch.int64),
                                         u=t(c["u"]), uniforms=t(c["uniforms"][:1]))
    assert orc.same_bits(got[0].cpu().numpy(), c["res"]) and orc.same_bits(got[1].cpu().numpy(), c["best"])


def test_packed_sampler_in_place_and_result():
    data, (n, eu, ev, w, add, order_n, order_e) = data_of("BA_100_ID0")
    M, R = 64, 2
    start = start_chains(n, M * R, 12)
    x = packed().pack(t(start))
    res0 = data.result(x)
    assert orc.same_bits(res0.cpu().numpy(), ((F(w.sum()) - orc.score(eu, ev, w, start > 0.5)) / F(2)).astype(F))
    uni = draws(2, eu.shape[0], M * R, 12)
    v, expected = orc.sweep(n, eu, ev, w, order_e, add, start, int(order_n[0]), 2, uni)
    res, best, value = orc.returns(v, expected, M, float(w.sum()))
    best_val, best_x, val, xs = me().sampler_maxcut_edge_packed(data, x, 2, M, R, uniforms=t(uni))
    assert xs is x
    assert orc.same_bits(best_val.cpu().numpy(), res) and np.array_equal(best_x.unpack().cpu().numpy(), best)
    assert np.array_equal(xs.unpack().cpu().numpy(), v) and orc.same_bits(val.cpu().numpy(), value)


# ----------------------------------------------------------------------------------------------------- MCPGRound, run_mcpg
def replay_round(name, samples, num_ls, seed, gids, M, res, info):
    """One round restated: the oracle on the round's metro output with the restated production draws of its seed, best of
    repeats and the merge in numpy (oracle_np.mcpg_merge_best)."""
    from oracle import oracle_np as onp
    _, (n, eu, ev, w, add, order_n, order_e) = data_of(name)
    uni = orc.production_uniforms(seed, gids, num_ls, eu.shape[0])
    v, expected = orc.sweep(n, eu, ev, w, order_e, add, samples, int(order_n[0]), num_ls, uni)
    idx = orc.first_min(expected, M)
    cut = ((F(w.sum()) - expected[idx]) / F(2)).astype(F)
    res, info, temp, now_max, now_idx = onp.mcpg_merge_best(cut, v[:, idx].astype(np.uint8), res, info)
    return expected, res, info, temp, now_max, now_idx


def hooked(data, seeds, seen=None):
    hook = data.round_local_search

    def recording(samples, num_ls, seed, out, chain_ids):
        seeds.append(seed)
        if seen is not None:
            seen.append(samples.unpack().cpu().numpy())
        return hook(samples, num_ls, seed, out, chain_ids)

    data.round_local_search = recording


def test_mcpg_round_three_rounds():
    from rlsolver_amd.methods.MCPG import MCPGRound
    name = "BA_100_ID0"
    data, (n, eu, ev, w, *_r) = data_of(name)
    M, R = 64, 2
    rng = np.random.RandomState(31)
    xs0 = (rng.rand(n, M) < 0.5).astype(F)
    res = ((F(w.sum()) - orc.score(eu, ev, w, xs0 > 0.5)) / F(2)).astype(F)
    info = xs0.astype(np.uint8)
    vs0 = data.result(t(xs0))
    assert orc.same_bits(vs0.cpu().numpy(), res)
    assert data.num_edges == int(w.sum()) and data.num_graph_edges == eu.shape[0]
    rnd = MCPGRound(data, t(xs0), vs0, M, R, num_ls=2, seed=17)
    probs = torch.full((n,), 0.5, device=dev())
    seeds = []
    hooked(data, seeds)
    try:
        for k in range(3):
            value, best = rnd.step(probs)
            expected, res, info, temp, now_max, now_idx = replay_round(name, rnd.samples.unpack().cpu().numpy(), 2, seeds[k], np.arange(M * R),
                                                                       M, res, info)
            assert orc.same_bits(rnd.expected.cpu().numpy(), expected)
            assert orc.same_bits(value.cpu().numpy(), (t(expected) - t(expected).mean()).cpu().numpy())
            assert orc.same_bits(rnd.now_max_res.cpu().numpy(), res) and np.array_equal(rnd.now_max_info.unpack().cpu().numpy(), info)
            assert np.array_equal(rnd.start.unpack().cpu().numpy(), temp)
            assert float(best) == float(now_max)
            assert torch.isfinite(rnd.get_return(probs.clone().requires_grad_(True)))
    finally:
        del data.round_local_search
    v, x = rnd.best_solution()
    assert v == float(now_max) and np.array_equal(x.cpu().numpy().astype(np.uint8), info[:, now_idx])
    assert len(set(seeds)) == 3


def test_run_mcpg_two_rounds():
    from rlsolver_amd.methods.MCPG import run_mcpg
    name = "BA_100_ID0"
    data, (n, eu, ev, w, *_r) = data_of(name)
    M, R = 64, 2
    xs0 = (np.random.RandomState(32).rand(n, M) < 0.5).astype(F)
    seeds, seen = [], []
    hooked(data, seeds, seen)
    try:
        v, x, rates = run_mcpg(data, t(xs0), data.result(t(xs0)), M, R, 2, 2, sample_epoch_num=2, log=lambda *a: None, seed=3)
    finally:
        del data.round_local_search
    res = ((F(w.sum()) - orc.score(eu, ev, w, xs0 > 0.5)) / F(2)).astype(F)
    info = xs0.astype(np.uint8)
    assert len(seen) == 2 and len(rates) == 2
    for k, samples in enumerate(seen):
        assert samples.shape == (n, M * R)
        _, res, info, temp, now_max, now_idx = replay_round(name, samples, 2, seeds[k], np.arange(M * R), M, res, info)
    assert v == float(now_max) and np.array_equal(x.cpu().numpy().astype(np.uint8), info[:, now_idx])


def test_two_shard_round_equals_the_whole():
    """M = 128 kept chains, two rounds: (a) the whole batch unsharded; (b) the whole batch in the sharded code path, its exchange
    recorded through stat_hook; (c) two shards (kept_offset 0 and M / 2) replaying that exchange.  Chains, expected, value,
    incumbents, start states and the best are (a)'s: every draw is keyed by the global chain id and the values are integers or
    half-integers."""
    from rlsolver_amd.methods.MCPG import MCPGRound
    from test_gpu_shard_invariance import StatTape
    name = "BA_100_ID0"
    data, (n, eu, ev, w, *_r) = data_of(name)
    M, R, rounds = 128, 2, 2
    xs0 = t((np.random.RandomState(33).rand(n, M) < 0.5).astype(F))
    vs0 = data.result(xs0)
    probs = torch.full((n,), 0.5, device=dev())

    def run(m0, Ml, hook, force_sharded=False):
        rnd = MCPGRound(data, xs0[:, m0:m0 + Ml].contiguous(), vs0[m0:m0 + Ml].clone(), Ml, R, 1, kept_offset=m0, total_kept=M, seed=5)
        rnd.stat_hook = hook
        if force_sharded:
            rnd.sharded = True
        log = []
        for _ in range(rounds):
            value, best = rnd.step(probs)
            log.append(dict(samples=rnd.samples.unpack(), expected=rnd.expected.clone(), value=value.clone(), best=best.clone(),
                            res=rnd.now_max_res.clone(), info=rnd.now_max_info.unpack(), start=rnd.start.unpack()))
        return log

    a = run(0, M, None)
    tape = StatTape()
    b = run(0, M, tape.recorder(), force_sharded=True)
    for ra, rb in zip(a, b):
        for k in ra:
            assert torch.equal(ra[k], rb[k]), k
    h = M // 2
    for m0 in (0, h):
        c = run(m0, h, tape.replayer())
        cols = torch.tensor([r * M + m0 + j for r in range(R) for j in range(h)], device=dev())
        for ra, rc in zip(a, c):
            assert torch.equal(rc["samples"], ra["samples"][:, cols]), "a shard's chains are not the whole batch's"
            assert torch.equal(rc["expected"], ra["expected"][cols]) and torch.equal(rc["value"], ra["value"][cols])
            assert torch.equal(rc["res"], ra["res"][m0:m0 + h]) and torch.equal(rc["info"], ra["info"][:, m0:m0 + h])
            assert torch.equal(rc["start"], ra["start"][:, m0:m0 + h]) and torch.equal(rc["best"], ra["best"])


# -------------------------------------------------------------------------------------------------------------------- op
def test_op_rejects_bad_arguments():
    from rlsolver_amd import ops_mcpg_tsp as mops
    data, (n, eu, *_rest) = data_of("loops_isolated")
    E = eu.shape[0]
    x = packed().empty(n, 64, dev())
    x.words.zero_()
    stream, ew, A, W = data.stream(), data._edge_w, data.max_abs_degree, data.weight_abs_sum
    call = mops.mcpg_maxcut_edge_local_search
    with pytest.raises(TypeError, match="PackedChains"):
        call(data.graph, ew, x.unpack(), stream, A, W, 1)
    with pytest.raises((ValueError, TypeError), match="visit_stream"):                       # dtype
        call(data.graph, ew, x, stream.long(), A, W, 1)
    with pytest.raises((ValueError, TypeError), match="visit_stream"):                       # device
        call(data.graph, ew, x, stream.cpu(), A, W, 1)
    with pytest.raises((ValueError, TypeError), match="edge_weights"):                       # one weight short
        call(data.graph, ew[:-1].contiguous(), x, stream, A, W, 1)
    with pytest.raises(ValueError, match="nodes"):                                           # node count
        call(data.graph, ew, packed().empty(n + 1, 64, dev()), stream, A, W, 1)
    with pytest.raises(ValueError, match="out must be"):
        call(data.graph, ew, x, stream, A, W, 1, out=packed().empty(n, 128, dev()))
    with pytest.raises((ValueError, TypeError), match="uniforms"):                           # [num_ls, E, 3, C]
        call(data.graph, ew, x, stream, A, W, 1, uniforms=torch.zeros((1, E, 2, 64), device=dev()))
    op = torch.ops.rlsolver_hip.maxcut_edge_local_search
    h = data.graph.handle
    e = torch.empty(64, device=dev())
    with pytest.raises(RuntimeError, match="visit_stream"):                                  # fewer than 7 E words
        op(h, ew, x.words, 64, x.words, 64, stream[:7 * E - 1].contiguous(), A, W, -1, 1, None, 0, e)
    with pytest.raises(RuntimeError, match="expected"):
        op(h, ew, x.words, 64, x.words, 64, stream, A, W, -1, 1, None, 0, e[:63])
    with pytest.raises(RuntimeError, match="expected"):
        op(h, ew, x.words, 64, x.words, 64, stream, A, W, -1, 1, None, 0, e.double())
    with pytest.raises(RuntimeError, match="gauge_node"):
        op(h, ew, x.words, 64, x.words, 64, stream, A, W, n, 1, None, 0, e)
    with pytest.raises(RuntimeError, match="gauge_node"):
        op(h, ew, x.words, 64, x.words, 64, stream, A, W, -2, 1, None, 0, e)
    with pytest.raises(RuntimeError, match="num_ls"):
        op(h, ew, x.words, 64, x.words, 64, stream, A, W, -1, -1, None, 0, e)
    with pytest.raises(RuntimeError, match="uniforms"):
        op(h, ew, x.words, 64, x.words, 64, stream, A, W, -1, 2, torch.zeros((1, E, 3, 64), device=dev()), 0, e)
    with pytest.raises(RuntimeError, match="edge_weights"):
        op(h, ew.float(), x.words, 64, x.words, 64, stream, A, W, -1, 1, None, 0, e)
    x2 = packed().empty(n, 128, dev())
    with pytest.raises(RuntimeError, match="in-place"):                                      # broadcast in place
        op(h, ew, x2.words[:1], 64, x2.words, 128, stream, A, W, -1, 1, None, 0, torch.empty(128, device=dev()))
    with pytest.raises(RuntimeError, match="multiple of 64"):                                # chain_ids: a period that is no tile
        op(h, ew, x.words, 64, x.words, 64, stream, A, W, -1, 1, None, 0, e, 0, 32, 32)
    with pytest.raises(NotImplementedError):
        op(h, ew.cpu(), x.words.cpu(), 64, x.words.cpu(), 64, stream.cpu(), A, W, -1, 1, None, 0, torch.empty(64))
    op(h, ew, x.words, 64, x.words, 64, stream, A, W, -1, 1, None, 0, e)                     # and the good call runs
    # a stream that does not describe this graph ends the pass instead of reading outside: a record pointing past N, a length
    # running past the end
    s1 = stream.clone()
    s1[0] = n + 5
    _, e1 = call(data.graph, ew, x, s1, A, W, 1, out=packed().empty(n, 64, dev()))
    s2 = stream.clone()
    s2[2] = 1 << 20
    _, e2 = call(data.graph, ew, x, s2, A, W, 1, out=packed().empty(n, 64, dev()))
    _, e0 = call(data.graph, ew, x, stream, A, W, 0, out=packed().empty(n, 64, dev()))
    assert torch.equal(e1, e0) and torch.equal(e2, e0)


def test_fuzz_slice():
    spec = importlib.util.spec_from_file_location("fuzz_maxcut_edge", os.path.join(ROOT, "tools", "fuzz", "fuzz_maxcut_edge.py"))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    assert mod.run(5.0, seed=1234) >= 5
