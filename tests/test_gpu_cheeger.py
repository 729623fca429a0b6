"""Cheeger-cut family on the GPU: the sweep + score kernel, the two reference-shaped samplers, the packed sampler, MCPGRound and
run_mcpg against the numpy oracle (tests/cheeger_oracle.py) and the fixture recorded from the reference.  Every comparison is
exact: arrays bit for bit, NaN positions required to coincide."""
import importlib.util
import os

import numpy as np
import pytest
import torch

import cheeger_oracle as orc

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def dev():
    return torch.device("cuda:0")


def mc():
    from rlsolver_amd.methods import MCPG_cheeger
    return MCPG_cheeger


def packed():
    from rlsolver_amd.ops_mcpg_tsp import PackedChains
    return PackedChains


def t(a, dt=torch.float32):
    return torch.from_numpy(np.ascontiguousarray(a)).to(dev(), dt)


# ---------------------------------------------------------------------------------------------------------------- cases
def graph_case(name):
    """(n, eu, ev, w, visiting order) of the named graph."""
    rng = np.random.RandomState(sum(map(ord, name)))
    if name == "n1":
        n, eu, ev = 1, [], []
    elif name == "n2_edge":
        n, eu, ev = 2, [0], [1]
    elif name == "path7":
        n, eu, ev = 7, list(range(6)), list(range(1, 7))
    elif name == "star300":
        n, eu, ev = 301, [0] * 300, list(range(1, 301))
    elif name == "edgeless10":
        n, eu, ev = 10, [], []
    elif name == "loops_dups":
        n, eu, ev = 9, [0, 1, 1, 2, 3, 3, 4, 1, 5, 5, 8], [1, 1, 2, 1, 3, 4, 3, 0, 6, 6, 8]
    elif name == "signed":
        n = 30
        eu, ev = rng.randint(0, n, 90).tolist(), rng.randint(0, n, 90).tolist()
    elif name == "gnm2000":
        from rlsolver_amd.graph import generate_gnm
        g = np.asarray(generate_gnm(2000, 19990, 5), dtype=np.int64)
        n, eu, ev = 2000, g[:, 0].tolist(), g[:, 1].tolist()
    else:
        raise KeyError(name)
    eu, ev = np.asarray(eu, dtype=np.int64), np.asarray(ev, dtype=np.int64)
    w = rng.choice([-3, -2, -1, 1, 2], eu.shape[0]).astype(np.int64) if name == "signed" else np.ones(eu.shape[0], np.int64)
    return n, eu, ev, w, rng.permutation(n)


CASES = ["n1", "n2_edge", "path7", "star300", "edgeless10", "loops_dups", "signed", "gnm2000"]
_DATA = {}


def data_of(name):
    """The data object of a case, built once (nothing below changes it but test_two_orders, which restores it)."""
    if name not in _DATA:
        n, eu, ev, w, order = graph_case(name)
        _DATA[name] = (mc().make_data(n, eu, ev, w, dev(), sorted_degree_nodes=order), (n, eu, ev, w, order))
    return _DATA[name]


def start_chains(n, c, seed):
    """Chains drawn at p = 0.05 / 0.5 / 0.95 by column, with an all-0, an all-1 and a one-hot chain planted in columns 0, 1, 2."""
    rng = np.random.RandomState(seed)
    x = (rng.rand(n, c) < np.asarray([0.05, 0.5, 0.95])[np.arange(c) % 3][None, :]).astype(np.float32)
    for col in range(min(c, 3)):
        x[:, col] = 1.0 if col == 1 else 0.0
        if col == 2:
            x[seed % n, col] = 1.0
    return x


def check_kernel(name, C, num_ls, normalized, c_in=None, form="packed", seed=0):
    """Sweep + score of `C` chains (started from `c_in` of them, broadcast) in one output form: chains, h, cut and size equal the
    oracle's; nothing is written past chain C.  Returns the kernel's outputs."""
    data, (n, eu, ev, w, order) = data_of(name)
    c_in = C if c_in is None else c_in
    start = start_chains(n, c_in, seed)
    want_x, want_h, want_cut, want_size = orc.local_search(n, eu, ev, w, order, start[:, np.arange(C) % c_in], num_ls, normalized)
    xin = packed().pack(t(start))
    out = {"packed": packed().empty(n, C, dev()), "inplace": xin, "f32": None}[form]
    if form == "packed":
        out.words.fill_(-1)
    xs, h, cut, size = data.local_search(xin, num_ls, normalized, out=out, num_chains=C)
    assert form != "inplace" or xs is xin
    got = (xs if form == "f32" else xs.unpack()).cpu().numpy()
    assert got.shape == (n, C) and np.array_equal(got, want_x), (name, C, num_ls, normalized, form)
    for g, wnt, what in ((h, want_h, "h"), (cut, want_cut, "cut"), (size, want_size, "size")):
        assert g.dtype == torch.float32 and g.shape == (C,) and orc.same_bits(g.cpu().numpy(), wnt), (name, C, num_ls, normalized, form, what)
    if form != "f32" and C % 64:                          # the layout's rule: bits of chains past C are zero
        last = xs.words[-1].cpu().numpy().view(np.uint64)
        assert not (last >> np.uint64(C % 64)).any()
    return xs, h, cut, size


# ---------------------------------------------------------------------------------------------------------------- kernel
@pytest.mark.parametrize("normalized", [False, True], ids=["ratio", "normalised"])
@pytest.mark.parametrize("name", CASES)
def test_kernel_equals_oracle(name, normalized):
    C = 256 if name == "gnm2000" else 70
    for num_ls in (0, 1, 3):
        _, h, _, _ = check_kernel(name, C, num_ls, normalized, seed=num_ls)
        hn = h.cpu().numpy()
        unit = name != "signed"
        if num_ls == 0 and unit:
            assert np.isnan(hn[:2]).all()                  # the all-0 and the all-1 chain on unit weights: 0 / 0
        if num_ls == 0 and not unit:
            assert np.isinf(hn[:2]).any()                  # an empty side under a non-zero cut
        if num_ls >= 1 and unit and graph_case(name)[0] >= 2:
            assert not np.isnan(hn).any()                  # the first visit of an empty-side chain always flips


def test_signed_weights_keep_minus_inf():
    """W < E on an empty side: cut < 0, h = -inf, and -inf < nh keeps it through every pass."""
    n, eu, ev = 6, np.arange(5), np.arange(1, 6)
    w = np.array([-2, 1, -1, 1, -3])
    order = np.arange(n)
    data = mc().make_data(n, eu, ev, w, dev(), sorted_degree_nodes=order)
    start = start_chains(n, 64, 1)
    for nrm in (False, True):
        want = orc.local_search(n, eu, ev, w, order, start, 2, nrm)
        xs, h, cut, size = data.local_search(packed().pack(t(start)), 2, nrm)
        assert np.array_equal(xs.cpu().numpy(), want[0]) and orc.same_bits(h.cpu().numpy(), want[1])
        assert np.isneginf(want[1][0]) and want[0][:, 0].sum() == 0


@pytest.mark.parametrize("C", [1, 63, 64, 65, 130])
def test_chain_counts(C):
    for form in ("packed", "f32"):
        check_kernel("loops_dups", C, 2, False, form=form, seed=C)
        check_kernel("path7", C, 1, True, form=form, seed=C)


def test_outputs_past_C_are_not_written():
    data, (n, eu, ev, w, order) = data_of("star300")
    from rlsolver_amd.torch_ops import ops as _t
    for C in (1, 63, 65, 130):
        start = start_chains(n, C, C)
        xin = packed().pack(t(start))
        out = packed().empty(n, C, dev())
        big = [torch.full((C + 64,), -7.0, device=dev()) for _ in range(3)]
        h, cut, size = (b[:C] for b in big)
        _t.cheeger_local_search(data.graph.handle, xin.words, C, out.words, C, data.stream(), 0, 2, float(data.edge_weight_sum), h, cut, size)
        want = orc.local_search(n, eu, ev, w, order, start, 2, False)
        for b, wnt in zip(big, want[1:]):
            assert orc.same_bits(b[:C].cpu().numpy(), wnt) and bool((b[C:] == -7.0).all())


def test_broadcast_start():
    for nrm in (False, True):
        check_kernel("gnm2000", 192, 1, nrm, c_in=64, seed=4)
        check_kernel("loops_dups", 192, 2, nrm, c_in=64, form="f32", seed=5)


def test_in_place_and_float32_equal_packed():
    for name in ("path7", "star300", "gnm2000"):
        a = check_kernel(name, 128, 2, True, form="packed", seed=9)
        b = check_kernel(name, 128, 2, True, form="inplace", seed=9)
        c = check_kernel(name, 128, 2, True, form="f32", seed=9)
        assert torch.equal(a[0].words, b[0].words) and torch.equal(a[0].unpack(), c[0])
        for i in (1, 2, 3):
            assert torch.equal(a[i], b[i]) and torch.equal(a[i], c[i])


def test_two_orders():
    data, (n, eu, ev, w, order) = data_of("gnm2000")
    other = np.random.RandomState(77).permutation(n)
    start = start_chains(n, 64, 3)
    got = []
    try:
        for o in (order, other):
            data.sorted_degree_nodes = torch.from_numpy(o)              # replaced: the stream is rebuilt
            xs, h, _, _ = data.local_search(packed().pack(t(start)), 1, False)
            want = orc.local_search(n, eu, ev, w, o, start, 1, False)
            assert np.array_equal(orc.decode_stream(data.stream().cpu().numpy(), n)[0], o)
            assert np.array_equal(xs.cpu().numpy(), want[0]) and orc.same_bits(h.cpu().numpy(), want[1])
            got.append(xs)
    finally:
        data.sorted_degree_nodes = torch.from_numpy(order)
    assert not torch.equal(got[0], got[1])


def test_cut_and_size_are_a_recount():
    from rlsolver_amd import ops
    for name in ("gnm2000", "star300", "path7"):
        data, _ = data_of(name)
        for nrm in (False, True):
            xs, h, cut, size = check_kernel(name, 130, 2, nrm, form="f32", seed=6)
            assert torch.equal(size, xs.sum(dim=0))
            assert torch.equal(cut, ops.maxcut_obj(data.graph, xs.t().contiguous().bool()).float())      # unit weights: cut edges


def test_largest_supported_num_nodes():
    from rlsolver_amd import ops_mcpg_tsp as mops
    from rlsolver_amd.graph import build_csr
    from rlsolver_amd.methods import MCPG_maxcut
    from rlsolver_amd.methods.MCPG import build_cheeger_stream
    nmax = mc().supported_limit()
    rng = np.random.RandomState(8)
    eu, ev = rng.randint(0, nmax, 30000), rng.randint(0, nmax, 30000)
    eu[0], ev[0] = 0, nmax - 1
    w = np.ones(30000, np.int64)
    order = rng.permutation(nmax)
    data = mc().make_data(nmax, eu, ev, w, dev(), sorted_degree_nodes=order)
    start = start_chains(nmax, 64, 2)
    xs, h, cut, size = data.local_search(packed().pack(t(start)), 1, False, out=packed().empty(nmax, 64, dev()))
    want = orc.local_search(nmax, eu, ev, w, order, start, 1, False)
    assert np.array_equal(xs.unpack().cpu().numpy(), want[0])
    for g, wnt in zip((h, cut, size), want[1:]):
        assert orc.same_bits(g.cpu().numpy(), wnt)
    with pytest.raises(ValueError, match=f"{nmax}"):                         # the Python layer names the limit
        mc().make_data(nmax + 1, eu, ev, w, dev())
    big = MCPG_maxcut.make_data(nmax + 1, eu, ev, w, dev(), sorted_degree_nodes=np.arange(nmax + 1))
    stream = t(build_cheeger_stream(build_csr((eu, ev, w), num_nodes=nmax + 1, keep_loops=True), np.arange(nmax + 1)), torch.int32)
    x = packed().empty(nmax + 1, 64, dev())
    with pytest.raises(RuntimeError, match=f"\\(-2\\).*{nmax}"):              # RLS_EUNSUPPORTED from the entry point itself
        mops.mcpg_cheeger_local_search(big.graph, x, stream, False, 0, 30000.0, out=x)


# -------------------------------------------------------------------------------------------------------------- samplers
ENTRIES = list(orc.fixture_entries())
_FIX = {}


def fixture_data(e):
    key = e["name"].split("/")[0]
    if key not in _FIX:
        _FIX[key] = mc().make_data(e["n"], e["eu"], e["ev"], e["w"], dev(), sorted_degree_nodes=e["order"])
    return _FIX[key]


@pytest.mark.parametrize("gname", ["BA_5_ID0", "PL_20_ID0", "BA_100_ID0", "ER_100_ID0", "gset_14_stub"])
def test_samplers_against_the_reference_fixture(gname):
    """mcpg_sampling_rcheegercut / mcpg_sampling_ncheegercut with the reference's recorded walk: their four returns, and the packed
    sampler on the same raw samples."""
    seen = 0
    for e in ENTRIES:
        if not e["name"].startswith(gname + "/"):
            continue
        seen += 1
        data = fixture_data(e)
        fn = mc().mcpg_sampling_ncheegercut if e["normalized"] else mc().mcpg_sampling_rcheegercut
        T = e["index"].shape[0]
        got = fn(data, t(e["start"]), t(e["probs"]), e["num_ls"], e["change_times"], e["M"],
                 index=t(e["index"], torch.int64) if T else None, u=t(e["u"]) if T else None)
        want = (e["neg_h"], e["best"].astype(np.float32), e["raw"].astype(np.float32), e["value"])
        for g, wnt, what in zip(got, want, ("-h[best]", "best", "raw", "value")):
            assert g.dtype == torch.float32 and g.device.type == "cuda" and orc.same_bits(g.cpu().numpy(), wnt), (e["name"], what)
        best_val, best, value, xs = mc().sampler_cheeger_packed(data, packed().pack(got[2]), e["num_ls"], e["M"], e["R"],
                                                                normalized=e["normalized"], in_place=False)
        assert torch.equal(best_val, got[0]) and torch.equal(best.unpack(), got[1]) and torch.equal(value, got[3])
    assert seen == 16


def test_packed_sampler_in_place_and_result():
    data, (n, eu, ev, w, order) = data_of("gnm2000")
    M, R = 64, 2
    start = start_chains(n, M * R, 12)[:, ::-1].copy()        # (the planted chains last: no NaN among the first repeats)
    x = packed().pack(t(start))
    res0 = data.result(x)
    _, h0, _, _ = orc.local_search(n, eu, ev, w, order, start, 0, False)
    assert orc.same_bits(res0.cpu().numpy(), -h0)
    want = orc.sampler(n, eu, ev, w, order, start, 2, M, False)
    best_val, best, value, xs = mc().sampler_cheeger_packed(data, x, 2, M, R)
    assert xs is x
    assert orc.same_bits(best_val.cpu().numpy(), want[0]) and np.array_equal(best.unpack().cpu().numpy(), want[1])
    assert orc.same_bits(value.cpu().numpy(), want[2]) and np.array_equal(xs.unpack().cpu().numpy(), want[4])


# ----------------------------------------------------------------------------------------------------- MCPGRound, run_mcpg
def ba100():
    e = next(e for e in ENTRIES if e["name"].startswith("BA_100_ID0/"))
    return fixture_data(e), e


def replay_round(e, samples, num_ls, normalized, M, res, info):
    """One round restated: the oracle on the round's metro output, best of repeats and the merge in numpy (oracle_np.mcpg_merge_best).
    The round's mean is the device's reduction of expected = 2 h; it is taken here the same way, from the ORACLE's h."""
    from oracle import oracle_np as onp
    xs, h, _, _ = orc.local_search(e["n"], e["eu"], e["ev"], e["w"], e["order"], samples, num_ls, normalized)
    idx = orc.first_min(h, M)
    res, info, temp, now_max, now_idx = onp.mcpg_merge_best(-h[idx], xs[:, idx], res, info)
    h2 = t(h) * 2
    value = ((h2 - h2.mean()) * 0.5).cpu().numpy()
    assert orc.same_bits(value, (t(h) - t(h).mean()).cpu().numpy())            # doubling commutes with float32 rounding
    return h, res, info, temp, now_max, now_idx, value


@pytest.mark.parametrize("normalized", [False, True], ids=["ratio", "normalised"])
def test_mcpg_round_three_rounds(normalized):
    from rlsolver_amd.methods.MCPG import MCPGRound
    data, e = ba100()
    data.normalized = normalized
    n, M, R = e["n"], 64, 2
    rng = np.random.RandomState(31)
    xs0 = (rng.rand(n, M) < 0.5).astype(np.float32)
    res = -orc.local_search(n, e["eu"], e["ev"], e["w"], e["order"], xs0, 0, normalized)[1]
    info = xs0.astype(np.uint8)
    vs0 = data.result(t(xs0))
    assert orc.same_bits(vs0.cpu().numpy(), res)
    rnd = MCPGRound(data, t(xs0), vs0, M, R, num_ls=2, seed=17)
    probs = torch.full((n,), 0.5, device=dev())
    for _ in range(3):
        value, best = rnd.step(probs)
        h, res, info, temp, now_max, now_idx, want_value = replay_round(e, rnd.samples.unpack().cpu().numpy(), 2, normalized, M, res, info)
        assert orc.same_bits(rnd.expected.cpu().numpy(), 2 * h)
        assert orc.same_bits(value.cpu().numpy(), want_value)
        assert orc.same_bits(rnd.now_max_res.cpu().numpy(), res) and np.array_equal(rnd.now_max_info.unpack().cpu().numpy(), info)
        assert np.array_equal(rnd.start.unpack().cpu().numpy(), temp)
        assert float(best) == float(now_max)
        assert torch.isfinite(rnd.get_return(probs.clone().requires_grad_(True)))
    v, x = rnd.best_solution()
    assert v == float(now_max) and np.array_equal(x.cpu().numpy().astype(np.uint8), info[:, now_idx])
    data.normalized = False


def test_run_mcpg_two_rounds():
    from rlsolver_amd.methods.MCPG import run_mcpg
    data, e = ba100()
    n, M, R = e["n"], 64, 2
    rng = np.random.RandomState(32)
    xs0 = (rng.rand(n, M) < 0.5).astype(np.float32)
    seen = []
    hook = data.round_local_search

    def recording(samples, num_ls, seed, out, chain_ids):
        seen.append(samples.unpack().cpu().numpy())
        return hook(samples, num_ls, seed, out, chain_ids)

    data.round_local_search = recording
    try:
        v, x, rates = run_mcpg(data, t(xs0), data.result(t(xs0)), M, R, 2, 2, sample_epoch_num=2, log=lambda *a: None, seed=3)
    finally:
        del data.round_local_search
    res = -orc.local_search(n, e["eu"], e["ev"], e["w"], e["order"], xs0, 0, False)[1]
    info = xs0.astype(np.uint8)
    assert len(seen) == 2 and len(rates) == 2
    for k, samples in enumerate(seen):
        if k:                                              # the next round walks from the merged kept chains
            assert samples.shape == (n, M * R)
        _, res, info, temp, now_max, now_idx, _ = replay_round(e, samples, 2, False, M, res, info)
    assert v == float(now_max) and np.array_equal(x.cpu().numpy().astype(np.uint8), info[:, now_idx])


def test_sharded_round_is_refused():
    from rlsolver_amd.methods.MCPG import MCPGRound
    data, e = ba100()
    xs0 = torch.zeros((e["n"], 64), device=dev())
    xs0[0] = 1
    with pytest.raises(NotImplementedError, match="MAXLOC"):
        MCPGRound(data, xs0, data.result(xs0), 64, 2, num_ls=1, kept_offset=0, total_kept=128)
    MCPGRound(data, xs0, data.result(xs0), 64, 2, num_ls=1)                   # unsharded: accepted


# -------------------------------------------------------------------------------------------------------------------- op
def test_op_rejects_bad_arguments():
    from rlsolver_amd import ops_mcpg_tsp as mops
    data, (n, *_rest) = data_of("loops_dups")
    x = packed().empty(n, 64, dev())
    x.words.zero_()
    stream = data.stream()
    bad = (RuntimeError, ValueError, TypeError)
    with pytest.raises(bad):                                                  # a short stream
        mops.mcpg_cheeger_local_search(data.graph, x, stream[:-1].contiguous(), False, 1, 1.0)
    with pytest.raises(bad):                                                  # dtype
        mops.mcpg_cheeger_local_search(data.graph, x, stream.long(), False, 1, 1.0)
    with pytest.raises(bad):                                                  # device
        mops.mcpg_cheeger_local_search(data.graph, x, stream.cpu(), False, 1, 1.0)
    with pytest.raises(bad):                                                  # node count
        mops.mcpg_cheeger_local_search(data.graph, packed().empty(n + 1, 64, dev()), stream, False, 1, 1.0)
    with pytest.raises(bad):
        mops.mcpg_cheeger_local_search(data.graph, x, stream, False, 1, 1.0, out=packed().empty(n, 128, dev()))
    op = torch.ops.rlsolver_hip.cheeger_local_search
    h = torch.empty(64, device=dev())
    with pytest.raises(RuntimeError):                                         # the op itself: short stream, h of another size / dtype
        op(data.graph.handle, x.words, 64, x.words, 64, stream[:-1].contiguous(), 0, 1, 1.0, h, None, None)
    with pytest.raises(RuntimeError):
        op(data.graph.handle, x.words, 64, x.words, 64, stream, 0, 1, 1.0, h[:63], None, None)
    with pytest.raises(RuntimeError):
        op(data.graph.handle, x.words, 64, x.words, 64, stream, 0, 1, 1.0, h.double(), None, None)
    with pytest.raises(RuntimeError):
        op(data.graph.handle, x.words, 64, x.words, 64, stream, 0, 1, 1.0, h, h[:5], None)
    with pytest.raises(RuntimeError):
        op(data.graph.handle, x.words, 64, x.words, 64, stream, 2, 1, 1.0, h, None, None)
    with pytest.raises(RuntimeError):                                         # broadcast in place
        op(data.graph.handle, x.words, 64, x.words, 128, stream, 0, 1, 1.0, torch.empty(128, device=dev()), None, None)
    with pytest.raises(NotImplementedError):
        op(data.graph.handle, x.words.cpu(), 64, x.words.cpu(), 64, stream.cpu(), 0, 1, 1.0, torch.empty(64), None, None)
    op(data.graph.handle, x.words, 64, x.words, 64, stream, 0, 1, float(data.edge_weight_sum), h, None, None)      # and the good call runs


def test_fuzz_slice():
    spec = importlib.util.spec_from_file_location("fuzz_cheeger", os.path.join(ROOT, "tools", "fuzz", "fuzz_cheeger.py"))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    assert mod.run(5.0, seed=1234) >= 5
