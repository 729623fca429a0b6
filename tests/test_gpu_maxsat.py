"""MaxSAT family on the GPU: the sweep + score kernel, the reference-shaped sampler, MCPGRound and run_mcpg against the numpy
oracle (tests/maxsat_oracle.py) and the fixture recorded from the reference, bit for bit, with recorded draws.

Recorded uniforms are prepared first (maxsat_oracle.prepare_uniforms: a draw with 0 < 1/2 - u <= 2^-10 becomes 0.25) and every
instance keeps each variable's listed weight below 2^13, so ulp(|old|) / 2 <= 2^-11 and the kernel's coin "u < 1/2" is the
reference's float32 rule; each case asserts that on the CPU (coin_rule_agrees)."""
import os

import numpy as np
import pytest
import torch

import maxsat_oracle as orc

pytestmark = pytest.mark.gpu
GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "maxsat.npz")


def dev():
    return torch.device("cuda:0")


def ms():
    from rlsolver_amd.methods import MCPG_maxsat
    return MCPG_maxsat


def packed():
    from rlsolver_amd.ops_mcpg_tsp import PackedChains
    return PackedChains


@pytest.fixture(scope="module")
def fx():
    return np.load(GOLDEN)


def three_sat(rng, nvar, n):
    return [[int(v + 1) * (1 if rng.rand() < 0.5 else -1) for v in rng.choice(nvar, 3, replace=False)] for _ in range(n)]


def build(nvar, clauses, weights=None, top=None, nclause=None, order=None):
    order = np.arange(nvar) if order is None else np.asarray(order)
    data = ms().make_data(nvar, clauses, weights, top, nclause, dev(), sorted_nodes=order)
    return data, orc.Instance(nvar, clauses, weights, top, nclause), order


def recorded_draws(rng, shape):
    """Uniforms as a recorded run has them, prepared (maxsat_oracle.prepare_uniforms): what every test of this file draws."""
    return orc.prepare_uniforms(rng.rand(max(shape[0], 1), *shape[1:]).astype(np.float32)[:shape[0]])


def check_kernel(data, inst, order, C, num_ls, seed, c_in=None, packed_out=True, draw=recorded_draws, start=None, in_place=False):
    """Sweep + score on random chains (or on `start` 0|1 [nvar, c_in]) with the uniforms of `draw(rng, shape)`: chains and
    expected equal the oracle's.  Chain c of a broadcast start (c_in < C) starts from chain c % c_in."""
    rng = np.random.RandomState(seed)
    c_in = C if c_in is None else c_in
    start = (rng.rand(inst.nvar, c_in) < 0.5).astype(np.float32) if start is None else np.asarray(start, dtype=np.float32)
    assert start.shape == (inst.nvar, c_in)
    uni = draw(rng, (num_ls, inst.nvar, C))
    s = (start[:, np.arange(C) % c_in].T * 2 - 1).astype(np.float32)
    assert orc.coin_rule_agrees(inst, s, order, num_ls, uni)
    orc.sweep(inst, s, order, num_ls, uni)
    coins = ms().maxsat_tie_coins_from_uniforms(torch.from_numpy(uni).to(dev())) if num_ls else None
    xin = packed().pack(torch.from_numpy(start).to(dev()))
    out = (xin if in_place else packed().empty(inst.nvar, C, dev())) if packed_out else None
    xs, expected = data.local_search(xin, num_ls, coins=coins, out=out, num_chains=C)
    assert not in_place or xs is xin
    got = (xs.unpack() if packed_out else xs).cpu().numpy()
    assert np.array_equal(got, (s.T + 1) / 2)
    assert np.array_equal(expected.cpu().numpy(), -orc.score(inst, s))
    return xs, expected


def listed_weight(inst):
    """Largest sum of |neg| over the clauses listed for one variable (each clause once per listing)."""
    best = 0
    for ci, ng in zip(inst.nci, inst.nneg):
        seen, tot = set(), 0
        for c, w in zip(ci, ng):
            if c not in seen:
                seen.add(c)
                tot += abs(w)
        best = max(best, tot)
    return best


@pytest.fixture(scope="module")
def rand70():
    rng = np.random.RandomState(70)
    return build(70, three_sat(rng, 70, 300), order=rng.permutation(70))


def test_one_variable():
    for clauses in ([], [[1]], [[-1]], [[], []]):                   # (the last: clauses, but no literal at all)
        data, inst, order = build(1, clauses)
        for num_ls in (0, 1, 2):
            check_kernel(data, inst, order, 64, num_ls, seed=num_ls)


@pytest.mark.parametrize("num_ls", [0, 1, 3])
def test_random_3sat(rand70, num_ls):
    data, inst, order = rand70
    assert listed_weight(inst) < (1 << 13)
    check_kernel(data, inst, order, 64, num_ls, seed=1)
    check_kernel(data, inst, order, 192, num_ls, seed=2, c_in=64)
    check_kernel(data, inst, order, 200, num_ls, seed=3, packed_out=False)          # the f32 surface, a ragged last tile


def test_in_place(rand70):
    data, inst, order = rand70
    rng = np.random.RandomState(5)
    start = (rng.rand(70, 128) < 0.5).astype(np.float32)
    uni = orc.prepare_uniforms(rng.rand(2, 70, 128).astype(np.float32))
    s = orc.sweep(inst, (start.T * 2 - 1).astype(np.float32), order, 2, uni)
    x = packed().pack(torch.from_numpy(start).to(dev()))
    xs, _ = data.local_search(x, 2, coins=ms().maxsat_tie_coins_from_uniforms(torch.from_numpy(uni).to(dev())), out=x)
    assert xs is x and np.array_equal(x.unpack().cpu().numpy(), (s.T + 1) / 2)


def test_every_odd_clause_form():
    long40 = [int(v) * (1 if v % 3 else -1) for v in range(1, 41)]
    clauses = [[1, 1, 2], [3, -3, 4], [], [5], [-6], [7], long40, [-1, 2, -2, 8], [9, 9, 9], [44, -43]]
    rng = np.random.RandomState(9)
    clauses += three_sat(rng, 44, 30)                                                # variable 45 is in no clause
    data, inst, order = build(45, clauses, nclause=len(clauses) + 3, order=rng.permutation(45))
    assert data.num_edges == len(clauses) + 3
    for num_ls in (0, 2):
        check_kernel(data, inst, order, 64, num_ls, seed=num_ls)


def test_hub_of_600_clauses():
    rng = np.random.RandomState(600)
    clauses = [[(1 if rng.rand() < 0.5 else -1)] + [int(v + 1) * (1 if rng.rand() < 0.5 else -1) for v in rng.choice(np.arange(1, 50), 2, replace=False)]
               for _ in range(600)]
    data, inst, order = build(50, clauses, order=rng.permutation(50))
    planes = (data.schedule()[0].cpu().numpy().view(np.uint32)[:-1] >> 24) & 31
    assert planes.max() == 10 and planes.min() <= 5 and listed_weight(inst) < (1 << 13)      # every counter width up to the hub's
    check_kernel(data, inst, order, 64, 2, seed=4)


def test_chain_of_levels_and_a_single_level():
    n = 40
    rng = np.random.RandomState(40)
    sgn = lambda v: int(v) * (1 if rng.rand() < 0.5 else -1)         # noqa: E731
    data, inst, order = build(n, [[sgn(i + 1), sgn(i + 2)] for i in range(n - 1)])
    assert data.schedule()[0].numel() - 1 == n                        # nvar levels
    check_kernel(data, inst, order, 64, 2, seed=6)
    data, inst, order = build(n, [[sgn(i + 1)] for i in range(n)])
    assert data.schedule()[0].numel() - 1 == 1                        # one level, one group
    check_kernel(data, inst, order, 128, 2, seed=7)


def test_wcnf_weights():
    # x1: one soft clause of weight 3 against three of weight 1 -- make == break in weight, not in count
    wc = [(3, [1]), (1, [-1]), (1, [-1]), (1, [-1]), (20, [2, -3]), (20, [4]), (3, [-4, 5]), (1, [5, 5, -6]), (3, [2, -2, 7])]
    rng = np.random.RandomState(12)
    for _ in range(40):
        vs = rng.choice(np.arange(1, 13), size=rng.randint(1, 4), replace=False)
        wc.append((int(rng.choice([1, 3, 20])), [int(v) * (1 if rng.rand() < 0.5 else -1) for v in vs]))
    data, inst, order = build(12, [c for _, c in wc], [w for w, _ in wc], 20, order=rng.permutation(12))
    nhard = sum(1 for w, _ in wc if w == 20)
    assert data.num_edges == len(wc) - nhard + 20 * nhard and listed_weight(inst) < (1 << 13)
    for num_ls in (0, 1, 3):
        check_kernel(data, inst, order, 64, num_ls, seed=num_ls)
    check_kernel(data, inst, order, 200, 2, seed=8, packed_out=False)


def test_largest_supported_nvar():
    from rlsolver_amd import _abi
    nmax, _ = ms().supported_limits()
    rng = np.random.RandomState(3)
    clauses = [[int(v + 1) * (1 if rng.rand() < 0.5 else -1) for v in rng.choice(nmax, 3, replace=False)] for _ in range(99)]
    clauses.append([nmax, -1])
    data = ms().make_data(nmax, clauses, device=dev(), sorted_nodes=np.arange(nmax))
    start = (rng.rand(nmax, 64) < 0.5)
    xin = packed().pack(torch.from_numpy(start.astype(np.float32)).to(dev()))
    # every decision away from the 100 clauses is a coin: all-zero coins leave those variables as they are
    coins = torch.zeros((nmax, 1), dtype=torch.int64, device=dev())
    xs, expected = data.local_search(xin, 1, coins=coins, out=packed().empty(nmax, 64, dev()))
    touched = sorted({abs(l) - 1 for cl in clauses for l in cl})
    small = orc.Instance(nmax, clauses)
    s = (start.T * 2 - 1).astype(np.float32)
    # the oracle's sweep over the touched variables only (the others keep their value under zero coins)
    for i in touched:
        idx, seg, ng = np.asarray(small.nvi[i]), np.asarray(small.nci[i]), np.asarray(small.nneg[i], dtype=np.float32)
        old = orc._segment_max_sum(s[:, idx] * ng, seg)
        s[:, i] = -s[:, i]
        new = orc._segment_max_sum(s[:, idx] * ng, seg)
        s[:, i] = np.where(new > old, s[:, i], -s[:, i])
    assert np.array_equal(xs.unpack().cpu().numpy(), (s.T + 1) / 2)
    assert np.array_equal(expected.cpu().numpy(), -orc.score(small, s))
    with pytest.raises(_abi.RlsError, match=f"RLS_EUNSUPPORTED.*{nmax}"):
        ms().make_data(nmax + 1, clauses, device=dev())
    with pytest.raises(RuntimeError, match=f"{nmax}"):                       # the entry point itself refuses the tile
        bad = packed().empty(nmax + 1, 64, dev())
        data.local_search(bad, 0, out=bad)


def test_production_draws_shards_and_fair_coins(rand70):
    data, inst, order = rand70
    rng = np.random.RandomState(11)
    M, R = 128, 2                                                    # chain = repeat * M + kept
    start = packed().pack(torch.from_numpy((rng.rand(70, M * R) < 0.5).astype(np.float32)).to(dev()))
    whole, e_whole = data.local_search(start, 2, seed=1234, out=packed().empty(70, M * R, dev()))
    w = whole.unpack()
    st = start.unpack()
    for half in (0, 1):
        cols = torch.cat([torch.arange(r * M + half * 64, r * M + half * 64 + 64) for r in range(R)]).to(dev())
        shard = packed().pack(st[:, cols].contiguous())
        xs, e = data.local_search(shard, 2, seed=1234, out=packed().empty(70, 64 * R, dev()), chain_ids=(half * 64, 64, M - 64))
        assert torch.equal(xs.unpack(), w[:, cols]) and torch.equal(e, e_whole[cols])
    other, _ = data.local_search(start, 2, seed=1235, out=packed().empty(70, M * R, dev()))
    assert not torch.equal(other.words, whole.words)
    # variables in no clause: every decision is a coin; x ^= coin on an all-zero start leaves the XOR of the passes' coins
    nvar, C, num_ls = 257, 4096, 1
    free = ms().make_data(nvar, [], device=dev(), sorted_nodes=np.arange(nvar))
    zero = packed().pack(torch.zeros((nvar, C), device=dev()))
    xs, e = free.local_search(zero, num_ls, seed=99, out=packed().empty(nvar, C, dev()))
    n = nvar * C * num_ls
    mean = float(xs.unpack().double().mean())
    assert abs(mean - 0.5) <= 5 * 0.5 / np.sqrt(n), mean
    assert torch.equal(e, torch.zeros_like(e))


def test_sampler_against_the_reference_fixture(fx):
    """mcpg_sampling_maxsat with the reference's recorded walk and sweep draws: its four returns."""
    for name in [str(n) for n in fx["names"]]:
        inst = orc.parse(str(fx[f"{name}/text"]), str(fx[f"{name}/ext"]))
        M, R, num_ls, T = fx[f"{name}/params"].tolist()
        order = fx[f"{name}/order"]
        uni = orc.prepare_uniforms(fx[f"{name}/uniforms"])
        assert listed_weight(inst) < (1 << 13)
        want = orc.sampling(inst, order, fx[f"{name}/start"].astype(np.float32), fx[f"{name}/probs"], num_ls, T, M,
                            fx[f"{name}/index"].astype(np.int64), fx[f"{name}/u"], uni)
        assert orc.coin_rule_agrees(inst, (want[2].T * 2 - 1).astype(np.float32), order, num_ls, uni)
        if np.array_equal(uni, fx[f"{name}/uniforms"]):              # no draw had to be moved: the oracle's run IS the reference's
            assert np.array_equal(want[0], fx[f"{name}/max_res"]) and np.array_equal(want[3], fx[f"{name}/value"])
        data = ms().make_data(inst.nvar, inst.clauses, inst.weights, inst.top, inst.nclause, dev(), sorted_nodes=order)
        t = lambda a, dt=torch.float32: torch.from_numpy(np.ascontiguousarray(a)).to(dev(), dt)        # noqa: E731
        got = ms().mcpg_sampling_maxsat(data, t(fx[f"{name}/start"]), t(fx[f"{name}/probs"]), num_ls, T, M,
                                        index=t(fx[f"{name}/index"], torch.int64) if len(fx[f"{name}/index"]) else None,
                                        u=t(fx[f"{name}/u"]) if len(fx[f"{name}/u"]) else None, uniforms=t(uni))
        for g, w, what in zip(got, want[:4], ("max_res", "best", "raw", "value")):
            assert g.dtype == torch.float32 and np.array_equal(g.cpu().numpy(), w), (name, what)


def test_packed_sampler_and_result(rand70):
    data, inst, order = rand70
    rng = np.random.RandomState(21)
    M, R = 64, 2
    start = (rng.rand(70, M * R) < 0.5).astype(np.float32)
    x = packed().pack(torch.from_numpy(start).to(dev()))
    res0 = data.result(x).cpu().numpy()
    assert np.array_equal(res0, orc.result(inst, (start.T * 2 - 1).astype(np.float32)))
    max_res, best, value, xs = ms().sampler_maxsat_packed(data, x, 2, M, R, seed=7)
    s = (xs.unpack().cpu().numpy().T * 2 - 1).astype(np.float32)
    res = orc.result(inst, s)
    pick = np.argmax(res.reshape(R, M), axis=0) * M + np.arange(M)
    assert np.array_equal(max_res.cpu().numpy(), res[pick])
    assert np.array_equal(best.unpack().cpu().numpy(), ((s.T + 1) / 2)[:, pick])
    np.testing.assert_allclose(value.cpu().numpy(), -(res - res.mean()), rtol=0, atol=1e-4)


def test_mcpg_round_three_rounds(rand70):
    from rlsolver_amd.methods.MCPG import MCPGRound
    data, inst, _ = rand70
    torch.manual_seed(5)
    M, R = 64, 2
    xs0 = (torch.rand((70, M), device=dev()) < 0.5).float()
    rnd = MCPGRound(data, xs0, data.result(xs0), M, R, num_ls=2, seed=17)
    probs = torch.full((70,), 0.5, device=dev())
    last = float(data.result(xs0).max())
    for _ in range(3):
        value, best = rnd.step(probs)
        assert value.shape == (M * R,) and float(best) >= last
        last = float(best)
        loss = rnd.get_return(probs.clone().requires_grad_(True))
        assert torch.isfinite(loss)
    v, x = rnd.best_solution()
    s = (x.float().cpu().numpy()[None, :] * 2 - 1).astype(np.float32)
    assert v == last and v == float(orc.result(inst, s)[0])
    np.testing.assert_allclose(rnd.value.cpu().numpy(), (rnd.expected - rnd.expected.mean()).cpu().numpy() / 2, rtol=0, atol=1e-5)


def test_run_mcpg_two_rounds():
    from rlsolver_amd.methods.MCPG import run_mcpg
    rng = np.random.RandomState(60)
    data, inst, _ = build(60, three_sat(rng, 60, 250), order=rng.permutation(60))
    torch.manual_seed(6)
    xs0 = (torch.rand((60, 64), device=dev()) < 0.5).float()
    v, x, rates = run_mcpg(data, xs0, data.result(xs0), 64, 2, 2, 2, sample_epoch_num=2, log=lambda *a: None, seed=3)
    s = (x.float().cpu().numpy()[None, :] * 2 - 1).astype(np.float32)
    assert v == float(orc.result(inst, s)[0]) and v >= float(data.result(xs0).max()) and len(rates) == 2


def test_op_rejects_bad_arguments(rand70):
    data, _, _ = rand70
    x = packed().empty(70, 64, dev())
    lv_ptr, lv_data = data.schedule()
    from rlsolver_amd import ops_mcpg_tsp as mops
    with pytest.raises((RuntimeError, ValueError, TypeError)):
        mops.mcpg_maxsat_local_search(x, lv_ptr, lv_data, data._clause_ptr.cpu(), data._lit, None, 1)
    with pytest.raises((RuntimeError, ValueError, TypeError)):
        mops.mcpg_maxsat_local_search(x, lv_ptr, lv_data, data._clause_ptr, data._lit.long(), None, 1)
    with pytest.raises((RuntimeError, ValueError, TypeError)):
        mops.mcpg_maxsat_local_search(x, lv_ptr, lv_data, data._clause_ptr, data._lit, None, 1,
                                      coins=torch.zeros((70, 2), dtype=torch.int64, device=dev()))
    with pytest.raises(NotImplementedError):
        torch.ops.rlsolver_hip.maxsat_local_search(x.words.cpu(), 64, x.words.cpu(), 64, lv_ptr.cpu(), lv_data.cpu(), 0, None, 0,
                                                   data._clause_ptr.cpu(), data._lit.cpu(), None, torch.zeros(64), 0, 0, 0)
