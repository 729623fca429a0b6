"""MIMO detection family on the GPU: the block Gauss-Seidel kernel in every launch form, the reference-shaped sampler, the packed
sampler, MCPGRound and run_mcpg against the numpy oracle (tests/mimo_oracle.py) and the fixture recorded from the reference.
Integer-valued instances are compared bit for bit; real-valued ones bit for bit on the chains whose decisions all clear the
float32 bound of the oracle (at least 90 % of them, asserted first), and by value on every chain."""
import ctypes as C

import numpy as np
import pytest
import torch

import mimo_oracle as orc

pytestmark = pytest.mark.gpu
F = np.float32


def dev():
    return torch.device("cuda:0")


def mm():
    from rlsolver_amd.methods import MCPG_mimo
    return MCPG_mimo


def mops():
    from rlsolver_amd import ops_mcpg_tsp
    return ops_mcpg_tsp


def packed():
    from rlsolver_amd.ops_mcpg_tsp import PackedChains
    return PackedChains


def t(a, dt=torch.float32):
    return torch.from_numpy(np.ascontiguousarray(a)).to(dev(), dt)


def same_bits(a, b):
    a, b = np.ascontiguousarray(a, dtype=F), np.ascontiguousarray(b, dtype=F)
    return a.shape == b.shape and bool((a.view(np.uint32) == b.view(np.uint32)).all())


_FORMS = {}


def form_chains():
    """form -> a RAGGED chain count that rls_mimo_local_search_supported reports the form for, searched upward from 64 (the
    thresholds depend on the CU count: none is written down here)."""
    if not _FORMS:
        m = 1
        while m <= (1 << 16) and len(_FORMS) < 3:
            for c in (64 * m + 36, 96 * m + 36):
                ok, form = mops().mimo_launch_form(100, c)
                assert ok
                _FORMS.setdefault(form, c)
            m *= 2
    return _FORMS


def test_all_three_forms_are_reached():
    assert sorted(form_chains()) == [0, 1, 2]
    assert all(c % 64 != 0 for c in form_chains().values())


_ORACLE = {}


def oracle_run(n, seed, num_ls, diag=False, even_diag=False, unique=128):
    """The integer instance + `unique` random chains + the oracle's sweep (float32: exact on these instances), computed once."""
    key = (n, seed, num_ls, diag, even_diag, unique)
    if key not in _ORACLE:
        Sigma, Diag, sca, x01 = orc.integer_case(n, seed, unique, diag=diag, even_diag=even_diag)
        assert 2 * np.abs(Sigma).sum(axis=1).max() + np.abs(Diag).max() < 2 ** 24 and np.abs(Sigma).sum() + np.abs(Diag).sum() < 2 ** 24
        _ORACLE[key] = (Sigma, Diag, sca, x01, orc.local_search(Sigma, Diag, x01, num_ls, np.float32))
    return _ORACLE[key]


def run_kernel(Sigma, Diag, x01, num_ls, **kw):
    xs = packed().pack(t(x01))
    out, expected = mops().mcpg_mimo_local_search(t(Sigma), t(Diag), xs, num_ls, **kw)
    torch.cuda.synchronize()
    return xs, out, expected


def check_padding(out):
    """Bits of chains past C leave as 0."""
    rest = out.num_chains % 64
    if rest:
        assert int(((out.words[-1] >> rest) != 0).sum()) == 0


# ---------------------------------------------------------------------------------------------------------------- 1. golden
@pytest.mark.parametrize("c", list(orc.fixture_cases()), ids=lambda c: c["case"])
def test_sampler_equals_fixture(c):
    Sigma, Diag = c["Sigma"], c["Diag"]
    z = np.load(orc.GOLDEN)
    data = mm().make_data(Sigma, Diag, z[f"{c['name']}/X"], c["sca"], float(z[f"{c['name']}/noise"]), dev())
    max_res, best, raw, value = mm().mcpg_sampling_mimo(data, t(c["start"]), t(c["probs"]), c["num_ls"], c["change_times"], c["M"],
                                                        index=t(c["index"], torch.int64), u=t(c["u"]))
    assert np.array_equal(raw.cpu().numpy().astype(np.uint8), c["raw"])
    assert best.dtype == torch.float32 and np.array_equal(best.cpu().numpy().astype(np.uint8), c["best"])
    o = orc.sampler(Sigma, Diag, c["sca"], c["raw"], c["num_ls"], c["M"])
    Cc = c["M"] * c["R"]
    tol = 2 * Cc * 2.0 ** -24 * float(np.abs(o["expected"]).max())
    assert max_res.dtype == torch.float32 and value.dtype == torch.float32 and tuple(value.shape) == (Cc,)
    if c["integer"]:
        assert same_bits(max_res.cpu().numpy(), c["max_res"])
    else:
        assert np.abs(max_res.cpu().numpy().astype(np.float64) - c["max_res"]).max() <= tol
    assert np.abs(value.cpu().numpy().astype(np.float64) - c["value"]).max() <= tol


# ---------------------------------------------------------------------------------------------------------------- 2. forms
@pytest.mark.parametrize("form", [0, 1, 2])
@pytest.mark.parametrize("num_ls", [1, 3])
@pytest.mark.parametrize("n", [1, 31, 32, 33, 100, 257])
def test_every_form_bit_for_bit(n, num_ls, form):
    """Integer instances, ragged C: 128 distinct chains tiled over the batch, so that every workgroup of the launch is checked
    against one oracle run."""
    Cc = form_chains()[form]
    assert mops().mimo_launch_form(n, Cc) == (True, form)
    Sigma, Diag, _, x128, o = oracle_run(n, 100 + n, num_ls)
    reps = -(-Cc // 128)
    x01 = np.tile(x128, (1, reps))[:, :Cc]
    _, out, expected = run_kernel(Sigma, Diag, x01, num_ls, out=packed().empty(n, Cc, dev()))
    want = np.tile(((o["info"] + 1) / 2).astype(np.uint8), (1, reps))[:, :Cc]
    assert np.array_equal(out.unpack().cpu().numpy().astype(np.uint8), want)
    assert same_bits(expected.cpu().numpy(), np.tile(o["expected"].astype(F), reps)[:Cc])
    check_padding(out)


@pytest.mark.parametrize("num_ls", [1, 3])
@pytest.mark.parametrize("kind", ["ragged100", "upper_half_empty", "broadcast", "in_place", "diagonal", "even_diag", "f32_out"])
def test_layouts_and_quirks(kind, num_ls):
    n = 100
    Sigma, Diag, _, x128, o = oracle_run(n, 7, num_ls, diag=kind == "diagonal", even_diag=kind == "even_diag")
    want_x, want_e = ((o["info"] + 1) / 2).astype(np.uint8), o["expected"].astype(F)
    if kind == "diagonal":
        assert (np.diag(Sigma) != 0).any()
    if kind == "even_diag":
        assert o["ties"] >= 1                                                  # exact ties r == thr occur and resolve to -1
    if kind == "broadcast":                                                    # 64 chains in, 256 out: chain c reads chain c % 64
        xs = packed().pack(t(x128[:, :64]))
        out, expected = mops().mcpg_mimo_local_search(t(Sigma), t(Diag), xs, num_ls, out=packed().empty(n, 256, dev()), num_chains=256)
        assert np.array_equal(out.unpack().cpu().numpy().astype(np.uint8), np.tile(want_x[:, :64], (1, 4)))
        assert same_bits(expected.cpu().numpy(), np.tile(want_e[:64], 4))
        return
    Cc = {"ragged100": 100, "upper_half_empty": 70}.get(kind, 128)
    xs = packed().pack(t(x128[:, :Cc]))
    if kind == "in_place":
        out, expected = mops().mcpg_mimo_local_search(t(Sigma), t(Diag), xs, num_ls, out=xs)
        assert out is xs
    elif kind == "f32_out":
        before = xs.words.clone()
        out, expected = mops().mcpg_mimo_local_search(t(Sigma), t(Diag), xs, num_ls)
        assert out.dtype == torch.float32 and tuple(out.shape) == (n, Cc) and torch.equal(xs.words, before)
        assert np.array_equal(out.cpu().numpy().astype(np.uint8), want_x[:, :Cc])
        assert same_bits(expected.cpu().numpy(), want_e[:Cc])
        return
    else:
        out, expected = mops().mcpg_mimo_local_search(t(Sigma), t(Diag), xs, num_ls, out=packed().empty(n, Cc, dev()))
    assert np.array_equal(out.unpack().cpu().numpy().astype(np.uint8), want_x[:, :Cc])
    assert same_bits(expected.cpu().numpy(), want_e[:Cc])
    check_padding(out)


def test_packed_sampler_and_result():
    n, M, R, num_ls = 100, 64, 2, 2
    Sigma, Diag, sca, x128, o = oracle_run(n, 7, num_ls)
    data = mm().make_data(Sigma, Diag, np.ones(n), sca, 0.0, dev())
    xs = packed().pack(t(x128))
    best_val, best, value, xs_loc = mm().sampler_mimo_packed(data, xs, num_ls, M, R)
    e = o["expected"].astype(F)
    idx = orc.first_min(e, M)
    assert xs_loc is xs and same_bits(best_val.cpu().numpy(), -(e[idx] + F(sca)))
    assert np.array_equal(best.unpack().cpu().numpy().astype(np.uint8), ((o["info"] + 1) / 2).astype(np.uint8)[:, idx])
    assert same_bits(value.cpu().numpy(), orc.value_of(e))
    # result(): the value of +-1 chains, nothing swept, the chains untouched
    before = xs.words.clone()
    res = data.result(xs)
    assert torch.equal(xs.words, before)
    assert same_bits(res.cpu().numpy(), -e)                                   # (the swept chains' value is what the sweep reported)
    assert same_bits(data.result(t(x128)).cpu().numpy(), -orc.value_f64(Sigma, Diag, 2.0 * x128 - 1).astype(F))


# ---------------------------------------------------------------------------------------------------------------- 3. real values
@pytest.mark.parametrize("n,num_ls", orc.REAL_SHAPES)
@pytest.mark.parametrize("snr", orc.REAL_SNRS)
def test_real_valued_instances(n, num_ls, snr):
    Sigma, Diag, x01 = orc.real_case(n, snr)
    o = orc.real_run(n, snr, num_ls)
    safe = o["safe"]
    print(f"n={n} num_ls={num_ls} SNR={snr}: {int(safe.sum())} of {safe.shape[0]} chains clear the bound")
    assert safe.mean() >= 0.90
    _, out, expected = run_kernel(Sigma, Diag, x01, num_ls, out=packed().empty(n, x01.shape[1], dev()))
    got = out.unpack().cpu().numpy()
    want = ((o["info"] + 1) / 2)
    wrong = (got != want).any(axis=0)
    print(f"  chains that differ from the oracle: {int(wrong.sum())} in all, {int((wrong & safe).sum())} among those that clear the bound")
    assert not (wrong & safe).any()
    err = np.abs(expected.cpu().numpy().astype(np.float64) - orc.value_f64(Sigma, Diag, 2.0 * got - 1))
    print(f"  largest |expected - float64 value of the returned spins| = {err.max():.3e}, bound {orc.value_bound(Sigma, Diag):.3e}")
    assert err.max() <= orc.value_bound(Sigma, Diag)


# ---------------------------------------------------------------------------------------------------------------- 4. round
def _round_data():
    inst = mm().mimo_instance(50, 50, 12, 11, integer=True)
    data = mm().data_from_instance(inst, dev(), 1.0)
    return data, data[0].cpu().numpy(), data[1].cpu().numpy(), float(data[3])


def test_mcpg_round_three_rounds():
    from oracle import oracle_np as onp
    from rlsolver_amd.methods.MCPG import MCPGRound, metro_sampling_packed
    data, Sigma, Diag, sca = _round_data()
    n, M, R, num_ls = 100, 64, 4, 2
    xs0 = np.random.RandomState(41).randint(0, 2, size=(n, M)).astype(np.float32)
    res = (-orc.value_f64(Sigma, Diag, 2.0 * xs0 - 1)).astype(F)
    info = xs0.astype(np.uint8)
    vs0 = data.result(t(xs0))
    assert same_bits(vs0.cpu().numpy(), res)
    rnd = MCPGRound(data, t(xs0), vs0, M, R, num_ls=num_ls, seed=17)
    from rlsolver_amd.seeding import SeedStream
    twin_start, twin_seeds = packed().pack(t(xs0)), SeedStream(17)
    probs = torch.full((n,), 0.5, device=dev())
    for _ in range(3):
        value, best = rnd.step(probs)
        # the same round assembled by hand: walk (same seed sequence), kernel, then the oracle's pick and merge
        samples = metro_sampling_packed(probs, twin_start, rnd.change_times, num_chains=M * R, seed=twin_seeds.next())
        twin_seeds.next()                                                # (the round draws one more seed for the sweep)
        assert torch.equal(samples.words, rnd.samples.words)
        xs_loc, expected = mops().mcpg_mimo_local_search(data[0], data[1], samples, num_ls, out=packed().empty(n, M * R, dev()))
        o = orc.local_search(Sigma, Diag, samples.unpack().cpu().numpy(), num_ls, np.float32)
        e = o["expected"].astype(F)
        chains = ((o["info"] + 1) / 2).astype(np.uint8)
        assert same_bits(expected.cpu().numpy(), e) and np.array_equal(xs_loc.unpack().cpu().numpy().astype(np.uint8), chains)
        assert same_bits(rnd.expected.cpu().numpy(), 2 * e)
        idx = orc.first_min(e, M)
        res, info, temp, now_max, now_idx = onp.mcpg_merge_best(-e[idx], chains[:, idx], res, info)
        e2 = t(e) * 2
        assert same_bits(value.cpu().numpy(), ((e2 - e2.mean()) * 0.5).cpu().numpy())
        assert same_bits(rnd.now_max_res.cpu().numpy(), res) and np.array_equal(rnd.now_max_info.unpack().cpu().numpy(), info)
        assert np.array_equal(rnd.start.unpack().cpu().numpy(), temp)
        assert float(best) == float(now_max)
        twin_start = packed().pack(t(temp))
        assert torch.isfinite(rnd.get_return(probs.clone().requires_grad_(True)))
    v, x = rnd.best_solution()
    assert v == float(now_max) and np.array_equal(x.cpu().numpy().astype(np.uint8), info[:, now_idx])


def test_run_mcpg_objective_is_the_value_of_the_returned_x():
    from rlsolver_amd.methods.MCPG import run_mcpg
    data, Sigma, Diag, sca = _round_data()
    n, M, R = 100, 64, 2
    xs0 = np.random.RandomState(42).randint(0, 2, size=(n, M)).astype(np.float32)
    v, x, rates = run_mcpg(data, t(xs0), data.result(t(xs0)), M, R, 2, 2, sample_epoch_num=2, log=lambda *a: None, seed=3)
    assert len(rates) == 2
    spins = 2.0 * x.cpu().numpy().astype(np.float64) - 1
    want = orc.value_f64(Sigma, Diag, spins[:, None])[0]                        # an integer below 2^24: exact in float32 too
    assert v == -want
    assert data.objective(v) == -(want + sca)
    H_res = -(want + sca)
    assert H_res <= 0                                                        # -|Y - H x|^2


def test_sharded_round_is_refused():
    from rlsolver_amd.methods.MCPG import MCPGRound
    data, *_ = _round_data()
    xs0 = torch.zeros((100, 64), device=dev())
    with pytest.raises(NotImplementedError, match="MAXLOC"):
        MCPGRound(data, xs0, data.result(xs0), 64, 2, num_ls=1, kept_offset=0, total_kept=128)
    MCPGRound(data, xs0, data.result(xs0), 64, 2, num_ls=1)                   # unsharded: accepted


# ---------------------------------------------------------------------------------------------------------------- 5. refusals
def test_refusals_come_before_any_device_work():
    from rlsolver_amd import _abi
    n = 40
    Sigma, Diag, _, x128, _ = oracle_run(n, 9, 1)
    S, D = t(Sigma), t(Diag)
    xs = packed().pack(t(x128))
    before = xs.words.clone()
    out = packed().empty(n, 128, dev())
    with pytest.raises(ValueError, match="num_ls"):
        mops().mcpg_mimo_local_search(S, D, xs, 0, out=out)
    with pytest.raises(TypeError, match="HIP device"):
        mops().mcpg_mimo_local_search(S.cpu(), D, xs, 1, out=out)
    with pytest.raises(ValueError, match="Diag"):
        mops().mcpg_mimo_local_search(S, D[:-1].contiguous(), xs, 1, out=out)
    with pytest.raises(ValueError, match="in-place"):                        # a broadcast cannot be written over its own input
        mops().mcpg_mimo_local_search(S, D, packed()(xs.words[:1], 64), 1, out=xs, num_chains=128)
    assert torch.equal(xs.words, before)
    # the LDS limit, by the query: no launch, no allocation of an n x n matrix
    big = mm().supported_limit(128) + 1
    assert mops().mimo_launch_form(big - 1, 128)[0] and not mops().mimo_launch_form(big, 128)[0]
    assert not mops().mimo_launch_form(0, 128)[0]
    lib = _abi.lib()
    ptr = C.c_void_p(256)                                                     # never dereferenced: both calls return before a launch
    assert lib.rls_mimo_local_search(ptr, ptr, big, ptr, 128, ptr, 128, 1, ptr, None) == -2          # RLS_EUNSUPPORTED
    assert lib.rls_mimo_local_search(ptr, ptr, n, ptr, 128, ptr, 128, 0, ptr, None) == -1            # RLS_EINVAL: num_ls < 1
    assert lib.rls_mimo_local_search(ptr, ptr, n, ptr, 96, ptr, 128, 1, ptr, None) == -1             # C_in no multiple of 64
    op = torch.ops.rlsolver_hip.mimo_local_search
    e = torch.empty(128, device=dev())
    with pytest.raises(RuntimeError, match="num_ls"):
        op(S, D, xs.words, 128, out.words, 128, 0, e)
    with pytest.raises(RuntimeError):
        op(S, D, xs.words, 128, out.words, 128, 1, e[:100])
    with pytest.raises(RuntimeError):
        op(S[:, :-1].contiguous(), D, xs.words, 128, out.words, 128, 1, e)
    huge = torch.empty((big, big), device=dev())                              # allocated, never touched
    with pytest.raises(ValueError, match="LDS limit"):
        mops().mcpg_mimo_local_search(huge, torch.empty(big, device=dev()), packed().empty(big, 128, dev()), 1)
