"""The exact optimum by enumeration (rls_spin_exhaustive_pack / rls_spin_exhaustive, ops.spin_exhaustive, the envs'
_calc_over_range / calculate_best_energy / calculate_best) against the reference's own `_calc_over_range` (tests/golden/
spin_exhaustive.npz) and the numpy restatement of tests/exhaustive_oracle.py.  Everything is integers and halves: every
comparison is exact.

Sizes: N = 1 .. 16 against brute force (the chunk of a thread is 2^10 states: 11, 12, 13 and 16 hold more than one, 1 .. 5 less
than the unrolled 2^4), planted instances where brute force ends (32-bit words to N = 32, 64-bit words above; indices past 2^31,
2^32 and up to 2^48 - 1).  The largest enumeration is 2^26 states.

At import this file also registers the two ops' valid calls with tests/op_contract.py, so that the completeness test and the
refusal sweep of tests/test_gpu_op_contract.py cover them unchanged: pytest imports test modules in name order while it collects,
and this name sorts before that one.  Running tests/test_gpu_op_contract.py on its own no longer sees these rows (its completeness
test then names the two ops): run it together with this file."""
import functools
import json
import os
import subprocess
import sys

import numpy as np
import pytest
import torch

from tests import exhaustive_oracle as xo
from tests import op_contract as oc

gpu = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
DEV = oc.DEV
CHUNK = 1 << 10


def _ops():
    from rlsolver_amd import ops
    return ops


# ---------------------------------------------------------------------------------------------------------------- contract rows
CONTRACT_G, CONTRACT_N = 5, 13
CONTRACT_RANGE = (3, (1 << CONTRACT_N) - 5)


def _contract_matrix():
    r = oc.rng(31)
    return oc.t(np.stack([xo.random_couplings(r, CONTRACT_N, 0.5, diagonal=True) for _ in range(CONTRACT_G)]), torch.float32)


@oc.row("spin_exhaustive_pack", outs=("pos", "neg", "flags"))
def _():
    return oc.taken("spin_exhaustive_pack", lambda: _ops().spin_exhaustive(_contract_matrix(), *CONTRACT_RANGE))


@oc.row("spin_exhaustive")                      # (key is read and written: no result-only argument)
def _():
    return oc.taken("spin_exhaustive", lambda: _ops().spin_exhaustive(_contract_matrix(), *CONTRACT_RANGE))


# ---------------------------------------------------------------------------------------------------------------- helpers
def dev_matrix(Ws, dtype=torch.float64):
    return oc.t(np.array(Ws, dtype=np.float64), dtype)             # (a copy: the drawn matrices are read-only)


def keys(Ws, i0=0, i1=None, maximize=False, dtype=torch.float64, **kw):
    key, half_trace = _ops().spin_exhaustive(dev_matrix(Ws, dtype), i0, i1, maximize, **kw)
    assert key.dtype == torch.int64 and half_trace.dtype == torch.float64
    assert half_trace.tolist() == [np.trace(W) / 2 for W in Ws]
    return key.tolist()


@functools.lru_cache(maxsize=None)
def drawn(kind, N, G, seed=7):
    """G matrices from the package's own generators (BA carries the diagonal of its seed clique), as a read-only numpy array"""
    from rlsolver_amd.envs.util_envs_PECO import RandomBAGraphGenerator, RandomERGraphGenerator
    if kind == "ER":
        gg = RandomERGraphGenerator(n_spins=N, p_connection=0.5, num_envs=G, device=DEV, dtype=torch.float64)
    else:
        gg = RandomBAGraphGenerator(n_spins=N, m_insertion_edges=min(4, N - 1), num_envs=G, device=DEV, dtype=torch.float64)
    Ws = gg.get(seed=seed).cpu().numpy()
    Ws.setflags(write=False)
    return Ws


@functools.lru_cache(maxsize=None)
def want_keys(kind, N, G, maximize):
    return [xo.key_of(W, 0, 1 << N, maximize) for W in drawn(kind, N, G)]


class Fixed:
    """a single-instance generator: n_spins and get() -> [N, N]"""

    def __init__(self, W):
        self.W, self.n_spins = np.asarray(W, dtype=np.float64), len(W)

    def get(self, with_padding=False):
        return self.W.copy()


def basis(spins, binary):
    return (1 - spins) / 2 if binary else spins


# ---------------------------------------------------------------------------------------------------------------- golden
@gpu
@pytest.mark.parametrize("dtype", [torch.float32, torch.float64])
def test_ranges_of_the_reference_s_calc_over_range(golden, dtype):
    z = golden("spin_exhaustive")
    for tag in z["cases"]:
        W = z[f"{tag}/W"]
        for k, (i0, i1) in enumerate(z[f"{tag}/ranges"]):
            (key,) = keys([W], int(i0), int(i1), dtype=dtype)
            e, i = xo.key_decode(key)
            assert e - np.trace(W) / 2 == z[f"{tag}/energy"][k], (tag, k)
            assert np.array_equal(xo.spins_of(i, len(W)), z[f"{tag}/spins"][k]), (tag, k)


@gpu
def test_both_env_classes_reproduce_the_reference_s_calc_over_range(golden):
    from rlsolver_amd.envs.spinsystem import SpinSystem, SpinSystemUnbiased
    from rlsolver_amd.envs.util_envs_PECO import SetGraphGenerator
    z = golden("spin_exhaustive")
    for tag in z["cases"]:
        W = z[f"{tag}/W"]
        one = SpinSystemUnbiased(None, None, graph_generator=Fixed(W), device=DEV)
        for dt in (torch.float32, torch.float64):
            many = SpinSystem(None, None, 2, device=DEV, dtype=dt, graph_generator=SetGraphGenerator(torch.from_numpy(np.stack([W, W])), device=DEV))
            for k, (i0, i1) in enumerate(z[f"{tag}/ranges"]):
                want_e, want_s = z[f"{tag}/energy"][k], z[f"{tag}/spins"][k]
                e, s = many._calc_over_range(int(i0), int(i1))
                assert e.dtype == s.dtype == dt and e.shape == (2,) and s.shape == (2, len(W)) and e.is_cuda
                assert e.tolist() == [want_e] * 2 and np.array_equal(s.cpu().numpy(), np.stack([want_s] * 2)), (tag, k)
                if dt == torch.float64:
                    e, s = one._calc_over_range(i0, i1)
                    assert isinstance(e, float) and s.dtype == np.float64 and s.shape == (len(W),)
                    assert e == want_e and np.array_equal(s, want_s), (tag, k)


# ---------------------------------------------------------------------------------------------------------------- oracle
CASES = [("ER", 1, 1), ("ER", 1, 3), ("ER", 2, 3), ("BA", 2, 3), ("ER", 5, 1), ("BA", 5, 3), ("ER", 5, 65), ("BA", 5, 65), ("ER", 11, 3),
         ("BA", 11, 3), ("ER", 12, 1), ("BA", 12, 3), ("ER", 12, 65), ("BA", 12, 65), ("BA", 16, 1), ("ER", 16, 3)]


@gpu
@pytest.mark.parametrize("kind,N,G", CASES)
def test_full_range_against_brute_force(kind, N, G):
    Ws = drawn(kind, N, G)
    if kind == "BA" and N > 2:
        assert np.trace(Ws[0]) != 0                           # the seed clique's self-loops: the trace term is real
    for maximize in (False, True):
        want = want_keys(kind, N, G, maximize)
        for dt in (torch.float32, torch.float64):
            got = keys(Ws, maximize=maximize, dtype=dt)
            assert got == want, (maximize, dt)
        # global-flip symmetry: of the pair (s, -s) the one with spin 0 = -1 comes first
        assert all(xo.key_decode(k)[1] < 1 << (N - 1) for k in want)


@gpu
def test_launches_cut_anywhere_fold_to_the_same_key():
    Ws = drawn("BA", 12, 3)
    want = want_keys("BA", 12, 3, False)
    for per in (1, 3 * 1000, 3 * 1024, 3 * 1500, 1 << 34):
        if per == 1:                                          # one state per launch: a short range of it
            assert keys(Ws, 4090, 4096, states_per_launch=1) == [xo.key_of(W, 4090, 4096) for W in Ws]
        else:
            assert keys(Ws, states_per_launch=per) == want, per


# ---------------------------------------------------------------------------------------------------------------- envs
N_ENV = 11


@functools.lru_cache(maxsize=None)
def env_answers(kind="BA"):
    """per matrix of drawn(kind, N_ENV, 3): (min-energy state: energy, cut, spins), (max-cut state: cut, spins)"""
    out = []
    for W in drawn(kind, N_ENV, 3):
        e, _, s = xo.calc_over_range(W, 0, 1 << N_ENV)
        _, _, smax = xo.calc_over_range(W, 0, 1 << N_ENV, maximize=True)
        out.append(((e, xo.cut(W, s), s), (xo.cut(W, smax), smax)))
    return out


@gpu
@pytest.mark.parametrize("binary", [False, True])
@pytest.mark.parametrize("target", ["CUT", "ENERGY"])
def test_single_instance_env_best_energy_and_best(binary, target):
    from rlsolver_amd.envs.spinsystem import OptimisationTarget, SpinBasis, SpinSystemUnbiased
    for W, ((e, c, s), (cmax, smax)) in zip(drawn("BA", N_ENV, 3), env_answers()):
        env = SpinSystemUnbiased(None, None, graph_generator=Fixed(W), device=DEV, spin_basis=SpinBasis.BINARY if binary else SpinBasis.SIGNED,
                                 optimisation_target=OptimisationTarget[target])
        assert np.array_equal(env.matrix, W)
        first, spins = env.calculate_best_energy()
        assert isinstance(first, float) and spins.dtype == np.float64 and spins.shape == (N_ENV,)
        assert first == (c if target == "CUT" else e) and np.array_equal(spins, basis(s, binary))
        first, spins = env.calculate_best()
        if target == "CUT":
            assert first == cmax and np.array_equal(spins, basis(smax, binary))
            assert first == env.calculate_cut(spins)          # the env's own cut of the state it names
        else:
            assert first == e and np.array_equal(spins, basis(s, binary))
            assert first == env.calculate_energy(spins)


@gpu
@pytest.mark.parametrize("binary", [False, True])
@pytest.mark.parametrize("dtype", [torch.float32, torch.float64])
def test_batched_env_best_energy_and_best(binary, dtype):
    from rlsolver_amd.envs.spinsystem import SpinBasis, SpinSystem
    from rlsolver_amd.envs.util_envs_PECO import SetGraphGenerator
    Ws, ans = drawn("BA", N_ENV, 3), env_answers()
    sb = SpinBasis.BINARY if binary else SpinBasis.SIGNED
    env = SpinSystem(None, None, 3, device=DEV, dtype=dtype, spin_basis=sb, graph_generator=SetGraphGenerator(torch.from_numpy(Ws.copy()), device=DEV))
    first, spins = env.calculate_best_energy()
    assert first.dtype == spins.dtype == dtype and first.shape == (3,) and spins.shape == (3, N_ENV)
    assert first.tolist() == [a[0][1] for a in ans] and np.array_equal(spins.cpu().numpy(), np.stack([basis(a[0][2], binary) for a in ans]))
    first, spins = env.calculate_best()
    assert first.tolist() == [a[1][0] for a in ans] and np.array_equal(spins.cpu().numpy(), np.stack([basis(a[1][1], binary) for a in ans]))
    # one shared graph (an edge list) answers for every env
    W = xo.random_couplings(oc.rng(3), N_ENV, 0.5)
    edges =[(int(a), int(b), int(W[a, b])) for a in range(N_ENV) for b in range(a + 1, N_ENV) if W[a, b]]
    shared = SpinSystem(edges, N_ENV, 4, device=DEV, dtype=dtype, spin_basis=sb)
    _, _, smax = xo.calc_over_range(W, 0, 1 << N_ENV, maximize=True)
    first, spins = shared.calculate_best()
    assert first.tolist() == [xo.cut(W, smax)] * 4 and np.array_equal(spins.cpu().numpy(), np.stack([basis(smax, binary)] * 4))
    e, s = shared._calc_over_range(5, 1500)
    we, _, ws = xo.calc_over_range(W, 5, 1500)
    assert e.tolist() == [we] * 4 and np.array_equal(s.cpu().numpy(), np.stack([ws] * 4))


# ---------------------------------------------------------------------------------------------------------------- ranges
N_RANGE = 13
FULL = 1 << N_RANGE
RANGES = {"inner": (3, FULL - 5), "one_state": (777, 778), "first_state": (0, 1), "last_state": (FULL - 1, FULL),
          "inside_a_chunk": (CHUNK + 6, CHUNK + 500), "across_a_chunk_boundary": (CHUNK - 24, CHUNK + 26), "whole_chunk": (CHUNK, 2 * CHUNK),
          "to_the_end": (FULL - 7, FULL), "chunks_and_a_bit": (2 * CHUNK - 1, 5 * CHUNK + 1)}


@gpu
@pytest.mark.parametrize("name", sorted(RANGES))
def test_ranges(name):
    i0, i1 = RANGES[name]
    Ws = drawn("BA", N_RANGE, 3)
    for maximize in (False, True):
        assert keys(Ws, i0, i1, maximize) == [xo.key_of(W, i0, i1, maximize) for W in Ws]
    # an edgeless graph: every state has E_off = 0, the first of the range wins
    assert keys([np.zeros((N_RANGE, N_RANGE))], i0, i1) == [xo.key_encode(0, i0)]
    assert keys([np.diag(np.arange(N_RANGE, dtype=np.float64))], i0, i1, True) == [xo.key_encode(0, i0)]


@gpu
@pytest.mark.parametrize("cut", [FULL // 2, CHUNK + 77, 1, FULL - 1])
def test_sub_ranges_fold_and_combine_to_the_whole(cut):
    ops = _ops()
    Ws = drawn("ER", N_RANGE, 3)
    m = dev_matrix(Ws)
    whole = ops.spin_exhaustive(m)[0]
    assert whole.tolist() == [xo.key_of(W, 0, FULL) for W in Ws]
    for first, second in (((0, cut), (cut, FULL)), ((cut, FULL), (0, cut))):
        key = torch.full((3,), ops.EXHAUSTIVE_KEY_EMPTY, dtype=torch.int64, device=DEV)
        got = ops.spin_exhaustive(m, *first, key=key)[0]
        assert got.data_ptr() == key.data_ptr()
        ops.spin_exhaustive(m, *second, key=key)
        assert torch.equal(key, whole), (first, second)
    a, b = ops.spin_exhaustive(m, 0, cut)[0], ops.spin_exhaustive(m, cut, FULL)[0]
    assert torch.equal(torch.minimum(a, b), whole)


CHILD = r"""
import json, os, sys
sys.path.insert(0, os.environ["RLS_ROOT"])
sys.path.insert(0, os.path.join(os.environ["RLS_ROOT"], "tests"))
import numpy as np, torch, torch.distributed as dist
import exhaustive_oracle as xo
from rlsolver_amd import dist as rdist, ops
rank, local_rank, world = rdist.init_from_env()
assert dist.is_initialized() and dist.get_backend() == "nccl" and (rank, world) == (0, 1)
dev = torch.device("cuda", local_rank)
rng = np.random.RandomState(5)
Ws = np.stack([xo.random_couplings(rng, 12, 0.5, True) for _ in range(3)])
m = torch.from_numpy(Ws).to(dev)
alone = ops.spin_exhaustive(m, 3, 4000)[0]
grouped = ops.spin_exhaustive(m, 3, 4000, group=dist.group.WORLD)[0]
ok = torch.equal(alone, grouped) and alone.tolist() == [xo.key_of(W, 3, 4000) for W in Ws]
dist.barrier(device_ids=[local_rank])
dist.destroy_process_group()
print(json.dumps({"ok": bool(ok)}))
"""


@gpu
def test_one_rank_group_gives_the_result_of_no_group():
    from tests.test_gpu_rccl import _env
    p = subprocess.run([sys.executable, "-c", CHILD], env=_env(), stdout=subprocess.PIPE, stderr=subprocess.PIPE, text=True, timeout=600)
    assert p.returncode == 0, p.stderr[-3000:]
    assert json.loads([ln for ln in p.stdout.splitlines() if ln.startswith("{")][-1])["ok"] is True


# ---------------------------------------------------------------------------------------------------------------- planted instances
WINDOW = 1 << 22


def planted_case(N, low_side):
    """W_pq = t_p t_q on a path with chords (connected): the ground states are +-t, E_off = -|edges|.  low_side: the smaller of
    the two indices has every bit above the low 22 set but the first (it lies in the last 2^22 states below 2^(N-1)); else t is
    -1 but for low bits, so that -t lies in the last 2^22 states of the range."""
    r = oc.rng(N * 2 + int(low_side))
    t = 2 * r.randint(0, 2, N) - 1
    t[:max(N - 22, 1)] = 1 if low_side else -1
    t[0] = -1
    edges = [(a, a + 1) for a in range(N - 1)] + [(0, N // 2), (1, N - 1), (N // 3, N - 2)]
    return xo.planted(N, t, edges), len(edges), xo.index_of(t), xo.index_of(-t)


@gpu
@pytest.mark.parametrize("N", [24, 26])
def test_planted_ground_state_over_the_full_range(N):
    W, m, lo, hi = planted_case(N, True)
    assert (1 << (N - 1)) - WINDOW <= lo < 1 << (N - 1) <= hi
    assert keys([W], dtype=torch.float32) == [xo.key_encode(-m, lo)]
    assert keys([-W], maximize=True) == [xo.key_encode(-m, lo)]           # the maximum of -W: the masks swapped back


@gpu
@pytest.mark.parametrize("N", [31, 32, 33, 47, 48])
def test_planted_ground_state_in_windows_at_the_word_and_index_edges(N):
    top = 1 << N
    # around the planted index: the window crosses 2^(N-1), where the first node's bit turns
    W, m, lo, hi = planted_case(N, True)
    assert (top >> 1) - WINDOW <= lo < top >> 1
    a = lo - WINDOW // 2
    assert keys([W], a, a + WINDOW) == [xo.key_encode(-m, lo)]
    assert keys([W], lo, lo + 1) == [xo.key_encode(-m, lo)] and keys([W], hi, hi + 1) == [xo.key_encode(-m, hi)]
    # at the very top of the range: -t is the one ground state in the window
    W, m, lo, hi = planted_case(N, False)
    assert lo < WINDOW and top - WINDOW <= hi < top
    assert keys([W], top - WINDOW, top, dtype=torch.float32) == [xo.key_encode(-m, hi)]
    assert keys([W], 0, WINDOW) == [xo.key_encode(-m, lo)]
    if N == 48:                                               # the last index of all: one state, every bit of the index field set
        assert keys([np.zeros((N, N))], top - 1, top) == [xo.key_encode(0, top - 1)]


# ---------------------------------------------------------------------------------------------------------------- refusals
def _fresh_key(G):
    return torch.full((G,), xo.KEY_EMPTY, dtype=torch.int64, device=DEV)


@gpu
@pytest.mark.parametrize("where", ["first", "last"])
@pytest.mark.parametrize("what", ["two", "half", "asymmetric"])
def test_couplings_outside_the_contract_are_refused(where, what):
    Ws = drawn("ER", 12, 3).copy()
    g = 0 if where == "first" else 2
    if what == "asymmetric":
        Ws[g, 3, 7], Ws[g, 7, 3] = 1.0, -1.0
    else:
        Ws[g, 3, 7] = Ws[g, 7, 3] = 2.0 if what == "two" else 0.5
    key = _fresh_key(3)
    for dt in (torch.float32, torch.float64):
        with pytest.raises(ValueError, match=f"graph {g} "):
            _ops().spin_exhaustive(dev_matrix(Ws, dt), key=key)
    assert key.tolist() == [xo.KEY_EMPTY] * 3
    flags = _ops().spin_exhaustive_pack(dev_matrix(Ws))[2].tolist()
    assert flags == [(2 if what == "asymmetric" else 1) if k == g else 0 for k in range(3)]
    Ws[g, 5, 5] = 0.5                                         # any diagonal is allowed
    assert _ops().spin_exhaustive_pack(dev_matrix(Ws))[2].tolist() == flags


@gpu
def test_sizes_and_ranges_outside_the_contract_are_refused():
    from rlsolver_amd.envs.spinsystem import SpinSystemUnbiased
    ops = _ops()
    with pytest.raises(ValueError, match="N = 49"):
        ops.spin_exhaustive(torch.zeros((1, 49, 49), device=DEV))
    z = lambda g, n: torch.zeros((g, n), dtype=torch.int64, device=DEV)       # noqa: E731
    with pytest.raises(RuntimeError):
        torch.ops.rlsolver_hip.spin_exhaustive_pack(torch.zeros((1, 49, 49), device=DEV), z(1, 49), z(1, 49), torch.zeros(1, dtype=torch.uint8, device=DEV))
    key = _fresh_key(1)
    with pytest.raises(RuntimeError):
        torch.ops.rlsolver_hip.spin_exhaustive(z(1, 49), z(1, 49), 0, 1, key)
    W = drawn("ER", 12, 1)
    m = dev_matrix(W)
    pos, neg, _ = ops.spin_exhaustive_pack(m)
    for i0, i1 in ((5, 5), (6, 5), (0, (1 << 12) + 1), (-1, 5), (1 << 12, (1 << 12) + 1)):
        with pytest.raises(ValueError):
            ops.spin_exhaustive(m, i0, i1, key=key)
        with pytest.raises(RuntimeError):
            torch.ops.rlsolver_hip.spin_exhaustive(pos, neg, i0, i1, key)
    torch.cuda.synchronize()
    assert key.tolist() == [xo.KEY_EMPTY]
    env = SpinSystemUnbiased(None, None, graph_generator=Fixed(W[0]), device=DEV)
    for call in (lambda: env.calculate_best(max_spins=11), lambda: env.calculate_best_energy(max_spins=11), lambda: env._calc_over_range(0, 8, max_spins=11),
                 lambda: env.calculate_best(max_spins=49)):
        with pytest.raises(ValueError, match="max_spins"):
            call()
    assert env.calculate_best(max_spins=12)[0] == env.calculate_best()[0]
    big = SpinSystemUnbiased(None, None, graph_generator=Fixed(planted_case(41, True)[0]), device=DEV)
    with pytest.raises(ValueError, match="max_spins"):
        big.calculate_best()                                   # 2^41 states are not enumerated unasked
