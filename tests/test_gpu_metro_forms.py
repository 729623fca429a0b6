"""Every form of the MCPG metro walk (K9: rls_mcpg_metro_rounds, rls_mcpg_metro_stop) against tests/metro_oracle.py, bit for bit.

The launcher picks among three kernels and eight forms:

    k_mcpg_metro<float | uint8_t, PROBS_LDS = true | false>    node-major chains; probs leave LDS once 12 N + 4 T + 16 > 160 KB
    k_mcpg_metro_packed<GIVEN = true | false, QG = false>      bit-packed chains, draw windows in LDS
    k_mcpg_metro_packed<GIVEN = true | false, QG = true>       bit-packed chains, draw windows in caller scratch: taken for
                                                               6145 <= N <= 10240, the only packed form for 16385 <= N <= 20480

One helper (check_case) runs a case through a named form and compares (a) the state after EVERY prefix of rounds -- one launch
per T' with t_limit on the device --, (b) the accept counts row by row, past the limit, and of a dry pass, (c) the bits past C of
the packed output, (d) the start state of an out-of-place launch.  A verdict taken from a stale word re-couples with the true
chain within a few rounds, so the final state alone hides it; the prefixes and the per-round counts do not.  The draws that make
the packed walker's look-ahead repairs matter are metro_oracle.pattern_draws (tests/test_metro_oracle.py proves that they do)."""
import contextlib

import numpy as np
import pytest
import torch

from oracle import oracle_np as onp
from rlsolver_amd import _abi
from rlsolver_amd import ops_mcpg_tsp as mops
from rlsolver_amd.methods import MCPG as amcpg
from rlsolver_amd.ops_mcpg_tsp import PackedChains
from tests import metro_oracle as mo
from tests.gpu_util import DEV

pytestmark = pytest.mark.gpu

FORMS = ("f32", "u8", "packed_lds", "packed_scratch")
LDS_BYTES = 160 * 1024
BIG_N = (6145, 16385)          # where the scratch form starts, and where it becomes the only packed form


def dev(a):
    a = np.ascontiguousarray(a)
    return torch.from_numpy(a.view(np.int64) if a.dtype == np.uint64 else a).to(DEV)


def kernel_form(form, N, T, given, accepts):
    """The kernel instance the launcher takes (its own arithmetic, restated)."""
    if form in ("f32", "u8"):
        probs_lds = 12 * N + (4 * T if accepts else 0) + 16 <= LDS_BYTES
        return f"k_mcpg_metro<{'float' if form == 'f32' else 'uint8_t'},PROBS_LDS={str(probs_lds).lower()}>"
    return f"k_mcpg_metro_packed<GIVEN={str(given).lower()},QG={str(form == 'packed_scratch').lower()}>"


@contextlib.contextmanager
def windows(form):
    """packed_lds: the draw windows are kept in LDS also where the launcher would take scratch (the RLS_METRO_QG knob)."""
    if form == "packed_lds":
        _abi.tuning_set("RLS_METRO_QG", 0)
    try:
        yield
    finally:
        _abi.tuning_unset("RLS_METRO_QG")


def to_form(form, x):
    """bool [N, C] -> the chains on the device in the form's layout."""
    if form == "f32":
        return dev(x.astype(np.float32))
    if form == "u8":
        return dev(x.astype(np.uint8))
    return PackedChains(dev(mo.pack(x)), x.shape[1])


def junk(form, N, C):
    """An output buffer whose every bit is wrong until the kernel writes it."""
    if form == "f32":
        return torch.full((N, C), 7.0, dtype=torch.float32, device=DEV)
    if form == "u8":
        return torch.full((N, C), 255, dtype=torch.uint8, device=DEV)
    return PackedChains(torch.full(((C + 63) // 64, N), -1, dtype=torch.int64, device=DEV), C)


def read(form, obj):
    """What the device holds: packed -> the words themselves (bits past C included), node-major -> bool, after checking 0 | 1."""
    if form.startswith("packed"):
        return obj.words.cpu().numpy().view(np.uint64)
    a = obj.cpu().numpy()
    assert ((a == 0) | (a == 1)).all(), "a node-major state holds something other than 0 and 1"
    return a != 0


def surface(form, x):
    """A Walker's, or a bool [N, C] state's, expected contents of read()."""
    if isinstance(x, mo.Walker):
        return x.words if form.startswith("packed") else x.x
    return mo.pack(x) if form.startswith("packed") else np.asarray(x, bool)


def same(got, exp, what):
    if not np.array_equal(got, exp):
        bad = np.argwhere(got != exp)
        raise AssertionError(f"{what}: {len(bad)} entries differ, first at {bad[0].tolist()}")


def rows_of(acc, rows):
    """accepts bool [T, C] -> what the kernels add into accepts [rows, T]: tile k (64 chains) adds into row k % rows."""
    T, C = acc.shape
    tiles = (C + 63) // 64
    pad = np.zeros((T, tiles * 64), np.int64)
    pad[:, :C] = acc
    per_tile = pad.reshape(T, tiles, 64).sum(axis=2)
    out = np.zeros((rows, T), np.int64)
    for k in range(tiles):
        out[k % rows] += per_tile[:, k]
    return out


def check_case(form, N, C, T, probs, start, index=None, u=None, seed=0, chain_ids=None, t_offset=0, rows=(1, 3, 7), accepts=True,
               prefixes=None):
    """One case through one form; index / u are indexed by the ABSOLUTE round (t_offset + T rows at least), None = production draws
    of (seed, chain_ids).  start is bool [N, C_in]; C_in < C is the packed broadcast (chain c starts from chain c % C_in)."""
    probs = np.asarray(probs, np.float32)
    given = index is not None
    if given:
        ix, uu = index[t_offset:t_offset + T], u[t_offset:t_offset + T]
        d_index, d_u = dev(index), dev(u)
    else:
        ix, uu = mo.production_draws(seed, mo.global_ids(C, chain_ids), t_offset, T, N)
        d_index = d_u = None
    assert ix.min() >= 0 and ix.max() < N
    c_in = start.shape[1]
    x0 = start[:, np.arange(C) % c_in]
    need = int(_abi.lib().rls_mcpg_metro_scratch_bytes(N, C))
    assert need > 0 or form != "packed_scratch", f"N = {N} does not take the scratch form"
    scratch = torch.full((need,), 0xA5, dtype=torch.uint8, device=DEV) if form.startswith("packed") and need > 0 else None
    d_probs, d_start, d_x0 = dev(probs), to_form(form, start), to_form(form, x0)
    exp_start, exp_x0 = surface(form, start), surface(form, x0)
    lim = torch.zeros(1, dtype=torch.int64, device=DEV)

    def run(samples, t_limit=None, write_back=True, acc=None, samples_in=None):
        mops.mcpg_metro_rounds(samples, d_probs, T, d_index, d_u, seed, t_limit, write_back, acc, t_offset=t_offset, samples_in=samples_in,
                               chain_ids=chain_ids, scratch=scratch)

    wk = mo.Walker(x0, probs)
    acc = np.zeros((T, C), bool)
    with windows(form):
        # (a) + (c) + (d): every prefix, out of place, into a buffer of wrong bits
        for tl in (-5, 0):
            out = junk(form, N, C)
            run(out, lim.fill_(tl), samples_in=d_start)
            same(read(form, out), exp_x0, f"t_limit = {tl}")
        for tp in range(1, T + 1):
            acc[tp - 1] = wk.step(ix[tp - 1], uu[tp - 1])
            if prefixes is not None and tp not in prefixes and tp != T:
                continue
            out = junk(form, N, C)
            run(out, lim.fill_(tp), samples_in=d_start)
            same(read(form, out), surface(form, wk), f"state after {tp} of {T} rounds")
        out = junk(form, N, C)
        run(out, lim.fill_(T + 9), samples_in=d_start)
        same(read(form, out), surface(form, wk), "t_limit past T")
        out = junk(form, N, C)
        run(out, None, samples_in=d_start)
        same(read(form, out), surface(form, wk), "no t_limit")
        same(read(form, d_start), exp_start, "the start state of an out-of-place launch")
        # in place, without counts
        s = d_x0.clone()
        run(s)
        same(read(form, s), surface(form, wk), "in place")
        if not accepts:
            return
        # (b) accept counts: row by row, added to what the buffer held, nothing at or past the limit; a dry pass writes no state
        for R in rows:
            fill = (np.arange(R * T, dtype=np.int64).reshape(R, T) * 7 + 3)
            for tl in (None, T - T // 3, 0):
                t_end = T if tl is None else tl
                exp = rows_of(acc, R) * (np.arange(T) < t_end)
                a = dev(fill)
                s = d_x0.clone()
                run(s, None if tl is None else lim.fill_(tl), write_back=False, acc=a)
                same(read(form, s), exp_x0, f"dry pass, rows = {R}, limit {tl}: the state")
                got = a.cpu().numpy() - fill
                assert np.array_equal(got, exp), f"dry pass, rows = {R}, limit {tl}: counts differ at {np.argwhere(got != exp)[:4].tolist()}"
            a = dev(fill)
            s = d_x0.clone()
            run(s, acc=a)
            same(read(form, s), surface(form, wk), f"direct pass with counts, rows = {R}")
            assert np.array_equal(a.cpu().numpy() - fill, rows_of(acc, R)), f"direct pass, rows = {R}: counts"
        a = torch.zeros(T, dtype=torch.int64, device=DEV)              # accepts [T]: one row
        s = d_x0.clone()
        run(s, acc=a)
        assert np.array_equal(a.cpu().numpy(), acc.sum(axis=1)) and np.array_equal(read(form, s), surface(form, wk))


# ------------------------------------------------------------------------------------------ cases
def spread(index, N):
    """Node ids 0 .. 9 -> the first five and the last five nodes of N."""
    return np.where(index < 5, index, N - 10 + index)


def big_case(N, n, T, C, seed):
    """pattern draws over min(n, 10) nodes, placed on the first and the last five nodes of an N-node state."""
    n = min(n, 10)
    index, u, p = mo.pattern_draws(n, T, C, seed)
    rng = np.random.RandomState(seed + 1)
    probs = (rng.rand(N) * 0.6 + 0.2).astype(np.float32)
    probs[spread(np.arange(n), N)] = p
    return spread(index, N), u, probs, rng.randint(0, 2, size=(N, C)).astype(bool)


def small_case(n, T, C, seed):
    index, u, probs = mo.pattern_draws(n, T, C, seed)
    return index, u, probs, np.random.RandomState(seed + 1).randint(0, 2, size=(n, C)).astype(bool)


def edge_draws(N, T, C, seed):
    """Two chains in three: pattern draws on the first / last five nodes; the third: uniform over all N nodes."""
    index, u, probs, start = big_case(N, 10, T, C, seed)
    anyn = np.random.RandomState(seed + 2).randint(0, N, size=(T, C))
    return np.where(np.arange(C) % 3 == 2, anyn, index).astype(np.int64), u, probs, start


def hazard_params():
    for form in FORMS:
        for n, T, C, seed in mo.HAZARDS:
            for N in (BIG_N if form == "packed_scratch" else (n,)):
                yield pytest.param(form, N, n, T, C, seed, id=f"{form}-N{N}-{n}x{T}x{C}")
    for n, T, C, seed in mo.HAZARDS[2:]:
        yield pytest.param("packed_lds", BIG_N[0], n, T, C, seed, id=f"packed_lds-N{BIG_N[0]}-{n}x{T}x{C}")


@pytest.mark.parametrize("form,N,n,T,C,seed", list(hazard_params()))
def test_hazards(form, N, n, T, C, seed):
    """Draws that revisit a node one and two rounds later, across blocks of eight, window edges and a ragged last window."""
    index, u, probs, start = small_case(n, T, C, seed) if N == n else big_case(N, n, T, C, seed)
    check_case(form, N, C, T, probs, start, index, u)


@pytest.mark.parametrize("T", [1, 7, 8, 9, 63, 64, 65, 127, 128, 129])
@pytest.mark.parametrize("form", FORMS)
def test_round_counts(form, T):
    """Launch lengths around the walker's block of 8 and window of 64 rounds, five nodes."""
    N = BIG_N[0] if form == "packed_scratch" else 5
    index, u, probs, start = small_case(5, T, 70, T) if N == 5 else big_case(N, 5, T, 70, T)
    check_case(form, N, 70, T, probs, start, index, u, rows=(1, 3))


P_EDGES = np.array([0.0, 1.0, 0.5, 1e-8, 1 - 6e-8, 0.25], np.float32)


@pytest.mark.parametrize("form", FORMS)
def test_probs_edges(form):
    """p in {0, 1, 1/2, 1e-8, 1 - 2^-24, 1/4}: q = 0 gives rate inf (accept), q = 1 gives 0 (reject), as numpy's float32 does; u is
    exactly the float32 rate of the chain's current state (a reject: the test is <), one ulp below (an accept), or random."""
    N, C, T = (BIG_N[0] if form == "packed_scratch" else 6), 70, 96
    nodes = np.arange(6) if N == 6 else spread(np.array([0, 1, 2, 7, 8, 9]), N)
    rng = np.random.RandomState(6)
    probs = (rng.rand(N) * 0.6 + 0.2).astype(np.float32)
    probs[nodes] = P_EDGES
    start = rng.randint(0, 2, size=(N, C)).astype(bool)
    index = nodes[rng.randint(0, 6, size=(T, C))].astype(np.int64)
    u = np.empty((T, C), np.float32)
    wk, col = mo.Walker(start, probs), np.arange(C)
    seen = set()
    for t in range(T):
        val = wk.x[index[t], col]
        rate = mo.accept_rate(np.where(val, probs[index[t]], np.float32(1) - probs[index[t]]))
        below = np.nextafter(rate, np.float32(-1)).astype(np.float32)
        kind = (col + t) % 3
        one = np.nextafter(np.float32(1), np.float32(0))
        ut = np.where(kind == 0, np.minimum(rate, np.float32(1)), np.where(kind == 1, np.clip(below, np.float32(0), one), rng.rand(C)))
        u[t] = ut.astype(np.float32)
        acc = wk.step(index[t], u[t])
        seen |= set(zip(rate[kind < 2].tolist(), kind[kind < 2].tolist(), acc[kind < 2].tolist()))
    rates = {r for r, _, _ in seen}
    assert float("inf") in rates and 0.0 in rates and 1.0 in rates and 3.0 in rates            # p = 0 | 1, 1/2, 1/4 were all met
    assert all(a == (k == 1 and r > 0) for r, k, a in seen if r <= 1)                            # at the rate: reject; an ulp below: accept
    check_case(form, N, C, T, probs, start, index, u)


@pytest.mark.parametrize("kind", ["given", "hash"])
@pytest.mark.parametrize("N", [6143, 6144, 6145, 10240, 10241, 16384, 16385, 20479, 20480])
def test_packed_lds_limits(N, kind):
    """Both sides of every N at which the packed launcher changes form (and an odd N: the tile moves by 8-byte words)."""
    C, T = 70, 130
    index, u, probs, start = edge_draws(N, T, C, N)
    form = "packed_scratch" if 6145 <= N <= 10240 or N >= 16385 else "packed_lds"
    assert (_abi.lib().rls_mcpg_metro_scratch_bytes(N, C) > 0) == (form == "packed_scratch")
    if kind == "given":
        check_case(form, N, C, T, probs, start, index, u)
    else:
        check_case(form, N, C, T, probs, start, seed=N)
    if form == "packed_scratch" and N <= 10240:                      # the size allows both forms: the same bits from either
        check_case("packed_lds", N, C, T, probs, start, *((index, u) if kind == "given" else (None, None)), seed=N, rows=(3,),
                   prefixes=(1, 2, 3, 64, 65, 66))


def refused(call):
    with pytest.raises(RuntimeError, match=r"failed \(-2\)"):       # RLS_EUNSUPPORTED, a host check before any launch
        call()


def test_packed_refusals():
    for N, knob in ((20481, None), (16385, 0)):
        index, u, probs, start = edge_draws(N, 4, 70, 1)
        s, before = to_form("packed_lds", start), mo.pack(start)
        with windows("packed_lds" if knob == 0 else "packed_scratch"):
            refused(lambda: mops.mcpg_metro_rounds(s, dev(probs), 4, dev(index), dev(u)))
            refused(lambda: mops.mcpg_metro_rounds(s, dev(probs), 4, seed=3))
        assert np.array_equal(read("packed_lds", s), before)
    assert mops.mcpg_metro_max_rounds(20481, 0) == 0 and mops.mcpg_metro_max_rounds(16385, 0) == 0


@pytest.mark.parametrize("form", ["f32", "u8"])
@pytest.mark.parametrize("N,T,accepts", [(13652, 130, False), (13653, 130, False), (13652, 100, True), (20477, 2, True),
                                         (20478, 130, False)])
def test_nodemajor_lds_limits(form, N, T, accepts):
    """12 N + 16 <= 160 KB keeps probs in LDS (N <= 13652); T counts beside them push probs out; 8 N + 4 T + 16 is the hard limit."""
    C = 70
    want_form = {(13652, False): "true", (13653, False): "false", (13652, True): "false", (20477, True): "false", (20478, False): "false"}
    assert kernel_form(form, N, T, True, accepts).endswith(f"PROBS_LDS={want_form[N, accepts]}>")
    index, u, probs, start = edge_draws(N, T, C, N + T)
    check_case(form, N, C, T, probs, start, index, u, accepts=accepts, rows=(1, 3), prefixes=(1, 2, 63, 64, 65, 99, 100, 129))
    check_case(form, N, C, T, probs, start, seed=N, accepts=accepts, rows=(3,), prefixes=(1, 64, 65))


@pytest.mark.parametrize("form", ["f32", "u8"])
def test_nodemajor_refusals(form):
    C = 70
    for N, T, with_acc in ((20477, 3, True), (20479, 2, False)):
        index, u, probs, start = edge_draws(N, T, C, 2)
        s = to_form(form, start)
        a = torch.zeros((1, T), dtype=torch.int64, device=DEV) if with_acc else None
        refused(lambda: mops.mcpg_metro_rounds(s, dev(probs), T, dev(index), dev(u), accepts=a))
        refused(lambda: mops.mcpg_metro_rounds(s, dev(probs), T, seed=1, accepts=a))
        assert np.array_equal(read(form, s), start) and (a is None or int(a.abs().sum()) == 0)
    assert mops.mcpg_metro_max_rounds(20477, 4) == 2 and mops.mcpg_metro_max_rounds(20478, 1) == 0


@pytest.mark.parametrize("C", [1, 63, 64, 65, 130])
@pytest.mark.parametrize("form", FORMS)
def test_chain_counts(form, C):
    N, T = (BIG_N[0] if form == "packed_scratch" else 37), 70
    index, u, probs, start = small_case(N, T, C, C) if N == 37 else big_case(N, 10, T, C, C)
    check_case(form, N, C, T, probs, start, index, u)
    check_case(form, N, C, T, probs, start, seed=C, rows=(2,), prefixes=(1, 2, 64, 65))


@pytest.mark.parametrize("kind", ["given", "hash"])
@pytest.mark.parametrize("form", ["packed_lds", "packed_scratch"])
def test_packed_broadcast_start(form, kind):
    """C_in = 64 -> C = 192: chain c starts from chain c % 64 of a start state that is not materialised."""
    N, T, C = (BIG_N[0] if form == "packed_scratch" else 37), 70, 192
    index, u, probs, _ = small_case(N, T, C, 11) if N == 37 else big_case(N, 10, T, C, 11)
    start = np.random.RandomState(12).randint(0, 2, size=(N, 64)).astype(bool)
    if kind == "given":
        check_case(form, N, C, T, probs, start, index, u)
    else:
        check_case(form, N, C, T, probs, start, seed=5)


@pytest.mark.parametrize("kind", ["given", "hash"])
@pytest.mark.parametrize("t_offset", [0, 64, 100])
@pytest.mark.parametrize("form", FORMS)
def test_round_offset(form, t_offset, kind):
    """Draws are indexed by the absolute round: a launch that starts at t_offset reads rows t_offset .. of index / u, or hashes them."""
    N, T, C = (BIG_N[0] if form == "packed_scratch" else 23), 66, 70
    index, u, probs, start = small_case(N, t_offset + T, C, 7) if N == 23 else big_case(N, 10, t_offset + T, C, 7)
    if kind == "given":
        check_case(form, N, C, T, probs, start, index, u, t_offset=t_offset, rows=(3,))
    else:
        check_case(form, N, C, T, probs, start, seed=99, t_offset=t_offset, rows=(3,))


@pytest.mark.parametrize("seed,chain_ids,C", [(0, None, 130), (77, None, 130), (2 ** 32 + 5, None, 130), (2 ** 63 + 1, None, 130),
                                              (77, (2 ** 32 + 64, 0, 0), 130), (2 ** 63 + 1, (2 ** 32 + 64, 64, 192), 128)],
                         ids=["seed0", "seed77", "seed2p32", "seed2p63", "chain2p32", "grid2d"])
@pytest.mark.parametrize("form", FORMS)
def test_production_draws(form, seed, chain_ids, C):
    """The counter hash (seed halves, global chain id halves, absolute round) restated in numpy; the last case is the two-
    dimensional launch of a shard: period = 64, skip = 192."""
    N, T = (BIG_N[1] if form == "packed_scratch" else 300), 70
    rng = np.random.RandomState(C)
    probs = (rng.rand(N) * 0.6 + 0.2).astype(np.float32)
    start = rng.randint(0, 2, size=(N, C)).astype(bool)
    check_case(form, N, C, T, probs, start, seed=seed, chain_ids=chain_ids, t_offset=3)


EIGHT = [("f32", 300, True, True), ("f32", 13653, True, False), ("u8", 300, False, True), ("u8", 13653, False, False),
         ("packed_lds", 300, True, None), ("packed_lds", 300, False, None), ("packed_scratch", 10240, True, None),
         ("packed_scratch", 10240, False, None)]


@pytest.mark.parametrize("form,N,given,probs_lds", EIGHT, ids=[kernel_form(f, n, 40, g, False) for f, n, g, _ in EIGHT])
def test_each_kernel_form(form, N, given, probs_lds):
    """The eight instances by name, each at a size that reaches it; where two layouts hold the same chains, the same bits."""
    C, T = 130, 40
    index, u, probs, start = edge_draws(N, T, C, 8)
    if probs_lds is not None:
        assert (12 * N + 16 <= LDS_BYTES) == probs_lds
    draws = (index, u) if given else (None, None)
    check_case(form, N, C, T, probs, start, *draws, seed=21, rows=(3,))
    if form != "f32":                                                 # against the f32 node-major kernel directly
        a, b = to_form("f32", start), to_form(form, start)
        d = [None if v is None else dev(v) for v in draws]
        mops.mcpg_metro_rounds(a, dev(probs), T, *d, seed=21)
        mops.mcpg_metro_rounds(b, dev(probs), T, *d, seed=21)
        same(read(form, b), surface(form, read("f32", a)), "against the f32 node-major kernel")


# ------------------------------------------------------------------------------------------ the stop kernel alone
@pytest.mark.parametrize("rows", [1, 3, 64])
@pytest.mark.parametrize("T", [1, 63, 64, 65, 1024, 4096, 4097, 5000])
def test_stop_kernel(T, rows):
    """rls_mcpg_metro_stop against metro_oracle.stop: the stop round at round 0, at lanes 63 / 64, on both sides of the seam between
    two waves' runs, at T - 1, one accept short of ever, never; counts up to 2^33 per round; every `first`, live and dead ctl."""
    rng = np.random.RandomState(T * 100 + rows)
    blocks = (T + 63) // 64
    per = (blocks + 15) // 16                                         # blocks of 64 rounds per wave (16 waves)
    places = {0, 63, 64, T - 1} | {per * 64 * w + d for w in (1, 2, 15) for d in (-1, 0)}
    places = sorted(p for p in places if 0 <= p < T)
    cases, outs = [], []
    for big in (False, True):
        col = rng.randint(0, 2 ** 33 + 1, size=T).astype(np.int64) if big else rng.randint(0, 4, size=T).astype(np.int64)
        col[rng.rand(T) < 0.3] = 0
        col[places] = np.maximum(col[places], 1)                      # an accept at the round the target is reached at
        owner = rng.randint(0, rows, size=T)
        acc = np.zeros((rows, T), np.int64)
        acc[owner, np.arange(T)] = col - col // 2
        acc[(owner + 1) % rows, np.arange(T)] += col // 2
        assert np.array_equal(acc.sum(axis=0), col)
        d_acc = dev(acc)
        run = np.cumsum(col)
        for first in (0, 1, 2):
            for ctl in ([0, 1, T], [12345, 1, T], [7, 1, max(T // 2, 1)], [99, 0, 0]):
                before = 0 if first == 1 else ctl[0]
                targets = [before + int(run[p]) for p in places] + [before + int(run[-1]) + 1, 2 ** 62, 0]
                for target in targets:
                    for with_limit in (True, False):
                        cases.append((acc, target, first, ctl, with_limit))
                        io = torch.tensor(ctl + [-77], dtype=torch.int64, device=DEV)
                        mops.mcpg_metro_stop(d_acc, target, first, 17, io[:3], io[3:] if with_limit else None)
                        outs.append(io)
    got = torch.stack(outs).cpu().numpy()
    for (acc, target, first, ctl, with_limit), g in zip(cases, got):
        ctl2, lim = mo.stop(acc, target, first, 17, ctl)
        assert g[:3].tolist() == ctl2 and int(g[3]) == (lim if with_limit else -77), \
            f"target {target} first {first} ctl {ctl}: got {g.tolist()}, want {ctl2} limit {lim}"


# ------------------------------------------------------------------------------------------ the stop rule end to end
def _chosen_accepts(N, T, C, stop_round, seed):
    """probs = 1/2 (rate exactly 1) and u in {0, 1}: the accept matrix is the test's.  Every proposal of rounds 0 .. T - 2 is
    accepted, round T - 1 is one short of the target C * T, the missing accept comes in round stop_round - 1 (1-based stop_round;
    None: never), and every round after it accepts everything again -- a walk that runs on changes the state."""
    rng = np.random.RandomState(seed)
    A = np.ones((5 * T, C), bool)
    if stop_round != T:
        A[T - 1, rng.randint(C)] = False
        last = 5 * T if stop_round is None else stop_round - 1
        A[T:last] = False
        if stop_round is not None:
            A[last] = False
            A[last, rng.randint(C)] = True
    index = rng.randint(0, N, size=(5 * T, C)).astype(np.int64)
    u = np.where(A, np.float32(0), np.float32(1)).astype(np.float32)
    return np.full(N, 0.5, np.float32), rng.randint(0, 2, size=(N, C)).astype(np.float32), index, u


@pytest.mark.parametrize("where", ["at_T", "first_of_chunk", "last_of_chunk", "at_5T", "never"])
@pytest.mark.parametrize("surface", ["packed", "nodemajor"])
def test_stop_rule_end_to_end(surface, where):
    N, T, C = 50, 7, 130
    stop_round = {"at_T": T, "first_of_chunk": 2 * T + 1, "last_of_chunk": 4 * T, "at_5T": 5 * T, "never": None}[where]
    probs, start, index, u = _chosen_accepts(N, T, C, stop_round, seed=T)
    want_x, t_used = onp.metro_sampling(probs, start, T, index, u)
    assert t_used == (5 * T if stop_round is None else stop_round)
    if surface == "packed":
        got = amcpg.metro_sampling_packed(dev(probs), PackedChains.pack(dev(start)), T, index=dev(index), u=dev(u)).unpack()
    else:
        got = amcpg._metro_sampling_nodemajor(dev(probs), dev(start), T, DEV, dev(index), dev(u))
    assert np.array_equal(got.cpu().numpy(), want_x)
