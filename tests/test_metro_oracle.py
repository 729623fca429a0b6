"""tests/metro_oracle.py against oracle_np.metro_sampling (the reference's own loop), the hash's known values, and the proof that
the pattern draws of tests/test_gpu_metro_forms.py can tell a walker with a missing look-ahead repair from a correct one.  CPU only;
the two size queries are host logic of the library."""
import numpy as np
import pytest

from oracle import oracle_np as onp
from tests import metro_oracle as mo

HAZARDS = mo.HAZARDS        # (N, T, C, seed): the hazard cases tests/test_gpu_metro_forms.py runs on every form


def _draws_that_stop(N, T, C, seed):
    rng = np.random.RandomState(seed)
    probs = (rng.rand(N) * 0.6 + 0.2).astype(np.float32)
    start = rng.randint(0, 2, size=(N, C)).astype(np.float32)
    index = rng.randint(0, N, size=(5 * T, C)).astype(np.int64)
    u = rng.rand(5 * T, C).astype(np.float32)
    return probs, start, index, u


@pytest.mark.parametrize("N,T,C", [(300, 30, 192), (64, 6, 70), (1001, 100, 337), (12, 1, 64)])
def test_chunked_launches_with_stop_equal_the_reference_loop(N, T, C):
    probs, start, index, u = _draws_that_stop(N, T, C, seed=N + C)
    want, t_used = onp.metro_sampling(probs, start, T, index, u)
    assert T < t_used < 5 * T, "the draws must make the stop rule fire inside T .. 5T"
    for chunk in sorted({T, T // 3 + 1, 1}):
        got, used = mo.walk_chunks(probs, start, T, index, u, chunk)
        assert used == t_used, (chunk, used, t_used)
        assert np.array_equal(got, want.astype(bool)), chunk


def test_launch_trace_and_limits():
    probs, start, index, u = _draws_that_stop(40, 4, 70, seed=1)
    states, acc = mo.launch(start, probs, index, u)
    assert states.shape == (21, 40, 70) and acc.shape == (20, 70)
    assert np.array_equal(states[0], start.astype(bool))
    for lim in (-3, 0, 1, 7, 20, 25):
        s2, a2 = mo.launch(start, probs, index, u, t_limit=lim)
        k = min(max(lim, 0), 20)
        assert np.array_equal(s2[:k + 1], states[:k + 1]) and np.array_equal(s2[-1], states[k])
        assert np.array_equal(a2[:k], acc[:k]) and not a2[k:].any()
    # a round changes exactly the accepted (node, chain) pairs
    for t in range(20):
        changed = np.argwhere(states[t] != states[t + 1])
        want = np.stack([index[t][acc[t]], np.nonzero(acc[t])[0]], axis=1)
        assert sorted(map(tuple, changed)) == sorted(map(tuple, want))
    wk = mo.Walker(start, probs)
    for t in range(20):
        wk.step(index[t], u[t])
        assert np.array_equal(wk.words, mo.pack(states[t + 1]))


def test_accept_rate_edges_are_ieee():
    r = mo.accept_rate(np.array([0.0, 1.0, 0.5, 0.25], np.float32))
    assert np.isinf(r[0]) and r[0] > 0 and r[1] == 0 and r[2] == 1 and r[3] == 3 and r.dtype == np.float32


def test_hash_known_values_and_ranges():
    assert int(mo.fmix(0)) == 0 and int(mo.fmix(1)) == 0x514E28B7      # murmur3 fmix32
    assert int(mo.fmix(0xFFFFFFFF)) == 0x81F16F39
    for seed in (0, 77, 2 ** 32 + 5, 2 ** 63 + 1):
        gids = mo.global_ids(128, (2 ** 32 + 64, 64, 192))
        index, u = mo.production_draws(seed, gids, 100, 50, 7)
        assert index.dtype == np.int64 and u.dtype == np.float32
        assert index.min() >= 0 and index.max() < 7 and u.min() >= 0 and u.max() < 1
    assert mo.global_ids(130, None).tolist() == list(range(130))
    assert mo.global_ids(128, (5, 64, 192))[[0, 63, 64, 127]].tolist() == [5, 68, 261, 324]
    # every part of the key matters: seed halves, chain id halves, the round
    base = mo.production_draws(77, [3], 0, 64, 1 << 20)[0]
    for seed, gid, t0 in ((77 + 2 ** 32, 3, 0), (78, 3, 0), (77, 3 + 2 ** 32, 0), (77, 4, 0), (77, 3, 1)):
        assert not np.array_equal(mo.production_draws(seed, [gid], t0, 64, 1 << 20)[0], base)
    # rounds are absolute: a later launch continues the stream
    a = mo.production_draws(9, np.arange(70), 0, 100, 300)
    b = mo.production_draws(9, np.arange(70), 64, 36, 300)
    assert np.array_equal(a[0][64:], b[0]) and np.array_equal(a[1][64:], b[1])


def test_stop_rule_restated():
    acc = np.array([[1, 0, 2, 0], [0, 0, 1, 5]])                          # column sums 1 0 3 5
    assert mo.stop(acc, 4, 1, 9, [99, 0, 0]) == ([9, 0, 0], 4)            # first chunk: hit by the total, applied whole
    assert mo.stop(acc, 10, 1, 9, [99, 0, 0]) == ([9, 1, 9], 4)
    assert mo.stop(acc, 4, 0, 9, [0, 1, 4]) == ([9, 0, 0], 3)             # dry pass: stop after round 2 (1-based 3)
    assert mo.stop(acc, 4, 0, 9, [0, 1, 2]) == ([9, 0, 0], 2)             # the chunk's own limit is lower
    assert mo.stop(acc, 13, 0, 9, [3, 1, 4]) == ([12, 1, 9], 4)           # one short: never
    assert mo.stop(acc, 12, 0, 9, [3, 1, 4]) == ([12, 0, 0], 4)           # reached at the last round
    assert mo.stop(acc, 3, 0, 9, [3, 0, 0]) == ([12, 0, 0], 0)            # dead walk: limit 0
    assert mo.stop(acc, 4, 2, 9, [3, 1, 4]) == ([12, 0, 0], 4)            # first = 2: applied directly, ctl read


def test_pattern_draws_follow_their_patterns():
    index, u, probs = mo.pattern_draws(300, 24, 18, seed=4)
    assert index.shape == (24, 18) and u.dtype == np.float32 and probs.dtype == np.float32
    assert 0 <= u.min() and u.max() < 1 and 0.2 <= probs.min() and probs.max() <= 0.8
    for c in range(18):
        col, a = index[:, c], index[0, c]
        b = {0: a, 1: col[1], 2: col[2], 3: col[2]}.get(c % 6)
        if c % 6 < 4:
            assert b == a if c % 6 == 0 else b != a
            want = {0: [a] * 24, 1: [a, b] * 12, 2: [a, a, b] * 8, 3: [a, a, b, b] * 6}[c % 6]
            assert col.tolist() == want
        elif c % 6 == 4:
            assert col.max() < 3
    assert (mo.pattern_draws(1, 70, 64, seed=0)[0] == 0).all()


@pytest.mark.parametrize("N,T,C,seed", HAZARDS + [(5, T, 64, T) for T in (1, 7, 8, 9, 63, 64, 65, 127, 128, 129)])
def test_read_order_model_without_drops_is_the_walk(N, T, C, seed):
    index, u, probs = mo.pattern_draws(N, T, C, seed)
    start = np.random.RandomState(T).randint(0, 2, size=(N, C)).astype(bool)
    assert np.array_equal(mo.stale_walk(start, probs, index, u), mo.launch(start, probs, index, u)[1])


@pytest.mark.parametrize("drop", mo.DROPS)
@pytest.mark.parametrize("N,T,C,seed", [h for h in HAZARDS if h[1] >= 66])
def test_pattern_draws_separate_every_missing_repair(N, T, C, seed, drop):
    """At least one chain in eight takes a different verdict somewhere when one repair is missing: the GPU cases built from these
    draws can see such a walker.  (Uniform node picks at the suite's older shapes separate zero to a dozen chains.)"""
    index, u, probs = mo.pattern_draws(N, T, C, seed)
    start = np.random.RandomState(T).randint(0, 2, size=(N, C)).astype(bool)
    good = mo.launch(start, probs, index, u)[1]
    bad = mo.stale_walk(start, probs, index, u, drop)
    differ = int((good != bad).any(axis=0).sum())
    print(f"pattern draws ({N}, {T}, {C}) without '{drop}': {differ} of {C} chains differ")
    assert differ * 8 >= C


# ---- the launcher's size queries (host logic: nothing is launched)
def test_scratch_query_bands():
    from rlsolver_amd import _abi
    q = _abi.lib().rls_mcpg_metro_scratch_bytes
    for N in (6143, 6144, 10241, 16383, 16384, 20481):
        assert q(N, 64) == 0, N
    for N in (6145, 10239, 10240, 16385, 20479, 20480):
        assert q(N, 64) == 32768, N
    for C in (65, 130):
        assert q(6145, C) == -(-C // 64) * 32768 and q(20480, C) == -(-C // 64) * 32768


def test_max_rounds_query_limits():
    from rlsolver_amd import _abi
    q = _abi.lib().rls_mcpg_metro_max_rounds
    assert q(20477, 4) == 2 and q(20478, 4) == 0
    assert q(20477, 1) == 2 and q(20478, 1) == 0
    assert q(16384, 0) > 0 and q(16385, 0) == 0
