"""Every form of every TSP entry point against the numpy oracles, at the smallest size at which the form exists, on asymmetric
matrices and on inputs whose moves are rejected (tests/tsp_cases.py).  Each case first asserts, through rls_tsp_launch_form --
the launchers' own planner --, the form it means to reach; the closing test checks that every reachable (entry point, form)
pair was run.  Discrete outputs (indices, ban, tours, perms, best pairs) and the exact 2-opt values are compared exactly; K13's
logratio by the project's rule (rtol 1e-5, atol 1e-5 max tour length / T).

log_acc: the existing rule, rtol 2e-5 / atol 1e-4, unwidened.  Measured on the CPU, float32 oracle against the same oracle in
float64 on exactly these inputs (tools/tsp_tolerance_ratio.py; tests/test_tsp_cases.py re-measures):

    case            N     T       largest gap   twice the gap   bound at the case's largest |log_acc|
    n3_all_banned   3     0.5     4.6e-2        9.2e-2          60      (log_acc = -3e6: rtol)
    n4_k1, n4_k2    4     0.5     1.9e-1        3.7e-1          80      (log_acc = -4e6: rtol)
    n65 / _prod     65    0.35    2.2e-6        4.3e-6          1.7e-4
    n65_asym        65    1.0     1.3e-6        2.5e-6          1.2e-4
    n193            193   0.08    9.6e-7        2.0e-6          2.1e-4
    n194 / _prod    194   0.08    1.6e-6        3.1e-6          1.7e-4
    n194_asym       194   1.0     1.7e-6        3.4e-6          1.1e-4
    n2561           2561  0.0015  1.8e-6        3.5e-6          1.7e-4
    n5121           5121  0.0005  8.2e-7        1.7e-6          1.5e-4

Twice the gap lies inside the existing rule on every env, so no case needed a wider bound.  No env of any case has a Gumbel
argmax decided within the rule (the rows that may be left out of the exact `cur` comparison, 3 % at most): all are compared.
"""
import numpy as np
import pytest
import torch

from oracle import oracle_np as onp
from rlsolver_amd import _abi
from rlsolver_amd import ops_mcpg_tsp as mops
from rlsolver_amd.ops import _ptr, _s64, _stream, _t
from tests import tsp_cases as tc
from tests.gpu_util import DEV

pytestmark = pytest.mark.gpu

RAN = set()            # (entry point, form) pairs that ran with their form asserted
CANARY = 0x5A5A5A5A5A5A5A5A

# every reachable (entry point, form).  K13: (drawn, lds_d, tab8, block) -- k_tsp_swap_delta_all<false, true, true> is compiled
# but never launched (tab8 implies lds_d: tests/test_tsp_cases.py), so it is not listed.
REACHABLE = {
    ("tsp_tour_length", 1), ("tsp_tour_length", 0),
    ("tsp_swap_delta_all", 1, 1, 1, 1024), ("tsp_swap_delta_all", 1, 1, 0, 1024), ("tsp_swap_delta_all", 1, 0, 0, 1024),
    ("tsp_swap_delta_all", 1, 0, 0, 256), ("tsp_swap_delta_all", 0, 1, 0, 1024), ("tsp_swap_delta_all", 0, 0, 0, 1024),
    ("tsp_swap_delta_all", 0, 0, 0, 256),
    ("tsp_apply_swap",), ("tsp_2opt_delta",),
    ("tsp_2opt_best", "delta", "one slice"), ("tsp_2opt_best", "delta", "slices"),
    ("tsp_2opt_best", "exact", "one slice"), ("tsp_2opt_best", "exact", "slices"),
    ("rand_perms", "lds", "16-byte stores"), ("rand_perms", "lds", "rows"), ("rand_perms", "global"),
    ("isco_tsp_step", 1, 4), ("isco_tsp_step", 0, 4), ("isco_tsp_step", 0, 2), ("isco_tsp_step", 0, 1),
}


def dev(a, dtype=None):
    a = np.ascontiguousarray(a)
    t = torch.from_numpy(a if a.flags.writeable else a.copy()).to(DEV)       # (the shared instances are read-only)
    return t.to(dtype) if dtype is not None else t


def reach(what, N, K=0, tab8=False, **want):
    """assert the form a launch at these sizes takes, before making it"""
    f = _abi.tsp_launch_form(what, N, K, tab8)
    assert f.supported == 1
    got = {k: getattr(f, k) for k in want}
    assert got == want, (what, N, K, tab8, got, want)
    return f


def perms_np(rng, B, N):
    return np.stack([rng.permutation(N) for _ in range(B)]).astype(np.int64)


def forced_partners(rng, pn):
    """partner cities with the placements that matter forced by construction: env 0 two positions ahead (c3), env 1 two behind
    (the partner's successor is the position's predecessor), env 2 / 3 adjacent (banned), env 4 all of them in turn, the rest
    anywhere but the position itself"""
    B, N = pn.shape
    off = rng.randint(1, N, size=(B, N))
    for b, o in enumerate((2 % N, (N - 2) % N, 1, N - 1)):
        if b < B and o:
            off[b] = o
    if B > 4 and N > 4:
        off[4] = np.resize([2, N - 2, 1, N - 1, 3], N)
    return np.take_along_axis(pn, (np.arange(N)[None, :] + off) % N, axis=1)


# ------------------------------------------------------------------------------------------------ K12
@pytest.mark.parametrize("N,lds_d", [(1, 1), (2, 1), (3, 1), (63, 1), (64, 1), (65, 1), (201, 1), (202, 0)])
def test_tour_length_forms(N, lds_d):
    """K12 on an asymmetric matrix with a non-zero diagonal (N = 1: the tour's one edge IS the diagonal), B on both sides of the
    four tours a wave takes per trip and one past a full grid trip of a workgroup."""
    f = reach(_abi.TSP_TOUR_LENGTH, N, lds_d=lds_d, block=1024)
    rng = np.random.RandomState(N)
    dist = (rng.rand(N, N) + 0.1).astype(np.float32)
    d = dev(dist)
    for B in (1, 2, 3, 5, 4 * f.waves + 1):
        pn = perms_np(rng, B, N)
        got = mops.tsp_tour_length(d, dev(pn)).cpu().numpy()
        np.testing.assert_allclose(got, onp.tsp_tour_length_f64(dist, pn), rtol=1e-5, atol=0)
    RAN.add(("tsp_tour_length", lds_d))


# ------------------------------------------------------------------------------------------------ K13
def _check_k13(dist, pn, sel, T, got, what):
    lr_w, idx_w, ban_w = onp.tsp_swap_delta_all(dist, pn, sel, T)
    lr, idx, ban = (g.cpu().numpy() for g in got)
    assert np.array_equal(idx, idx_w) and np.array_equal(ban, ban_w), what
    scale = onp.tsp_tour_length_f64(dist, pn).max() / T
    np.testing.assert_allclose(lr, lr_w, rtol=1e-5, atol=1e-5 * scale, err_msg=what)
    return idx_w, ban_w


@pytest.mark.parametrize("N,lds_d,tab8,block", [(168, 1, 1, 1024), (169, 1, 0, 1024), (186, 1, 0, 1024), (187, 0, 0, 1024),
                                                (256, 0, 0, 1024), (257, 0, 0, 256)])
def test_swap_delta_forms(N, lds_d, tab8, block):
    """K13 on an asymmetric matrix: recorded partners with every placement forced; then drawn in the kernel at K = 1, 20, N - 2
    from the int32 tables and from the byte tables -- the drawn cities are the numpy restatement's, the outputs the oracle's."""
    from rlsolver_amd.graph import generate_tsp_coords, tsp_tables
    rng = np.random.RandomState(N)
    B, T = 37, 0.5
    coords = generate_tsp_coords(N, seed=N)
    sym = tsp_tables(coords, K=1)[0]
    dist = tc.asym(sym, rng)
    d = dev(dist)
    pn = perms_np(rng, B, N)
    perms = dev(pn)
    # recorded partners
    reach(_abi.TSP_SWAP_DELTA, N, lds_d=lds_d, tab8=0, block=block)
    sel = forced_partners(rng, pn)
    idx_w, ban_w = _check_k13(dist, pn, sel, T, mops.tsp_swap_delta_all(d, perms, dev(sel), T), "recorded")
    assert (idx_w[0] == (np.arange(N) + 2) % N).all() and not ban_w[:2].any() and ban_w[2:4].all()
    RAN.add(("tsp_swap_delta_all", 0, lds_d, 0, block))
    # drawn in the kernel
    seed, off = 0x1234567ABCDEF, (1 << 32) + 7000
    env = (np.arange(B, dtype=np.uint64) + np.uint64(off))[:, None]
    pos = np.arange(N, dtype=np.uint64)[None, :]
    for K in (1, 20, N - 2):
        _, near, rnd = tsp_tables(coords, K=K)
        near32, rnd32 = dev(near.astype(np.int32)), dev(rnd.astype(np.int32))
        thr = float(np.float32(K / (K + 1)))
        up = tc.unit_np(tc.isco_draw_np(seed, env, pos, 0, 3))
        rn = ((tc.isco_draw_np(seed, env, pos, 0, 4) * np.uint64(K)) >> np.uint64(32)).astype(np.int64)
        rr = ((tc.isco_draw_np(seed, env, pos, 0, 5) * np.uint64(N - K - 1)) >> np.uint64(32)).astype(np.int64)
        want = np.where(up < np.float32(thr), near[pn, rn], rnd[pn, rr])
        t8 = mops.tsp_tables8(near32, rnd32)
        assert (t8 is None) == (N > 256)
        outs = []
        for tables8 in ((None, t8) if t8 is not None else (None,)):
            f = reach(_abi.TSP_SWAP_DELTA, N, K, tables8 is not None, lds_d=lds_d, block=block)
            if K == 20:
                assert f.tab8 == (tab8 if tables8 is not None else 0)
            lr, idx, ban, s = mops.tsp_swap_delta_all(d, perms, None, T, nearest=near32, random=rnd32, near_threshold=thr, seed=seed,
                                                      env_offset=off, return_selected=True, tables8=tables8)
            assert np.array_equal(s.cpu().numpy(), want), (K, tables8 is not None)
            _check_k13(dist, pn, want, T, (lr, idx, ban), f"drawn K={K} tables8={tables8 is not None}")
            outs.append((lr, idx, ban))
            RAN.add(("tsp_swap_delta_all", 1, f.lds_d, f.tab8, f.block))
        assert all(torch.equal(a, b) for a, b in zip(outs[0], outs[-1]))


def test_swap_delta_at_its_size_limit():
    """N = 5088: the last size whose per-wave scratch fits (recorded partners, matrix in global memory, 4 waves); N = 5089 is
    refused before any launch."""
    N, B, T = 5088, 5, 0.5
    reach(_abi.TSP_SWAP_DELTA, N, lds_d=0, tab8=0, block=256, lds_bytes=32 * N)
    rng = np.random.RandomState(N)
    dist = (rng.rand(N, N).astype(np.float32) + np.float32(0.1))
    pn = perms_np(rng, B, N)
    sel = forced_partners(rng, pn)
    _check_k13(dist, pn, sel, T, mops.tsp_swap_delta_all(dev(dist), dev(pn), dev(sel), T), "N=5088")
    RAN.add(("tsp_swap_delta_all", 0, 0, 0, 256))
    N = 5089
    assert _abi.tsp_launch_form(_abi.TSP_SWAP_DELTA, N).supported == 0
    pn = perms_np(rng, 2, N)
    d0 = torch.zeros((N, N), dtype=torch.float32, device=DEV)
    with pytest.raises(RuntimeError, match="too large"):
        mops.tsp_swap_delta_all(d0, dev(pn), dev(np.roll(pn, 1, axis=1)), T)
    lr = torch.full((2, N), 7.0, device=DEV)
    idx = torch.full((2, N), CANARY, dtype=torch.int64, device=DEV)
    ban = torch.zeros((2, N), dtype=torch.uint8, device=DEV)
    sel = dev(np.roll(pn, 1, axis=1))
    with pytest.raises(_abi.RlsError) as e:
        _abi.call("rls_tsp_swap_delta_all", _ptr(d0), N, _ptr(dev(pn)), 2, _ptr(sel), None, 0, None, 0, None, 0.0, 0, 0, None, T, _ptr(lr),
                  _ptr(idx), _ptr(ban), _stream(DEV))
    assert e.value.code == -2
    torch.cuda.synchronize()
    assert bool((lr == 7.0).all()) and bool((idx == CANARY).all())          # nothing ran


def test_swap_delta_refuses_a_draw_without_a_far_table():
    """selected == NULL with K = N - 1: the far draw's range N - K - 1 is empty (the reference's randint(0, 0) raises).  Refused
    with RLS_EINVAL before any launch, the message retrievable; rls_tsp_tables8_bytes has no byte form for that K; K = N - 2 runs."""
    from rlsolver_amd.graph import generate_tsp_coords, tsp_tables
    N, B = 30, 5
    coords = generate_tsp_coords(N, seed=1)
    dist, near, rnd = tsp_tables(coords, K=N - 1)
    assert near.shape == (N, N - 1) and rnd.shape == (N, N - 1)
    d, near32, rnd32 = dev(dist), dev(near.astype(np.int32)), dev(rnd.astype(np.int32))
    perms = dev(perms_np(np.random.RandomState(0), B, N))
    lr = torch.full((B, N), 7.0, device=DEV)
    idx = torch.full((B, N), CANARY, dtype=torch.int64, device=DEV)
    ban = torch.zeros((B, N), dtype=torch.uint8, device=DEV)
    with pytest.raises(_abi.RlsError) as e:
        _abi.call("rls_tsp_swap_delta_all", _ptr(d), N, _ptr(perms), B, None, _ptr(near32), N - 1, _ptr(rnd32), N - 1, None,
                  float(np.float32((N - 1) / N)), 3, 0, None, 0.5, _ptr(lr), _ptr(idx), _ptr(ban), _stream(DEV))
    assert e.value.code == -1 and "N-2" in str(e.value)
    torch.cuda.synchronize()
    assert bool((lr == 7.0).all()) and bool((idx == CANARY).all())          # nothing ran
    with pytest.raises(RuntimeError, match="N-2"):
        mops.tsp_swap_delta_all(d, perms, None, 0.5, nearest=near32, random=rnd32, near_threshold=0.9, seed=3)
    assert _abi.lib().rls_tsp_tables8_bytes(N, N - 1) == 0 and mops.tsp_tables8(near32, rnd32) is None
    _, near, rnd = tsp_tables(coords, K=N - 2)
    near32, rnd32 = dev(near.astype(np.int32)), dev(rnd.astype(np.int32))
    assert mops.tsp_tables8(near32, rnd32) is not None
    mops.tsp_swap_delta_all(d, perms, None, 0.5, nearest=near32, random=rnd32, near_threshold=0.9, seed=3)


# ------------------------------------------------------------------------------------------------ switch, 2-opt delta
@pytest.mark.parametrize("N", [3, 64])
def test_apply_swap_edges(N):
    """pos = -1 (no swap), pos = N - 1 (position pos + 1 wraps to 0), a partner AT position pos + 1 (the swap is the identity)"""
    rng = np.random.RandomState(N)
    B = 70
    pn = perms_np(rng, B, N)
    idx = rng.randint(0, N, size=(B, N)).astype(np.int64)
    pos = rng.randint(-1, N, size=B).astype(np.int64)
    pos[:6] = [-1, N - 1, N - 1, 0, 1, N - 2]
    idx[2, N - 1] = 0                                   # j == (pos + 1) % N after the wrap
    idx[3, 0] = 1                                       # j == pos + 1
    x = dev(pn)
    mops.tsp_apply_swap(x, dev(pos), dev(idx))
    want = onp.tsp_switch(pn, pos, idx)
    assert np.array_equal(x.cpu().numpy(), want)
    assert np.array_equal(want[0], pn[0]) and np.array_equal(want[2], pn[2]) and np.array_equal(want[3], pn[3])
    assert want[1, 0] == pn[1, idx[1, N - 1]]
    RAN.add(("tsp_apply_swap",))


@pytest.mark.parametrize("N", [3, 65])
def test_2opt_delta_edges(N):
    """(i, j) = (0, N - 1): the whole tour reversed, delta 0; (1, N - 1): the segment ends at the last position and its successor
    wraps to position 0; i == j; against the length difference of the reversed tour in float64 (symmetric matrix: the formula's
    premise)."""
    from rlsolver_amd.graph import generate_tsp_coords, tsp_tables
    rng = np.random.RandomState(N)
    B = 70
    dist = tsp_tables(generate_tsp_coords(N, seed=N), K=1)[0]
    pn = perms_np(rng, B, N)
    i = rng.randint(0, N, size=B)
    j = np.array([rng.randint(a, N) for a in i])
    i[:4], j[:4] = [0, 1, 0, N - 1], [N - 1, N - 1, 0, N - 1]
    got = mops.tsp_2opt_delta(dev(dist), dev(pn), dev(i.astype(np.int64)), dev(j.astype(np.int64))).cpu().numpy()
    want = onp.tsp_2opt_delta(dist, pn, np.arange(B), i, j)
    np.testing.assert_allclose(got, want, rtol=0, atol=2e-5 * onp.tsp_tour_length_f64(dist, pn).max())
    assert got[0] == 0.0
    RAN.add(("tsp_2opt_delta",))


# ------------------------------------------------------------------------------------------------ 2-opt best
def _best_delta_np(d, t):
    """the most negative reversal delta, the first in (i, j) order among equals; (-1, -1, 0) when none is negative"""
    N = len(t)
    i, j = np.triu_indices(N, 1)                                  # (i, j) order
    keep = ~((i == 0) & (j == N - 1))
    i, j = i[keep], j[keep]
    a, b, c, e = t[i - 1], t[i], t[j], t[(j + 1) % N]
    v = (d[a, c] + d[b, e]) - (d[a, b] + d[c, e])
    k = int(np.argmin(v)) if v.size else 0
    return (int(i[k]), int(j[k]), float(v[k])) if v.size and v[k] < 0 else (-1, -1, 0.0)


def _best_exact_np(d, t, cur):
    """the shortest candidate by its whole length (integer matrix: the sum is exact in any order), first among equals"""
    N = len(t)
    i, j = np.triu_indices(N, 1)
    k = np.arange(N)[None, :]
    inside = (k >= i[:, None]) & (k <= j[:, None])
    tours = t[np.where(inside, i[:, None] + j[:, None] - k, k)]
    v = d[tours, np.roll(tours, -1, axis=1)].sum(axis=1)
    m = int(np.argmin(v))
    return (int(i[m]), int(j[m]), float(v[m])) if v[m] < cur else (-1, -1, float(cur))


@pytest.mark.parametrize("N", [3, 2000])
def test_2opt_best_delta_ranking(N):
    """One tour, an integer matrix (ties everywhere: the first of equals in (i, j) order must win), 1, 7 and the default number
    of workgroups.  At N = 2000 the candidate index c < 1 999 000 is decoded through a float64 sqrt; every row boundary is in."""
    reach(_abi.TSP_2OPT_BEST, N, block=256, lds_bytes=4096 + 4 * N)
    rng = np.random.RandomState(N)
    c = rng.rand(N, 2) * 100
    d = np.rint(np.sqrt(((c[:, None] - c[None]) ** 2).sum(-1)) / 10.0)
    t = rng.permutation(N).astype(np.int64)
    want = _best_delta_np(d, t)
    assert N == 3 or want[0] >= 0
    for sl in (1, 7, None):
        bi, bj, bv = mops.tsp_2opt_best(dev(d), dev(t[None, :]), None, slices=sl)
        assert (int(bi[0]), int(bj[0]), float(bv[0])) == want, sl
        RAN.add(("tsp_2opt_best", "delta", "one slice" if sl == 1 or (sl is None and N == 3) else "slices"))


@pytest.mark.parametrize("N", [3, 65, 200])
def test_2opt_best_exact_ranking(N):
    """The whole-length ranking on an ASYMMETRIC integer matrix (a reversal's inner edges change direction), three tours."""
    reach(_abi.TSP_2OPT_BEST_EXACT, N, block=256, lds_bytes=4096 + 8 * (N + 1) + 4 * N)
    rng = np.random.RandomState(N)
    d = rng.randint(1, 30, size=(N, N)).astype(np.float64)
    pn = perms_np(rng, 3, N)
    cur = d[pn, np.roll(pn, -1, axis=1)].sum(axis=1)
    want = [_best_exact_np(d, pn[b], cur[b]) for b in range(3)]
    assert N == 3 or all(w[0] >= 0 for w in want)
    for sl in (1, 7, None):
        bi, bj, bv = mops.tsp_2opt_best(dev(d), dev(pn), dev(cur), slices=sl)
        assert [(int(bi[b]), int(bj[b]), float(bv[b])) for b in range(3)] == want, sl
        RAN.add(("tsp_2opt_best", "exact", "one slice" if sl == 1 or (sl is None and N == 3) else "slices"))


# ------------------------------------------------------------------------------------------------ rand_perms
@pytest.mark.parametrize("N,kernel", [(1, "lds"), (2, "lds"), (63, "lds"), (64, "lds"), (65, "lds"), (620, "lds"), (621, "global")])
def test_rand_perms_forms(N, kernel):
    """Exact against the numpy shuffle under a global env id past 2^32 (its high word reaches the key), for batches around the 64
    tours of a workgroup, into a buffer with canary words on both sides.  Even N on a 16-byte-aligned base leaves as 16-byte
    stores; the same output placed one int64 further takes the row path."""
    f = reach(_abi.TSP_RAND_PERMS, N, kernel=_abi.TSP_KERNEL_PERMS_LDS if kernel == "lds" else _abi.TSP_KERNEL_PERMS_GLOBAL)
    assert f.lds_bytes == (132 * N if kernel == "lds" else 0)
    seed, off = 77, (3 << 32) + 5
    for B in (1, 63, 64, 65, 129):
        want = onp.rand_perms(B, N, seed, off)
        assert np.array_equal(np.sort(want, axis=1), np.tile(np.arange(N), (B, 1)))
        for shift in (0, 1):
            arena = torch.full((B * N + 34,), CANARY, dtype=torch.int64, device=DEV)
            assert arena.data_ptr() % 16 == 0
            out = arena[2 + shift:2 + shift + B * N].view(B, N)
            _t.rand_perms(out, _s64(seed), off)
            assert np.array_equal(out.cpu().numpy(), want), (B, shift)
            assert bool((arena[:2 + shift] == CANARY).all()) and bool((arena[2 + shift + B * N:] == CANARY).all()), (B, shift)
            RAN.add(("rand_perms", "global") if kernel == "global" else
                    ("rand_perms", "lds", "16-byte stores" if N % 2 == 0 and shift == 0 else "rows"))
    assert not np.array_equal(onp.rand_perms(5, max(N, 8), seed, off), onp.rand_perms(5, max(N, 8), seed, off & 0xFFFFFFFF))


# ------------------------------------------------------------------------------------------------ the fused step
def _run_step(c, s, x, draws, seed=0, env_offset=0):
    """rls_isco_tsp_step through its op -> numpy (y, cur, log_acc, acc)"""
    B, N = x.shape
    y, cur = torch.empty((B, N), dtype=torch.int64, device=DEV), torch.empty((B, N), dtype=torch.int64, device=DEV)
    log_acc, acc = torch.empty(B, device=DEV), torch.empty(B, device=DEV)
    d = {k: dev(v) for k, v in draws.items()} if draws is not None else {}
    _t.isco_tsp_step(s["d"], s["near32"], float(np.float32(c.K / (c.K + 1))), s["rnd32"], dev(x), y, c.L, float(c.T), d.get("u_partner"),
                     d.get("r_near"), d.get("r_rand"), d.get("u_gumbel"), d.get("u_accept"), _s64(seed), env_offset, log_acc, acc, cur)
    return tuple(t.cpu().numpy() for t in (y, cur, log_acc, acc))


def _device_instance(name):
    s = dict(tc.step_inputs(name))
    s["d"], s["near32"], s["rnd32"] = dev(s["dist"]), dev(s["near"].astype(np.int32)), dev(s["rnd"].astype(np.int32))
    return s


def _check_step(c, s, got, what):
    y, cur, log_acc, acc = got
    r = tc.step_oracle(c.name)
    sure, decided, rejected = tc.step_gates(c, r)
    tol = tc.log_acc_tol(c, r["log_acc"])
    err = np.abs(log_acc.astype(np.float64) - r["log_acc"])
    same = (cur == r["cur_x"]).all(axis=1)
    got_rejected = (y != cur).any(axis=1)
    print(f"{what}: cur differs on {(~same).sum()} of {c.B} envs ({(~decided).sum()} undecided), largest log_acc error / bound "
          f"{(err / tol)[decided].max():.3f} (|log_acc| <= {np.abs(r['log_acc']).max():.4g}), oracle rejects {rejected.mean():.2f}, "
          f"kernel output shows {got_rejected.mean():.2f} rejected, sure {sure.mean():.2f}")
    assert (~decided).mean() <= tc.MAX_UNDECIDED
    assert np.array_equal(cur[decided], r["cur_x"][decided]), what                    # the walked tour: exact
    assert (err[decided] <= tol[decided]).all(), what
    assert (np.abs(acc - np.exp(r["log_acc"]))[decided] <= tol[decided] + 1e-5).all(), what
    ok = sure & decided
    assert np.array_equal(y[ok], r["y"][ok]), what
    assert all(np.array_equal(y[b], cur[b]) or np.array_equal(y[b], s["x"][b]) for b in range(c.B))
    if c.reject:                                                                      # the rejected rows are really there
        assert 0.25 <= got_rejected.mean() <= 0.75 and ok.mean() >= 0.9
        assert np.array_equal(y[got_rejected], s["x"][got_rejected])
        assert np.array_equal(got_rejected[ok], (rejected & (r["cur_x"] != s["x"]).any(axis=1))[ok])


@pytest.mark.parametrize("name", [c.name for c in tc.STEP_CASES if not c.production])
def test_step_forms_recorded_draws(name):
    """The fused step in each of its forms against the oracle with recorded draws, from the circle start at the temperature
    that rejects about half the envs (and on two asymmetric matrices; N = 3: every position banned; N = 4: the c3 branch)."""
    c = tc.STEP_BY_NAME[name]
    reach(_abi.TSP_STEP, c.N, lds_d=c.form[0], waves=c.form[1], block=64 * c.form[1])
    s = _device_instance(name)
    _check_step(c, s, _run_step(c, s, s["x"], s["draws"]), name)
    RAN.add(("isco_tsp_step",) + c.form)


@pytest.mark.parametrize("name", [c.name for c in tc.STEP_CASES if c.production])
def test_step_production_draws(name):
    """Production draws under an explicit seed and an env offset past 2^32 == the same kernel fed step_draws_np's numbers as
    recorded draws, bit for bit; the oracle agrees on those draws; a half batch under its own offset is the whole batch's half."""
    c = tc.STEP_BY_NAME[name]
    reach(_abi.TSP_STEP, c.N, lds_d=c.form[0], waves=c.form[1])
    s = _device_instance(name)
    prod = _run_step(c, s, s["x"], None, seed=tc.PROD_SEED, env_offset=tc.PROD_OFFSET)
    rec = _run_step(c, s, s["x"], s["draws"])
    for a, b, what in zip(prod, rec, ("y", "cur", "log_acc", "acc")):
        assert np.array_equal(a, b), what
    _check_step(c, s, prod, name)
    h = c.B // 2
    half = _run_step(c, s, s["x"][h:], None, seed=tc.PROD_SEED, env_offset=tc.PROD_OFFSET + h)
    for a, b, what in zip(half, prod, ("y", "cur", "log_acc", "acc")):
        assert np.array_equal(a, b[h:]), what
    RAN.add(("isco_tsp_step",) + c.form)


def test_step_refuses_bad_arguments_before_any_launch():
    """perm_out aliasing perm_in, K = N - 1, a partial set of test draws, T <= 0: RLS_EINVAL from the C ABI, outputs untouched."""
    N, K, B, L = 12, 3, 5, 2
    dist, near, rnd = tc.circle_instance(N, K)
    d, near32, rnd32 = dev(dist), dev(near.astype(np.int32)), dev(rnd.astype(np.int32))
    x = dev(tc.circle_starts(N, B, 0))
    y = torch.full((B, N), CANARY, dtype=torch.int64, device=DEV)
    log_acc = torch.full((B,), 7.0, device=DEV)
    dr = {k: dev(v) for k, v in tc.recorded_draws(np.random.RandomState(0), L, B, N, K).items()}
    near_full = dev(tc.circle_instance(N, N - 1)[1].astype(np.int32))
    thr = float(np.float32(K / (K + 1)))

    def call(perm_out=y, k=K, near_t=near32, T=0.5, draws=(None,) * 5):
        _abi.call("rls_isco_tsp_step", _ptr(d), N, _ptr(near_t), k, thr, _ptr(rnd32), N - 1, _ptr(x), _ptr(perm_out), B, L, T,
                  *[_ptr(t) for t in draws], 1, 0, _ptr(log_acc), None, None, _stream(DEV))

    full = (dr["u_partner"], dr["r_near"], dr["r_rand"], dr["u_gumbel"], dr["u_accept"])
    for kw, msg in ((dict(perm_out=x), "alias"), (dict(k=N - 1, near_t=near_full), "N-2"), (dict(draws=full[:4] + (None,)), "all together"),
                    (dict(draws=(None,) + full[1:]), "all together"), (dict(T=0.0), "temperature"), (dict(T=-1.0), "temperature")):
        with pytest.raises(_abi.RlsError) as e:
            call(**kw)
        assert e.value.code == -1 and msg in str(e.value), (kw.keys(), str(e.value))
    torch.cuda.synchronize()
    assert bool((y == CANARY).all()) and bool((log_acc == 7.0).all())                 # nothing ran
    assert np.array_equal(x.cpu().numpy(), tc.circle_starts(N, B, 0))
    call(draws=full)                                                                  # the same arguments, complete: runs
    torch.cuda.synchronize()
    assert bool((y != CANARY).all())
    with pytest.raises(RuntimeError):                                                 # the op's own check of the same alias
        _t.isco_tsp_step(d, near32, thr, rnd32, x, x, L, 0.5, None, None, None, None, None, 1, 0, None, None, None)
    # past the last size: RLS_EUNSUPPORTED from the planner, before the pointers are looked at
    assert _abi.tsp_launch_form(_abi.TSP_STEP, 10241).supported == 0


# ------------------------------------------------------------------------------------------------ the registry
def test_zz_every_reachable_form_was_run(request):
    """Runs last in this file: every reachable (entry point, form) pair ran above with its form asserted.  Only meaningful
    when the whole file ran; a selection (-k, a node id) skips."""
    if request.config.getoption("-k") or any("::" in a for a in request.config.args):
        pytest.skip("the form registry is checked when the whole file runs")
    assert RAN == REACHABLE, (sorted(REACHABLE - RAN, key=str), sorted(RAN - REACHABLE, key=str))
