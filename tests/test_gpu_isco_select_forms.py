"""The selection pipeline the three ISCO steps share (rls_isco_maxcut_step, rls_isco_mis_step, rls_pisco_step: threshold ->
compaction -> sort or extraction -> path log-probabilities -> accept) in every kernel form, at the smallest shapes that reach the
form, on the edges of the selection: clamped path lengths, a selection of exactly / one past the list's capacity, equal keys, draws
of u = 0, keys of both signs, cold and hot temperatures.

Against the float64-aware oracles (oracle/oracle_isco.py, tests/mis_oracle.py, tests/pisco_oracle.py) with recorded draws under the
rules of tests/isco_tol.py: mask and count exact (a sample is left out of the mask comparison only where the oracle's L-th and
(L+1)-th largest perturbed values of DIFFERENT value nearly tie, mis_oracle.MASK_GAP, at most MASK_CAP samples per case -- the
oracle alone stays within it for the committed seeds, test_the_oracle_alone_stays_within_the_mask_cap); ll_x, ll_y and the energy
to RTOL; the path terms within ll_atol; the accepted sample wherever the accept margin clears the tolerance.  Samples below
MIN_MASS of remaining mass -- every L = N row -- are compared on the discrete outputs only.

Every case asserts through rls_isco_launch_plan that it runs the form it names before it launches.  Whether a wave keeps its keys
in registers is not part of the plan: isco_threshold_wave switches at N = 32 * 64, restated here as KEYS_IN_REGISTERS.

u = 0 (isco_unit returns it once in 2^24 draws, torch.rand too): pert = lp - log(-log 0) = -inf, the key isco_sort_list pads its
list with.  Before the fix a pad (index -1) sorted in front of such an entry whenever count was no power of two -- the model of the
network below shows it, test_sort_network_model -- and the step used node -1.  Read on the other paths:
  extraction (isco_order_by_extraction): fkey(-inf) = 0x007FFFFF > 0 = the running maximum's start, so a -inf key is found like any
      other once the larger keys are taken; two of them leave lowest node first; no index but a node's is ever written to `ord`.
  noreplacement_ll_sum: it reads lp[node], which stays finite (a log-softmax of finite scores); pert is not read after the sort.
The zero-draw cases here run on the fixed kernel only.
"""
import contextlib
import functools

import numpy as np
import pytest
import torch

from oracle import oracle_isco as oi
from rlsolver_amd import _abi
from rlsolver_amd.envs.env_ISCO_maxcut import isco_launch_plan
from tests import mis_oracle as mo
from tests import pisco_oracle as po
from tests.gpu_util import DEV
from tests.isco_tol import MIN_MASS, RTOL, ll_atol

gpu = pytest.mark.gpu
F = np.float32
LAM = 1.001
MASK_CAP = 2                         # samples per case that may be left out of the mask comparison
KEYS_IN_REGISTERS = 32 * 64          # isco_threshold_wave: up to here a lane holds its keys in registers
U_TOP = float(F(1) - F(2.0 ** -24))  # the largest draw below 1
KNOBS = ("RLS_ISCO_SEL_CAP", "RLS_ISCO_FORCE_WG", "RLS_ISCO_GLOBAL_ROWS")

REGS, LDSKEYS, WG, SCRATCH = "wave, keys in registers", "wave, keys from LDS", "workgroup", "workgroup, rows in scratch"
GRAPH_SHAPES = [(REGS, n) for n in (1, 2, 63, 64, 65, 2047, 2048)] + [(LDSKEYS, 2049)] + [(WG, n) for n in (256, 257, 1024, 1025)] + \
               [(SCRATCH, n) for n in (256, 1025)]
DENSE_SHAPES = [(REGS, n) for n in (8, 64, 72, 2048)] + [(LDSKEYS, 2056)] + [(WG, n) for n in (256, 264, 1032)]
# K disjoint copies of an n0-node graph: every key tied K-fold
GRAPH_TIES = [(REGS, 20, 3), (REGS, 32, 2), (LDSKEYS, 683, 3), (WG, 86, 3), (WG, 128, 2), (SCRATCH, 86, 3)]
DENSE_TIES = [(REGS, 24, 3), (REGS, 32, 2), (LDSKEYS, 1032, 2), (WG, 88, 3), (WG, 128, 2)]


# ------------------------------------------------------------------------------------------------ the sort, modelled
PAD_OLD, PAD_NEW = -1, 0x7FFFFFFF


def sort_network(keys, idx, tie, fixed):
    """isco_sort_list line for line on the host -> the whole padded list (keys, indices).  ``fixed``: pads carry PAD_NEW and keys
    of -inf order by index (the kernel as it is); else the network before the fix (pads -1, keys only / key then index)."""
    count = len(keys)
    P2 = 1
    while P2 < count:
        P2 <<= 1
    k = [float(v) for v in keys] + [-np.inf] * (P2 - count)
    i = [int(v) for v in idx] + [PAD_NEW if fixed else PAD_OLD] * (P2 - count)
    size = 2
    while size <= P2:
        stride = size >> 1
        while stride >= 1:
            for t in range(P2 >> 1):
                lo = (t // stride) * (stride << 1) + t % stride
                hi = lo + stride
                desc = (lo & size) == 0
                k0, k1, i0, i1 = k[lo], k[hi], i[lo], i[hi]
                if tie:
                    lt = k0 < k1 or (k0 == k1 and i0 > i1)
                elif fixed:
                    lt = k0 < k1 or (k1 == -np.inf and k0 == k1 and i0 > i1)
                else:
                    lt = k0 < k1
                if lt == desc:
                    k[lo], k[hi], i[lo], i[hi] = k1, k0, i1, i0
            stride >>= 1
        size <<= 1
    return k, i


def test_sort_network_model():
    """Random lists whose count is no power of two.  With a key of -inf among the real entries the network before the fix leaves
    a pad among the first `count` positions in most lists (both TIE variants); the fixed one never does, keeps the keys in
    descending order and, under TIE, equal keys lowest node first.  Finite keys -- equal ones included -- leave both networks in
    the same order."""
    rng = np.random.RandomState(0)
    bad = {(tie, fixed): 0 for tie in (False, True) for fixed in (False, True)}
    lists = 0
    for trial in range(300):
        count = int(rng.randint(3, 100))
        if count & (count - 1) == 0:
            continue
        lists += 1
        idx = rng.permutation(500)[:count]
        keys = rng.randint(-6, 6, size=count).astype(np.float64) if trial % 2 else rng.randn(count)        # with and without equal keys
        for tie in (False, True):
            (k0, i0), (k1, i1) = sort_network(keys, idx, tie, False), sort_network(keys, idx, tie, True)
            assert k0 == k1 and i0[:count] == i1[:count] and set(i0[count:]) <= {PAD_OLD}                   # finite keys: unchanged
        keys[rng.permutation(count)[:1 + trial % 3]] = -np.inf
        for tie in (False, True):
            for fixed in (False, True):
                k, i = sort_network(keys, idx, tie, fixed)
                head = i[:count]
                if any(v in (PAD_OLD, PAD_NEW) for v in head):
                    bad[tie, fixed] += 1
                    continue
                assert sorted(head) == sorted(idx.tolist()) and all(a >= b for a, b in zip(k[:count], k[1:count]))
                if tie:
                    assert all(a < b for a, b, ka, kb in zip(head, head[1:], k, k[1:]) if ka == kb)
                elif fixed:
                    assert all(a < b for a, b, ka, kb in zip(head, head[1:], k, k[1:]) if ka == kb == -np.inf)
    print(f"{lists} lists; a pad among the first count entries: {bad}")
    assert bad[False, True] == 0 and bad[True, True] == 0
    assert bad[False, False] > lists // 2 and bad[True, False] > lists // 2


# ------------------------------------------------------------------------------------------------ inputs, shared by the tests
def _graph_edges(n, seed):
    """average degree about 6 (fewer where the graph cannot hold them)"""
    from rlsolver_amd.graph import generate_gnm
    m = min(3 * n, n * (n - 1) // 2)
    if m == 0:
        return np.zeros(0, np.int64), np.zeros(0, np.int64)
    g = np.asarray(generate_gnm(n, m, seed), dtype=np.int64)
    return g[:, 0].copy(), g[:, 1].copy()


def _dense_matrix(Np, seed):
    """integer weights |w| <= 2, about 6 per row, the last columns padding (Np >= 64)"""
    n = Np - 3 if Np >= 64 else Np - 1
    return po.dense_graph(n, min(0.6, 6.0 / n), 2, seed)


def _distinct_draws(rng, B, n, hi=1.0):
    """B rows of n different draws in (0, hi): no two keys of a row tie by their draw"""
    u = (np.stack([rng.permutation(n) for _ in range(B)]) + rng.uniform(0.25, 0.75, size=(B, 1))) / n
    return (u * hi).astype(F).clip(1e-7, U_TOP)


def _tile(vals, B):
    return np.resize(np.asarray(vals, dtype=np.int64), B)


def _wave_batch(N, dense):
    """For the wave forms: the smallest batch whose last workgroup is partial with and without the 16-entry list (the two plans
    may seat a different number of samples), from the query."""
    waves = []
    for cap in (None, 16):
        with _knobs(RLS_ISCO_FORCE_WG=0, RLS_ISCO_SEL_CAP=cap):
            waves.append(isco_launch_plan(N, 1, 256, dense)["waves"])
    B = max(waves) + 1
    while any(B % w == 0 for w in waves if w > 1):
        B += 1
    return B


@contextlib.contextmanager
def _knobs(**kn):
    try:
        for k, v in kn.items():
            if v is not None:
                _abi.tuning_set(k, v)
        yield
    finally:
        for k in KNOBS:
            _abi.tuning_unset(k)


def _form_knobs(form, N):
    if form == SCRATCH:
        return dict(RLS_ISCO_GLOBAL_ROWS=1)
    if form in (REGS, LDSKEYS):
        return dict(RLS_ISCO_FORCE_WG=0) if N >= 256 else {}         # below 256 nodes the wave kernel is the default
    return {}


def _batch_size(form, N, dense, at_least=1):
    return max(_wave_batch(N, dense) if form in (REGS, LDSKEYS) else 3, at_least)


class Problem:
    """One step's model on one instance: how the oracle and the sampler are called."""

    def __init__(self, step, N, eu=None, ev=None, adj=None):
        self.step, self.N, self.eu, self.ev, self.adj = step, N, eu, ev, adj
        self.dense = step == "pisco"

    def local_dist(self, x, T):
        if self.step == "maxcut":
            return oi.maxcut_local_dist(x, self.eu, self.ev, T)[1]
        if self.step == "mis":
            return mo.mis_local_dist(x, self.eu, self.ev, LAM, T)[1]
        return po.local_dist(x, self.adj, T, True)[1]

    def oracle(self, x, pl, T, ug, ua):
        with np.errstate(divide="ignore", invalid="ignore"):
            if self.step == "maxcut":
                return oi.maxcut_step(x, self.eu, self.ev, pl, T, ug, ua)
            if self.step == "mis":
                return mo.mis_step(x, self.eu, self.ev, LAM, pl, T, ug, ua)
            return po.step(x, self.adj, pl, T, ug, ua, True)

    def perturbed(self, x, T, ug):
        with np.errstate(divide="ignore"):
            return (self.local_dist(x.astype(F), T) - np.log(-np.log(ug))).astype(F)

    def random_x(self, rng, B, n=None):
        n = self.N if n is None else n
        return (rng.rand(B, n) < (0.25 if self.step == "mis" else 0.5)).astype(F)

    def sampler(self, B, csr_walk=False):
        if self.dense:
            from rlsolver_amd.envs.env_ISCO import PISCO_maxcut
            iu, ju = np.nonzero(np.triu(self.adj.astype(np.float64)))
            return PISCO_maxcut({"num_nodes": self.N, "num_edges": len(iu), "edge_from": torch.from_numpy(iu).to(DEV),
                                 "edge_to": torch.from_numpy(ju).to(DEV),
                                 "adj_matrix": torch.from_numpy(np.ascontiguousarray(self.adj, dtype=np.float16)).to(DEV)},
                                batch_size=B, device=DEV)
        from rlsolver_amd import ops
        from rlsolver_amd.envs.env_ISCO import ISCO_MIS, ISCO_maxcut
        params = {"num_nodes": self.N, "num_edges": len(self.eu), "edge_from": torch.from_numpy(self.eu).to(DEV),
                  "edge_to": torch.from_numpy(self.ev).to(DEV)}
        s = ISCO_maxcut(params, batch_size=B, device=DEV) if self.step == "maxcut" else ISCO_MIS(params, batch_size=B, device=DEV, lam=LAM)
        if csr_walk:         # a handle with weights has no slab path
            s.graph = ops.DeviceGraph(s.graph.csr, DEV, use_weights=True)
        assert (s.graph.wgt is not None) == csr_walk
        return s

    def run(self, s, x, pl, T, ug, ua):
        xt = torch.from_numpy(np.ascontiguousarray(x.astype(np.float16 if self.dense else F))).to(DEV)
        out = s.step(xt, torch.from_numpy(pl).to(DEV), T, draws={"u_gumbel": torch.from_numpy(ug), "u_accept": torch.from_numpy(ua)},
                     want_terms=True)
        return [o.cpu().numpy() for o in out]


def _decided(pert, L):
    """mis_oracle.mask_is_decided's rule on the oracle's perturbed values; an EXACT tie at the threshold is decided too: equal keys
    are all selected, by the oracle and by the kernel (equal scores give equal log-probabilities in either)."""
    p64 = pert.astype(np.float64)
    srt = -np.sort(-p64, axis=-1)
    B, N = pert.shape
    rows = np.arange(B)
    thr = srt[rows, L - 1]
    nxt = np.where(L < N, srt[rows, np.minimum(L, N - 1)], -np.inf)
    with np.errstate(invalid="ignore"):
        return ((thr - nxt) >= mo.MASK_GAP * np.maximum(1.0, np.abs(thr))) | (thr == nxt)


def _batch(prob, name, x, pl, T, ug, ua, **opts):
    """One launch's inputs with what the oracle says of them (path lengths clamped for the oracle, as the step clamps them)."""
    B, N = x.shape
    L = np.clip(pl, 1, N)
    want = prob.oracle(x, L, T, ug, ua)
    return dict(name=name, x=x, pl=pl, L=L, T=T, ug=ug, ua=ua, want=want, decided=_decided(prob.perturbed(x, T, ug), L), **opts)


@functools.lru_cache(maxsize=None)
def _problem(step, N):
    if step == "pisco":
        return Problem(step, N, adj=_dense_matrix(N, N))
    return Problem(step, N, *_graph_edges(N, N))


@functools.lru_cache(maxsize=None)
def _edge_batches(step, N, B):
    """The edges of the selection at one shape -> [batch].  Shared by the forms and walks that run the shape."""
    prob = _problem(step, N)
    rng = np.random.RandomState(1000 + N)
    x = prob.random_x(rng, B)
    ua = rng.rand(B).astype(F)
    out = []
    # 1. path lengths the step clamps: L < 1 -> 1, L > N -> N; L = N selects the whole row
    out.append(_batch(prob, "clamps", x, _tile([-3, 0, 1, N - 1, N, N + 5], B), 1.0, _distinct_draws(rng, B, N), ua))
    if N >= 63:
        # 2. around a 16-entry list: count = cap (sorted), cap + 1 (extraction), both kinds of sample in one workgroup of waves
        out.append(_batch(prob, "list boundary", x, _tile([15, 16, 17, 40], B), 1.0, _distinct_draws(rng, B, N), ua, same_bits=True))
        # 5. keys of both signs: lp ~ -log N at T = 50, the largest draw on m nodes lifts exactly those above 0.  The m nodes
        #    have m different scores: with one draw, equal scores would be equal keys of nodes whose lp differ AFTER the flip, and
        #    ll_y2x would depend on an order of ties that neither the reference (torch.argsort) nor the kernels define -- the
        #    kernel and the oracle's stable order differed by 3e-4 there, 1.5 x the tolerance.  Equal keys are edge 3's.
        m = 5
        ug = _distinct_draws(rng, B, N, hi=0.5)                  # -log(-log 0.5) = 0.37 < log N - |score spread|: the others stay below 0
        lp = prob.local_dist(x, 50.0)
        for b in range(B):
            first = np.unique(lp[b], return_index=True)[1]
            assert len(first) >= m, (step, N, b, len(first))
            ug[b, rng.permutation(first)[:m]] = U_TOP
        bt = _batch(prob, "both signs", x, _tile([m - 1, m, m + 1], B), 50.0, ug, ua)
        assert ((prob.perturbed(x, 50.0, ug) > 0).sum(axis=1) == m).all(), (step, N)
        out.append(bt)
    if N >= 3:
        # 4. draws of u = 0: one node (L = N), two nodes (L = N), one node (L = N - 1: the only entry not selected)
        ug = _distinct_draws(rng, B, N)
        z = rng.permutation(N)[:4]
        ug[0, z[0]] = 0.0
        ug[1, z[1]] = ug[1, z[2]] = 0.0
        ug[2, z[3]] = 0.0
        pl = _tile([3, 7, 1], B)
        pl[:3] = (N, N, N - 1)
        # sample 1's two keys of -inf tie, and the two nodes' lp differ after the flip: its ll_y2x depends on which of them the
        # reverse path undoes first.  No order of ties is defined (torch.argsort in the reference; the oracle's two stable sorts
        # are not even each other's reverse, the kernel's reverse path is) -- measured at N = 64: 0.037 apart at a tolerance of
        # 0.005 -- so that sample is compared on mask, count, y in {x, x ^ mask} and finiteness, as the other two are by their mass
        bt = _batch(prob, "zero draws", x, pl, 1.0, ug, ua, zero=True, unordered=(1,))
        assert bt["want"]["mask"].sum(axis=1)[:3].tolist() == [N, N, N - 1]
        out.append(bt)
    # 6. cold and hot.  Cold: expf underflows in the renormalisation; at least half the batch draws ONE node, whose remaining mass
    #    is 1 in both directions whatever the temperature, so the path terms of those samples are always compared
    out.append(_batch(prob, "cold", x, np.minimum(_tile([1, 2, 1, 3, 1, 5, 1, 4], B), N), 0.05, _distinct_draws(rng, B, N), ua))
    out.append(_batch(prob, "hot", x, np.minimum(_tile([1, 7, max(1, N // 2), 20], B), N), 50.0, _distinct_draws(rng, B, N), ua))
    return out


@functools.lru_cache(maxsize=None)
def _tie_problem(step, n0, K):
    if step == "pisco":
        a = po.dense_graph(n0, min(0.6, 6.0 / n0), 2, n0)
        assert a.shape == (n0, n0)
        adj = np.zeros((K * n0, K * n0), np.float16)
        for c in range(K):
            adj[c * n0:(c + 1) * n0, c * n0:(c + 1) * n0] = a
        return Problem(step, K * n0, adj=adj)
    eu, ev = _graph_edges(n0, n0)
    return Problem(step, K * n0, np.concatenate([eu + c * n0 for c in range(K)]), np.concatenate([ev + c * n0 for c in range(K)]))


@functools.lru_cache(maxsize=None)
def _tie_batches(step, n0, K, B):
    """3. K copies of the sample and of its draws on K copies of the graph: every key tied K-fold, the tied nodes equal in lp
    before and after the flip, so no term depends on how a tie is ordered.  count = K * ceil(L / K); with a 16-entry list, K = 3
    and L = 16 that is 18 > 16 >= L: extraction entered by ties alone."""
    prob = _tie_problem(step, n0, K)
    N = K * n0
    rng = np.random.RandomState(2000 + N)
    x = np.tile(prob.random_x(rng, B, n0), (1, K))
    ug = np.tile(_distinct_draws(rng, B, n0), (1, K))
    bt = _batch(prob, f"ties x{K}", x, _tile([1, 16, 17, N], B), 1.0, ug, rng.rand(B).astype(F), ties=K)
    assert (bt["want"]["mask"].sum(axis=1) == K * -(-bt["L"] // K)).all()
    return [bt]


# ------------------------------------------------------------------------------------------------ the comparison
def _ll_close(actual, desired, mass, L, use, what):
    """isco_tol.assert_ll_close where the expected value is finite; the same infinity / NaN where it is not."""
    actual, desired = actual.astype(np.float64), np.asarray(desired, np.float64)
    fin = np.isfinite(desired)
    assert np.array_equal(actual[use & ~fin], desired[use & ~fin], equal_nan=True), what
    err = np.abs(actual - np.where(fin, desired, 0))
    tol = ll_atol(mass, L) + RTOL * np.abs(np.where(fin, desired, 0))
    ok = (mass >= MIN_MASS) & use & fin
    bad = ok & ~(err <= tol)
    print(f"{what}: {int(ok.sum())} samples, largest error / tolerance {np.where(ok, err / tol, 0).max():.3f}")
    assert not bad.any(), f"{what}: samples {np.flatnonzero(bad).tolist()} err {err[bad]} tol {tol[bad]} mass {mass[bad]} L {L[bad]}"
    return ok


def _compare(prob, bt, got, what):
    y, energy, acc, terms, mask = got
    want, x, L, decided = bt["want"], bt["x"], bt["L"], bt["decided"]
    B, N = x.shape
    mass, margin = want["remaining_mass"], want["accept_margin"]
    y = y.astype(F)
    mask = mask.astype(np.uint8)
    wmask = np.asarray(want["mask"]).astype(np.uint8)
    assert np.array_equal(mask[decided], wmask[decided]), f"{what}: mask"
    count = mask.sum(axis=1)
    assert (count >= L).all() and (count[decided] == wmask.sum(axis=1)[decided]).all(), f"{what}: count {count} L {L}"
    if bt.get("ties"):
        K = bt["ties"]
        assert (count == K * -(-L // K))[decided].all(), f"{what}: count {count} for L {L}, every key tied {K}-fold"
    assert set(np.unique(y)) <= {0.0, 1.0}, what
    flipped = y != x
    assert all((not flipped[b].any()) or np.array_equal(flipped[b], mask[b].astype(bool)) for b in range(B)), f"{what}: y is neither x nor x ^ mask"
    for name, a, w in (("ll_x", terms[:, 0], want["ll_x"]), ("ll_y", terms[:, 2], want["ll_y"]), ("energy", energy, want["energy"]),
                       ("ll_x2y", terms[:, 1], want["ll_x2y"]), ("ll_y2x", terms[:, 3], want["ll_y2x"]), ("log_acc", terms[:, 4], want["log_acc"]),
                       ("acc", acc, want["acc"])):
        fin = np.isfinite(np.asarray(w, np.float64))
        assert np.isfinite(a[fin & decided]).all(), f"{what}: {name} {a} is not finite where the oracle's {w} is"
    use = np.ones(B, bool)
    use[list(bt.get("unordered", ()))] = False
    np.testing.assert_allclose(terms[:, 0], want["ll_x"], rtol=RTOL, atol=1e-5, err_msg=f"{what}: ll_x")
    np.testing.assert_allclose(terms[decided, 2], want["ll_y"][decided], rtol=RTOL, atol=1e-5, err_msg=f"{what}: ll_y")
    np.testing.assert_allclose(energy[decided], want["energy"][decided], rtol=RTOL, atol=1e-5, err_msg=f"{what}: energy")
    oks = [_ll_close(terms[:, c], want[k], mass, L, decided & use, f"{what}/{k}") for c, k in ((1, "ll_x2y"), (3, "ll_y2x"), (4, "log_acc"))]
    ok = oks[0] & oks[1] & oks[2]
    fin = np.isfinite(want["log_acc"])
    assert (np.abs(acc - want["acc"])[ok] <= 2 * ll_atol(mass, L)[ok]).all(), f"{what}: acc"
    sure = decided & use & fin & (margin > 2 * (ll_atol(mass, L) + RTOL * np.abs(np.where(fin, want["log_acc"], 0))))
    assert np.array_equal(y[sure], np.asarray(want["y"])[sure].astype(F)), f"{what}: accepted sample"
    # the samples that draw the whole row keep (about) no mass: their path terms are not compared, by rule, and are not counted
    # as left out; of the others at least half must have been compared
    whole = L >= N
    if not bt.get("zero"):
        assert int(ok.sum()) >= min(B // 2, int((~whole).sum())), \
            f"{what}: path terms compared on {int(ok.sum())} of {B} samples ({int(whole.sum())} draw the whole row: discrete outputs only)"
    return int((~decided).sum())


def _run_case(prob, s, form, batches, what, scratch_guard=False):
    """Every batch with the list as the plan sizes it and with a 16-entry list (longer selections: by extraction)."""
    N, left_out = prob.N, 0
    for bt in batches:
        B = len(bt["x"])
        runs = []
        for cap in (None, 16):
            with _knobs(RLS_ISCO_SEL_CAP=cap, **_form_knobs(form, N)):
                plan = s.launch_plan(B)
                names = f"{what} / {bt['name']} / cap {cap}"
                assert plan["err"] == 0 and plan["form"] == ("wave" if form in (REGS, LDSKEYS) else form), (names, plan)
                if form in (REGS, LDSKEYS):
                    assert (N <= KEYS_IN_REGISTERS) == (form == REGS) and B % plan["waves"] != 0 and B > plan["waves"], (names, plan)
                assert cap is None or plan["Pw" if form in (REGS, LDSKEYS) else "P"] <= 16, (names, plan)
                if scratch_guard and bt.get("zero"):
                    # the f32 rows 64 bytes into a buffer of NaN: an index of -1 reads one from in front of sample 0's lp row
                    need = B * N * 8
                    guard = torch.full(((need + 128) // 4,), float("nan"), dtype=torch.float32, device=DEV)
                    s._scratch = guard.view(torch.uint8)[64:64 + need]
                    assert s._step_scratch(B).data_ptr() == guard.data_ptr() + 64
                got = prob.run(s, bt["x"], bt["pl"], bt["T"], bt["ug"], bt["ua"])
                if scratch_guard and bt.get("zero"):
                    s._scratch = None
            n = _compare(prob, bt, got, names)
            runs.append(got)
        left_out += n
        if bt.get("same_bits"):      # no equal keys in this batch: the sorted list and the extraction give the same bits
            assert int((runs[0][4].sum(axis=1) > 16).sum()) >= 1
            for a, b in zip(*runs):
                assert np.array_equal(a, b, equal_nan=True), f"{what} / {bt['name']}: a 16-entry list changes the result"
    assert left_out <= MASK_CAP, f"{what}: {left_out} samples left out of the mask comparison"


def _all_cases():
    for step in ("maxcut", "mis"):
        for form, N in GRAPH_SHAPES:
            yield step, form, N, _edge_batches(step, N, _batch_size(form, N, False, 6 if form in (WG, SCRATCH) else 1))
        for form, n0, K in GRAPH_TIES:
            yield step, form, K * n0, _tie_batches(step, n0, K, _batch_size(form, K * n0, False, 4))
    for form, N in DENSE_SHAPES:
        yield "pisco", form, N, _edge_batches("pisco", N, _batch_size(form, N, True, 6 if form == WG else 1))
    for form, n0, K in DENSE_TIES:
        yield "pisco", form, K * n0, _tie_batches("pisco", n0, K, _batch_size(form, K * n0, True, 4))
    yield "maxcut", REGS, 65, _edgeless_batches("maxcut", _wave_batch(65, False))


@functools.lru_cache(maxsize=None)
def _edgeless_batches(step, B):
    """65 nodes, no edge: every score is 0 (MaxCut), so lp is uniform and the keys are the draws' alone."""
    prob = Problem(step, 65, np.zeros(0, np.int64), np.zeros(0, np.int64))
    rng = np.random.RandomState(65)
    x = prob.random_x(rng, B)
    return [_batch(prob, "edgeless", x, _tile([-3, 0, 1, 64, 65, 70, 16, 17], B), 1.0, _distinct_draws(rng, B, 65), rng.rand(B).astype(F))]


def test_the_oracle_alone_stays_within_the_mask_cap():
    """For the committed seeds: the samples whose L-th and (L+1)-th largest perturbed values (different ones) nearly tie, per
    case, counted from the oracle alone; and the workgroup forms' batches hold every path length of their edges."""
    worst = 0
    for step, form, N, batches in _all_cases():
        left = sum(int((~bt["decided"]).sum()) for bt in batches)
        worst = max(worst, left)
        assert left <= MASK_CAP, (step, form, N, left)
        for bt in batches:
            assert len(bt["x"]) >= (3 if form in (WG, SCRATCH) else 2) and bt["x"].shape[1] == N
    print(f"most samples left out in one case: {worst}")


# ------------------------------------------------------------------------------------------------ the GPU cases
def _ids(v):
    return str(v).replace(", ", "-").replace(" ", "_")


@gpu
@pytest.mark.parametrize("walk", ["slabs", "csr"])
@pytest.mark.parametrize("form,N", GRAPH_SHAPES, ids=_ids)
@pytest.mark.parametrize("step", ["maxcut", "mis"])
def test_graph_steps_every_form_at_every_edge(step, form, N, walk):
    B = _batch_size(form, N, False, 6 if form in (WG, SCRATCH) else 1)      # the workgroup forms: one sample per clamped path length
    prob = _problem(step, N)
    s = prob.sampler(B, csr_walk=walk == "csr")
    _run_case(prob, s, form, _edge_batches(step, N, B), f"{step} {form} N={N} {walk}", scratch_guard=form == SCRATCH)


@gpu
@pytest.mark.parametrize("walk", ["slabs", "csr"])
@pytest.mark.parametrize("form,n0,K", GRAPH_TIES, ids=_ids)
@pytest.mark.parametrize("step", ["maxcut", "mis"])
def test_graph_steps_equal_keys(step, form, n0, K, walk):
    """The wave sort (no tie-break), the workgroup sort (by node id) and the extraction (lowest node first) each against the
    oracle; they need not agree with each other bit for bit on tied keys, and are not asked to."""
    B = _batch_size(form, K * n0, False, 4)
    prob = _tie_problem(step, n0, K)
    s = prob.sampler(B, csr_walk=walk == "csr")
    _run_case(prob, s, form, _tie_batches(step, n0, K, B), f"{step} {form} {K} x {n0} {walk}")


@gpu
def test_maxcut_step_on_an_edgeless_graph():
    B = _wave_batch(65, False)
    bts = _edgeless_batches("maxcut", B)
    prob = Problem("maxcut", 65, np.zeros(0, np.int64), np.zeros(0, np.int64))
    _run_case(prob, prob.sampler(B), REGS, bts, "maxcut edgeless N=65")


@gpu
@pytest.mark.parametrize("form,Np", DENSE_SHAPES, ids=_ids)
def test_dense_step_every_form_at_every_edge(form, Np):
    B = _batch_size(form, Np, True, 6 if form == WG else 1)
    prob = _problem("pisco", Np)
    _run_case(prob, prob.sampler(B), form, _edge_batches("pisco", Np, B), f"pisco {form} Np={Np}")


@gpu
@pytest.mark.parametrize("form,n0,K", DENSE_TIES, ids=_ids)
def test_dense_step_equal_keys(form, n0, K):
    """Small-integer weights in a block-diagonal matrix: the f16 product is exact in any accumulation order, the ties are exact."""
    B = _batch_size(form, K * n0, True, 4)
    prob = _tie_problem("pisco", n0, K)
    _run_case(prob, prob.sampler(B), form, _tie_batches("pisco", n0, K, B), f"pisco {form} {K} x {n0}")
