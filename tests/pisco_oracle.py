"""CPU ORACLE for the PISCO_maxcut sampler step -- TEST INFRASTRUCTURE, NOT PRODUCT CODE.

Restates in numpy rlsolver/envs/env_ISCO.py:384-444 (PISCO_maxcut.step / proposal / get_local_dist / ll_y2x /
tensor_core_energy) with every random draw passed in.  The local distribution is the closed form of the reference's half matmul
and autograd, in float64 and then rounded where the reference rounds (``half_rounding``):
    r        = delta . A                         float64; f16(.) = round-to-nearest-even of the exact sum
    energy   = f32(f16(-0.25) * f16(sum_k r_k delta_k)) / T      the sum rounded to f16 ONCE (torch sums half in float)
    score_k  = delta_k r_k / (2T)                f32 (the factors -0.25 and 2 are powers of two)
    log_prob = log_softmax(score) over all Np columns (torch's, on the CPU: the one op here that is not numpy)
With ``half_rounding`` off nothing is rounded to f16 (r and the sum go to f32).  The proposal's row is a second product here,
not the kernel's rank-L update: on integer-valued matrices both are exact.  Everything around the energy model -- multinomial,
reverse_ll, remaining_mass, mh_accept -- is oracle/oracle_isco.py's.  Pinned against tests/golden/pisco.npz (captured from the
reference's own class on the CPU): tests/test_pisco_oracle.py.

Tolerance of the path log-probabilities: tests/isco_tol.py's form scaled by K_TOL, the factor tests/mis_oracle.py derives for
scores that are not small integers over 2T (weighted gains are not).  The mask rule is the MIS one (MASK_GAP).
"""
from __future__ import annotations

import numpy as np

from oracle import oracle_isco as oi
from tests.mis_oracle import K_TOL, MASK_EXEMPT_ONE_IN, MASK_GAP  # noqa: F401

F = np.float32


def pad8(n):
    return (n + 7) // 8 * 8


def product(x01, adj):
    """delta . A in float64 (exact on integer-valued A)."""
    return (np.asarray(x01, np.float64) * 2 - 1) @ np.asarray(adj, np.float64)


def local_dist(x01, adj, temperature, half_rounding=True):
    """get_local_dist, env_ISCO.py:407-416 -> (energy f32 [B], log_prob f32 [B, Np])."""
    T = F(temperature)
    d = (np.asarray(x01, np.float64) * 2 - 1)
    r = product(x01, adj)
    with np.errstate(over="ignore"):
        r = (r.astype(np.float16) if half_rounding else r).astype(F)
        s = (r.astype(np.float64) * d).sum(axis=-1)
        s = (s.astype(np.float16) if half_rounding else s).astype(F)
    energy = ((F(-0.25) * s) / T).astype(F)
    score = ((d.astype(F) * r) / (F(2) * T)).astype(F)
    # the reference's own op on the closed-form score: numpy's log_softmax differs from it in the last bit (4.8e-7 on the
    # committed traces), and the fixture comparison of this oracle is bit for bit
    import torch
    return energy, torch.log_softmax(torch.from_numpy(score), dim=-1).numpy()


def step(x01, adj, path_length, temperature, u_gumbel, u_accept, half_rounding=True):
    """PISCO_maxcut.step, env_ISCO.py:384-392.  The dictionary of oracle_isco.maxcut_step."""
    x01 = np.asarray(x01).astype(F)
    ll_x, log_prob = local_dist(x01, adj, temperature, half_rounding)
    mask, perturbed, ll_sel = oi.multinomial(log_prob, path_length, u_gumbel)
    y = (x01 * (1 - mask) + mask * (1 - x01)).astype(F)
    ll_x2y = ll_sel.sum(axis=-1, dtype=F)
    ll_y, log_prob_y = local_dist(y, adj, temperature, half_rounding)
    ll_y2x = oi.reverse_ll(log_prob_y, mask, perturbed)
    with np.errstate(invalid="ignore"):           # -inf - -inf where the f16 energy sum overflowed: NaN, as in the reference
        log_acc = np.minimum(ll_y + ll_y2x - ll_x - ll_x2y, F(0)).astype(F)
    use = oi.mh_accept(log_acc, u_accept)
    out = np.where(use[:, None], y, x01)
    cond = np.minimum(oi.remaining_mass(log_prob, mask, perturbed, True), oi.remaining_mass(log_prob_y, mask, perturbed, False))
    return dict(ll_x=ll_x, ll_x2y=ll_x2y, mask=mask, y_prop=y, ll_y=ll_y, ll_y2x=ll_y2x, log_acc=log_acc, y=out,
                energy=(ll_y * F(temperature)).astype(F), acc=np.exp(log_acc).astype(F), remaining_mass=cond,
                accept_margin=np.abs(np.log((u_accept + F(1e-24)).astype(np.float64)) - log_acc), log_prob=log_prob)


def mask_is_decided(x01, adj, path_length, temperature, u_gumbel, half_rounding=True):
    """bool [B]: mis_oracle.mask_is_decided's rule -- the oracle's gap between the L-th and (L+1)-th largest perturbed value is at
    least MASK_GAP * max(1, |threshold|)."""
    _, log_prob = local_dist(np.asarray(x01).astype(F), adj, temperature, half_rounding)
    pert = (log_prob - np.log(-np.log(u_gumbel))).astype(F).astype(np.float64)
    srt = -np.sort(-pert, axis=-1)
    B, N = pert.shape
    L = np.clip(np.asarray(path_length), 1, N)
    rows = np.arange(B)
    thr = srt[rows, L - 1]
    nxt = np.where(L < N, srt[rows, np.minimum(L, N - 1)], -np.inf)
    return (thr - nxt) >= MASK_GAP * np.maximum(1.0, np.abs(thr))


def dense_graph(n, density, wmax, seed, signed=True):
    """A symmetric integer-weight matrix, f16 [Np, Np], zero diagonal, zero-padded from n to Np; weights uniform in
    [-wmax, wmax] without 0 (``signed``) or in [1, wmax]."""
    r = np.random.RandomState(seed)
    Np = pad8(n)
    keep = np.triu(r.rand(n, n) < density, 1)
    w = r.randint(1, wmax + 1, size=(n, n)) * (r.choice([-1, 1], size=(n, n)) if signed else 1)
    U = np.where(keep, w, 0)
    A = np.zeros((Np, Np), np.float64)
    A[:n, :n] = U + U.T
    return A.astype(np.float16)


# The GPU oracle tests' shapes (n, density, wmax, scale, B, largest path length, half_rounding values): every kernel form at the
# smallest shape that reaches it (tests/test_gpu_pisco.py says which knob forces which).  Weights are integers in +-wmax times
# `scale`, temperatures EDGE_TEMPERATURES times `scale`: the scores delta r / 2T are those of the unscaled graph.  They are kept
# small (a few units) because the path terms of a peaked distribution are ill-conditioned in the reference itself (tests/
# isco_tol.py): with weights in +-7 at 30 % density only 2 of 70 samples keep 1e-6 of remaining mass, with these all or most do.
# scale = 41 on the second shape makes sum_k r_k delta_k an even number of several thousands, which f16 cannot always hold:
# there the two half_rounding forms give different energies (asserted in tests/test_pisco_oracle.py).  Every sum stays an
# exact f32 integer (Np^2 * wmax * scale < 2^24), so the rank-L update and the oracle's second product agree exactly.
# Path lengths stay <= 60 on the 2000- and 2104-column shapes: a threshold deep inside 2000 perturbed values ties within
# MASK_GAP too often for the mask rule (tests/test_pisco_oracle.py counts the undecided pairs of every case).
EDGE_CASES = ((64, 0.15, 2, 1, 5, 32, (True, False)), (333, 0.03, 2, 41, 70, 166, (True, False)), (2100, 0.05, 3, 1, 8, 60, (True,)),
              (2000, 0.05, 3, 1, 40, 60, (True,)))
EDGE_TEMPERATURES = (1.0, 0.4)


def edge_case(n, density, wmax, scale, B, pl_hi, seed=9):
    """-> adj f16 [Np, Np], x f32 [B, Np] (set bits in the padded columns too), [(T, path_length, u_gumbel, u_accept)]."""
    adj = (dense_graph(n, density, wmax, seed).astype(np.float64) * scale).astype(np.float16)
    Np = adj.shape[0]
    rng = np.random.RandomState(n)
    x = (rng.rand(B, Np) < 0.5).astype(F)
    draws = []
    for T in EDGE_TEMPERATURES:
        pl = rng.randint(1, pl_hi, size=B).astype(np.int64)
        pl[0], pl[-1] = 1, (Np if Np < 100 else pl_hi - 1)
        ug = rng.rand(B, Np).astype(F).clip(1e-7, 1 - 1e-7)
        draws.append((float(F(T * scale)), pl, ug, rng.rand(B).astype(F)))
    return adj, x, draws
