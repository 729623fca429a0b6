"""The conditions that keep tests/test_gpu_tsp_forms.py from hiding a failure, checked on the host: the oracle alone on the step
cases of tests/tsp_cases.py (the rejected share, the sure share, log_acc < 0, the banned and c3 branches at N = 3 / 4, the float32
against float64 gap behind the log_acc bound), the asymmetric instances, the numpy restatement of the production draws, and the
form query rls_tsp_launch_form on both sides of every dispatch boundary -- each boundary derived here from kLdsBytes."""
import ctypes as C

import numpy as np
import pytest

from oracle import oracle_isco as oi
from tests import tsp_cases as tc

KLDS = tc.KLDS
REJECT_CASES = [c.name for c in tc.STEP_CASES if c.reject]


def form(what, N, K=0, tab8=False):
    from rlsolver_amd import _abi
    f = _abi.tsp_launch_form(what, N, K, tab8)
    return dict(lds_d=f.lds_d, tab8=f.tab8, block=f.block, waves=f.waves, lds=f.lds_bytes, kernel=f.kernel, supported=f.supported)


def largest(pred, hi=1 << 20):
    """the largest N >= 1 with pred(N), pred monotone"""
    lo = 0
    while hi - lo > 1:
        mid = (lo + hi) // 2
        lo, hi = (mid, hi) if pred(mid) else (lo, mid)
    return lo


a16 = lambda b: (b + 15) // 16 * 16


# ------------------------------------------------------------------------------------------------ the oracle on the step cases
@pytest.mark.parametrize("name", REJECT_CASES)
def test_reject_cases_really_reject(name):
    """A case that claims to exercise rejection: the oracle rejects a quarter to three quarters of its envs, nine in ten are
    sure (the accept test sits outside the tolerance) and nine in ten have log_acc < 0 -- so `y` is compared on rows where it
    differs from `cur`, and log_acc against numbers that are not zeros."""
    c = tc.STEP_BY_NAME[name]
    r = tc.step_oracle(name)
    sure, decided, rejected = tc.step_gates(c, r)
    assert 0.25 <= rejected.mean() <= 0.75, rejected.mean()
    assert sure.mean() >= 0.9 and (r["log_acc"] < 0).mean() >= 0.9
    # the rejected rows are visible in the outputs: the walked tour differs from the start and y is the start
    moved = (r["cur_x"] != tc.step_inputs(name)["x"]).any(axis=1)
    assert (rejected & moved).mean() >= 0.25 and np.array_equal(r["y"][rejected], tc.step_inputs(name)["x"][rejected])


@pytest.mark.parametrize("name", [c.name for c in tc.STEP_CASES if c.asym])
def test_asymmetric_cases_have_informative_log_acc(name):
    r = tc.step_oracle(name)
    assert (r["log_acc"] < 0).mean() >= 0.5


@pytest.mark.parametrize("name", [c.name for c in tc.STEP_CASES])
def test_log_acc_bound_covers_twice_the_reference_gap(name):
    """float32 oracle against the same oracle in float64, on exactly the case's inputs: the two walk the same tours on all but
    3 % of the envs at most, the gap is within its record in STEP_CASES, and twice the gap lies inside the bound on every env.
    No more than 3 % of the envs have a Gumbel argmax within the bound (the rows the GPU test may leave out of `cur`)."""
    c = tc.STEP_BY_NAME[name]
    r32, r64 = tc.step_oracle(name), tc.step_oracle(name, True)
    same = (r32["cur_x"] == r64["cur_x"]).all(axis=1)
    assert (~same).mean() <= tc.MAX_UNDECIDED
    gap = np.abs(r32["log_acc"].astype(np.float64) - r64["log_acc"])
    assert gap[same].max() <= c.gap, (gap[same].max(), c.gap)
    assert (2 * gap[same] <= tc.log_acc_tol(c, r32["log_acc"])[same]).all()
    sure, decided, rejected = tc.step_gates(c, r32)
    assert (~decided).mean() <= tc.MAX_UNDECIDED
    assert same[decided].all()                       # where the rule calls the argmax decided, the two runs agree


def test_n3_every_position_is_banned():
    """N = 3, K = 1: the partner is always a neighbour of position i + 1, so every position of every env is banned in every
    round: log_acc ~ -1e6 L, never accepted, the tour never moves."""
    c = tc.STEP_BY_NAME["n3_all_banned"]
    s, r = tc.step_inputs(c.name), tc.step_oracle(c.name)
    d = s["draws"]
    for i in range(c.L):
        _, _, ban = oi.tsp_opt_2(s["x"], s["dist"], s["near"], s["rnd"], c.K, c.T, d["u_partner"][i], d["r_near"][i], d["r_rand"][i])
        assert ban.all()
    assert r["banned"].all() and np.array_equal(r["cur_x"], s["x"])
    np.testing.assert_allclose(r["log_acc"], -1e6 * c.L, rtol=1e-5)
    assert not oi.mh_accept(r["log_acc"], d["u_accept"]).any()


@pytest.mark.parametrize("name", ["n4_k1", "n4_k2"])
def test_n4_takes_the_c3_branch(name):
    """N = 4: a partner that is not banned sits two positions ahead (the c3 branch, env_ISCO.py:320-324) -- at least a third
    of the non-banned positions; both banned and non-banned positions occur, and some round selects either kind."""
    c = tc.STEP_BY_NAME[name]
    s, r = tc.step_inputs(name), tc.step_oracle(name)
    d = s["draws"]
    _, idx, ban = oi.tsp_opt_2(s["x"], s["dist"], s["near"], s["rnd"], c.K, c.T, d["u_partner"][0], d["r_near"][0], d["r_rand"][0])
    c3 = idx == (np.arange(c.N)[None, :] + 2) % c.N
    assert ban.any() and (~ban).any()
    assert c3[~ban].mean() >= 1 / 3
    assert r["banned"].any() and (~r["banned"]).any()


@pytest.mark.parametrize("name", [c.name for c in tc.STEP_CASES if c.N >= 65])
def test_step_cases_select_banned_and_c3_positions_by_construction(name):
    """From the circle start the K nearest cities are the tour neighbours: the partner one position behind or ahead is banned,
    the one two ahead takes c3.  Every such case has hundreds of each in round 0."""
    c = tc.STEP_BY_NAME[name]
    s = tc.step_inputs(name)
    d = s["draws"]
    _, idx, ban = oi.tsp_opt_2(s["x"], s["dist"], s["near"], s["rnd"], c.K, c.T, d["u_partner"][0], d["r_near"][0], d["r_rand"][0])
    c3 = (idx == (np.arange(c.N)[None, :] + 2) % c.N) & ~ban
    assert ban.sum() >= 100 and c3.sum() >= 100 and (~ban & ~c3).sum() >= 100


# ------------------------------------------------------------------------------------------------ instances and draws
@pytest.mark.parametrize("N", [3, 65, 194])
def test_asym_differs_from_its_transpose_in_every_row(N):
    dist, near, rnd = tc.circle_instance(N, min(20, N - 2))
    assert np.array_equal(dist, dist.T) and not dist.diagonal().any()
    a = tc.asym(dist, np.random.RandomState(N))
    assert a.dtype == np.float32 and a.shape == dist.shape
    assert ((a != a.T).sum(axis=1) >= N - 1).all()              # every off-diagonal pair of every row
    assert (a.diagonal() != 0).all()
    assert 0.25 * dist.mean() < np.abs(a - dist).mean() < dist.mean()
    for name in ("n65_asym", "n194_asym"):
        d = tc.step_inputs(name)["dist"]
        assert ((d != d.T).sum(axis=1) >= d.shape[0] - 1).all() and (d.diagonal() != 0).all()


def test_circle_start_is_the_optimum():
    """every non-banned move of round 0 lengthens the tour: its logratio is negative"""
    for name in ("n65", "n193", "n2561"):
        c, s = tc.STEP_BY_NAME[name], tc.step_inputs(name)
        d = s["draws"]
        lr, _, ban = oi.tsp_opt_2(s["x"], s["dist"], s["near"], s["rnd"], c.K, c.T, d["u_partner"][0], d["r_near"][0], d["r_rand"][0])
        assert (lr[~ban] < 0).all()
    x = tc.circle_starts(7, 40, 1)
    assert np.array_equal(np.sort(x, axis=1), np.tile(np.arange(7), (40, 1)))
    step = (x[:, 1] - x[:, 0]) % 7
    assert set(step.tolist()) == {1, 6}                          # both orientations
    assert len(set(x[:, 0].tolist())) > 3                        # rotated


def test_step_draws_np_layout_and_ranges():
    B, N, K, L = 5, 9, 3, 4
    d = tc.step_draws_np(tc.PROD_SEED, tc.PROD_OFFSET, B, N, K, L)
    for k in ("u_partner", "r_near", "r_rand", "u_gumbel"):
        assert d[k].shape == (L, B, N)
    assert d["u_accept"].shape == (B,) and d["u_partner"].dtype == np.float32 and d["r_near"].dtype == np.int64
    assert (d["r_near"] >= 0).all() and (d["r_near"] < K).all() and (d["r_rand"] >= 0).all() and (d["r_rand"] < N - K - 1).all()
    assert (d["u_partner"] >= 0).all() and (d["u_partner"] < 1).all()
    # one entry by hand: env b, position i, round it, stream 6 -> (h >> 8) * 2^-24
    b, i, it = 3, 7, 2
    h = int(tc.isco_draw_np(tc.PROD_SEED, tc.PROD_OFFSET + b, i, it, 6))
    assert d["u_gumbel"][it, b, i] == np.float32((h >> 8) * 2.0 ** -24)
    assert d["u_accept"][b] == np.float32((int(tc.isco_draw_np(tc.PROD_SEED, tc.PROD_OFFSET + b, 0xFFFFFFFF, 0, 7)) >> 8) * 2.0 ** -24)
    # a half batch under its own offset draws the whole batch's half; the high word of the offset reaches the key
    h2 = tc.step_draws_np(tc.PROD_SEED, tc.PROD_OFFSET + 2, B - 2, N, K, L)
    assert all(np.array_equal(h2[k], d[k][:, 2:] if d[k].ndim == 3 else d[k][2:]) for k in d)
    lo = tc.step_draws_np(tc.PROD_SEED, tc.PROD_OFFSET & 0xFFFFFFFF, B, N, K, L)
    assert not np.array_equal(lo["u_gumbel"], d["u_gumbel"])
    # the production cases' Gumbel uniforms never hit 0 (log(-log(0)) would be infinite on both sides of the comparison)
    for c in tc.STEP_CASES:
        if c.production:
            assert (tc.step_inputs(c.name)["draws"]["u_gumbel"] > 0).all()


# ------------------------------------------------------------------------------------------------ the form query
def test_form_boundaries_k12_tour_length():
    from rlsolver_amd import _abi
    # the matrix alone beside the 1 KiB margin: 4 N^2 <= kLdsBytes - 1024
    edge = largest(lambda N: 4 * N * N <= KLDS - 1024)
    assert edge == 201
    assert form(_abi.TSP_TOUR_LENGTH, edge)["lds_d"] == 1 and form(_abi.TSP_TOUR_LENGTH, edge)["lds"] == 4 * edge * edge
    assert form(_abi.TSP_TOUR_LENGTH, edge + 1) == dict(lds_d=0, tab8=0, block=256 if edge + 1 > 256 else 1024, waves=16, lds=0, kernel=0, supported=1)
    # 1024 threads up to N = 256, 256 above
    assert form(_abi.TSP_TOUR_LENGTH, 256)["block"] == 1024 and form(_abi.TSP_TOUR_LENGTH, 257)["block"] == 256
    for N in (1, 2, 3, 63, 64, 65):
        assert form(_abi.TSP_TOUR_LENGTH, N)["lds_d"] == 1


def test_form_boundaries_k13_swap_delta():
    from rlsolver_amd import _abi
    K = 20
    W = _abi.TSP_SWAP_DELTA
    # per wave the tour and its inverse, int32 each: 16 waves (block 1024, N <= 256) x 2 x 4 N = 128 N bytes of scratch
    scratch = lambda N: (1024 if N <= 256 else 256) // 64 * 2 * 4 * N
    tabs = lambda N: a16(N * K) + a16(N * (N - K - 1))
    # (LDS_D, TAB8) = (1, 1): matrix + scratch + byte tables <= kLdsBytes - 1024
    e11 = largest(lambda N: N <= 256 and 4 * N * N + scratch(N) + tabs(N) <= KLDS - 1024)
    # (1, 0): matrix + scratch
    e10 = largest(lambda N: 4 * N * N + scratch(N) <= KLDS - 1024)
    assert (e11, e10) == (168, 186)
    assert (form(W, e11, K, True)["lds_d"], form(W, e11, K, True)["tab8"]) == (1, 1)
    assert form(W, e11, K, True)["lds"] == 4 * e11 * e11 + scratch(e11) + tabs(e11)
    assert (form(W, e11 + 1, K, True)["lds_d"], form(W, e11 + 1, K, True)["tab8"]) == (1, 0)
    assert (form(W, e10, K, True)["lds_d"], form(W, e10, K, True)["tab8"]) == (1, 0)
    assert (form(W, e10 + 1, K, True)["lds_d"], form(W, e10 + 1, K, True)["tab8"]) == (0, 0)
    assert form(W, e10 + 1, K, True)["lds"] == scratch(e10 + 1)
    # without tables8 (or with recorded `selected`): the matrix stays up to the same N
    assert form(W, e10, K, False)["lds_d"] == 1 and form(W, e10 + 1, K, False)["lds_d"] == 0
    assert form(W, e11, K, False)["tab8"] == 0
    # tab8 implies lds_d at every size and K: <false, true, true> is never launched
    for N in range(3, 260):
        for k in (1, 20, N - 2):
            if 1 <= k <= N - 2:
                f = form(W, N, k, True)
                assert not (f["tab8"] and not f["lds_d"])
    # the block drops from 1024 to 256 above N = 256 (4 waves: 32 N bytes of scratch)
    assert (form(W, 256)["block"], form(W, 256)["waves"]) == (1024, 16) and (form(W, 257)["block"], form(W, 257)["waves"]) == (256, 4)
    # refused when the scratch alone passes kLdsBytes - 1024: 32 N
    top = largest(lambda N: scratch(N) <= KLDS - 1024)
    assert top == 5088
    assert form(W, top)["supported"] == 1 and form(W, top)["lds"] == 32 * top
    assert form(W, top + 1) == dict(lds_d=0, tab8=0, block=0, waves=0, lds=0, kernel=0, supported=0)
    # K = N - 1 has no byte form (and the draw refuses it)
    assert _abi.lib().rls_tsp_tables8_bytes(30, 29) == 0 and _abi.lib().rls_tsp_tables8_bytes(30, 28) == a16(30 * 28) + a16(30)
    assert form(W, 30, 29, True)["tab8"] == 0 and form(W, 30, 28, True)["tab8"] == 1


def test_form_boundaries_step():
    from rlsolver_amd import _abi
    W = _abi.TSP_STEP
    # per wave tour, inverse, logits, partner | ban: 16 N bytes; four waves beside the matrix: 4 N^2 + 64 N <= kLdsBytes - 1024
    e_lds = largest(lambda N: 4 * N * N + 4 * 16 * N <= KLDS - 1024)
    # matrix in global memory: as many of 4 / 2 / 1 waves as the whole LDS holds
    e4, e2, e1 = (largest(lambda N, w=w: w * 16 * N <= KLDS) for w in (4, 2, 1))
    assert (e_lds, e4, e2, e1) == (193, 2560, 5120, 10240)
    assert form(W, e_lds) == dict(lds_d=1, tab8=0, block=256, waves=4, lds=4 * e_lds * e_lds + 64 * e_lds, kernel=0, supported=1)
    assert form(W, e_lds + 1) == dict(lds_d=0, tab8=0, block=256, waves=4, lds=64 * (e_lds + 1), kernel=0, supported=1)
    assert form(W, e4)["waves"] == 4 and form(W, e4 + 1) == dict(lds_d=0, tab8=0, block=128, waves=2, lds=32 * (e4 + 1), kernel=0, supported=1)
    assert form(W, e2)["waves"] == 2 and form(W, e2 + 1) == dict(lds_d=0, tab8=0, block=64, waves=1, lds=16 * (e2 + 1), kernel=0, supported=1)
    assert form(W, e1)["supported"] == 1 and form(W, e1 + 1)["supported"] == 0
    # every step case reaches the form it names
    for c in tc.STEP_CASES:
        f = form(W, c.N)
        assert (f["lds_d"], f["waves"]) == c.form, c.name
        assert c.B % f["waves"] != 0 or f["waves"] == 1, f"{c.name}: no ragged last workgroup"
    assert {c.form for c in tc.STEP_CASES} == {(1, 4), (0, 4), (0, 2), (0, 1)}


def test_form_boundaries_rand_perms_and_2opt():
    from rlsolver_amd import _abi
    # 64 tours as uint16, 66 halfwords per position: 132 N bytes in half the LDS
    edge = largest(lambda N: N <= 65535 and 132 * N <= KLDS // 2)
    assert edge == 620
    assert form(_abi.TSP_RAND_PERMS, edge) == dict(lds_d=0, tab8=0, block=64, waves=1, lds=132 * edge, kernel=_abi.TSP_KERNEL_PERMS_LDS, supported=1)
    assert form(_abi.TSP_RAND_PERMS, edge + 1) == dict(lds_d=0, tab8=0, block=256, waves=4, lds=0, kernel=_abi.TSP_KERNEL_PERMS_GLOBAL, supported=1)
    # 2-opt: 256 (value, key) pairs, the tour, and for the exact ranking N + 1 running sums
    e_delta = largest(lambda N: 4096 + 4 * N <= KLDS)
    e_exact = largest(lambda N: 4096 + 8 * (N + 1) + 4 * N <= KLDS)
    assert form(_abi.TSP_2OPT_BEST, 2000) == dict(lds_d=0, tab8=0, block=256, waves=4, lds=4096 + 8000, kernel=0, supported=1)
    assert form(_abi.TSP_2OPT_BEST_EXACT, 200)["lds"] == 4096 + 8 * 201 + 800
    assert form(_abi.TSP_2OPT_BEST, e_delta)["supported"] == 1 and form(_abi.TSP_2OPT_BEST, e_delta + 1)["supported"] == 0
    assert form(_abi.TSP_2OPT_BEST_EXACT, e_exact)["supported"] == 1 and form(_abi.TSP_2OPT_BEST_EXACT, e_exact + 1)["supported"] == 0


def test_form_query_refuses_bad_arguments():
    from rlsolver_amd import _abi
    lib = _abi.lib()
    f = _abi.RlsTspForm()
    assert lib.rls_tsp_launch_form(_abi.TSP_STEP, 0, 1, 0, C.byref(f)) == -1
    assert lib.rls_tsp_launch_form(6, 10, 1, 0, C.byref(f)) == -1 and b"what" in lib.rls_last_error_string()
    assert lib.rls_tsp_launch_form(-1, 10, 1, 0, C.byref(f)) == -1
    assert lib.rls_tsp_launch_form(_abi.TSP_STEP, 10, 1, 0, None) == -1
    assert lib.rls_tsp_launch_form(_abi.TSP_STEP, 10, 1, 0, C.byref(f)) == 0 and f.supported == 1
