"""PISCO_maxcut on the GPU: the f16 matrix-core product (rls_pisco_product) against exact integer products, the fused step
(rls_pisco_step) against traces of the reference's own class (tests/golden/pisco.npz) and against the numpy oracle
(tests/pisco_oracle.py) at every kernel form, against ISCO_maxcut on a unit-weight graph, its contract checks and its
production draws.

Discrete results are exact.  The mask may leave out a sample only where the oracle's L-th and (L+1)-th largest perturbed values
nearly tie (pisco_oracle.mask_is_decided), at most one in 50 per test; tests/test_pisco_oracle.py counts them for the committed
seeds.  Path log-probabilities: tests/isco_tol.py against the reference's traces, scaled by pisco_oracle.K_TOL against the oracle
(the factor tests/mis_oracle.py measured between two implementations whose reductions differ)."""
import ctypes as C

import numpy as np
import pytest
import torch

from tests import pisco_oracle as po
from tests.gpu_util import DEV
from tests.isco_tol import MIN_MASS, RTOL, ll_atol

pytestmark = pytest.mark.gpu


def _h(a):
    return torch.from_numpy(np.ascontiguousarray(a, dtype=np.float16)).to(DEV)


def _sampler(adj, n, B, **kw):
    from rlsolver_amd.envs.env_ISCO import PISCO_maxcut
    iu, ju = np.nonzero(np.triu(adj.astype(np.float64)))
    params = {"num_nodes": n, "num_edges": len(iu), "edge_from": torch.from_numpy(iu).to(DEV), "edge_to": torch.from_numpy(ju).to(DEV),
              "adj_matrix": _h(adj)}
    return PISCO_maxcut(params, batch_size=B, device=DEV, **kw)


def _step(s, x, pl, T, ug, ua):
    out = s.step(_h(x), torch.from_numpy(pl).to(DEV), T, draws={"u_gumbel": torch.from_numpy(ug), "u_accept": torch.from_numpy(ua)},
                 want_terms=True)
    assert out[0].dtype == torch.float16 and tuple(out[0].shape) == x.shape
    return [o.cpu().numpy() for o in out]


# ------------------------------------------------------------------------------------------------ the product
@pytest.mark.parametrize("Np", [8, 24, 40, 104, 264])
def test_product_exact_on_integer_weights(Np):
    """K tail and column tail (Np no multiple of 16 / 32 / 64), one column block and several, one sample, a ragged 16-row tile
    (5), a full one (16), a second one holding one sample (17) -- the split-K kernel of small batches -- and the 64-row tiles of
    the large-batch kernel, the second ragged (70 = 64 + 6).  Samples have set bits in the padded columns: the zero rows of A
    must silence them (their delta is -1, not 0)."""
    from rlsolver_amd import ops
    n = Np - 3
    adj = po.dense_graph(n, 0.6, 7, seed=Np)
    assert adj.shape == (Np, Np) and not adj[n:].any() and adj.any() and np.abs(adj).max() <= 7
    A = _h(adj)
    rng = np.random.RandomState(Np)
    for B in (1, 5, 16, 17, 70):
        x = (rng.rand(B, Np) < 0.5).astype(np.float16)
        x[:, n:] = 1                                                       # what a step can put there
        x[0, n:] = (0, 1, 0)
        r = ops.pisco_product(A, _h(x)).cpu().numpy()
        want = (x.astype(np.int64) * 2 - 1) @ adj.astype(np.int64)
        assert r.dtype == np.float32 and np.array_equal(r.astype(np.int64), want) and np.array_equal(r, want.astype(np.float32)), (Np, B)


def test_product_does_not_assume_symmetry_or_zero_padding():
    """delta . A for any A: an asymmetric matrix with nonzero entries in every row and column catches a transposed operand or
    result tile, which a symmetric A hides."""
    from rlsolver_amd import ops
    Np = 104
    rng = np.random.RandomState(3)
    adj = rng.randint(-7, 8, size=(Np, Np)).astype(np.float16)
    assert not np.array_equal(adj, adj.T)
    for B in (21, 85):                                   # either product kernel
        x = (rng.rand(B, Np) < 0.5).astype(np.float16)
        r = ops.pisco_product(_h(adj), _h(x)).cpu().numpy()
        assert np.array_equal(r, ((x.astype(np.int64) * 2 - 1) @ adj.astype(np.int64)).astype(np.float32)), B


def test_product_real_valued_within_the_f32_accumulation_bound():
    """f16 weights uniform in [-1, 1]: a product of two f16 values is exact in f32, so the error is the accumulation's:
    |r - r64|_j <= Np * 2^-24 * sum_i |A_ij|."""
    from rlsolver_amd import ops
    Np = 264
    rng = np.random.RandomState(11)
    U = np.triu(rng.uniform(-1, 1, size=(Np, Np)), 1)
    adj = (U + U.T).astype(np.float16)
    a64 = adj.astype(np.float64)
    bound = Np * 2.0 ** -24 * np.abs(a64).sum(axis=0)
    for B in (17, 70):                                   # either product kernel
        x = (rng.rand(B, Np) < 0.5).astype(np.float16)
        r = ops.pisco_product(_h(adj), _h(x)).cpu().numpy().astype(np.float64)
        err = np.abs(r - (x.astype(np.float64) * 2 - 1) @ a64)
        print(f"B={B}: largest error / bound {float((err / bound[None, :]).max()):.3f}")
        assert (err <= bound[None, :]).all()


# ------------------------------------------------------------------------------------------------ the step
def _ll_close(actual, desired, mass, pl, use, what, scale):
    """isco_tol's comparison where the expected value is finite; the same infinity / NaN where it is not."""
    actual, desired = actual.astype(np.float64), np.asarray(desired, np.float64)
    fin = np.isfinite(desired)
    assert np.array_equal(actual[use & ~fin], desired[use & ~fin], equal_nan=True), what
    err = np.abs(actual - np.where(fin, desired, 0))
    tol = scale * ll_atol(mass, pl) + RTOL * np.abs(np.where(fin, desired, 0))
    ok = (mass >= 1e-6) & use & fin
    bad = ok & ~(err <= tol)
    print(f"{what}: {int(ok.sum())} samples, largest error / tolerance {np.where(ok, err / tol, 0).max():.3f}")
    assert not bad.any(), f"{what}: samples {np.flatnonzero(bad).tolist()} err {err[bad]} tol {tol[bad]} mass {mass[bad]}"
    return int(ok.sum())


def _check_step(got, x, want, pl, decided, what, scale):
    y, energy, acc, terms, mask = got
    mass, margin = want["remaining_mass"], want["accept_margin"]
    assert y.dtype == np.float16 and y.shape == x.shape and set(np.unique(y)) <= {0.0, 1.0}, what
    assert np.array_equal(mask.astype(np.uint8)[decided], np.asarray(want["mask"]).astype(np.uint8)[decided]), what
    assert bool((mask.sum(axis=1) >= np.clip(pl, 1, x.shape[1])).all()), what
    np.testing.assert_allclose(terms[:, 0], want["ll_x"], rtol=1e-6, err_msg=what)
    np.testing.assert_allclose(terms[decided, 2], want["ll_y"][decided], rtol=1e-6, err_msg=what)
    np.testing.assert_allclose(energy[decided], want["energy"][decided], rtol=1e-6, err_msg=what)
    n_ok = [_ll_close(terms[:, c], want[k], mass, pl, decided, f"{what}/{k}", scale) for c, k in ((1, "ll_x2y"), (3, "ll_y2x"), (4, "log_acc"))]
    fin = np.isfinite(want["log_acc"])
    # the accept test is compared wherever its margin clears the tolerance of log_acc (ll_atol clamps the remaining mass at MIN_MASS)
    sure = decided & (~fin | (margin > 2 * (scale * ll_atol(mass, pl) + RTOL * np.abs(np.where(fin, want["log_acc"], 0)))))
    low = sure & fin & (mass < MIN_MASS)
    if low.any():       # the figures of the samples whose path terms are not compared but whose decision is
        print(f"{what}: below {MIN_MASS} of remaining mass, log_acc here {terms[low, 4]} expected {np.asarray(want['log_acc'])[low]}")
    assert np.array_equal(y[sure].astype(np.float32), np.asarray(want["y"])[sure].astype(np.float32)), what
    # every sample is its input (rejected) or its input with exactly the selected columns flipped (accepted)
    flipped = y.astype(np.float32) != x.astype(np.float32)
    assert all((not flipped[b].any()) or np.array_equal(flipped[b], mask[b].astype(bool)) for b in range(len(x))), what
    return min(n_ok[:2]), int(sure.sum())      # (log_acc is not finite where the reference's f16 energy sum overflows)


def _exempt_cap(left_out, pairs, what):
    assert left_out <= pairs // po.MASK_EXEMPT_ONE_IN, f"{what}: {left_out} of {pairs} samples left out of the mask comparison"


CASES = ["BA_100_ID0", "w3_20", "dense_61"]
# What each step of each trace compares, of its 12 samples: (path terms: samples with MIN_MASS of remaining mass and finite
# reference values, accepted sample: samples whose accept margin clears the tolerance or whose log_acc is not finite) -- counted
# from the fixture and the oracle alone.  Sample 1 draws all Np columns (no mass remains); at T = 0.2 the +-3 weights of w3_20
# leave 3 samples conditioned; dense_61's energies overflow f16 in the reference (-inf, NaN) and its scores are in the hundreds.
COMPARED = {"BA_100_ID0": ((12, 12), (11, 12), (11, 12)), "w3_20": ((12, 12), (11, 12), (3, 11)), "dense_61": ((1, 5), (2, 4), (1, 3))}


@pytest.mark.parametrize("case", CASES)
def test_pisco_step_golden(golden, case):
    """Recorded draws, half_rounding on, against the reference's own class: masks and proposals equal; ll_x, ll_y and the energy
    to 1e-6 relative, ll_x * T bit for bit (integer matrices); path terms within tests/isco_tol.py; accepted samples equal
    wherever the accept test clears the tolerance."""
    z = golden("pisco")
    adj, n = z[f"{case}/adj"], int(z[f"{case}/num_nodes"])
    Np = adj.shape[0]
    s = _sampler(adj, n, 12)
    padded_flips = 0
    for k in range(3):
        t = f"{case}/step{k}"
        T, x, pl = float(z[f"{t}/temperature"]), z[f"{t}/x"].astype(np.float16), z[f"{t}/path_length"]
        ug, ua = z[f"{t}/rand_gumbel"], z[f"{t}/rand_accept"]
        r = po.step(x, adj, pl, T, ug, ua)                  # conditioning / accept margin of every sample: test infrastructure only
        want = {kk: z[f"{t}/{kk}"] for kk in ("mask", "ll_x", "ll_x2y", "ll_y", "ll_y2x", "log_acc", "energy", "acc", "y")}
        want["remaining_mass"], want["accept_margin"] = r["remaining_mass"], r["accept_margin"]
        got = _step(s, x, pl, T, ug, ua)
        assert got[0].shape == (12, Np)
        everyone = np.ones(12, bool)
        n_ok, n_sure = _check_step(got, x, want, pl, everyone, t, 1)
        print(f"{t}: path terms compared on {n_ok} samples, accepted sample on {n_sure}")
        assert n_ok >= COMPARED[case][k][0] and n_sure >= COMPARED[case][k][1], t
        mask = got[4].astype(bool)
        assert np.array_equal(np.where(mask, 1 - x, x).astype(np.uint8), z[f"{t}/y_prop"]), t              # the proposal
        f = np.float32
        assert np.array_equal((got[3][:, 0] * f(T)).astype(f), (z[f"{t}/ll_x"] * f(T)).astype(f), equal_nan=True), t
        padded_flips += int(z[f"{t}/mask"][:, n:].sum())
        # the composed ops against the fused kernel: the energy and the log-probabilities a single draw implies
        e_x, lp_x = s.get_local_dist(_h(x), T)
        assert np.array_equal(e_x.cpu().numpy(), got[3][:, 0], equal_nan=True), t
        one = mask.sum(axis=1) == 1
        assert one[0]
        np.testing.assert_allclose(got[3][one, 1], lp_x.cpu().numpy()[one, mask.argmax(axis=1)[one]], rtol=1e-5, atol=1e-5)
    for T in (1.0, 0.37):
        energy, logp = s.get_local_dist(_h(z[f"{case}/x"]), torch.tensor(T))
        assert energy.dtype == torch.float32 and tuple(logp.shape) == (12, Np)
        assert np.array_equal(energy.cpu().numpy(), z[f"{case}/T{T}/energy"])
        np.testing.assert_allclose(logp.cpu().numpy(), z[f"{case}/T{T}/log_prob"], rtol=1e-5, atol=1e-5)
        e2, grad = s.tensor_core_energy(_h(z[f"{case}/x"]), T)
        assert torch.equal(e2, energy) and tuple(grad.shape) == (12, Np)
    if case == "BA_100_ID0":
        assert padded_flips >= 1           # a padded column takes part in the softmax and the selection


@pytest.mark.parametrize("case", ["BA_100_ID0", "w3_20"])
def test_pisco_composed_pieces_golden(golden, case, monkeypatch):
    """proposal / ll_y2x / select_sample -- the pieces of a step as the reference exposes them, composed here from the product kernel
    and torch ops -- with torch.rand replaced by the recorded draws, against the reference's traces."""
    z = golden("pisco")
    adj, n = z[f"{case}/adj"], int(z[f"{case}/num_nodes"])
    s = _sampler(adj, n, 12)
    for k in range(3):
        t = f"{case}/step{k}"
        T, x, pl = float(z[f"{t}/temperature"]), z[f"{t}/x"].astype(np.float16), z[f"{t}/path_length"]
        draws = [torch.from_numpy(z[f"{t}/rand_gumbel"]).to(DEV), torch.from_numpy(z[f"{t}/rand_accept"]).to(DEV)]
        monkeypatch.setattr(torch, "rand", lambda *a, **kw: draws.pop(0))
        xt = _h(x)
        ll_x, y, traj = s.proposal(xt, torch.from_numpy(pl).to(DEV), torch.tensor(T))
        ll_y, ll_y2x = s.ll_y2x(traj, y, torch.tensor(T))
        log_acc = torch.from_numpy(z[f"{t}/log_acc"]).to(DEV)          # the reference's: select_sample alone is under test
        out = s.select_sample(log_acc, xt, y)
        monkeypatch.undo()
        assert not draws and y.dtype == torch.float16 and out.dtype == torch.float16
        mask = traj["selected_idx"]["selected_mask"].cpu().numpy()
        assert np.array_equal(mask.astype(np.uint8), z[f"{t}/mask"]) and np.array_equal(y.cpu().numpy().astype(np.uint8), z[f"{t}/y_prop"])
        np.testing.assert_allclose(ll_x.cpu().numpy(), z[f"{t}/ll_x"], rtol=1e-6)
        np.testing.assert_allclose(ll_y.cpu().numpy(), z[f"{t}/ll_y"], rtol=1e-6)
        r = po.step(x, adj, pl, T, z[f"{t}/rand_gumbel"], z[f"{t}/rand_accept"])
        everyone = np.ones(12, bool)
        n1 = _ll_close(traj["ll_x2y"].cpu().numpy(), z[f"{t}/ll_x2y"], r["remaining_mass"], pl, everyone, f"{t}/ll_x2y composed", 1)
        n2 = _ll_close(ll_y2x.cpu().numpy(), z[f"{t}/ll_y2x"], r["remaining_mass"], pl, everyone, f"{t}/ll_y2x composed", 1)
        assert min(n1, n2) >= COMPARED[case][k][0]
        clear = r["accept_margin"] > 1e-4                                # log(u) on the device against the reference's on the host
        assert clear.sum() >= 10 and np.array_equal(out.cpu().numpy().astype(np.uint8)[clear], z[f"{t}/y"][clear]), t


def test_pisco_example_runs_and_its_numbers_agree(monkeypatch, capsys):
    """examples/pisco_maxcut.py in-process on its generated +-1 graph (100 nodes: padded to 104, so record() meets the driver's
    shapes), both precisions: exit status 0 = the sampler's own number equals the recomputed weighted cut."""
    import os
    import runpy
    import sys
    path = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "examples", "pisco_maxcut.py")
    for extra in ([], ["--full-precision"]):
        monkeypatch.setattr(sys, "argv", [path, "--batch-size", "16", "--chain-length", "60"] + extra)
        with pytest.raises(SystemExit) as e:
            runpy.run_path(path, run_name="__main__")
        assert e.value.code == 0, capsys.readouterr().out
        assert "weighted cut" in capsys.readouterr().out


FORMS = {64: "wave kernel, keys in registers; again with a 16-entry list", 333: "workgroup kernel, rows no multiple of 64, rank updates of up to 165 rows, f16 rounding of the energy active",
         2100: "wave kernel with keys re-read from LDS (RLS_ISCO_FORCE_WG = 0); again with a 16-entry list",
         2000: "workgroup kernel; again with a 16-entry list: selections ordered by extraction, the order in scratch"}


@pytest.mark.parametrize("n,density,wmax,scale,B,pl_hi,halves", po.EDGE_CASES, ids=[str(c[0]) for c in po.EDGE_CASES])
def test_pisco_step_vs_oracle_at_every_kernel_form(n, density, wmax, scale, B, pl_hi, halves):
    from rlsolver_amd import _abi
    assert n in FORMS
    adj, x0, draws = po.edge_case(n, density, wmax, scale, B, pl_hi)
    Np = adj.shape[0]
    try:
        if n == 2100:
            _abi.tuning_set("RLS_ISCO_FORCE_WG", 0)
        for half in halves:
            s = _sampler(adj, n, B, half_rounding=half)
            x, left_out = x0, 0
            for T, pl, ug, ua in draws:
                assert pl[0] == 1
                r = po.step(x, adj, pl, T, ug, ua, half)
                decided = po.mask_is_decided(x, adj, pl, T, ug, half)
                got = _step(s, x.astype(np.float16), pl, T, ug, ua)
                n_ok, _ = _check_step(got, x, r, pl, decided, f"n={n} half={half} T={T}", po.K_TOL)
                assert n_ok >= B // 4
                left_out += int((~decided).sum())
                # a 16-entry list: selections past it are ordered by extraction, the order in the caller's scratch -- in either
                # kernel (wave per sample: n = 64 and 2100), the same bits
                _abi.tuning_set("RLS_ISCO_SEL_CAP", 16)
                assert int(pl.max()) > 16 and int((got[4].sum(axis=1) > 16).sum()) >= 1
                cap16 = _step(s, x.astype(np.float16), pl, T, ug, ua)
                _abi.tuning_unset("RLS_ISCO_SEL_CAP")
                for a, b in zip(got, cap16):
                    assert np.array_equal(a, b, equal_nan=True)
                x = r["y"]
            _exempt_cap(left_out, len(draws) * B, f"n={n} half={half}")
    finally:
        for k in ("RLS_ISCO_FORCE_WG", "RLS_ISCO_SEL_CAP"):
            _abi.tuning_unset(k)


def test_pisco_and_isco_maxcut_agree_on_a_unit_weight_graph():
    """Same graph (64 nodes, no padding), same x, path lengths and recorded draws: the same masks and accepted samples; the
    energies differ by exactly num_edges / (2T) (PISCO's energy is cut - sum(A) / 4); path terms within tests/isco_tol.py."""
    from rlsolver_amd.envs.env_ISCO import ISCO_maxcut
    from rlsolver_amd.graph import generate_gnm
    n, m, B = 64, 300, 16
    g = np.asarray(generate_gnm(n, m, 4), dtype=np.int64)
    adj = np.zeros((n, n), np.float16)
    adj[g[:, 0], g[:, 1]] = adj[g[:, 1], g[:, 0]] = 1
    p = _sampler(adj, n, B)
    q = ISCO_maxcut({"num_nodes": n, "num_edges": m, "edge_from": torch.from_numpy(g[:, 0].copy()).to(DEV),
                     "edge_to": torch.from_numpy(g[:, 1].copy()).to(DEV)}, batch_size=B, device=DEV)
    rng = np.random.RandomState(5)
    x = (rng.rand(B, n) < 0.5).astype(np.float32)
    for T in (1.0, 0.5):
        pl = rng.randint(1, 20, size=B).astype(np.int64)
        pl[0] = 1
        ug, ua = rng.rand(B, n).astype(np.float32).clip(1e-7, 1 - 1e-7), rng.rand(B).astype(np.float32)
        d = {"u_gumbel": torch.from_numpy(ug), "u_accept": torch.from_numpy(ua)}
        yp, ep, ap, tp, mp = [o.cpu().numpy() for o in p.step(_h(x), torch.from_numpy(pl).to(DEV), T, draws=d, want_terms=True)]
        yq, eq, aq, tq, mq = [o.cpu().numpy() for o in q.step(torch.from_numpy(x).to(DEV), torch.from_numpy(pl).to(DEV), T, draws=d, want_terms=True)]
        assert np.array_equal(mp, mq) and np.array_equal(yp.astype(np.float32), yq)
        shift = np.float32(m / (2 * T))
        assert np.array_equal(tq[:, 0] - tp[:, 0], np.full(B, shift)) and np.array_equal(tq[:, 2] - tp[:, 2], np.full(B, shift))
        assert np.array_equal(eq - ep, np.full(B, np.float32(m / 2)))
        r = po.step(x, adj, pl, T, ug, ua)
        for c in (1, 3, 4):
            err = np.abs(tp[:, c].astype(np.float64) - tq[:, c])
            tol = ll_atol(r["remaining_mass"], pl) + RTOL * np.abs(tq[:, c])
            ok = r["remaining_mass"] >= 1e-6
            assert ok.sum() >= B // 2 and (err <= tol)[ok].all(), (T, c, err, tol)
        x = yq


# ------------------------------------------------------------------------------------------------ contract
def test_pisco_step_contract_checks_come_before_any_launch():
    """Aliasing, a short scratch, Np = 12 and temperature = 0 return RLS_EINVAL, an Np past the rows-in-LDS limit
    RLS_EUNSUPPORTED (a size check: it comes before the pointer and scratch checks, so the real, small buffers reach it);
    nothing is launched: the outputs keep their fill.  B = 0 is a no-op."""
    from rlsolver_amd import _abi
    Np, B = 64, 3
    adj = _h(po.dense_graph(Np, 0.5, 3, 1))
    x = _h((np.random.RandomState(0).rand(B, Np) < 0.5))
    y = torch.full((B, Np), 7, dtype=torch.float16, device=DEV)
    pl = torch.ones(B, dtype=torch.int64, device=DEV)
    energy = torch.full((B,), -77.0, device=DEV)
    scratch = torch.zeros(B * Np * 8, dtype=torch.uint8, device=DEV)
    ptr = lambda t: C.c_void_p(t.data_ptr())

    def call(**over):
        a = dict(adj=ptr(adj), Np=Np, x=ptr(x), y_out=ptr(y), B=B, path_length=ptr(pl), temperature=1.0, half=1, ug=None, ua=None,
                 seed=1, off=0, energy=ptr(energy), acc=None, terms=None, mask=None, scratch=ptr(scratch),
                 scratch_bytes=scratch.numel(), stream=None)
        a.update(over)
        _abi.call("rls_pisco_step", *a.values())

    for over, code in ((dict(y_out=ptr(x)), "EINVAL"), (dict(scratch_bytes=scratch.numel() - 1), "EINVAL"), (dict(Np=12), "EINVAL"),
                       (dict(temperature=0.0), "EINVAL"), (dict(Np=20000), "EUNSUPPORTED")):
        with pytest.raises(_abi.RlsError) as e:
            call(**over)
        assert code in str(e.value), over
    call(B=0)
    torch.cuda.synchronize()
    assert bool((y == 7).all()) and bool((energy == -77.0).all()) and not bool(scratch.any())
    call()                                                   # and the same arguments unchanged do run
    torch.cuda.synchronize()
    assert set(np.unique(y.cpu().numpy())) <= {0.0, 1.0} and bool((energy != -77.0).all())


# ------------------------------------------------------------------------------------------------ production draws
def _ba104():
    from rlsolver_amd.graph import generate_ba
    g = np.asarray(generate_ba(100, 4, 0), dtype=np.int64)
    adj = np.zeros((104, 104), np.float16)
    adj[g[:, 0], g[:, 1]] = adj[g[:, 1], g[:, 0]] = 1
    return adj


def _pad(x, Np):
    return torch.nn.functional.pad(x, (0, Np - x.shape[1]), mode="constant", value=0).contiguous()


def test_pisco_production_draws_shard_invariance_and_seeds():
    adj = _ba104()
    n, Np, B = 100, 104, 64

    def run(off, count, steps, seed=3):
        s = _sampler(adj, n, count, env_offset=off)
        torch.manual_seed(seed)
        x = _pad(s.random_gen_init_sample(), Np)
        assert x.dtype == torch.float16 and tuple(x.shape) == (count, Np)
        outs = [x.clone()]
        for t in range(steps):
            x, e, acc = s.step(x, torch.full((count,), 4, dtype=torch.int64, device=DEV), 0.5)
            assert bool(((acc >= 0) & (acc <= 1)).all())
            outs += [x.clone(), e.clone(), acc.clone()]
        return outs

    w = run(0, B, 30)
    assert set(np.unique(w[-3].cpu().numpy())) <= {0.0, 1.0} and not torch.equal(w[-3], w[0])
    for a, b in zip(run(0, B, 30), w):
        assert torch.equal(a, b)
    for off in (0, B // 2):
        for a, b in zip(run(off, B // 2, 3), w):
            assert torch.equal(a, b[off:off + B // 2])
    other = run(0, B, 3, seed=4)
    assert not torch.equal(other[0], w[0]) and not torch.equal(other[3], w[3])


def test_pisco_example_loop_keeps_acceptance_and_mu_in_range():
    """200 steps of main_PISCO_maxcut.py's loop (Poisson path lengths, mu adapted towards 0.574 acceptance, linear temperature)
    on a 104-column graph: batch acceptance rates stay inside (0, 1) and mu inside [1, Np]."""
    adj = _ba104()
    n, Np, B, steps = 100, 104, 64, 200
    s = _sampler(adj, n, B, chain_length=steps)
    torch.manual_seed(7)
    x = _pad(s.random_gen_init_sample(), Np)
    mu = torch.full((B,), 10.0, device=DEV)
    rates = []
    for it in range(steps):
        pl = torch.clamp(torch.poisson(mu), min=1, max=n).long()
        T = s.init_temperature - it / s.chain_length * (s.init_temperature - s.final_temperature)
        x, en, acc = s.step(x, pl, T)
        mu = torch.clamp(mu + 0.01 * (acc - 0.574), min=1.0, max=float(n))
        rates.append(acc.mean())
    rates = torch.stack(rates).cpu().numpy()
    print(f"acceptance rate min {rates.min():.3f} max {rates.max():.3f}, mu in [{float(mu.min()):.2f}, {float(mu.max()):.2f}]")
    assert (rates > 0).all() and (rates < 1).all()
    assert float(mu.min()) >= 1.0 and float(mu.max()) <= Np


# ------------------------------------------------------------------------------------------------ anneal
def _components_graph(seed):
    """64 nodes, +-1 weights: four 16-node components, each small enough for the host to enumerate."""
    r = np.random.RandomState(seed)
    A = np.zeros((64, 64), np.int64)
    for c in range(4):
        for u in range(16 * c, 16 * c + 16):
            for v in range(u + 1, 16 * c + 16):
                if r.rand() < 0.5:
                    A[u, v] = A[v, u] = r.choice([-1, 1])
    return A


def _best_cut_gray(S):
    """Maximum cut of a small weighted graph by a Gray-code walk over the assignments of all nodes but the last."""
    n = len(S)
    d = -np.ones(n, np.int64)
    r = d @ S
    cut = best = int((S.sum() - r @ d) // 4)
    for i in range(1, 1 << (n - 1)):
        k = (i & -i).bit_length() - 1
        cut += int(d[k] * r[k])                      # flipping k: every edge to a same-side node becomes cut, and the reverse
        d[k] = -d[k]
        r += 2 * d[k] * S[k]
        best = max(best, cut)
    return best


def test_pisco_anneals_to_the_optimum_of_a_signed_graph():
    """64 chains x 400 steps of the example's schedule on a +-1-weighted 64-node graph whose optimum the host finds by Gray code
    (four 16-node components: 64 nodes at once cannot be enumerated): at least one chain reaches the optimum cut, and
    0.25 * sum(A) + the best energy equals the weighted cut of that sample recomputed from ops.maxcut_delta_all on the weighted CSR."""
    from rlsolver_amd import ops
    from rlsolver_amd.envs.env_PISCO_maxcut import record
    from tests.gpu_util import device_graph
    A = _components_graph(1)
    opt = sum(_best_cut_gray(A[16 * c:16 * c + 16, 16 * c:16 * c + 16]) for c in range(4))
    n, B, steps = 64, 64, 400
    s = _sampler(A.astype(np.float16), n, B, chain_length=steps)
    torch.manual_seed(11)
    x = s.random_gen_init_sample()
    mu = torch.full((B,), 10.0, device=DEV)
    best_e = torch.tensor(-1e9, device=DEV)
    best_x = torch.zeros(n, dtype=torch.float16, device=DEV)
    for it in range(steps):
        pl = torch.clamp(torch.poisson(mu), min=1, max=n).long()
        T = s.init_temperature - it / s.chain_length * (s.init_temperature - s.final_temperature)
        x, en, acc = s.step(x, pl, T)
        mu = torch.clamp(mu + 0.01 * (acc - 0.574), min=1.0, max=float(n))
        # `en` is the PROPOSAL's energy (as the reference returns it), accepted or not: record the energy of the kept samples
        best_e, best_x = record(best_e, best_x, s.tensor_core_energy(x, 1.0)[0], x)
    # ops.maxcut_obj (K1) counts cut edges; the WEIGHTED cut comes from K3's weighted flip gains on the CSR form of the same graph,
    # sum_i gain_i = delta' A delta: an independent kernel on an independent layout
    iu, ju = np.nonzero(np.triu(A))
    g = device_graph(np.stack([iu, ju, A[iu, ju]], axis=1), n, False, use_weights=True)
    gains = ops.maxcut_delta_all(g, (best_x > 0)[None, :].contiguous())
    cut = (int(A.sum()) - int(gains.sum())) // 4
    d = best_x.cpu().numpy().astype(np.int64) * 2 - 1
    assert cut == int((A.sum() - d @ A @ d) // 4)
    sampler_cut = 0.25 * float(s.sum_A) + float(best_e)
    print(f"optimum {opt}, best cut {cut}, sampler's own number {sampler_cut}")
    assert sampler_cut == cut
    assert cut == opt, f"best cut {cut} of 64 chains x 400 steps, optimum {opt}"
