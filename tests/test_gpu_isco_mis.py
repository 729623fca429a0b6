"""ISCO_MIS on the GPU: the fused step (rls_isco_mis_step) and the composed get_local_dist / model against traces of the
reference's ISCO_MIS (tests/golden/isco_mis.npz) and against the numpy oracle (tests/mis_oracle.py) at every kernel form.

Discrete results are exact.  The mask may leave out an env only where the oracle's L-th and (L+1)-th largest perturbed values
nearly tie (mis_oracle.mask_is_decided), at most one env in 50 per test.  Path log-probabilities: the form of
tests/isco_tol.py scaled by mis_oracle.K_TOL (measured between oracle and reference, not against the kernel)."""
import numpy as np
import pytest
import torch

from tests import mis_oracle as mo
from tests.gpu_util import DEV
from tests.isco_tol import RTOL, ll_atol

pytestmark = pytest.mark.gpu
LAM = 1.001


def _sampler(eu, ev, n, B, **kw):
    from rlsolver_amd.envs.env_ISCO import ISCO_MIS
    params = {"num_nodes": n, "num_edges": len(eu), "edge_from": torch.from_numpy(np.ascontiguousarray(eu)).to(DEV),
              "edge_to": torch.from_numpy(np.ascontiguousarray(ev)).to(DEV)}
    return ISCO_MIS(params, batch_size=B, device=DEV, **kw)


def _step(s, x, pl, T, ug, ua):
    out = s.step(torch.from_numpy(x).to(DEV).float(), torch.from_numpy(pl).to(DEV), T,
                 draws={"u_gumbel": torch.from_numpy(ug), "u_accept": torch.from_numpy(ua)}, want_terms=True)
    return [o.cpu().numpy() for o in out]


def _ll_close(actual, desired, mass, pl, use, what):
    err = np.abs(actual.astype(np.float64) - desired)
    tol = mo.K_TOL * ll_atol(mass, pl) + RTOL * np.abs(desired)
    ok = (mass >= 1e-6) & use
    bad = ok & ~(err <= tol)
    print(f"{what}: {int(ok.sum())} envs, largest error / tolerance {np.where(ok, err / tol, 0).max():.3f}")
    assert not bad.any(), f"{what}: envs {np.flatnonzero(bad).tolist()} err {err[bad]} tol {tol[bad]} mass {mass[bad]}"
    return int(ok.sum())


def _check_mis(got, x, want, pl, decided, what):
    """_check_maxcut of tests/test_gpu_isco_steps.py with the mask rule and the scaled tolerance; -> (envs whose path
    log-probabilities were compared, envs whose accepted sample was compared)."""
    y, energy, acc, terms, mask = got
    mass, margin = want["remaining_mass"], want["accept_margin"]
    assert np.array_equal(mask.astype(np.uint8)[decided], want["mask"].astype(np.uint8)[decided]), what
    assert bool((mask.sum(axis=1) >= np.clip(pl, 1, x.shape[1])).all()), what
    np.testing.assert_allclose(terms[:, 0], want["ll_x"], rtol=RTOL, atol=1e-5)
    np.testing.assert_allclose(terms[decided, 2], want["ll_y"][decided], rtol=RTOL, atol=1e-5)
    np.testing.assert_allclose(energy[decided], want["energy"][decided], rtol=RTOL, atol=1e-5)
    n_ok = [_ll_close(terms[:, c], want[k], mass, pl, decided, f"{what}/{k}") for c, k in ((1, "ll_x2y"), (3, "ll_y2x"), (4, "log_acc"))]
    ok = (mass >= 1e-6) & decided
    assert bool((np.abs(acc - want["acc"])[ok] <= 2 * mo.K_TOL * ll_atol(mass, pl)[ok]).all()), what
    sure = decided & (margin > 2 * (mo.K_TOL * ll_atol(mass, pl) + RTOL * np.abs(want["log_acc"])))
    assert np.array_equal(y[sure], want["y"][sure].astype(np.float32)), what
    assert set(np.unique(y)) <= {0.0, 1.0}
    # every sample is its input (rejected) or its input with exactly the selected nodes flipped (accepted)
    flipped = y != x
    assert all((not flipped[b].any()) or np.array_equal(flipped[b], mask[b].astype(bool)) for b in range(len(x))), what
    return min(n_ok), int(sure.sum())


def _exempt_cap(left_out, envs, what):
    assert left_out <= envs // mo.MASK_EXEMPT_ONE_IN, f"{what}: {left_out} of {envs} envs left out of the mask comparison"


GRAPHS = ["BA_100_ID0", "PL_20_ID0", "loader_13"]


@pytest.mark.parametrize("gname", GRAPHS)
def test_isco_mis_local_dist_golden(golden, gname):
    z = golden("isco_mis")
    g = z[f"{gname}/graph"]
    n = z[f"{gname}/x"].shape[1]
    s = _sampler(g[:, 0], g[:, 1], n, 12, lam=float(z["lam"]))
    x = torch.from_numpy(z[f"{gname}/x"]).to(DEV).float()
    for T in (1.0, 0.37):
        energy, logp = s.get_local_dist(x, torch.tensor(T))
        assert energy.dtype == torch.float32 and logp.shape == (12, n)
        np.testing.assert_allclose(energy.cpu().numpy(), z[f"{gname}/T{T}/energy"], rtol=1e-6)
        np.testing.assert_allclose(logp.cpu().numpy(), z[f"{gname}/T{T}/log_prob"], rtol=1e-5, atol=1e-5)
        np.testing.assert_allclose(s.model(x, T).cpu().numpy(), z[f"{gname}/T{T}/energy"], rtol=1e-6)


@pytest.mark.parametrize("gname", GRAPHS)
def test_isco_mis_step_golden(golden, gname):
    z = golden("isco_mis")
    g = z[f"{gname}/graph"]
    eu, ev, lam = g[:, 0], g[:, 1], float(z["lam"])
    n = z[f"{gname}/x"].shape[1]
    s = _sampler(eu, ev, n, 12, lam=lam)
    left_out = 0
    for k in range(3):
        t = f"{gname}/step{k}"
        T, x, pl = float(z[f"{t}/temperature"]), z[f"{t}/x"].astype(np.float32), z[f"{t}/path_length"]
        ug, ua = z[f"{t}/rand_gumbel"], z[f"{t}/rand_accept"]
        # conditioning / accept margin / threshold gap of every env: from the oracle, test infrastructure only
        r = mo.mis_step(x, eu, ev, lam, pl, T, ug, ua)
        decided = mo.mask_is_decided(x, eu, ev, lam, pl, T, ug)
        want = {kk: z[f"{t}/{kk}"] for kk in ("mask", "ll_x", "ll_x2y", "ll_y", "ll_y2x", "log_acc", "energy", "acc", "y")}
        want["remaining_mass"], want["accept_margin"] = r["remaining_mass"], r["accept_margin"]
        got = _step(s, x, pl, T, ug, ua)
        n_ok, n_sure = _check_mis(got, x, want, pl, decided, t)
        assert n_ok >= (10 if n > 13 else 8) and n_sure >= 8
        left_out += int((~decided).sum())
        # the fused kernel against the composed ops: the energies of x and of the proposal ...
        terms, mask = got[3], got[4].astype(bool)
        xt = torch.from_numpy(x).to(DEV)
        yp = torch.from_numpy(np.where(mask, 1 - x, x)).to(DEV)
        np.testing.assert_allclose(terms[:, 0], s.model(xt, T).cpu().numpy(), rtol=1e-6)
        np.testing.assert_allclose(terms[:, 2], s.model(yp, T).cpu().numpy(), rtol=1e-6)
        e_y, lp_y = s.get_local_dist(yp, T)
        np.testing.assert_allclose(terms[:, 2], e_y.cpu().numpy(), rtol=1e-6)
        # ... and its log-probabilities, which a single draw implies: ll_x2y = log_prob(x)[node], ll_y2x = log_prob(y)[node]
        one = mask.sum(axis=1) == 1
        node = mask.argmax(axis=1)
        lp_x = s.get_local_dist(xt, T)[1].cpu().numpy()
        assert one[0] and one.sum() >= 1
        np.testing.assert_allclose(terms[one, 1], lp_x[one, node[one]], rtol=1e-5, atol=1e-5)
        np.testing.assert_allclose(terms[one, 3], lp_y.cpu().numpy()[one, node[one]], rtol=1e-5, atol=1e-5)
    _exempt_cap(left_out, 36, gname)


# the knobs that force a case's kernel form (rows: mis_oracle.EDGE_CASES)
FORMS = {64: "wave kernel, keys in registers", 333: "workgroup kernel, rows no multiple of 64",
         2100: "wave kernel with keys re-read from LDS", 2000: "workgroup kernel, path lengths up to n / 2",
         3000: "rows in LDS, rows in scratch, selections past the list"}


@pytest.mark.parametrize("n,m,B,pl_hi", mo.EDGE_CASES, ids=[str(c[0]) for c in mo.EDGE_CASES])
def test_isco_mis_step_vs_oracle_at_every_kernel_form(n, m, B, pl_hi):
    from rlsolver_amd import _abi
    assert n in FORMS
    eu, ev, x, draws = mo.edge_case(n, m, B, pl_hi)
    assert (eu == ev).any() and len(np.unique(np.minimum(eu, ev) * n + np.maximum(eu, ev))) < m      # loops, repeated and reversed lines
    s = _sampler(eu, ev, n, B, lam=LAM)
    left_out = 0
    try:
        if n == 2100:
            _abi.tuning_set("RLS_ISCO_FORCE_WG", 0)
        for T, pl, ug, ua in draws:
            assert pl[0] == 1
            r = mo.mis_step(x, eu, ev, LAM, pl, T, ug, ua)
            decided = mo.mask_is_decided(x, eu, ev, LAM, pl, T, ug)
            got = _step(s, x, pl, T, ug, ua)
            n_ok, _ = _check_mis(got, x, r, pl, decided, f"n={n} T={T}")
            assert n_ok >= B // 2
            left_out += int((~decided).sum())
            if n == 3000:      # the MaxCut test's claim, for MIS: the same bits with the rows in scratch and by extraction
                assert s._step_scratch(B) is None
                _abi.tuning_set("RLS_ISCO_GLOBAL_ROWS", 1)
                assert s._step_scratch(B).numel() == B * n * 8
                rows = _step(s, x, pl, T, ug, ua)
                _abi.tuning_set("RLS_ISCO_SEL_CAP", 16)
                assert int(pl.max()) > 16
                rows16 = _step(s, x, pl, T, ug, ua)
                _abi.tuning_unset("RLS_ISCO_GLOBAL_ROWS")
                _abi.tuning_unset("RLS_ISCO_SEL_CAP")
                for a, b, c in zip(got, rows, rows16):
                    assert np.array_equal(a, b) and np.array_equal(a, c)
            x = r["y"]
    finally:
        for k in ("RLS_ISCO_FORCE_WG", "RLS_ISCO_GLOBAL_ROWS", "RLS_ISCO_SEL_CAP"):
            _abi.tuning_unset(k)
    _exempt_cap(left_out, 2 * B, f"n={n}")


@pytest.mark.parametrize("force_wg", [0, 1])
@pytest.mark.parametrize("slabs", [True, False])
def test_isco_mis_padding_and_loops(slabs, force_wg):
    """A hub whose slab row takes many batches of eight rounds beside degree-1 and isolated nodes of its 64-node group: their
    rows are padding (the node itself) almost everywhere, which a count of set neighbours over the slab would add to every
    set node.  Through the lane-per-node slabs and through the CSR (a graph handle with weights has no slab path), both
    kernels, with an all-ones and an all-zeros sample in the batch."""
    from rlsolver_amd import _abi, ops
    n, B, isolated = 700, 6, (3, 17, 40, 63, 64, 699)
    eu = np.array([0] * (n - 1 - len(isolated)) + [5, 0], dtype=np.int64)
    ev = np.array([v for v in range(1, n) if v not in isolated] + [5, 9], dtype=np.int64)     # a loop (5, 5), (0, 9) twice
    s = _sampler(eu, ev, n, B, lam=LAM)
    if not slabs:
        s.graph = ops.DeviceGraph(s.graph.csr, DEV, use_weights=True)
    assert int(s.graph.struct.ell_sym_ptr) != 0 and (s.graph.wgt is None) == slabs
    rng = np.random.RandomState(7)
    x = (rng.rand(B, n) < 0.25).astype(np.float32)
    x[0], x[1] = 1.0, 0.0
    x[2, 0], x[3, 0], x[2, 5], x[3, 5] = 1.0, 0.0, 1.0, 0.0
    _abi.tuning_set("RLS_ISCO_FORCE_WG", force_wg)
    try:
        left_out = 0
        for T in (1.0, 0.5):
            pl = rng.randint(1, 12, size=B).astype(np.int64)
            pl[0] = 1
            ug = rng.rand(B, n).astype(np.float32).clip(1e-7, 1 - 1e-7)
            ua = rng.rand(B).astype(np.float32)
            r = mo.mis_step(x, eu, ev, LAM, pl, T, ug, ua)
            decided = mo.mask_is_decided(x, eu, ev, LAM, pl, T, ug)
            got = _step(s, x, pl, T, ug, ua)
            _check_mis(got, x, r, pl, decided, f"slabs={slabs} wg={force_wg} T={T}")
            left_out += int((~decided).sum())
            f = np.float32
            assert got[3][0, 0] == (f(n) - f(LAM) * f(len(eu))) / f(T)          # all ones: every edge-list entry is inside the set
            assert got[3][1, 0] == 0.0                                           # all zeros
    finally:
        _abi.tuning_unset("RLS_ISCO_FORCE_WG")
    _exempt_cap(left_out, 2 * B, "padding and loops")


def _ba100():
    from rlsolver_amd.graph import generate_ba
    g = np.asarray(generate_ba(100, 4, 0), dtype=np.int64)
    return g[:, 0].copy(), g[:, 1].copy()


def test_isco_mis_production_draws():
    """torch.manual_seed reproduces a run; samples stay 0/1; half batches at env_offset 0 and B / 2 are the whole batch bit for
    bit (the sharding contract of tests/test_gpu_shard_invariance.py)."""
    eu, ev = _ba100()
    n, B = 100, 64

    def run(off, count, steps):
        s = _sampler(eu, ev, n, count, env_offset=off)
        torch.manual_seed(3)
        x = s.random_gen_init_sample()
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


def test_isco_mis_anneals_to_an_independent_set():
    """300 steps of the example's schedule (examples/isco_mis.py: linear temperature, path lengths around 4) on a BA-100
    graph: the batch mean of the energy rises and the best sample violates no edge.

    With lam = 1.001 a set of 44 nodes and one violated edge scores 42.999 against 43 for a clean set of 43, so after only
    300 steps which of the two is the batch's best depends on the draws: the same schedule run through tests/mis_oracle.py
    with numpy draws (64 chains, six seeds) ended with a clean best sample four times and one violated edge twice, the
    mean energy rising from about -47 to 42 every time.  The assertion reports the count."""
    eu, ev = _ba100()
    n, B, steps = 100, 64, 300
    s = _sampler(eu, ev, n, B, chain_length=steps)
    torch.manual_seed(11)
    x = s.random_gen_init_sample()
    e0 = float(s.model(x, 1.0).mean())
    mu = torch.full((B,), 4.0, device=DEV)
    for it in range(steps):
        pl = torch.clamp(torch.poisson(mu), min=1, max=n).long()
        T = s.init_temperature - it / s.chain_length * (s.init_temperature - s.final_temperature)
        x, en, acc = s.step(x, pl, T)
    e = s.model(x, 1.0)
    assert float(e.mean()) > e0
    best = x[int(e.argmax())].cpu().numpy()
    violated = int((best[eu] * best[ev]).sum())
    print(f"mean energy {e0:.2f} -> {float(e.mean()):.2f}, best set {int(best.sum())} nodes, {violated} violated edges")
    assert violated == 0, f"the best sample violates {violated} edges"
