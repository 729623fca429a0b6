"""Fuzz of the PISCO_maxcut sampler step (rls_pisco_product + rls_pisco_step) against the numpy oracle of tests/pisco_oracle.py
with recorded draws: random n (so random padding), density, integer weight range, batch, temperature, half_rounding and path
lengths, the wave-per-sample or the workgroup-per-sample kernel, the list capacity cut to 16 now and then.  The product is
compared exactly; the step by the rules of tests/test_gpu_pisco.py: the selected columns exactly unless the oracle's threshold
gap is below 1e-5 (at most one sample in 50 over the run), energies to 1e-6, path log-probabilities within K_TOL x the tolerance
of tests/isco_tol.py (log_acc: plus the float32 rounding of its four terms, as tools/fuzz/fuzz_isco.py allows), accepted
samples away from the accept margin, plus the invariants of a step.
`python tools/fuzz/fuzz_pisco.py [seconds] [seed]`."""
import sys, time
import numpy as np, torch
sys.path.insert(0, ".")
from tests import pisco_oracle as po
from tests.isco_tol import RTOL, ll_atol
from rlsolver_amd import _abi, ops
from rlsolver_amd.envs.env_ISCO import PISCO_maxcut

DEV = torch.device("cuda:0")
budget = float(sys.argv[1]) if len(sys.argv) > 1 else 60.0
rng = np.random.RandomState(int(sys.argv[2]) if len(sys.argv) > 2 else 0)
t_end = time.time() + budget
it = envs = left_out = 0
while time.time() < t_end:
    n = int(rng.choice([rng.randint(3, 64), rng.randint(64, 256), rng.randint(256, 900), rng.randint(900, 2300)]))
    wmax = int(rng.choice([1, 2, 3]))
    deg = float(rng.choice([2, 6, 20]))                    # mean degree: scores of a few units, so that most samples stay conditioned
    density = min(1.0, deg / n)
    # scale 41: sum_k r_k delta_k becomes an even number of thousands, past what f16 holds exactly (half_rounding then matters) but,
    # on these sizes, far below its overflow
    scale = int(rng.choice([1, 1, 41])) if n <= 400 and deg <= 6 else 1
    adj = (po.dense_graph(n, density, wmax, int(rng.randint(1 << 30))).astype(np.float64) * scale).astype(np.float16)
    Np = adj.shape[0]
    B = int(rng.choice([1, 7, 64, 600 if n < 1200 else 40]))
    T = float(np.float32(rng.choice([0.3, 0.7, 1.5]) * scale))
    half = bool(rng.rand() < 0.7)
    force_wg, cap16 = int(rng.randint(0, 2)), bool(rng.rand() < 0.25)
    tag = f"it={it} n={n} Np={Np} density={density:.3f} wmax={wmax} scale={scale} B={B} T={T} half={half} wg={force_wg} cap16={cap16}"
    if "-v" in sys.argv:
        print(tag, flush=True)
    iu, ju = np.nonzero(np.triu(adj.astype(np.float64)))
    A = torch.from_numpy(adj).to(DEV)
    s = PISCO_maxcut({"num_nodes": n, "num_edges": len(iu), "edge_from": torch.from_numpy(iu).to(DEV), "edge_to": torch.from_numpy(ju).to(DEV),
                      "adj_matrix": A}, batch_size=B, device=DEV, half_rounding=half)
    x = (rng.rand(B, Np) < rng.choice([0.1, 0.5])).astype(np.float32)        # set bits in the padded columns too
    pl = rng.randint(1, max(2, min(40, Np)), size=B).astype(np.int64)
    if rng.rand() < 0.3:
        pl[int(rng.randint(0, B))] = int(rng.randint(1, Np + 1))
    ug = rng.rand(B, Np).astype(np.float32).clip(1e-7, 1 - 1e-7)
    ua = rng.rand(B).astype(np.float32)
    xh = torch.from_numpy(x.astype(np.float16)).to(DEV)
    prod = ops.pisco_product(A, xh).cpu().numpy()
    assert np.array_equal(prod, po.product(x, adj).astype(np.float32)), "product " + tag
    _abi.tuning_set("RLS_ISCO_FORCE_WG", force_wg)
    if cap16:
        _abi.tuning_set("RLS_ISCO_SEL_CAP", 16)
    try:
        out = s.step(xh, torch.from_numpy(pl).to(DEV), T, draws={"u_gumbel": torch.from_numpy(ug), "u_accept": torch.from_numpy(ua)},
                     want_terms=True)
    finally:
        _abi.tuning_unset("RLS_ISCO_FORCE_WG")
        _abi.tuning_unset("RLS_ISCO_SEL_CAP")
    y, energy, acc, terms, mask = (o.cpu().numpy() for o in out)
    y = y.astype(np.float32)
    check = min(B, 64)                                    # the oracle sorts whole rows: a part of a large batch
    c = slice(0, check)
    r = po.step(x[c], adj, pl[c], T, ug[c], ua[c], half)
    decided = po.mask_is_decided(x[c], adj, pl[c], T, ug[c], half)
    envs, left_out = envs + check, left_out + int((~decided).sum())
    assert np.array_equal(mask[c][decided].astype(np.uint8), r["mask"][decided].astype(np.uint8)), "selected columns " + tag
    assert bool((mask.sum(1) >= np.minimum(pl, Np)).all()), "path length " + tag      # ties at the threshold are all selected
    np.testing.assert_allclose(terms[c, 0], r["ll_x"], rtol=1e-6, err_msg="ll_x " + tag)
    np.testing.assert_allclose(terms[c, 2][decided], r["ll_y"][decided], rtol=1e-6, err_msg="ll_y " + tag)
    mass = r["remaining_mass"]
    ok = (mass >= 1e-6) & decided
    tol0 = po.K_TOL * ll_atol(mass, pl[c])
    big_terms = 4e-7 * (np.abs(r["ll_x"]) + np.abs(r["ll_y"]) + np.abs(r["ll_x2y"]) + np.abs(r["ll_y2x"]))
    for col, key in ((1, "ll_x2y"), (3, "ll_y2x"), (4, "log_acc")):
        err = np.abs(terms[c, col].astype(np.float64) - r[key])
        tolv = tol0 + RTOL * np.abs(r[key]) + (big_terms if key == "log_acc" else 0.0)
        bad = ok & ~(err <= tolv)
        assert not bad.any(), f"{key} {tag} samples {np.flatnonzero(bad).tolist()} err {err[bad]} tol {tolv[bad]} mass {mass[bad]} L {pl[c][bad]}"
    # (ok: below 1e-6 of remaining mass log_acc itself is not compared, so neither is the decision taken on it -- fuzz_isco.py)
    sure = ok & (r["accept_margin"] > 2 * (tol0 + big_terms + RTOL * np.abs(r["log_acc"])))
    assert np.array_equal(y[c][sure], r["y"][sure].astype(np.float32)), "accepted samples " + tag
    prop = np.where(mask.astype(bool), 1 - x, x)
    changed = (y != x).any(1)
    assert np.array_equal(y[changed], prop[changed]) and set(np.unique(y)) <= {0.0, 1.0}, "an accepted sample is the proposal " + tag
    it += 1
assert left_out <= envs // po.MASK_EXEMPT_ONE_IN, f"{left_out} of {envs} samples left out of the mask comparison"
print(f"fuzz_pisco: {it} random configurations ({left_out} of {envs} samples with a tied threshold), no mismatch")
