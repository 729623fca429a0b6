"""Differential fuzz of the QUBO coordinate search (K11 on the matrix cores, and its CSR form: one wave in row order, and by
levels) against the reference's variable-by-variable loop (MCPG/sampling.py:332-337, :357-362), restated below in float64
over each row's nonzero entries -- the loop of oracle_np.qubo_local_search_value, kept here so that the fuzzer needs no more
of the oracle package than the suite slice that runs it.  Random sizes on both sides of every block boundary; symmetric,
upper / lower triangular and asymmetric patterns (the reference takes Q as given); integer or quarter-valued matrices (every
sum exact in float32), with and without a diagonal, dense, sparse, diagonal-only or zero; 0-3 sweeps; chain counts around
the 32 / 64-chain tiles and the wave split; the level kernel's waves per tile forced to 4 / 8 / 16 or left to the launcher.
`python tools/fuzz/fuzz_qubo.py [seconds] [seed]`."""
import sys, time
import numpy as np, torch
sys.path.insert(0, ".")
from rlsolver_amd import _abi
from rlsolver_amd.methods import MCPG_qubo as q

DEV = torch.device("cuda:0")


def reference_sweep(Qn, x0, num_ls, binary):
    """for cnt < num_ls: for i < n: s_i := 0; res = Q[i, :] . s; s_i := res > thr_i (0 for +-1 spins, -Q_ii / 2 for 0/1);
    then value = s^T Q s.  Any square Q (the reference neither symmetrises nor checks it).  -> (x 0/1 f32, value f32)"""
    Q = np.asarray(Qn, np.float64)
    rows = [(np.nonzero(Q[i])[0], Q[i][np.nonzero(Q[i])[0]]) for i in range(Q.shape[0])]
    s = x0.astype(np.float64) if binary else 2.0 * x0.astype(np.float64) - 1.0
    for cnt in range(num_ls):
        for i, (c, v) in enumerate(rows):
            s[i] = 0.0
            res = v @ s[c] if c.size else np.zeros(s.shape[1])
            hit = res > (-Q[i, i] / 2.0 if binary else 0.0)
            s[i] = hit if binary else 2.0 * hit - 1.0
    value = np.zeros(s.shape[1])
    for i, (c, v) in enumerate(rows):
        if c.size:
            value += s[i] * (v @ s[c])
    return (s if binary else (s + 1.0) / 2.0).astype(np.float32), value.astype(np.float32)


dev = lambda a: torch.from_numpy(np.ascontiguousarray(a)).to(DEV)
budget = float(sys.argv[1]) if len(sys.argv) > 1 else 60.0
rng = np.random.RandomState(int(sys.argv[2]) if len(sys.argv) > 2 else 0)
t_end = time.time() + budget
it = 0
while time.time() < t_end:
    n = int(rng.choice([rng.randint(1, 40), rng.randint(30, 70), rng.randint(60, 300), rng.randint(300, 700)]))
    C = int(rng.choice([1, 5, 31, 32, 33, 63, 64, 65, 130, 300]))
    density = float(rng.choice([1.0, 0.8, 0.2, 0.02, 0.0]))
    pattern = str(rng.choice(["symmetric", "upper", "lower", "asymmetric", "diagonal"]))
    quarters = bool(rng.rand() < 0.3)
    Qn = (rng.randint(-40, 41, size=(n, n)) * (rng.rand(n, n) < density)).astype(np.float32)
    if quarters:
        Qn = np.round(Qn / 5) / 4                                 # +-[0, 2] in quarters: |sums| < 700^2 * 2 < 2^22, still exact
    if pattern == "symmetric":
        Qn = np.triu(Qn) + np.triu(Qn, 1).T
    elif pattern == "upper":
        Qn = np.triu(Qn)
    elif pattern == "lower":
        Qn = np.tril(Qn)
    elif pattern == "asymmetric":                                 # Q_ij != 0 with Q_ji == 0, in both triangles
        drop = rng.rand(n, n) < 0.5
        Qn[drop & ~drop.T] = 0
    else:
        Qn = np.diag(np.diag(Qn)).astype(np.float32)
    if rng.rand() < 0.3:
        np.fill_diagonal(Qn, 0)
    num_ls = int(rng.randint(0, 4))
    binary = bool(rng.rand() < 0.5)
    waves = int(rng.choice([0, 4, 8, 16]))                        # 0: the launcher's choice
    x0 = rng.randint(0, 2, size=(n, C)).astype(np.float32)
    tag = (f"it={it} n={n} C={C} density={density} pattern={pattern} quarters={quarters} num_ls={num_ls} binary={binary} "
           f"waves={waves}")
    if "-v" in sys.argv:
        print(tag, flush=True)
    want_x, want_v = reference_sweep(Qn, x0, num_ls, binary)
    Q = dev(Qn)
    xd, vd = q.qubo_local_search_value(Q, dev(x0), num_ls, binary)
    assert np.array_equal(xd.cpu().numpy(), want_x), "dense x " + tag
    assert np.array_equal(vd.cpu().numpy(), want_v), "dense value " + tag
    csr = q.qubo_to_csr(Q)
    if waves:
        _abi.tuning_set("RLS_QUBO_LEVELS", waves)
    try:
        xs_, vs_ = q.qubo_sparse_local_search_value(csr, dev(x0), num_ls, binary)
    finally:
        _abi.tuning_unset("RLS_QUBO_LEVELS")
    assert np.array_equal(xs_.cpu().numpy(), want_x) and np.array_equal(vs_.cpu().numpy(), want_v), "sparse (levels) " + tag
    xs_, vs_ = q.qubo_sparse_local_search_value(csr[:3], dev(x0), num_ls, binary)
    assert np.array_equal(xs_.cpu().numpy(), want_x) and np.array_equal(vs_.cpu().numpy(), want_v), "sparse (sequential) " + tag
    it += 1
print(f"fuzz_qubo: {it} random configurations, no mismatch")
