"""Fuzz of the MIMO detection kernel (rls_mimo_local_search) against the numpy oracle of tests/mimo_oracle.py: random INTEGER
instances (the kernel is bit-exact on them) with n in 1..300 -- n < 32, one block, n no multiple of 32 --, Sigma with or without
a diagonal, dense or mostly zero, Diag odd, even (exact ties) or zero, starts drawn at p in {0.05, 0.5, 0.95} with an all-0 and an
all-1 chain planted, one tile, ragged and full tiles, a broadcast start (C_in < C), packed output (in place or not) or float32,
num_ls in 1..3.  Chains after the sweeps and expected must match bit for bit; bits of chains past C must be 0.
`python tools/fuzz/fuzz_mimo.py [seconds] [seed] [-v]`."""
import os
import sys
import time

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
for p in (ROOT, os.path.join(ROOT, "tests")):
    if p not in sys.path:
        sys.path.insert(0, p)
import mimo_oracle as orc  # noqa: E402


def random_case(rng):
    kind = rng.choice(["tiny", "block", "ragged", "ragged", "aligned"])
    n = {"tiny": int(rng.randint(1, 32)), "block": 32, "ragged": int(rng.randint(33, 301)), "aligned": 32 * int(rng.randint(2, 10))}[kind]
    style = rng.choice(["gram", "gram", "sparse", "asym"])
    if style == "gram":                                   # what the loaders build: H^T H with the diagonal zeroed, Diag = -2 Y^T H
        H = rng.randint(-3, 4, size=(n + int(rng.randint(0, 8)), n)).astype(np.float64)
        Y = H @ (rng.randint(0, 2, n) * 2.0 - 1) + rng.randint(-2, 3, H.shape[0])
        Sigma, Diag = H.T @ H, -2 * Y @ H
        np.fill_diagonal(Sigma, 0)
    else:
        Sigma = rng.randint(-40, 41, size=(n, n)).astype(np.float64)
        if style == "sparse":
            Sigma *= rng.rand(n, n) < 0.1
        Diag = rng.randint(-200, 201, size=n).astype(np.float64)
    dk = rng.choice(["asis", "even", "zero"])
    Diag = Diag if dk == "asis" else (2 * np.round(Diag / 2) if dk == "even" else np.zeros(n))
    if rng.rand() < 0.4:
        Sigma[np.arange(n), np.arange(n)] = rng.randint(-9, 10, size=n)
    assert 2 * np.abs(Sigma).sum(axis=1).max() + np.abs(Diag).max() < 2 ** 24 and np.abs(Sigma).sum() + np.abs(Diag).sum() < 2 ** 24
    return f"{kind}/{style}/{dk}", n, Sigma.astype(np.float32), Diag.astype(np.float32)


def random_start(rng, n, c):
    x = (rng.rand(n, c) < rng.choice([0.05, 0.5, 0.95], c)[None, :]).astype(np.float32)
    for col, val in zip(rng.permutation(c)[:2], (0.0, 1.0)):
        x[:, col] = val
    return x


def run(seconds=60.0, seed=0, verbose=False, device="cuda:0"):
    from rlsolver_amd import ops_mcpg_tsp as mops
    from rlsolver_amd.ops_mcpg_tsp import PackedChains
    dev = torch.device(device)
    rng = np.random.RandomState(seed)
    t_end = time.time() + seconds
    it = 0
    while time.time() < t_end:
        kind, n, Sigma, Diag = random_case(rng)
        C = int(rng.choice([1, 31, 33, 63, 64, 65, 100, 128, 130, 200, 256]))
        c_in = 64 if (C in (128, 256) and rng.rand() < 0.5) else C
        num_ls = int(rng.randint(1, 4))
        form = rng.choice(["packed", "inplace", "f32"]) if c_in == C else rng.choice(["packed", "f32"])
        tag = f"it={it} {kind} n={n} C={C} C_in={c_in} num_ls={num_ls} out={form}"
        if verbose:
            print(tag, flush=True)
        start = random_start(rng, n, c_in)
        want = orc.local_search(Sigma, Diag, np.tile(start, (1, C // c_in)), num_ls, np.float32)
        xin = PackedChains.pack(torch.from_numpy(start).to(dev))
        out = {"packed": PackedChains.empty(n, C, dev), "inplace": xin, "f32": None}[form]
        xs, expected = mops.mcpg_mimo_local_search(torch.from_numpy(Sigma).to(dev), torch.from_numpy(Diag).to(dev), xin, num_ls, out=out,
                                                   num_chains=C)
        got = (xs if form == "f32" else xs.unpack()).cpu().numpy()
        assert np.array_equal(got, (want["info"] + 1) / 2), "chains " + tag
        assert np.array_equal(expected.cpu().numpy().view(np.uint32), want["expected"].astype(np.float32).view(np.uint32)), "expected " + tag
        if form != "f32" and C % 64:
            assert int(((xs.words[-1] >> (C % 64)) != 0).sum()) == 0, "padding bits " + tag
        it += 1
    return it


if __name__ == "__main__":
    args = [a for a in sys.argv[1:] if a != "-v"]
    n_it = run(float(args[0]) if args else 60.0, int(args[1]) if len(args) > 1 else 0, "-v" in sys.argv)
    print(f"fuzz_mimo: {n_it} random configurations, no mismatch")
