"""Fuzz of the Cheeger-cut sampler kernel (rls_cheeger_local_search) against the numpy oracle of tests/cheeger_oracle.py: random
graphs (G(n, m) with self-loops and duplicate edges allowed, stars, paths, edgeless, N = 1 and 2), unit, small signed or 0-heavy
integer weights, random visiting orders, starts drawn at p in {0.05, 0.5, 0.95} with an all-0, an all-1 and a one-hot chain
planted, ragged and full tiles, a broadcast start (C_in < C), packed (in place or not) or float32 output, both cuts, num_ls in
0..3.  Chains after the sweep, h, cut and size must match bit for bit, NaN positions included.
`python tools/fuzz/fuzz_cheeger.py [seconds] [seed] [-v]`."""
import os
import sys
import time

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
for p in (ROOT, os.path.join(ROOT, "tests")):
    if p not in sys.path:
        sys.path.insert(0, p)
import cheeger_oracle as orc  # noqa: E402


def random_case(rng):
    kind = rng.choice(["gnm", "gnm", "star", "path", "edgeless", "tiny"])
    if kind == "tiny":
        n = int(rng.randint(1, 3))
        m = 0 if n == 1 and rng.rand() < 0.5 else int(rng.randint(0, 3))
        eu, ev = rng.randint(0, n, m), rng.randint(0, n, m)
    elif kind == "star":
        n = int(rng.choice([5, 70, 301]))
        hub = int(rng.randint(0, n))
        ev = np.delete(np.arange(n), hub)
        eu = np.full(n - 1, hub)
    elif kind == "path":
        n = int(rng.randint(2, 80))
        eu, ev = np.arange(n - 1), np.arange(1, n)
    elif kind == "edgeless":
        n, eu, ev = int(rng.randint(1, 40)), np.zeros(0, np.int64), np.zeros(0, np.int64)
    else:
        n = int(rng.choice([rng.randint(3, 40), rng.randint(40, 400)]))
        m = int(rng.randint(0, 6 * n))
        eu, ev = rng.randint(0, n, m), rng.randint(0, n, m)                # loops and duplicates as they fall
    wk = rng.choice(["unit", "signed", "zeros"])
    m = eu.shape[0]
    w = np.ones(m, np.int64) if wk == "unit" else (rng.choice([-3, -1, 1, 2], m) if wk == "signed" else rng.choice([0, 0, 1, -1], m))
    return kind + "/" + wk, n, eu.astype(np.int64), ev.astype(np.int64), w.astype(np.int64)


def random_start(rng, n, c):
    x = (rng.rand(n, c) < rng.choice([0.05, 0.5, 0.95], c)[None, :]).astype(np.float32)
    for col, val in zip(rng.permutation(c)[:3], ("zero", "one", "hot")):
        x[:, col] = 1.0 if val == "one" else 0.0
        if val == "hot":
            x[int(rng.randint(0, n)), col] = 1.0
    return x


def run(seconds=60.0, seed=0, verbose=False, device="cuda:0"):
    from rlsolver_amd.methods import MCPG_cheeger as mc
    from rlsolver_amd.ops_mcpg_tsp import PackedChains
    dev = torch.device(device)
    rng = np.random.RandomState(seed)
    t_end = time.time() + seconds
    it = 0
    while time.time() < t_end:
        kind, n, eu, ev, w = random_case(rng)
        order = rng.permutation(n)
        data = mc.make_data(n, eu, ev, w, dev, sorted_degree_nodes=order)
        C = int(rng.choice([1, 63, 64, 65, 128, 130, 200]))
        c_in = 64 if (C == 128 and rng.rand() < 0.5) else C
        num_ls, normalized = int(rng.randint(0, 4)), bool(rng.rand() < 0.5)
        form = rng.choice(["packed", "inplace", "f32"]) if c_in == C else rng.choice(["packed", "f32"])
        tag = f"it={it} {kind} n={n} E={eu.shape[0]} C={C} C_in={c_in} num_ls={num_ls} normalized={normalized} out={form}"
        if verbose:
            print(tag, flush=True)
        start = random_start(rng, n, c_in)
        want_x, want_h, want_cut, want_size = orc.local_search(n, eu, ev, w, order, np.tile(start, (1, C // c_in)), num_ls, normalized)
        xin = PackedChains.pack(torch.from_numpy(start).to(dev))
        out = {"packed": PackedChains.empty(n, C, dev), "inplace": xin, "f32": None}[form]
        xs, h, cut, size = data.local_search(xin, num_ls, normalized, out=out, num_chains=C)
        got = (xs if form == "f32" else xs.unpack()).cpu().numpy()
        assert np.array_equal(got, want_x), "chains " + tag
        assert orc.same_bits(h.cpu().numpy(), want_h), "h " + tag
        assert orc.same_bits(cut.cpu().numpy(), want_cut) and orc.same_bits(size.cpu().numpy(), want_size), "cut / size " + tag
        it += 1
    return it


if __name__ == "__main__":
    args = [a for a in sys.argv[1:] if a != "-v"]
    n_it = run(float(args[0]) if args else 60.0, int(args[1]) if len(args) > 1 else 0, "-v" in sys.argv)
    print(f"fuzz_cheeger: {n_it} random configurations, no mismatch")
