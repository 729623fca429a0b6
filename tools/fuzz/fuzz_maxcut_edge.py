"""Fuzz of the edge-flip MaxCut sampler kernel (rls_maxcut_edge_local_search) against the numpy oracle of tests/edge_oracle.py:
random multigraphs (loops and parallel edges as they fall, stars, paths, the one-edge graph, isolated nodes), signed integer
weights, the loader's edge order or a random one, starts drawn at p in {0.05, 0.5, 0.95}, uniforms with a fifth of them 0 (ties)
or the kernel's own draws against their numpy restatement, ragged and full tiles, a broadcast start (C_in < C), packed (in place
or not) or float32 output, with and without the gauge, num_ls in 0..3.  Chains and expected must match bit for bit.
`python tools/fuzz/fuzz_maxcut_edge.py [seconds] [seed] [-v]`."""
import os
import sys
import time

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
for p in (ROOT, os.path.join(ROOT, "tests")):
    if p not in sys.path:
        sys.path.insert(0, p)
import edge_oracle as orc  # noqa: E402


def random_case(rng):
    kind = rng.choice(["multi", "multi", "star", "path", "tiny"])
    if kind == "tiny":
        n = int(rng.randint(1, 4))
        m = int(rng.randint(1, 4))
        eu, ev = rng.randint(0, n, m), rng.randint(0, n, m)
    elif kind == "star":
        n = int(rng.choice([5, 40, 90]))
        hub = int(rng.randint(0, n))
        ev = np.delete(np.arange(n), hub)
        eu = np.full(n - 1, hub)
    elif kind == "path":
        n = int(rng.randint(2, 60))
        eu, ev = np.arange(n - 1), np.arange(1, n)
    else:
        n = int(rng.randint(3, 60))
        m = int(rng.randint(1, 3 * n))
        eu, ev = rng.randint(0, n, m), rng.randint(0, n, m)                # loops, duplicates and bare nodes as they fall
    m = eu.shape[0]
    w = rng.randint(1, int(rng.choice([2, 4, 1000])), m) * rng.choice([-1, 1], m)
    return kind, n, eu.astype(np.int64), ev.astype(np.int64), w.astype(np.int64)


def run(seconds=60.0, seed=0, verbose=False, device="cuda:0"):
    from rlsolver_amd.methods import MCPG_maxcut_edge as me
    from rlsolver_amd.ops_mcpg_tsp import PackedChains
    dev = torch.device(device)
    rng = np.random.RandomState(seed)
    t_end = time.time() + seconds
    it = 0
    while time.time() < t_end:
        kind, n, eu, ev, w = random_case(rng)
        E = eu.shape[0]
        order_e = rng.permutation(E) if rng.rand() < 0.5 else None
        data = me.make_data(n, eu, ev, w, dev, sorted_degree_nodes=rng.permutation(n), sorted_degree_edges=order_e)
        order_e = data.sorted_degree_edges.numpy()
        add, _, _, _ = orc.loader(n, eu, ev, w)
        C = int(rng.choice([1, 63, 64, 65, 128, 130]))
        c_in = 64 if (C == 128 and rng.rand() < 0.5) else C
        num_ls, gauge, own = int(rng.randint(0, 4)), bool(rng.rand() < 0.7), bool(rng.rand() < 0.3)
        form = rng.choice(["packed", "inplace", "f32"]) if c_in == C else rng.choice(["packed", "f32"])
        draw_seed = int(rng.randint(0, 2 ** 31)) * 2654435761 + 12345
        tag = f"it={it} {kind} n={n} E={E} C={C} C_in={c_in} num_ls={num_ls} gauge={gauge} own_draws={own} out={form}"
        if verbose:
            print(tag, flush=True)
        start = (rng.rand(n, c_in) < rng.choice([0.05, 0.5, 0.95], c_in)[None, :]).astype(np.float32)
        if own:
            uni = orc.production_uniforms(draw_seed, np.arange(C), num_ls, E)
        else:
            uni = rng.rand(num_ls, E, 3, C).astype(np.float32)
            uni[rng.rand(*uni.shape) < 0.2] = 0.0
        want_v, want_e = orc.sweep(n, eu, ev, w, order_e, add, np.tile(start, (1, C // c_in)), data.hub() if gauge else -1, num_ls, uni)
        xin = PackedChains.pack(torch.from_numpy(start).to(dev))
        out = {"packed": PackedChains.empty(n, C, dev), "inplace": xin, "f32": None}[form]
        xs, expected = data.local_search(xin, num_ls, None if own else torch.from_numpy(uni).to(dev), draw_seed, out=out, num_chains=C,
                                         gauge=gauge)
        if form == "f32":
            assert orc.same_bits(xs.cpu().numpy(), want_v), "chains " + tag
        else:
            assert np.array_equal(xs.unpack().cpu().numpy(), (want_v > 0.25).astype(np.float32)), "chains " + tag
        assert orc.same_bits(expected.cpu().numpy(), want_e), "expected " + tag
        it += 1
    return it


if __name__ == "__main__":
    args = [a for a in sys.argv[1:] if a != "-v"]
    n_it = run(float(args[0]) if args else 60.0, int(args[1]) if len(args) > 1 else 0, "-v" in sys.argv)
    print(f"fuzz_maxcut_edge: {n_it} random configurations, no mismatch")
