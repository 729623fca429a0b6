"""Fuzz of sub_set_sampling (rls_sub_set_sampling) against the numpy restatement of tests/subset_oracle.py: random S / N / R /
top_k on both sides of every edge (top_k = 0, >= N; N = 1; rows that are no multiple of 16 bytes; more repeats than one
workgroup writes), probabilities uniform, saturated like a softmax, quantised (ties at the selection boundary: lower node index)
or holding NaN / values outside [0, 1], uniforms with a fifth of them 0 or 1, an output that starts at any byte, and the kernel's
own draws against their torch restatement.  xs and probs must match bit for bit.
`python tools/fuzz/fuzz_subset.py [seconds] [seed] [-v]`."""
import os
import sys
import time

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
for p in (ROOT, os.path.join(ROOT, "tests")):
    if p not in sys.path:
        sys.path.insert(0, p)
import subset_oracle as orc  # noqa: E402


def random_probs(rng, S, N):
    kind = rng.choice(["uniform", "softmax", "quantised", "two_values", "half", "nan", "wide"])
    p = rng.rand(S, N).astype(np.float32)
    if kind == "softmax":                                   # near 0 | 1 with the callers' Gaussian noise
        p = ((p < 0.5).astype(np.float32) * 0.98 + 0.01 + rng.randn(S, N).astype(np.float32) * 0.02).astype(np.float32)
    elif kind == "quantised":
        p = (np.round(p * 16) / 16).astype(np.float32)
    elif kind == "two_values":
        p = rng.choice(np.array([0.3, 0.9], dtype=np.float32), size=(S, N))
    elif kind == "half":
        p[:] = 0.5
    elif kind == "nan":
        p[rng.rand(S, N) < 0.3] = np.nan
    elif kind == "wide":
        p = (1.4 * p - 0.2).astype(np.float32)
    return kind, p


def run(seconds=60.0, seed=0, verbose=False, device="cuda:0"):
    from rlsolver_amd import ops
    dev = torch.device(device)
    rng = np.random.RandomState(seed)
    t_end = time.time() + seconds
    it = 0
    while time.time() < t_end:
        N = int(rng.choice([1, 2, 15, 16, 17, 31, 33, 64, 100, 255, 257, int(rng.randint(1, 1500)), int(rng.randint(1500, 5000))]))
        S = int(rng.choice([1, 2, 3, 5, 64, int(rng.randint(1, 40))]))
        R = int(rng.choice([1, 2, 3, 7, 33, int(rng.randint(1, 50))]))
        if S * R * N > 4_000_000:
            S = max(1, 4_000_000 // (R * N))
        top_k = int(rng.choice([0, 1, N // 4, max(N - 1, 0), N, N + 5, int(rng.randint(0, N + 2))]))
        kind, probs = random_probs(rng, S, N)
        start = rng.rand(S, N) < rng.choice([0.05, 0.5, 0.95])
        own = bool(rng.rand() < 0.25)
        shift = int(rng.randint(0, 16)) if rng.rand() < 0.5 else 0
        draw_seed, off = int(rng.randint(0, 2 ** 31)) * 2654435761 + 12345, int(rng.choice([0, 7, 2 ** 33 + 5]))
        tag = f"it={it} S={S} N={N} R={R} top_k={top_k} probs={kind} own_draws={own} out_byte_offset={shift}"
        if verbose:
            print(tag, flush=True)
        d_probs, d_start = torch.from_numpy(probs).to(dev), torch.from_numpy(start).to(dev)
        p0, s0 = d_probs.clone(), d_start.clone()
        out = torch.empty(R * S * N + 16, dtype=torch.bool, device=dev)[shift:shift + R * S * N].view(R * S, N)
        if own:
            nodes = torch.topk((torch.from_numpy(orc.determinism(probs)[1].astype(np.int64)).to(dev) << 32)
                               | torch.arange(N, device=dev)[None, :], min(top_k, N), dim=1, largest=False)[0] & 0xFFFFFFFF
            uni = torch.full((R, S, N), 2.0, dtype=torch.float32, device=dev)
            if nodes.shape[1]:
                uni.scatter_(2, nodes[None].expand(R, S, -1), ops.sub_set_sampling_draws(draw_seed, off, R, S, nodes))
            uni = uni.view(R * S, N).cpu().numpy()
            xs, pr = ops.sub_set_sampling(d_probs, d_start, R, top_k, seed=draw_seed, env_offset=off, out=out)
        else:
            uni = rng.rand(R * S, N).astype(np.float32)
            coin = rng.rand(R * S, N)
            uni[coin < 0.1], uni[coin > 0.9] = 0.0, 1.0
            xs, pr = ops.sub_set_sampling(d_probs, d_start, R, top_k, uniforms=torch.from_numpy(uni).to(dev), out=out)
        want_xs, want_pr = orc.sub_set_sampling(probs, start, R, top_k, uni)
        assert xs.data_ptr() == out.data_ptr() and np.array_equal(xs.cpu().numpy(), want_xs), "xs " + tag
        assert np.array_equal(pr.cpu().numpy().view(np.uint32), want_pr.view(np.uint32)), "probs " + tag
        assert torch.equal(d_probs.view(torch.int32), p0.view(torch.int32)) and torch.equal(d_start, s0), "inputs changed " + tag
        it += 1
    return it


if __name__ == "__main__":
    args = [a for a in sys.argv[1:] if a != "-v"]
    n_it = run(float(args[0]) if args else 60.0, int(args[1]) if len(args) > 1 else 0, "-v" in sys.argv)
    print(f"fuzz_subset: {n_it} random configurations, no mismatch")
