#!/usr/bin/env python3
"""Record tests/golden/sub_set_sampling.npz from the reference's own sub_set_sampling (rlsolver/methods/L2A/transformer.py) on
the CPU.  The reference is IMPORTED (tools/gen_golden.py puts it on sys.path); nothing of it is written but data.

    PYTHONDONTWRITEBYTECODE=1 python tools/gen_golden.py --only sub_set_sampling        (or: python tools/gen_golden_l2a.py)

The reference draws one `rand_like` vector [R S] per selected rank; this tool wraps torch.rand_like and torch.topk for the call,
and rewrites the draws as `uniforms [R S, N]` indexed (row, node) with the reference's own top_ids.  Every entry the rule must NOT
read holds the value that would flip the start bit if it were read: 0.0 where the bit is 0 (0 < det), 1.0 where it is 1.
Every recorded row has distinct determinism values at its selection boundary (asserted), so the result does not depend on how
torch.topk breaks ties."""
import os
import sys

import numpy as np
import torch as th

TOOLS = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(TOOLS)
for p in (TOOLS, ROOT, os.path.join(ROOT, "tests")):
    if p not in sys.path:
        sys.path.insert(0, p)

KEY = "sub_set_sampling"


def _reference_fn():
    import gen_golden                                     # its import puts the reference on sys.path
    l2a = os.path.join(gen_golden.REF, "rlsolver", "methods", "L2A")
    if l2a not in sys.path:
        sys.path.insert(0, l2a)
    from rlsolver.methods.L2A.transformer import sub_set_sampling
    return sub_set_sampling


def record(fn, probs, start, R, top_k):
    """Run the reference once -> (uniforms [R S, N], xs, probs_out) as numpy."""
    import subset_oracle as orc
    S, N = probs.shape
    assert orc.boundary_is_distinct(probs.numpy(), top_k), "equal determinism at the selection boundary: pick another seed"
    draws, topk_out = [], []
    real_rand_like, real_topk = th.rand_like, th.topk

    def rand_like(t, *a, **kw):
        u = real_rand_like(t, *a, **kw)
        draws.append(u.clone())
        return u

    def topk(*a, **kw):
        out = real_topk(*a, **kw)
        topk_out.append(out)
        return out

    p0, s0 = probs.clone(), start.clone()
    th.rand_like, th.topk = rand_like, topk
    try:
        xs, probs_out = fn(probs=probs, start_xs=start, num_repeats=R, top_k=top_k)
    finally:
        th.rand_like, th.topk = real_rand_like, real_topk
    assert th.equal(probs.view(th.int32), p0.view(th.int32)) and th.equal(start, s0), "the reference modified an input"   # (bits: NaN)
    top_ids = topk_out[1][1]                              # the second topk: the selected nodes, [S, min(top_k, N)]
    k = top_ids.shape[1]
    assert len(draws) == k == min(top_k, N)
    uniforms = np.where(np.tile(start.numpy(), (R, 1)), np.float32(1.0), np.float32(0.0)).astype(np.float32)
    rows = np.arange(R * S)
    for i in range(k):
        uniforms[rows, top_ids[:, i].repeat(R).numpy()] = draws[i].numpy()
    return uniforms, xs.numpy().astype(np.uint8), probs_out.numpy().astype(np.float32)


def cases():
    """(tag, probs, start, R, top_k), every draw from an explicit generator."""
    g = th.Generator().manual_seed(20261020)
    rnd = lambda S, N: th.rand((S, N), generator=g, dtype=th.float32)                       # noqa: E731
    bits = lambda S, N: th.randint(0, 2, (S, N), generator=g, dtype=th.uint8).to(th.bool)   # noqa: E731
    out = []
    for S, N, R, k in ((8, 37, 4, 9), (3, 64, 1, 16), (2, 65, 5, 64), (1, 1, 3, 1), (4, 130, 3, 0), (4, 130, 3, 130), (4, 130, 2, 135),
                       (2, 257, 7, 64)):
        out.append((f"s{S}_n{N}_r{R}_k{k}", rnd(S, N), bits(S, N), R, k))
    out.append(("outside_unit_interval", 1.4 * rnd(4, 48) - 0.2, bits(4, 48), 3, 12))
    p = rnd(3, 50)
    p[0, 7] = float("nan")
    p[2, 0] = float("nan")
    out.append(("nan", p, bits(3, 50), 2, 10))
    p = rnd(3, 40)
    p = th.where((p - 0.5).abs() < 0.02, p + 0.25, p)                                       # nothing else this close to 0.5
    for s in range(3):
        for j, (a, b) in enumerate(((1, 30), (17, 4), (22, 39))):
            d = (j + 1 + s) / 4096.0                                                        # 0.5 +- d is exact in float32
            p[s, a], p[s, b] = 0.5 + d, 0.5 - d
    out.append(("equal_pairs_inside", p, bits(3, 40), 4, 16))
    return out


def generate(save):
    fn = _reference_fn()
    arrays, tags = {}, []
    for tag, probs, start, R, k in cases():
        uniforms, xs, probs_out = record(fn, probs, start, R, k)
        tags.append(tag)
        arrays[f"{tag}/probs"], arrays[f"{tag}/start"] = probs.numpy().copy(), start.numpy().astype(np.uint8)
        arrays[f"{tag}/R"], arrays[f"{tag}/top_k"] = np.int64(R), np.int64(k)
        arrays[f"{tag}/uniforms"], arrays[f"{tag}/xs"], arrays[f"{tag}/probs_out"] = uniforms, xs, probs_out
    arrays["cases"] = np.array(tags)
    arrays["source"] = np.array("recorded from the reference's sub_set_sampling on CPU; uniforms[row, node] = the reference's rand_like draw "
                                "at the selected (row, node), elsewhere 0.0 | 1.0 = the value that would flip the start bit if read")
    save(KEY, **arrays)


if __name__ == "__main__":
    import gen_golden
    gen_golden._CURRENT["key"] = KEY
    generate(gen_golden.save)
