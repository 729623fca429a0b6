"""The edge-flip MaxCut sampler of the MCPG package restated in numpy float32 (rlsolver/methods/MCPG/sampling.py:130-178 and its
loader, dataloader.py:87-101, :106-153): what tests/golden/maxcut_edge.npz was recorded from, one array operation per line of the
reference, all chains at once.  Written with plain loops over edges and rows, on purpose: nothing here shares code with the
package's own builders.

Every float32 operation is one numpy float32 operation (one rounding each).  The neighbour sums are half-integers that float32
holds exactly, so their order of addition does not matter; ``expected`` is an integer, and the fixture keeps C * sum|w| < 2^24, so
its sum over the chains is exact too and the mean is one correctly rounded division.

Also here: the kernel's integer path (2 t counted from the visit stream, ``fresh`` flags, bits and a written mask) emulated on the
host, and the production draws (murmur3 finaliser keyed by seed, global chain id, pass, position, which) restated."""
import functools
import os

import numpy as np

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "maxcut_edge.npz")
F = np.float32


def parse_text(text):
    """A graph file of the package (first line "N E", then 1-based "u v w" lines) -> (n, eu, ev, w) with 0-based endpoints."""
    lines = [ln.split() for ln in text.strip().splitlines()]
    n, E = int(lines[0][0]), int(lines[0][1])
    rows = lines[1:1 + E]
    assert len(rows) == E
    return (n, np.array([int(r[0]) - 1 for r in rows], np.int64), np.array([int(r[1]) - 1 for r in rows], np.int64),
            np.array([int(float(r[2])) for r in rows], np.int64))


def neighbor_rows(n, eu, ev, w):
    """dataloader.py:106-123: per node the (other endpoint, weight) of every incident edge, in edge order; a loop lists the node twice."""
    rows = [[] for _ in range(n)]
    for a, b, x in zip(np.asarray(eu).tolist(), np.asarray(ev).tolist(), np.asarray(w).tolist()):
        rows[a].append((b, x))
        rows[b].append((a, x))
    return rows


def row_less_first(row, other):
    """dataloader.py:136-146: the row without its FIRST entry whose neighbour is ``other``; returns (row, index removed)."""
    k = next(i for i, (v, _) in enumerate(row) if v == other)
    return row[:k] + row[k + 1:], k


def loader(n, eu, ev, w):
    """(add f32 [3, E], key int64 [E], wdeg, adeg) of dataloader.py:76-101."""
    eu, ev, w = (np.asarray(a, dtype=np.int64) for a in (eu, ev, w))
    E = eu.shape[0]
    wdeg, adeg = np.zeros(n, np.int64), np.zeros(n, np.int64)
    for a, b, x in zip(eu.tolist(), ev.tolist(), w.tolist()):
        wdeg[a] += x
        wdeg[b] += x
        adeg[a] += abs(x)
        adeg[b] += abs(x)
    add = np.zeros((3, E), F)
    key = np.zeros(E, np.int64)
    for e in range(E):
        r, c, x = int(eu[e]), int(ev[e]), F(w[e])
        add[0, e] = (F(-wdeg[r] / 2) + x) - F(0.05)
        add[1, e] = (F(-wdeg[c] / 2) + x) - F(0.05)
        add[2, e] = x + F(0.05)
        key[e] = abs(int(w[e])) * (adeg[r] + adeg[c])
    return add, key, wdeg, adeg


def stable_order(key):
    """Descending and stable: ties keep the edge order."""
    return np.argsort(-np.asarray(key, dtype=np.int64), kind="stable")


def gauge(raw, hub):
    """sampling.py:142-144 on 0|1 arrays: every chain XORed with its own value at the hub (hub < 0: none)."""
    x = np.asarray(raw).astype(np.uint8)
    return x ^ x[hub] if hub >= 0 else x.copy()


def sweep(n, eu, ev, w, order, add, raw, hub, num_ls, uniforms):
    """raw: 0|1 [n, C] after the walk; uniforms f32 [>= num_ls, E, 3, C].  Exactly ``num_ls`` passes (the reference's loop runs one
    with num_ls = 0; callers pass max(1, num_ls) for it).  Returns (v f32 [n, C]: 0 | 1, or -0.5 | 1.5 where never written,
    expected f32 [C] over the bits)."""
    eu, ev, w = (np.asarray(a, dtype=np.int64) for a in (eu, ev, w))
    rows = neighbor_rows(n, eu, ev, w)
    x = gauge(raw, hub)
    v = ((x.astype(F) - F(0.5)) * F(2) + F(0.5)).astype(F)                        # :145
    C = v.shape[1]
    for p in range(num_ls):
        for i, e in enumerate(np.asarray(order).tolist()):
            r, c = int(eu[e]), int(ev[e])
            rr, _ = row_less_first(rows[r], c)
            rc, _ = row_less_first(rows[c], r)
            t_r = sum((F(x) * v[k] for k, x in rr), np.zeros(C, F)).astype(F)
            t_c = sum((F(x) * v[k] for k, x in rc), np.zeros(C, F)).astype(F)
            u0, u1, u2 = (np.asarray(uniforms[p, i, j], dtype=F) for j in range(3))
            a = (t_r + u0 * F(0.1)) + add[0, e]
            b = (t_c + u1 * F(0.1)) + add[1, e]
            z = ((a + b) + u2 * F(0.1)) - add[2, e]
            assert a.dtype == F and b.dtype == F and z.dtype == F
            k = np.argmax(np.stack([z, a, b, np.zeros(C, F)]), axis=0)         # the first maximum
            v[r] = (k >> 1).astype(F)
            v[c] = (k & 1).astype(F)
    return v, score(eu, ev, w, v > F(0.25))


def score(eu, ev, w, x):
    """expected f32 [C] = sum_e w_e (2 x_u - 1)(2 x_v - 1) on bits."""
    s = 2 * np.asarray(x).astype(np.int64) - 1
    return (np.asarray(w, dtype=np.int64)[:, None] * s[np.asarray(eu)] * s[np.asarray(ev)]).sum(axis=0).astype(F)


def first_min(expected, M):
    return np.arange(M) + np.argmin(expected.reshape(-1, M), axis=0) * M


def returns(v, expected, M, edge_weight_sum):
    """sampling.py:173-178: (res f32 [M], best f32 [n, M], value f32 [C])."""
    idx = first_min(expected, M)
    res = ((F(edge_weight_sum) - expected[idx]) / F(2)).astype(F)
    mean = F(expected.sum(dtype=np.float64)) / F(expected.shape[0])
    return res, v[:, idx], (expected - mean).astype(F)


# ---------------------------------------------------------------------------------------------- the kernel's integer path
def decode_stream(stream, E):
    """Visit stream (rls_maxcut_edge_local_search) -> list of (r, c, add f32 [3], row_r, row_c); a row = (nbr, fresh, weight) arrays."""
    s = np.asarray(stream, dtype=np.int32)
    out, p = [], 0
    for _ in range(E):
        r, c, lr, lc = (int(s[p + j]) for j in range(4))
        add = s[p + 4:p + 7].copy().view(F)
        body = s[p + 7:p + 7 + 2 * (lr + lc)].view(np.uint32).astype(np.int64)
        nb, wt = body[0::2], body[1::2].astype(np.uint32).view(np.int32).astype(np.int64) if body.size else body[1::2]
        rows = []
        for lo, hi in ((0, lr), (lr, lr + lc)):
            rows.append((nb[lo:hi] & 0x7fffffff, nb[lo:hi] >> 31, wt[lo:hi]))
        out.append((r, c, add, rows[0], rows[1]))
        p += 7 + 2 * (lr + lc)
    assert p == s.shape[0]
    return out


def emulate_kernel(n, stream, E, raw, hub, num_ls, uniforms):
    """The kernel's arithmetic per chain: bits and a written mask, 2 t = sum w (fresh ? 4 x - 1 : 2 x) in integers (fresh read in
    pass 0 only), one conversion, then the float32 expression.  Returns (x uint8 [n, C], written bool [n])."""
    recs = decode_stream(stream, E)
    x = gauge(raw, hub).astype(np.int64)
    written = np.zeros(n, bool)
    C = x.shape[1]
    for p in range(num_ls):
        for i, (r, c, add, row_r, row_c) in enumerate(recs):
            ts = []
            for nb, fr, wt in (row_r, row_c):
                f = fr if p == 0 else np.zeros_like(fr)
                acc = (wt[:, None] * ((x[nb] << (1 + f)[:, None]) - f[:, None])).sum(axis=0) if nb.size else np.zeros(C, np.int64)
                assert np.abs(acc).max(initial=0) < 2 ** 24
                ts.append(acc.astype(np.int32).astype(F) * F(0.5))
            u0, u1, u2 = (np.asarray(uniforms[p, i, j], dtype=F) for j in range(3))
            a = (ts[0] + u0 * F(0.1)) + add[0]
            b = (ts[1] + u1 * F(0.1)) + add[1]
            z = ((a + b) + u2 * F(0.1)) - add[2]
            k = np.zeros(C, np.int64)
            best = z.copy()
            for j, cand in ((1, a), (2, b), (3, np.zeros(C, F))):
                take = cand > best
                best, k = np.where(take, cand, best), np.where(take, j, k)
            x[r] = k >> 1
            x[c] = k & 1
            written[r] = written[c] = True
    return x.astype(np.uint8), written


def as_float_output(x, written):
    """The kernel's float32 surface: the bit where written, 2 x - 0.5 where not."""
    xf = x.astype(F)
    return np.where(written[:, None], xf, F(2) * xf - F(0.5)).astype(F)


# ---------------------------------------------------------------------------------------------- the production draws
def fmix32(h):
    h = np.asarray(h, dtype=np.uint64) & 0xFFFFFFFF
    h ^= h >> 16
    h = (h * 0x85EBCA6B) & 0xFFFFFFFF
    h ^= h >> 13
    h = (h * 0xC2B2AE35) & 0xFFFFFFFF
    h ^= h >> 16
    return h


def production_uniforms(seed, gids, num_ls, E):
    """f32 [num_ls, E, 3, C]: what the kernel draws with uniforms = NULL for the chains of global ids ``gids``."""
    M32 = 0xFFFFFFFF
    seed = int(seed) & 0xFFFFFFFFFFFFFFFF
    g = np.asarray(gids, dtype=np.uint64)
    inner = fmix32(g & M32) ^ (((g >> 32) * 0x9E3779B1) & M32)
    chain_key = fmix32((seed & M32) ^ fmix32((seed >> 32) ^ inner))
    out = np.zeros((num_ls, E, 3, g.shape[0]), F)
    for p in range(num_ls):
        for i in range(E):
            k = chain_key ^ ((i * 0x9E3779B1) & M32) ^ ((p * 0x7FEB352D + 0x165667B1) & M32)
            for j in range(3):
                r = fmix32((k + (j + 1) * 0x27D4EB2F) & M32)
                out[p, i, j] = (r >> 8).astype(F) * F(1.0 / 16777216.0)
    return out


# ---------------------------------------------------------------------------------------------- the fixture
def bits(a, n):
    return np.unpackbits(a, axis=0, count=n)


@functools.lru_cache(maxsize=None)
def fixture():
    z = np.load(GOLDEN)
    return {k: z[k] for k in z.files}


def fixture_graph(gname):
    z = fixture()
    return dict(name=gname, n=int(z[f"{gname}/num_nodes"]), eu=z[f"{gname}/edges"][0].astype(np.int64), ev=z[f"{gname}/edges"][1].astype(np.int64),
                w=z[f"{gname}/weights"].astype(np.int64), add=z[f"{gname}/add"], edge_weight_sum=float(z[f"{gname}/edge_weight_sum"]),
                order_nodes=z[f"{gname}/sorted_degree_nodes"].astype(np.int64), order_edges=z[f"{gname}/sorted_degree_edges"].astype(np.int64),
                text=str(z[f"{gname}/text"]) if f"{gname}/text" in z else None)


def fixture_cases():
    """Every (graph, M x R, num_ls) entry with its graph and walk: dicts of plain arrays."""
    z = fixture()
    out = []
    for name in z["cases"].tolist():
        gname, cfg, ls = name.split("/")
        g = fixture_graph(gname)
        M, R = (int(v) for v in cfg.split("x"))
        key = f"{gname}/{cfg}"
        out.append(dict(g, case=name, M=M, R=R, num_ls=int(ls[2:]), probs=z[f"{key}/probs"], start=bits(z[f"{key}/start"], g["n"]),
                        change_times=int(z[f"{key}/change_times"]), index=z[f"{key}/index"].astype(np.int64), u=z[f"{key}/u"],
                        raw=bits(z[f"{key}/raw"], g["n"]), uniforms=z[f"{key}/uniforms"], res=z[f"{name}/res"], best=z[f"{name}/best"],
                        value=z[f"{name}/value"]))
    return out


def same_bits(a, b):
    a, b = np.ascontiguousarray(a, dtype=F), np.ascontiguousarray(b, dtype=F)
    return a.shape == b.shape and bool((a.view(np.uint32) == b.view(np.uint32)).all())


def random_graph(rng, n, E, wmax, loops=True, hub=False):
    """Random multigraph with signed weights in [-wmax, wmax] less 0, parallel edges, optionally loops and one hub."""
    eu, ev = rng.randint(0, n, E), rng.randint(0, n, E)
    if hub:
        eu[: E // 2] = 0
    if not loops:
        ev = np.where(ev == eu, (ev + 1) % n, ev)
    w = rng.randint(1, wmax + 1, E) * rng.choice([-1, 1], E)
    return eu.astype(np.int64), ev.astype(np.int64), w.astype(np.int64)
