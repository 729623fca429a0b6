"""The Cheeger-cut samplers of the MCPG package restated in numpy float32 (rlsolver/methods/MCPG/sampling.py:181-250): what
tests/golden/cheeger.npz was recorded from, one array operation per line of the reference, all chains at once.

Everything is float32 and IEEE: 1 / 0 = inf, 0 / 0 = NaN, 0 * inf = NaN, and the comparison stays ``h < nh``.  One step is not
numpy: the mean of ``h - mean(h)`` is torch's CPU reduction, as in the reference -- h is made of fractions, the sum depends on
the order of the additions, and that order is the library's."""
import os

import numpy as np

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "cheeger.npz")
F = np.float32


def neighbor_rows(n, eu, ev):
    """dataloader.py:106-123: per node the other endpoint of every incident edge, in edge order; a self-loop lists the node twice."""
    rows = [[] for _ in range(n)]
    for a, b in zip(np.asarray(eu).tolist(), np.asarray(ev).tolist()):
        rows[a].append(b)
        rows[b].append(a)
    return [np.asarray(r, dtype=np.int64) for r in rows]


def weighted_degrees(n, eu, ev, w):
    wd = np.zeros(n, dtype=np.int64)
    np.add.at(wd, np.asarray(eu, dtype=np.int64), np.asarray(w, dtype=np.int64))
    np.add.at(wd, np.asarray(ev, dtype=np.int64), np.asarray(w, dtype=np.int64))
    return wd


def _value(cut, size, n, normalized):
    with np.errstate(all="ignore"):
        if normalized:
            return (cut * (F(1) / size + F(1) / (F(n) - size))).astype(F)
        return (cut / np.minimum(size, F(n) - size)).astype(F)


def local_search(n, eu, ev, w, order, x, num_ls, normalized):
    """x: 0|1 [n, C] (any dtype) after the walk.  Returns (x after the sweep uint8 [n, C], h, cut, size f32 [C])."""
    eu, ev = np.asarray(eu, dtype=np.int64), np.asarray(ev, dtype=np.int64)
    rows, wdeg = neighbor_rows(n, eu, ev), weighted_degrees(n, eu, ev, w).astype(F)
    W = F(np.asarray(w, dtype=np.int64).sum())
    s = np.array(x, dtype=F)
    C = s.shape[1]
    edge_sum = ((2 * s[eu] - 1) * (2 * s[ev] - 1)).sum(axis=0, dtype=F) if eu.size else np.zeros(C, F)     # UNWEIGHTED (:190)
    cut = ((W - edge_sum) / F(2)).astype(F)
    size = s.sum(axis=0, dtype=F)
    h = _value(cut, size, n, normalized)
    for _ in range(num_ls):
        for node in np.asarray(order).tolist():
            c = s[rows[node]].sum(axis=0, dtype=F) if rows[node].size else np.zeros(C, F)
            sg = 2 * s[node] - 1
            ncut = (cut - sg * (wdeg[node] - 2 * c)).astype(F)
            nsize = (size - sg).astype(F)
            nh = _value(ncut, nsize, n, normalized)
            with np.errstate(invalid="ignore"):
                keep = (h < nh) | (np.minimum(nsize, F(n) - nsize) < F(0.0000001))
            s[node] = np.where(keep, s[node], 1 - s[node])
            cut, size, h = np.where(keep, cut, ncut), np.where(keep, size, nsize), np.where(keep, h, nh)
    return s.astype(np.uint8), h.astype(F), cut.astype(F), size.astype(F)


def mean_f32(h):
    """torch.mean of a float32 CPU tensor (sampling.py:214)."""
    import torch
    return torch.mean(torch.from_numpy(np.ascontiguousarray(h, dtype=F))).numpy()


def first_min(h, M):
    """Index of the first strict minimum over the repeats of each kept chain (np.argmin / torch.argmin where no NaN is present)."""
    return np.arange(M) + np.argmin(h.reshape(-1, M), axis=0) * M


def sampler(n, eu, ev, w, order, raw, num_ls, M, normalized):
    """The sampler's returns after the walk: (-h[best] f32 [M], best chains uint8 [n, M], h - mean(h) f32 [C]) + (h, chains)."""
    xs, h, _, _ = local_search(n, eu, ev, w, order, raw, num_ls, normalized)
    idx = first_min(h, M)
    return -h[idx], xs[:, idx], (h - mean_f32(h)).astype(F), h, xs


def decode_stream(stream, n):
    """Visit stream (rls_cheeger_local_search) -> (order, degrees, weighted degrees, neighbour rows in stream order)."""
    order, deg, wdeg, rows, p = [], [], [], [], 0
    for _ in range(n):
        order.append(int(stream[p])), deg.append(int(stream[p + 1])), wdeg.append(int(stream[p + 2]))
        rows.append(np.asarray(stream[p + 3:p + 3 + deg[-1]], dtype=np.int64))
        p += 3 + deg[-1]
    assert p == len(stream)
    return np.asarray(order), np.asarray(deg), np.asarray(wdeg), rows


def bits(a, n):
    """np.packbits(axis=0) of an [n, C] 0|1 array -> uint8 [n, C]."""
    return np.unpackbits(a, axis=0, count=n)


def same_bits(a, b):
    """Bitwise equality of two float32 arrays, NaN positions included."""
    a, b = np.ascontiguousarray(a, dtype=F), np.ascontiguousarray(b, dtype=F)
    return a.shape == b.shape and bool((np.isnan(a) == np.isnan(b)).all()) and bool((a.view(np.uint32)[~np.isnan(a)] == b.view(np.uint32)[~np.isnan(b)]).all())


def fixture_entries():
    """Every (sampler, num_ls) entry of the fixture with its graph and walk: dicts of plain arrays."""
    z = np.load(GOLDEN)
    for name in z["names"].tolist():
        gname, cfg, kind, fn, ls = name.split("/")
        n = int(z[f"{gname}/num_nodes"])
        M, R = (int(v) for v in cfg.split("x"))
        key = f"{gname}/{cfg}/{kind}"
        yield dict(name=name, n=n, eu=z[f"{gname}/edges"][0], ev=z[f"{gname}/edges"][1], w=z[f"{gname}/weights"],
                   order=z[f"{gname}/sorted_degree_nodes"].astype(np.int64), M=M, R=R, kind=kind, normalized=fn == "ncheegercut",
                   num_ls=int(ls[2:]), probs=z[f"{key}/probs"], start=bits(z[f"{key}/start"], n), change_times=int(z[f"{key}/change_times"]),
                   index=z[f"{key}/index"].astype(np.int64), u=z[f"{key}/u"], raw=bits(z[f"{key}/raw"], n),
                   neg_h=z[f"{name}/neg_h"], best=bits(z[f"{name}/best"], n), value=z[f"{name}/value"])
