"""The graph family, edge counts and states of tests/test_gpu_cut_counter.py (and their own CPU tests, tests/test_cut_graphs.py).

``bipartite_circulant(N, k, E)``: the first E of the edges (i, (i + o) mod N), o in {1, 3, .., 2k - 1}, listed i-major.  Every
offset is odd and N is even, so every edge joins an even node to an odd one: the parity state x[i] = i & 1 (and its complement) cuts
ALL stored edges -- the one input that drives a cut counter to its largest per-lane count.  2k - 1 < N / 2 keeps the edges
distinct as unordered pairs ((i, i + o) = (j + o', j) needs o + o' = 0 mod N, and o + o' <= 4k - 2 < N)."""
import numpy as np

# name -> (N, k): N * k edges available, largest degree 2k (out-degree k, in-degree k).  Every N is a multiple of 64.
SIZES = {"S12": (256, 17), "S16": (1024, 65), "S24": (8448, 125)}
MAX_DEGREE = {"S12": 34, "S16": 130, "S24": 250}
# a sparser graph with more than 2^16 edges: degrees <= 34, so the local-search weights still fit int8 there
SIZES_EXTRA = {"S16w": (4096, 17)}
LIMITS = (1 << 12, 1 << 16, 1 << 20)      # E' below which the counter takes 12 / 16 / 20 planes (24 below 2^24)
B = 97                                    # rows: a ragged last tile for 64-, 32-, 16- and 8-env tiles

# stored edges E' of the unidirectional graphs: the counter's blocks of 1024 edges (none, one ragged, whole blocks only, whole + ragged)
# and the first plane limit; the ragged block's owner among 4 / 8 / 16 waves (nfull = 7, 8, 15, 16, 17) and the second limit; the third
UNI_STORED = {
    "S12": (1, 63, 64, 65, 1023, 1024, 1025, 2048, 3073, 4095, 4096, 4097),
    "S16": (7 * 1024 + 5, 8 * 1024, 15 * 1024 + 1000, 16 * 1024, 17 * 1024, 65535, 65536, 65537),
    "S24": ((1 << 20) - 1, 1 << 20, (1 << 20) + 1),
}
# bidirectional graphs store both directions, E' = 2E: each limit - 2, the limit, + 2, and one count in the middle of a block
BIDIR_STORED = {
    "S12": (2600, 4094, 4096, 4098),
    "S16": (21000, 65534, 65536, 65538),
    "S24": (600000, (1 << 20) - 2, 1 << 20, (1 << 20) + 2),
}


def cases(sizes=("S12", "S16", "S24")):
    """Every (size, E', bidirectional) of the suite."""
    return [(s, e, False) for s in sizes for e in UNI_STORED[s]] + [(s, e, True) for s in sizes for e in BIDIR_STORED[s]]


def case_id(c):
    return f"{c[0]}-{c[1]}-{'bidir' if c[2] else 'uni'}"


def planes(stored):
    """pick_planes / plan_planes of the library: the counter planes for E' stored edges (0: refused)."""
    for p in (12, 16, 20, 24):
        if stored < (1 << p):
            return p
    return 0


def bipartite_circulant(N, k, E):
    """(u, v, w) int64 arrays for build_csr((u, v, w), num_nodes=N, if_bidirectional=...)."""
    if N % 2 or not 2 * k - 1 < N // 2 or not 1 <= E <= N * k:
        raise ValueError(f"bipartite_circulant({N}, {k}, {E}): N even, 2k - 1 < N / 2, 1 <= E <= N k")
    e = np.arange(E, dtype=np.int64)
    u = e // k
    v = (u + 2 * (e % k) + 1) % N
    return u, v, np.ones(E, np.int64)


def case_edges(c):
    """The edge list of a case: E = E' edges, or E' / 2 when both directions are stored."""
    size, stored, bidir = c
    N, k = {**SIZES, **SIZES_EXTRA}[size]
    assert not bidir or stored % 2 == 0
    return (N,) + bipartite_circulant(N, k, stored // 2 if bidir else stored)


def states(N, seed, rows=B):
    """bool [rows, N]: row 0 all zeros (cut 0), row 1 the parity state and row 2 its complement (every edge cut), the rest random."""
    xb = np.random.RandomState(seed).randint(0, 2, size=(rows, N)).astype(bool)
    xb[0] = False
    xb[1] = (np.arange(N) & 1).astype(bool)
    xb[2] = ~xb[1]
    return xb


def stored_cut(xb, u, v, bidir):
    """int64 [B]: how many STORED edges each row of xb cuts (an edge of a bidirectional graph is stored, and counted, twice) -- the
    plain count sum_e x[u_e] ^ x[v_e], gathered from the transposed rows in chunks (oracle_np.maxcut_obj's fancy index over
    columns takes seconds at 2^20 edges)."""
    xt = np.ascontiguousarray(np.asarray(xb).astype(bool).T).view(np.uint8)
    tot = np.zeros(xt.shape[1], np.int64)
    for s in range(0, len(u), 1 << 17):
        tot += (xt[u[s:s + (1 << 17)]] ^ xt[v[s:s + (1 << 17)]]).sum(axis=0, dtype=np.int64)
    return tot * (2 if bidir else 1)


def obj_of(xb, u, v, bidir):
    """EnvMaxcut.calculate_obj_values: the stored count, halved when bidirectional."""
    c = stored_cut(xb, u, v, bidir)
    return c // 2 if bidir else c
