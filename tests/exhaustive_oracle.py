"""The exact optimum of a spin system by enumeration, restated in numpy: vectorised over blocks of states, first-minimum rule.

State i of N spins is read MSB first: node k is +1 iff bit N-1-k of i is set (np.binary_repr(i, width=N)).  E(i) = -s'Ws / 2 in
float64; the minimum over i0 <= i < i1 is attained FIRST at the smallest such i (strict `<` in ascending order).  Everything here
is exact for integer-valued W: the sums are small integers and halves."""
import numpy as np

KEY_BIAS = 4096
KEY_EMPTY = (1 << 63) - 1


def spins_of(index, N):
    """signed spins f64 [..., N] of state indices (int or int64 array)"""
    idx = np.asarray(index, dtype=np.int64)
    return 2.0 * ((idx[..., None] >> np.arange(N - 1, -1, -1, dtype=np.int64)) & 1) - 1.0


def index_of(spins):
    """state index of signed spins [N]"""
    return int("".join("1" if v > 0 else "0" for v in np.asarray(spins)), 2)


def energies(W, i0, i1):
    """E(i) f64 for i0 <= i < i1"""
    W = np.asarray(W, dtype=np.float64)
    s = spins_of(np.arange(i0, i1, dtype=np.int64), W.shape[0])
    return -np.einsum("ij,ij->i", s @ W, s) / 2


def calc_over_range(W, i0, i1, maximize=False, block=1 << 15):
    """-> (optimal energy, the first index that attains it, its signed spins)"""
    assert 0 <= i0 < i1 <= 1 << np.asarray(W).shape[0]
    best_e, best_i = None, None
    for a in range(i0, i1, block):
        e = energies(W, a, min(a + block, i1))
        j = int(np.argmax(e) if maximize else np.argmin(e))          # the first occurrence
        if best_e is None or (e[j] > best_e if maximize else e[j] < best_e):
            best_e, best_i = float(e[j]), a + j
    return best_e, best_i, spins_of(best_i, np.asarray(W).shape[0])


def e_off(W, spins):
    """-sum_{p<q} W_pq s_p s_q"""
    W = np.asarray(W, dtype=np.float64)
    return float(-(np.triu(W, 1) * np.outer(spins, spins)).sum())


def cut(W, spins):
    """(1 / 4) sum_ij W_ij (1 - s_i s_j), the reference's calculate_cut"""
    W = np.asarray(W, dtype=np.float64)
    return float(0.25 * np.sum(W * (1 - np.outer(spins, spins))))


def key_encode(e, index):
    return ((int(e) + KEY_BIAS) << 48) | int(index)


def key_decode(key):
    key = int(key)
    return (key >> 48) - KEY_BIAS, key & ((1 << 48) - 1)


def key_of(W, i0, i1, maximize=False):
    """What the kernel's key holds after the range: E_off of the optimum (of -W under maximize: the masks are swapped) and its index."""
    W = np.asarray(W, dtype=np.float64)
    _, i, s = calc_over_range(W, i0, i1, maximize)
    e = e_off(W, s)
    return key_encode(-e if maximize else e, i)


def random_couplings(rng, N, density=0.5, diagonal=False):
    """symmetric f64 [N, N], off-diagonal entries in {-1, 0, +1}; `diagonal`: integers in [-2, 2] on it"""
    W = np.triu(rng.choice([-1.0, 1.0], size=(N, N)) * (rng.rand(N, N) < density), 1)
    W = W + W.T
    if diagonal:
        W[np.diag_indices(N)] = rng.randint(-2, 3, size=N)
    return W


def planted(N, t, edges):
    """W_pq = t_p t_q on `edges`: the ground states are +-t (the graph connected), E_off = -len(edges)"""
    W = np.zeros((N, N))
    for a, b in edges:
        W[a, b] = W[b, a] = t[a] * t[b]
    return W


def split_range(total, rank, world):
    return total * rank // world, total * (rank + 1) // world
