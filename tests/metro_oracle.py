"""Numpy restatement of the MCPG metro walk (K9) as include/rlsolver_hip.h states it: one rls_mcpg_metro_rounds launch, the
counter hash of its production draws, the stop rule of rls_mcpg_metro_stop -- and, for the CPU tests only, a model of the ORDER in
which the bit-packed walker reads its words (two rounds of look-ahead, repaired in registers), with single repairs removable.

No torch: every function takes and returns numpy arrays.  x is bool [N, C] (node-major, chains the fast axis), index int64 [T, C],
u float32 [T, C], probs float32 [N]; rows of index / u are the rounds of ONE launch (the caller slices t_offset away)."""
import numpy as np

F32 = np.float32
WIN = 64            # rounds per draw window of the packed walker
BLOCK = 8           # rounds whose entries the walker fetches at a time


# ------------------------------------------------------------------------------------------ one launch
def accept_rate(q):
    """(1 - q) / q as two IEEE float32 operations: q = 0 gives inf (always accept), q = 1 gives 0 (never)."""
    q = np.asarray(q, F32)
    with np.errstate(divide="ignore", invalid="ignore"):
        return ((F32(1) - q) / q).astype(F32)


def pack(x):
    """bool [N, C] -> uint64 [ceil(C / 64), N]: word (t, n) bit e = x[n, 64 t + e]; bits of chains >= C are 0."""
    x = np.asarray(x, bool)
    N, C = x.shape
    tiles = (C + 63) // 64
    padded = np.zeros((N, tiles * 64), bool)
    padded[:, :C] = x
    bits = padded.reshape(N, tiles, 64).astype(np.uint64) << np.arange(64, dtype=np.uint64)
    return np.ascontiguousarray(np.bitwise_or.reduce(bits, axis=2).T)


class Walker:
    """The chains of one launch, advanced a round at a time.  ``x`` bool [N, C] and ``words`` (its packed form) are kept in step,
    so a test can compare either surface after every round without repacking N * C bits."""

    def __init__(self, x, probs):
        self.x = np.array(x, dtype=bool)
        self.probs = np.asarray(probs, F32)
        self.words = pack(self.x)
        C = self.x.shape[1]
        self._col = np.arange(C)
        self._tile = self._col // 64
        self._bit = np.uint64(1) << (self._col % 64).astype(np.uint64)

    def step(self, idx, uu):
        """One round: chain c proposes node idx[c] with uniform uu[c].  Returns the accept row (bool [C])."""
        idx = np.asarray(idx, np.int64)
        val = self.x[idx, self._col]
        base = self.probs[idx]
        q = np.where(val, base, F32(1) - base).astype(F32)
        acc = np.asarray(uu, F32) < accept_rate(q)
        self.x[idx[acc], self._col[acc]] = ~val[acc]
        np.bitwise_xor.at(self.words, (self._tile[acc], idx[acc]), self._bit[acc])
        return acc


def launch(x, probs, index, u, t_limit=None):
    """One rls_mcpg_metro_rounds launch: rounds 0 .. min(T, max(t_limit, 0)) - 1 of index / u, no stop rule inside.
    Returns (states bool [T + 1, N, C] -- states[r] is the state after r rounds, rounds past the limit repeat the last one --,
    accepts bool [T, C], zero past the limit)."""
    T, C = np.asarray(index).shape
    t_end = T if t_limit is None else min(T, max(int(t_limit), 0))
    wk = Walker(x, probs)
    states = np.empty((T + 1,) + wk.x.shape, bool)
    acc = np.zeros((T, C), bool)
    states[0] = wk.x
    for t in range(T):
        if t < t_end:
            acc[t] = wk.step(index[t], u[t])
        states[t + 1] = wk.x
    return states, acc


# ------------------------------------------------------------------------------------------ production draws
def fmix(h):
    """murmur3's 32-bit finaliser on uint32 arrays (rls_chains.h: k7_fmix32)."""
    h = np.asarray(h, np.uint64) & np.uint64(0xFFFFFFFF)
    m = np.uint64(0xFFFFFFFF)
    h ^= h >> np.uint64(16)
    h = (h * np.uint64(0x85EBCA6B)) & m
    h ^= h >> np.uint64(13)
    h = (h * np.uint64(0xC2B2AE35)) & m
    h ^= h >> np.uint64(16)
    return h


def global_ids(C, chain_ids=None):
    """rls_chain_ids (offset, period, skip) -> the global id of every local chain."""
    off, per, skip = (0, 0, 0) if chain_ids is None else (int(v) for v in chain_ids)
    c = np.arange(C, dtype=np.int64)
    return off + c + ((c // per) * skip if per > 0 and skip > 0 else 0)


def production_draws(seed, chain_ids, t0, T, N):
    """The in-kernel draws of rounds t0 .. t0 + T - 1 for the chains with GLOBAL ids ``chain_ids`` (int array [C]) under the
    64-bit ``seed``: (index int64 [T, C], u float32 [T, C])."""
    m = np.uint64(0xFFFFFFFF)
    golden = np.uint64(0x9E3779B1)
    seed = int(seed) & ((1 << 64) - 1)
    s_lo, s_hi = np.uint64(seed & 0xFFFFFFFF), np.uint64(seed >> 32)
    gc = np.asarray(chain_ids, np.int64).astype(np.uint64)
    g_lo, g_hi = gc & m, gc >> np.uint64(32)
    key = fmix(s_lo ^ fmix(s_hi ^ fmix(g_lo) ^ ((g_hi * golden) & m)))                       # [C]
    t = (np.arange(t0, t0 + T, dtype=np.uint64) & m)[:, None]
    k = key[None, :] ^ ((t * golden) & m)                                                     # [T, C]
    r0 = fmix(k ^ np.uint64(0x4D455452))
    r1 = fmix((k + np.uint64(0x7FEB352D)) & m)
    index = ((r0 * np.uint64(N)) >> np.uint64(32)).astype(np.int64)
    u = ((r1 >> np.uint64(8)).astype(F32) * F32(2.0 ** -24)).astype(F32)
    return index, u


# ------------------------------------------------------------------------------------------ stop rule
def stop(acc, target, first, next_T, ctl):
    """rls_mcpg_metro_stop on accepts [rows, T] (or [T]): returns (ctl' = [total, live, limit of the next dry pass], apply_limit)
    as Python ints.  ``ctl`` is read unless first == 1."""
    acc = np.asarray(acc, np.int64)
    col = acc.reshape(-1, acc.shape[-1]).sum(axis=0)
    T = col.shape[0]
    before = 0 if first == 1 else int(ctl[0])
    run = before + np.cumsum(col)
    total = int(run[-1])
    reached = np.nonzero(run >= target)[0]
    stop_at = int(reached[0]) + 1 if reached.size else None
    live = first == 1 or int(ctl[1]) != 0
    limit = T if first else int(ctl[2])
    hit = (total >= target) if first else (stop_at is not None)
    apply_limit = min(limit, stop_at if (hit and not first) else T)
    go_on = live and not hit
    return [total, 1 if go_on else 0, int(next_T) if go_on else 0], apply_limit


def walk_chunks(probs, start, T, index, u, chunk):
    """metro_sampling as methods/MCPG.py: _walk_chunks calls the two entry points: chunks of ``chunk`` rounds, applied directly
    inside the first T rounds, dry pass -> stop -> apply pass after them.  Returns (final state bool [N, C], rounds applied)."""
    x = np.asarray(start).astype(bool)
    C = x.shape[1]
    Tmax = min(5 * T, len(index))
    target = C * T
    starts = list(range(0, Tmax, chunk))
    sizes = [min(chunk, Tmax - t0) for t0 in starts]
    ctl, used = [0, 0, 0], 0
    for k, (t0, tk) in enumerate(zip(starts, sizes)):
        next_tk = sizes[k + 1] if k + 1 < len(sizes) else 0
        ix, uu = index[t0:t0 + tk], u[t0:t0 + tk]
        if t0 + tk <= max(1, T):
            states, acc = launch(x, probs, ix, uu)
            ctl, _ = stop(acc.sum(axis=1), target, 1 if k == 0 else 2, next_tk, ctl)
            x, used = states[-1], used + tk
        else:
            _, acc = launch(x, probs, ix, uu, t_limit=ctl[2])
            ctl, lim = stop(acc.sum(axis=1), target, 0, next_tk, ctl)
            x, used = launch(x, probs, ix, uu, t_limit=lim)[0][-1], used + max(0, min(tk, lim))
    return x, used


# ------------------------------------------------------------------------------------------ draws that collide
def pattern_draws(N, T, C, seed):
    """Recorded draws that revisit nodes at the distances the packed walker's look-ahead has to repair.  Chain c follows pattern
    c % 6 on a base node a and one other node b:  a a a ... | a b a b ... | a a b a a b ... | a a b b ... | uniform over
    min(N, 3) nodes | uniform over N.  Returns (index int64 [T, C], u float32 [T, C] in [0, 1), probs float32 [N] in [0.2, 0.8])."""
    rng = np.random.RandomState(seed)
    a = rng.randint(0, N, size=C)
    b = (a + 1 + rng.randint(0, max(N - 1, 1), size=C)) % N          # another node (a itself when N = 1)
    t = np.arange(T)[:, None]
    pat = np.arange(C) % 6
    use_b = np.select([pat == 0, pat == 1, pat == 2, pat == 3], [t < 0, t % 2 == 1, t % 3 == 2, t % 4 >= 2], default=False)
    index = np.where(use_b, b[None, :], a[None, :])
    few = rng.randint(0, min(N, 3), size=(T, C))
    anyn = rng.randint(0, N, size=(T, C))
    index = np.where(pat == 4, few, np.where(pat == 5, anyn, index)).astype(np.int64)
    u = rng.rand(T, C).astype(F32)
    u[u >= 1] = F32(0)
    probs = (rng.rand(N) * 0.6 + 0.2).astype(F32)
    return index, u, probs


# (N, T, C, seed) of the hazard cases: one node, two, a handful, and a graph-sized N; T with a ragged last window and a ragged last
# block of eight.  The seeds are arbitrary but for N = 2, where the draw decides the only two probabilities there are: with both
# next to 1/2 (N * 1000 + T gives 0.490, 0.493) the rate (1 - q) / q is ~1 whatever the bit, nearly every proposal is accepted and
# no read order can be told from another; seed 7 gives 0.646, 0.719.
HAZARDS = [(1, 70, 64, 1070), (2, 70, 64, 7), (5, 130, 70, 5130), (3, 200, 130, 3200), (300, 131, 130, 300131)]


# ------------------------------------------------------------------------------------------ the packed walker's read order
DROPS = ("r1", "r2", "block_edge", "win_2nd", "win_3rd", "last_block")


def stale_walk(x, probs, index, u, drop=None):
    """The packed walker (k_mcpg_metro_packed) as a model of WHEN it reads: per window of 64 rounds the words of rounds 0 and 1 are
    read fresh, then round r reads the word of round r + 2 BEFORE it issues its own flip, so that word misses the flips of rounds r
    and r + 1 -- repaired in registers where they hit the same node ("r2": the flip of round r into the word of round r + 2; "r1":
    the flip of round r into the word of round r + 1).  ``drop`` removes repairs:
        None          the walker as written (equals launch())        "r1" / "r2"   that repair at every round
        "block_edge"  both, where the entry of round r + 2 comes from the next block of eight (r % 8 in 6, 7)
        "win_2nd"     r1 at a window's round 0 (its 2nd round reads stale)
        "win_3rd"     r2 at round 0 and r1 at round 1 (its 3rd round reads stale)
        "last_block"  both in a window's last block (rounds 56 .. 63)
    Returns the accept matrix bool [T, C].  A model of the order, not the kernel: it runs on the CPU only."""
    assert drop is None or drop in DROPS
    x = np.array(x, dtype=bool)
    probs = np.asarray(probs, F32)
    index = np.asarray(index, np.int64)
    u = np.asarray(u, F32)
    T, C = index.shape
    col = np.arange(C)
    # the producers' two verdicts per (round, chain): they do not depend on the state
    p = probs[index]
    a_set, a_clear = u < accept_rate(p), u < accept_rate(F32(1) - p)
    r = np.arange(WIN)
    keep1 = np.ones(WIN, bool)
    keep2 = np.ones(WIN, bool)
    if drop == "r1":
        keep1[:] = False
    elif drop == "r2":
        keep2[:] = False
    elif drop == "block_edge":
        keep1[r % BLOCK >= BLOCK - 2] = keep2[r % BLOCK >= BLOCK - 2] = False
    elif drop == "win_2nd":
        keep1[0] = False
    elif drop == "win_3rd":
        keep2[0] = keep1[1] = False
    elif drop == "last_block":
        keep1[WIN - BLOCK:] = keep2[WIN - BLOCK:] = False
    acc_out = np.zeros((T, C), bool)
    for w0 in range(0, T, WIN):
        rounds = min(WIN, T - w0)

        def node(k):                                   # entries past the window or the launch are 0: node 0, no verdict
            return index[w0 + k] if k < rounds else np.zeros(C, np.int64)
        i0, i1 = node(0), node(1)
        v0, v1 = x[i0, col].copy(), x[i1, col].copy()  # read fresh after the window barrier
        m1 = np.zeros(C, bool)
        for k in range(rounds):
            acc = np.where(v0, a_set[w0 + k], a_clear[w0 + k])
            i2 = node(k + 2) if k + 2 < WIN else np.zeros(C, np.int64)
            v2 = x[i2, col].copy()                     # the look-ahead read: issued before this round's flip
            x[i0[acc], col[acc]] ^= True
            m2 = acc & (i2 == i0) & keep2[k]
            m1 = m1 ^ (acc & (i1 == i0) & keep1[k])
            acc_out[w0 + k] = acc
            v0, i0, v1, m1, i1 = v1 ^ m1, i1, v2, m2, i2
    return acc_out
