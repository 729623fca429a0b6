"""Plain numpy restatements of the glue that ends every MCPG round (csrc/rls_mcpg.hip: rls_mcpg_pick_best, rls_mcpg_merge_best,
rls_mcpg_value_bit_sums, rls_mcpg_pack_chains, rls_mcpg_unpack_chains), and the launchers' dispatch arithmetic as constants.

Chains are bit-packed tile-major as in include/rlsolver_hip.h: words uint64 [ceil(C / 64), N], word (t, n) bit e = node n of
chain 64 t + e.  Nothing here builds an [N, C] array for the bit sums: they walk the tiles in chunks.  numpy only, no GPU;
tests/test_glue_oracle.py holds every function to the ones the project already trusts."""
import numpy as np

# ---- dispatch arithmetic, restated from the launchers (csrc/rls_mcpg.hip unless another file is named) ----
LDS_BYTES = 160 * 1024                                   # kLdsBytes, csrc/rls_host.h:10
BITSUM_THREADS = 512                                     # kBitSumThreads, :1106
BITSUM_REGS = 24                                         # kBitSumRegs, :1107
BITSUM_FIXED_LDS = (8 * 256 + 64) * 4                    # the eight tables and the tile's values, :1705
BITSUM_REG_MAX_N = BITSUM_REGS * BITSUM_THREADS          # `regs`, :1704: the register form up to 12 288 nodes
BITSUM_LDS_MIN_N = BITSUM_REG_MAX_N + 1                  # 12 289: the sums move to LDS
BITSUM_LDS_MAX_N = (LDS_BYTES // 2 - BITSUM_FIXED_LDS) // 4    # `lds <= kLdsBytes / 2`, :1706: 18 368
BITSUM_ATOMIC_MIN_N = BITSUM_LDS_MAX_N + 1               # 18 369: one atomic per (tile, node)
PACK_LINE_N_END = 1 << 21                                # the line-wide f32 pack takes N < 2^21, :1730
PACK_N_END = 1 << 22                                     # every pack is refused from N = 2^22, :1727
UNPACK_SWEEP_ROWS = 32768                                # rows one sweep of the unpack's grid.y covers, :1746
MERGE_THREADS = 1024                                     # the one workgroup of k_mcpg_merge_minmax, :1694
PICK_UNROLL = 8                                          # the argmin's unroll over repeats, :956


def bitsum_form(N):
    """The kernel rls_mcpg_value_bit_sums takes at N nodes: "regs", "lds" or "atomic" (:1704-1706)."""
    return "regs" if N <= BITSUM_REG_MAX_N else "lds" if N <= BITSUM_LDS_MAX_N else "atomic"


def bitsum_grid(N, C):
    """Workgroups of the two table forms (:1709-1712): the resident ones (by LDS and by 2048 threads per CU, 256 CUs), at most
    one per tile.  A launch with more tiles than this loops `tile += gridDim.x`."""
    lds = BITSUM_FIXED_LDS + (0 if N <= BITSUM_REG_MAX_N else 4 * N)
    assert lds <= LDS_BYTES // 2, "the atomic form has no resident grid"
    return min(256 * min(LDS_BYTES // lds, 2048 // BITSUM_THREADS), (C + 63) // 64)


BITSUM_REG_GRID = bitsum_grid(1, 1 << 30)                # 1024
BITSUM_LDS_GRID = bitsum_grid(BITSUM_LDS_MIN_N, 1 << 30)  # 512


# ---- words ----
def _bits(x):
    """The pack rule: float32 `> 0` (so -0.0, negatives and NaN are 0, 0.5 and 2 are 1), uint8 / bool `!= 0`."""
    x = np.asarray(x)
    return x > 0 if x.dtype.kind == "f" else x != 0


def pack_words(x):
    """[N, C] float32 / uint8 / bool -> uint64 [ceil(C / 64), N]; bits past C are zero."""
    b = _bits(x)
    N, C = b.shape
    words = np.zeros(((C + 63) // 64, N), np.uint64)
    for c in range(C):
        words[c >> 6] |= b[:, c].astype(np.uint64) << np.uint64(c & 63)
    return words


def unpack_words(words, C):
    """uint64 [ceil(C / 64), N] -> float32 [N, C] of 0.0 | 1.0; bits past C are ignored."""
    words = np.asarray(words).view(np.uint64)
    out = np.empty((words.shape[1], C), np.float32)
    for c in range(C):
        out[:, c] = ((words[c >> 6] >> np.uint64(c & 63)) & np.uint64(1)).astype(np.float32)
    return out


def mask_past(words, C):
    """`words` with the bits past chain C of the last tile cleared."""
    words = np.asarray(words).view(np.uint64).copy()
    if C % 64:
        words[-1] &= np.uint64((1 << (C % 64)) - 1)
    return words


def column(words, m):
    """Chain m as uint64 0 | 1 [N]."""
    return (words[m >> 6] >> np.uint64(m & 63)) & np.uint64(1)


def set_column(words, m, bits):
    sh = np.uint64(m & 63)
    words[m >> 6] = (words[m >> 6] & ~(np.uint64(1) << sh)) | (bits << sh)


# ---- pick ----
def pick(expected, M, R, num_edges):
    """Best of R repeats per kept chain, one loop per chain: start from repeat 0, replace on strict `<`.  A NaN in repeat 0
    therefore stays and a NaN later is skipped (methods/MCPG_cheeger.py's docstring states this rule).
    -> (best_index int64 [M] = m + r M, vs float32 [M] = (f32(num_edges) - best) / 2 in float32)."""
    expected = np.asarray(expected, np.float32)
    assert expected.shape == (M * R,)
    idx = np.empty(M, np.int64)
    vs = np.empty(M, np.float32)
    with np.errstate(invalid="ignore"):
        for m in range(M):
            best, br = expected[m], 0
            for r in range(1, R):
                v = expected[r * M + m]
                if v < best:
                    best, br = v, r
            idx[m] = m + br * M
            vs[m] = (np.float32(num_edges) - best) / np.float32(2.0)
    return idx, vs


# ---- merge ----
def first_extreme(v, greatest):
    """The kernel's best / worst rule: a value is taken if it compares greater (less) than the one held, or if none is held yet
    and it is not NaN.  Every value NaN: index 0.  On finite input this is the first argmax (argmin)."""
    at = None
    for m, x in enumerate(v):
        if x != x:
            continue
        if at is None or (x > v[at] if greatest else x < v[at]):
            at = m
    return 0 if at is None else at


def merge(temp_max, temp_info, now_res, now_info, replace_worst=True):
    """methods/MCPG.py:376-391 on packed words, on copies.  Per chain (as oracle_np.mcpg_merge_best): temp_max[m] > now_res[m]
    moves the value and the chain into the incumbent.  Then the best incumbent overwrites the worst (value, incumbent column,
    and temp_info's column, which seeds the next round), best and worst by first_extreme.
    -> (now_res, now_info, temp_info, values, indices): replace_worst: values = [best], indices = [its chain]; otherwise nothing
    is replaced and values = [max, min], indices = their first chains."""
    temp_max = np.asarray(temp_max, np.float32)
    now_res = np.asarray(now_res, np.float32).copy()
    now_info = np.asarray(now_info).view(np.uint64).copy()
    temp_info = np.asarray(temp_info).view(np.uint64).copy()
    for m in range(temp_max.shape[0]):
        if temp_max[m] > now_res[m]:
            now_res[m] = temp_max[m]
            set_column(now_info, m, column(temp_info, m))
    hi, lo = first_extreme(now_res, True), first_extreme(now_res, False)
    if not replace_worst:
        return now_res, now_info, temp_info, np.array([now_res[hi], now_res[lo]], np.float32), np.array([hi, lo], np.int64)
    best = now_res[hi]
    now_res[lo] = best
    src = column(now_info, hi)
    set_column(now_info, lo, src)
    set_column(temp_info, lo, src)
    return now_res, now_info, temp_info, np.array([best], np.float32), np.array([hi], np.int64)


# ---- bit sums ----
def bit_sums_many(words, C, values, chunk=8):
    """sum_c values[c, k] s[n, c] in float64 for K value vectors at once -> [N, K], tile chunk by tile chunk.  s is a SELECT, not
    a factor: a non-finite value counts only where its bit is set (inf - inf and NaN propagate from there)."""
    words = np.ascontiguousarray(np.asarray(words).view(np.uint64))
    tiles, N = words.shape
    assert tiles == (C + 63) // 64
    values = np.asarray(values, np.float64).reshape(C, -1)
    K = values.shape[1]
    finite = np.isfinite(values)
    V = np.zeros((tiles * 64, K))
    V[:C] = np.where(finite, values, 0.0)
    out = np.zeros((N, K))
    for t0 in range(0, tiles, chunk):
        t1 = min(t0 + chunk, tiles)
        bits = np.unpackbits(words[t0:t1].view(np.uint8).reshape(t1 - t0, N, 8), axis=2, bitorder="little")   # [t, N, 64]
        out += bits.transpose(1, 0, 2).reshape(N, (t1 - t0) * 64).astype(np.float64) @ V[t0 * 64:t1 * 64]
    with np.errstate(invalid="ignore"):
        for c, k in zip(*np.nonzero(~finite)):
            out[column(words, int(c)) != 0, k] += values[c, k]
    return out


def bit_sums_exact(words, C, value):
    """A[n] = sum_c value[c] s[n, c] as float64 [N] (exact for values that are small integers or halves, and 53 bits of a
    float32 sum otherwise)."""
    return bit_sums_many(words, C, np.asarray(value, np.float64)[:, None])[:, 0]


def bit_sums_abs(words, C, value):
    """sum_c |value[c]| s[n, c]: the scale of the float32 summation error bound  C 2^-24 bit_sums_abs(n)."""
    return bit_sums_many(words, C, np.abs(np.asarray(value, np.float64))[:, None])[:, 0]
