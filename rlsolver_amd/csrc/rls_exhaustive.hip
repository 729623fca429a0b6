// Exact optimum of a spin system by enumeration of all 2^N states for gfx950: SpinSystemBase.calculate_best_energy() and its
// helper _calc_over_range(i0, iMax) of ECO_S2V/src/envs/spinsystem.py:278-324, 615-651 (a Python loop over np.binary_repr(i)
// with two matmuls per state there).
//
// State index i is read MSB first: node k's spin is +1 iff bit N-1-k of i is set.  E = -s'Ws / 2 = -tr(W) / 2 + E_off with
// E_off = -sum_{p<q} W_pq s_p s_q; the couplings are 0 / +-1 off the diagonal, so a node's row is two bit masks (pos, neg) and
// its local field over a set M of nodes is  h_p(M) = sum_{q in M} W_pq s_q = 2 popc((x & pos & M) | (~x & neg & M)) - popc((pos | neg) & M)
// (pos and neg are disjoint: one bit-select and one popcount).
//
// A thread owns aligned chunks of 2^L consecutive indices (L = min(N, 10)).  With H the high N - L nodes and Lo the low L nodes
//     E_off = E_HH(x_hi) + E_LL(x_lo) - sum_{b in Lo} s_b g_b,        g_b = h_b(H)
// E_HH and the L cross fields g_b are computed once per chunk (N popcount steps).  E_LL depends on the low bits only: the workgroup
// builds the table tab[j] = (E_LL(gray(j)) << L) + gray(j) once, for all its chunks.  The chunk is then walked in reflected Gray
// order (step j flips bit ctz(j)); every lane of a wave walks the same j, so the flipped bit, its sign and tab[j] are wave-uniform
// and a state costs three VALU operations: V +- 2 g_b, + tab[j], min.  The low four Gray bits are unrolled (their g_b stay in
// registers and their signs are compile-time but for one step in sixteen); the other levels read g_b from LDS.  The lane's 32-bit
// running minimum ((E_off + 4096) << L | low index bits) becomes the 64-bit key once per chunk; a wave that holds a chunk cut by
// [i0, i1) -- the first and the last of a launch -- walks the checked form, which folds only the states inside.
// Reduction: lanes -> wave (shuffles) -> workgroup (LDS) -> one 64-bit atomicMin per workgroup and graph.  The lexicographic
// minimum of (energy, index) does not depend on any of this geometry.
#include "rls_common.h"
#include "rls_tile.h"

namespace rls {

constexpr int kExMaxN = 48;        // spins: the index field of the key is 48 bits
constexpr int kExL = 10;           // a chunk is 2^min(N, kExL) states
constexpr int kExU = 4;            // unrolled Gray levels (when the chunk has at least that many)
constexpr int kExBlock = 256;
constexpr int kExBias = 4096;      // key = ((E_off + kExBias) << 48) | index
constexpr int64_t kExMaxG = 1ll << 22;
constexpr uint32_t kExNone = 0xFFFFFFFFu;

__device__ __forceinline__ int ex_popc(uint32_t v) { return __popc(v); }
__device__ __forceinline__ int ex_popc(uint64_t v) { return __popcll(v); }

// sum_{q in the masks} W_pq s_q for the state x: a, b = the row's +1 / -1 masks (already cut to the node set)
template <typename Word> __device__ __forceinline__ int ex_field(Word x, Word a, Word b) {
    return 2 * ex_popc((Word)((x & a) | (~x & b))) - ex_popc((Word)(a | b));
}

template <typename T>
__global__ __launch_bounds__(kWave) void k_spin_exhaustive_pack(const T* __restrict__ matrix, int N, uint64_t* __restrict__ pos,
                                                                uint64_t* __restrict__ neg, uint8_t* __restrict__ flags) {
    __shared__ unsigned bad_any;
    const int p = threadIdx.x;
    const int64_t g = blockIdx.x;
    if (p == 0) bad_any = 0u;
    __syncthreads();
    if (p < N) {
        const T* m = matrix + g * N * N;
        uint64_t a = 0, b = 0;
        unsigned bad = 0u;
        for (int j = 0; j < N; ++j) {
            if (j == p) continue;
            const T v = m[(int64_t)p * N + j];
            if (v == (T)1) a |= 1ull << (N - 1 - j);
            else if (v == (T)-1) b |= 1ull << (N - 1 - j);
            else if (!(v == (T)0)) bad |= 1u;
            if (!(v == m[(int64_t)j * N + p])) bad |= 2u;
        }
        pos[g * N + p] = a;
        neg[g * N + p] = b;
        if (bad) atomicOr(&bad_any, bad);
    }
    __syncthreads();
    if (p == 0) flags[g] = (uint8_t)bad_any;
}

// One chunk in reflected Gray order -> min over its states of Vs + tab[j] (EDGE: over the states inside [i0, i1) only; kExNone if none).
// Vs = (E_HH + sum_b g_b + kExBias) << L: the chunk's energy without E_LL at low bits 0 (every low spin -1).
template <int U, bool EDGE>
__device__ __forceinline__ uint32_t ex_walk(uint32_t Vs, const int (&g2)[U > 0 ? U : 1], const int (*gsh)[kExBlock], const uint32_t* tab, int L,
                                            int tid, int64_t chunk_lo, int64_t i0, int64_t i1) {
    constexpr int kInner = 1 << U;
    const int nblk = (1 << L) >> U;
    const uint32_t lo_mask = (1u << L) - 1u;
    uint32_t best = kExNone;
    auto fold = [&](uint32_t t) {
        uint32_t k = Vs + t;
        if (EDGE) {
            const int64_t idx = chunk_lo + (int64_t)(t & lo_mask);
            k = (idx >= i0 && idx < i1) ? k : kExNone;
        }
        best = k < best ? k : best;
    };
    for (int jh = 0; jh < nblk; ++jh) {
        if (jh) {                                            // the step that flips a level above the unrolled ones
            const int b = U + __builtin_ctz(jh), m = (jh << U) - 1;
            const int d = gsh[b][tid];
            Vs += (((m >> b) ^ (m >> (b + 1))) & 1) ? (uint32_t)d : (uint32_t)-d;      // the bit before the flip: 1 -> the spin goes to -1
        }
        uint32_t tl[kInner];
        if (U == 4) {
            const uint4* t4 = reinterpret_cast<const uint4*>(tab) + jh * 4;
#pragma unroll
            for (int q = 0; q < 4; ++q) {
                const uint4 v = t4[q];
                tl[q * 4 + 0] = v.x; tl[q * 4 + 1] = v.y; tl[q * 4 + 2] = v.z; tl[q * 4 + 3] = v.w;
            }
        } else {
#pragma unroll
            for (int q = 0; q < kInner; ++q) tl[q] = tab[(jh << U) + q];
        }
        fold(tl[0]);
#pragma unroll
        for (int jl = 1; jl < kInner; ++jl) {
            const int b = __builtin_ctz(jl), m = jl - 1;
            const int prev = ((m >> b) ^ (b + 1 < U ? (m >> (b + 1)) : jh)) & 1;       // compile-time but for b = U - 1
            Vs += prev ? (uint32_t)g2[b] : (uint32_t)-g2[b];
            fold(tl[jl]);
        }
    }
    return best;
}

template <typename Word, int U>
__global__ __launch_bounds__(kExBlock) void k_spin_exhaustive(const uint64_t* __restrict__ pos, const uint64_t* __restrict__ neg, int N, int L,
                                                              int bx, int64_t i0, int64_t i1, unsigned long long* __restrict__ key) {
    __shared__ __attribute__((aligned(16))) uint32_t tab[1 << kExL];
    __shared__ int gsh[kExL][kExBlock];
    __shared__ Word ma[kExMaxN], mb[kExMaxN];               // the rows' masks cut to the high nodes
    __shared__ unsigned long long red[kExBlock / kWave];
    const int tid = threadIdx.x, lane = tid & (kWave - 1), w = tid >> 6;
    const int64_t g = (int64_t)blockIdx.x / bx;
    const int bxi = (int)((int64_t)blockIdx.x % bx);
    const uint64_t* P = pos + g * N;
    const uint64_t* Q = neg + g * N;
    const int n_lo = 1 << L;
    const Word lo_mask = (Word)(n_lo - 1);
    const Word full = N >= (int)(8 * sizeof(Word)) ? ~(Word)0 : (Word)(((Word)1 << N) - 1);
    const Word hi_mask = full & ~lo_mask;

    for (int p = tid; p < N; p += kExBlock) {
        ma[p] = (Word)P[p] & hi_mask;
        mb[p] = (Word)Q[p] & hi_mask;
    }
    // E_LL of every low pattern, in Gray order: tab[j] = (E_LL(gray(j)) << L) + gray(j)  (mod 2^32: E_LL may be negative)
    for (int j = tid; j < n_lo; j += kExBlock) {
        const Word lo = (Word)(j ^ (j >> 1));
        int s2 = 0;
        for (int b = 0; b < L; ++b) {
            const int f = ex_field<Word>(lo, (Word)P[N - 1 - b] & lo_mask, (Word)Q[N - 1 - b] & lo_mask);
            s2 += ((lo >> b) & 1) ? f : -f;
        }
        tab[j] = (uint32_t)(-(s2 >> 1) * n_lo) + (uint32_t)lo;
    }
    __syncthreads();

    const int64_t c_last = (i1 - 1) >> L;
    const int64_t stride = (int64_t)bx * kExBlock;
    unsigned long long mine = ~0ull;
    for (int64_t base = (i0 >> L) + (int64_t)bxi * kExBlock + w * kWave; base <= c_last; base += stride) {     // (wave-uniform)
        const int64_t c = base + lane;
        const int64_t chunk_lo = c << L;
        const bool inside = c <= c_last && chunk_lo >= i0 && chunk_lo + n_lo <= i1;
        const bool edge = ballot64(!inside) != 0;
        const Word xhi = (Word)chunk_lo & full;
        int s2 = 0;                                          // 2 E_HH = -sum_{p in H} s_p h_p(H)
#pragma unroll 4
        for (int p = 0; p < N - L; ++p) {
            const int f = ex_field<Word>(xhi, ma[p], mb[p]);
            s2 += ((xhi >> (N - 1 - p)) & 1) ? f : -f;
        }
        int V = -(s2 >> 1) + kExBias;
        int g2[U > 0 ? U : 1] = {0};
#pragma unroll
        for (int b = 0; b < U; ++b) {
            const int gb = ex_field<Word>(xhi, ma[N - 1 - b], mb[N - 1 - b]);
            V += gb;                                         // every low spin starts at -1
            g2[b] = 2 * gb * n_lo;
        }
        for (int b = U; b < L; ++b) {
            const int gb = ex_field<Word>(xhi, ma[N - 1 - b], mb[N - 1 - b]);
            V += gb;
            gsh[b][tid] = 2 * gb * n_lo;
        }
        const uint32_t Vs = (uint32_t)(V * n_lo);
        const uint32_t best = edge ? ex_walk<U, true>(Vs, g2, gsh, tab, L, tid, chunk_lo, i0, i1)
                                   : ex_walk<U, false>(Vs, g2, gsh, tab, L, tid, chunk_lo, i0, i1);
        if (best != kExNone) {
            const unsigned long long k = ((unsigned long long)(best >> L) << 48) | (unsigned long long)(chunk_lo + (int64_t)(best & (uint32_t)(n_lo - 1)));
            mine = k < mine ? k : mine;
        }
    }
#pragma unroll
    for (int d = kWave / 2; d >= 1; d >>= 1) {
        const unsigned long long o = __shfl_xor(mine, d, kWave);
        mine = o < mine ? o : mine;
    }
    if (lane == 0) red[w] = mine;
    __syncthreads();
    if (tid == 0) {
#pragma unroll
        for (int q = 1; q < kExBlock / kWave; ++q) mine = red[q] < mine ? red[q] : mine;
        if (mine != ~0ull) atomicMin(key + g, mine);
    }
}

template <typename Word, int U>
static void ex_launch(const uint64_t* pos, const uint64_t* neg, int64_t G, int N, int L, int64_t i0, int64_t i1, uint64_t* key, hipStream_t s) {
    const int64_t chunks = ((i1 - 1) >> L) - (i0 >> L) + 1;
    int64_t bx = ceil_div(chunks, kExBlock), cap = (int64_t)num_cus() * 8 / G;
    if (cap < 1) cap = 1;
    if (bx > cap) bx = cap;
    hipLaunchKernelGGL((k_spin_exhaustive<Word, U>), dim3((unsigned)(G * bx)), dim3(kExBlock), 0, s, pos, neg, N, L, (int)bx, i0, i1,
                       reinterpret_cast<unsigned long long*>(key));
}

}  // namespace rls

using namespace rls;

extern "C" {

int rls_spin_exhaustive_pack(const void* matrix, int state_bytes, int64_t G, int64_t N, uint64_t* pos, uint64_t* neg, uint8_t* flags,
                             void* stream) {
    RLS_REQUIRE(state_bytes == 4 || state_bytes == 8, RLS_EINVAL, "state_bytes must be 4 (float) or 8 (double), got %d", state_bytes);
    RLS_REQUIRE(N >= 1 && N <= kExMaxN, RLS_EINVAL, "spin_exhaustive_pack: N = %lld outside [1, %d]", (long long)N, kExMaxN);
    RLS_REQUIRE(G >= 0 && G < (1ll << 31), RLS_EINVAL, "spin_exhaustive_pack: G = %lld outside [0, 2^31)", (long long)G);
    if (G == 0) return RLS_OK;
    RLS_REQUIRE(matrix && pos && neg && flags, RLS_EINVAL, "NULL pointer");
    if (state_bytes == 4)
        hipLaunchKernelGGL(k_spin_exhaustive_pack<float>, dim3((unsigned)G), dim3(kWave), 0, as_stream(stream), (const float*)matrix, (int)N, pos, neg, flags);
    else
        hipLaunchKernelGGL(k_spin_exhaustive_pack<double>, dim3((unsigned)G), dim3(kWave), 0, as_stream(stream), (const double*)matrix, (int)N, pos, neg, flags);
    return check_launch("k_spin_exhaustive_pack");
}

int rls_spin_exhaustive(const uint64_t* pos, const uint64_t* neg, int64_t G, int64_t N, int64_t i0, int64_t i1, uint64_t* key,
                        void* stream) {
    RLS_REQUIRE(N >= 1 && N <= kExMaxN, RLS_EINVAL, "spin_exhaustive: N = %lld outside [1, %d]", (long long)N, kExMaxN);
    RLS_REQUIRE(G >= 0 && G <= kExMaxG, RLS_EINVAL, "spin_exhaustive: G = %lld outside [0, 2^22]", (long long)G);
    RLS_REQUIRE(i0 >= 0 && i0 < i1 && i1 <= (1ll << N), RLS_EINVAL, "spin_exhaustive: range [%lld, %lld) must be non-empty and inside [0, 2^%lld]",
                (long long)i0, (long long)i1, (long long)N);
    if (G == 0) return RLS_OK;
    RLS_REQUIRE(pos && neg && key, RLS_EINVAL, "NULL pointer");
    const int n = (int)N, L = n < kExL ? n : kExL;
    hipStream_t s = as_stream(stream);
    if (n <= 32) {
        if (L >= kExU) ex_launch<uint32_t, kExU>(pos, neg, G, n, L, i0, i1, key, s);
        else ex_launch<uint32_t, 0>(pos, neg, G, n, L, i0, i1, key, s);
    } else {
        ex_launch<uint64_t, kExU>(pos, neg, G, n, L, i0, i1, key, s);
    }
    return check_launch("k_spin_exhaustive");
}

}  // extern "C"
