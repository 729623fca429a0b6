// One best-improvement pass of methods_problem_specific/TSP/opt_3.py:42-105 (local_search_3_opt) for gfx950.
//
// The reference's "3-opt" moves no block: for every triple (i, j, k) of segments_3_opt(N) -- 0 <= i < j < N,
// j < k < N + (i > 0) -- the open tour t[0..N-1] is cut into
//     H = t[0..i]   S1 = t[i+1..j]   S2 = t[j+1..ke]   C = t[ke+1..N-1],   ke = min(k, N - 1)
// (Python slices: S2 is empty for j = N - 1, C for k >= N - 1) and the seven ways of reversing S1, S2 and C in place are tried in
// the reference's order, trial 0..6 = aBC AbC ABc Abc abC aBc abc (a lower-case letter: that block reversed).  Every candidate is
// evaluated against the SAME seed tour; the pass keeps the first strict minimum below the seed's length, first in (i, j, k, trial)
// order.  Degenerate trials (a one-city block, the seed itself) are evaluated like every other.
//
//   EXACT: the reference's own comparison value -- distance_calc of the closed candidate: float64, edge after edge from position
//          0, the closing edge last.  Positions 0..i are the seed's in all seven trials, so the sum resumes from the seed's running
//          sum S[i] (the same additions in the same order) and walks the edges of positions i..N-1.  A thread walks the seven
//          trials of its triple together: inside a block a trial adds either the straight edge D[t[p-1], t[p]] or the mirrored one
//          D[t[lo+hi-p+1], t[lo+hi-p]], so a position costs two matrix reads and seven independent float64 additions; where a
//          block begins, each trial reads its own edge (the city it stands on depends on the block before).  Any matrix.
//   else:  only the junctions between consecutive NON-EMPTY blocks change, in cyclic order H|S1, S1|S2, S2|C, C|t[0] (an empty
//          block is skipped: S1|C, S2|t[0], S1|t[0]).  With x_q the new and y_q the old edge of junction q = 1..m (m = 2..4),
//              value = ((x_1 + x_2) + x_3) + x_4  -  (((y_1 + y_2) + y_3) + y_4)      float64, left to right, one subtraction,
//          compared with 0 (an identity trial gives new == old bit for bit and never wins).  SYMMETRIC matrices only.
//
// Work is dealt round-robin to the waves of the tour's `slices` workgroups (item q to wave q mod waves-in-all); no root decodes
// an index, a wave steps its item forward.  What an item is follows the cost of a candidate:
//   else (O(1) per candidate): an item is an (i, j) pair, in order, and the lanes stride over k.  Short rows leave lanes idle
//          (N - 1 - j of 64 busy), but finding a lane's triple costs nothing.
//   EXACT (O(N) per candidate): for one i the triples' (j, k), in order, are a row of m (m - 1) / 2 + (i > 0) m entries, m = N - 1
//          - i; an item is a chunk of 64 consecutive entries of a row (the last chunk of a row ragged).  The wave finds the (j, k)
//          of its chunk's first entry by walking j's parts of the row, every lane walks on by its lane number: up to N steps,
//          small beside the walk of the tour, and every lane has a triple.  All lanes share i, so they start at the same position.
//   (Measured, 2^12 tours of 100 cities, the walk one position a trip: EXACT 51.8 ms in chunks, 66.9 ms in pairs; else 5.0 ms in
//   pairs, 7.4 ms in chunks.  The walk two positions a trip -- both positions' tour entries, then both positions' matrix entries,
//   in flight together instead of two dependent LDS round trips per position -- took EXACT in chunks to 40.4 ms.)
// Each thread keeps its best (value, key), key = ((i N + j)(N + 1) + k) 8 + trial in 64 bits (past 2^31 from N = 646); lanes fold by shuffles,
// waves through LDS.  With slices > 1 every workgroup leaves (value, key) in row blockIdx.y of the [slices, B] best_value /
// best_i and k_tsp_3opt_reduce folds the rows and splits the key.  The tour, S and the reduction scratch live in LDS, and so
// does the float64 matrix while it fits beside them (rls_tsp3_plan.h: N <= 142); above that it is read through L2.
#include "rls_ring.h"
#include "rls_tsp3_plan.h"

namespace rls {

// bit r set: trial r reverses the block
constexpr uint32_t kRevS1 = 0x71;   // aBC abC aBc abc = trials 0, 4, 5, 6
constexpr uint32_t kRevS2 = 0x5A;   // AbC Abc abC abc = trials 1, 3, 4, 6
constexpr uint32_t kRevC = 0x6C;    // ABc Abc aBc abc = trials 2, 3, 5, 6

// other (o, ok) replaces (v, key) when it is a candidate and better, or equal and earlier
__device__ __forceinline__ void tsp3_merge(double& v, int64_t& key, double o, int64_t ok) {
    if (ok >= 0 && (key < 0 || o < v || (o == v && ok < key))) { v = o; key = ok; }
}

template <bool EXACT, bool LDS_D>
__global__ __launch_bounds__(LDS_D ? kTsp3WavesStaged * kWave : kTsp3WavesGlobal * kWave)
void k_tsp_3opt_best(const double* __restrict__ dist, int64_t N, const int64_t* __restrict__ perm, int64_t B,
                     const double* __restrict__ cur, int64_t* __restrict__ best_i, int64_t* __restrict__ best_j,
                     int64_t* __restrict__ best_k, int64_t* __restrict__ best_trial, double* __restrict__ best_value) {
    extern __shared__ __attribute__((aligned(16))) unsigned char smem[];
    const int n = (int)N;
    const int tid = threadIdx.x, lane = tid & 63;
    const int wpb = blockDim.x >> 6;
    const int wib = __builtin_amdgcn_readfirstlane(tid >> 6);
    double* Dl = reinterpret_cast<double*>(smem);                                           // [N, N] (staged form)
    double* S = reinterpret_cast<double*>(smem + (LDS_D ? (size_t)n * n * 8 : 0));          // [N + 1] (EXACT)
    double* rd = S + (EXACT ? n + 1 : 0);                                                   // [waves]
    int64_t* rk = reinterpret_cast<int64_t*>(rd + wpb);                                     // [waves]
    int32_t* t = reinterpret_cast<int32_t*>(rk + wpb);                                      // [N]
    const int64_t b = blockIdx.x;

    if constexpr (LDS_D) {      // LDS-DMA of the matrix as dwords, 256 B per wave instruction, every chunk in flight at once
        const int ndw = 2 * n * n;
        const float* src = reinterpret_cast<const float*>(dist);
        float* dst = reinterpret_cast<float*>(Dl);
        for (int c = wib * kWave; c < ndw; c += blockDim.x)
            if (c + lane < ndw) glds4(src + c + lane, dst + c);
    }
    for (int k = tid; k < n; k += blockDim.x) {
        const int64_t c = perm[b * N + k];
        t[k] = (uint64_t)c < (uint64_t)N ? (int32_t)c : 0;          // (rows are permutations by contract: never index outside D)
    }
    if constexpr (LDS_D) asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
    __syncthreads();
    auto D = [&](int a, int c) -> double {
        if constexpr (LDS_D) return Dl[a * n + c];
        else return dist[(int64_t)a * N + c];
    };
    if constexpr (EXACT) {                                          // edges in parallel, then the one sequential sum
        for (int k = tid; k < n; k += blockDim.x) S[k + 1] = D(t[k], t[k + 1 == n ? 0 : k + 1]);
        __syncthreads();
        if (tid == 0) {
            double acc = 0.0;
            S[0] = 0.0;
            for (int k = 0; k < n; ++k) {
                acc = acc + S[k + 1];
                S[k + 1] = acc;
            }
        }
        __syncthreads();
    }

    double best = EXACT ? cur[b] : 0.0;                             // only strictly better candidates count
    int64_t key = -1;
    const int t0 = t[0];
    const int64_t gw = (int64_t)blockIdx.y * wpb + wib, nw = (int64_t)gridDim.y * wpb;      // this wave's items: gw, gw + nw, ..
    // the seven candidates of one triple against the thread's best so far
    auto consider = [&](int i, int j, int k) {
        const int ci = t[i], s1f = t[i + 1], s1l = t[j];
        const int ke = k < n - 1 ? k : n - 1;
        const bool has2 = j + 1 <= ke, hasc = ke + 1 <= n - 1;
        double v[7];
        int pc[7];                                              // the city trial r stands on
        if constexpr (EXACT) {
            const double s0 = S[i];
#pragma unroll
            for (int r = 0; r < 7; ++r) { v[r] = s0; pc[r] = ci; }
            // a block [lo, hi]: its first edge per trial, its inner edges straight or mirrored
            auto walk = [&](auto MASK, int lo, int hi) {
                constexpr uint32_t mask = decltype(MASK)::value;
                const int first = t[lo], last = t[hi];
#pragma unroll
                for (int r = 0; r < 7; ++r) v[r] = v[r] + D(pc[r], ((mask >> r) & 1) ? last : first);
                int qs = first, qr = last;
                int p = lo + 1;
                if ((hi - lo) & 1) {                            // an odd number of inner edges: one alone, then pairs
                    const int cs = t[p], cr = t[lo + hi - p];
                    const double es = D(qs, cs), er = D(qr, cr);
#pragma unroll
                    for (int r = 0; r < 7; ++r) v[r] = v[r] + (((mask >> r) & 1) ? er : es);
                    qs = cs;
                    qr = cr;
                    ++p;
                }
                for (; p < hi; p += 2) {      // two positions a trip: four tour entries, then four matrix entries, in flight together
                    const int cs1 = t[p], cr1 = t[lo + hi - p], cs2 = t[p + 1], cr2 = t[lo + hi - p - 1];
                    const double es1 = D(qs, cs1), er1 = D(qr, cr1), es2 = D(cs1, cs2), er2 = D(cr1, cr2);
#pragma unroll
                    for (int r = 0; r < 7; ++r) v[r] = (v[r] + (((mask >> r) & 1) ? er1 : es1)) + (((mask >> r) & 1) ? er2 : es2);
                    qs = cs2;
                    qr = cr2;
                }
#pragma unroll
                for (int r = 0; r < 7; ++r) pc[r] = ((mask >> r) & 1) ? first : last;
            };
            walk(std::integral_constant<uint32_t, kRevS1>{}, i + 1, j);
            if (has2) walk(std::integral_constant<uint32_t, kRevS2>{}, j + 1, ke);
            if (hasc) walk(std::integral_constant<uint32_t, kRevC>{}, ke + 1, n - 1);
#pragma unroll
            for (int r = 0; r < 7; ++r) v[r] = v[r] + D(pc[r], t0);
        } else {
            double old = D(ci, s1f);
            int po = s1l;
#pragma unroll
            for (int r = 0; r < 7; ++r) {
                const bool rev = (kRevS1 >> r) & 1;
                v[r] = D(ci, rev ? s1l : s1f);
                pc[r] = rev ? s1f : s1l;
            }
            auto junction = [&](auto MASK, int first, int last) {
                constexpr uint32_t mask = decltype(MASK)::value;
                old = old + D(po, first);
                po = last;
#pragma unroll
                for (int r = 0; r < 7; ++r) {
                    const bool rev = (mask >> r) & 1;
                    v[r] = v[r] + D(pc[r], rev ? last : first);
                    pc[r] = rev ? first : last;
                }
            };
            if (has2) junction(std::integral_constant<uint32_t, kRevS2>{}, t[j + 1], t[ke]);
            if (hasc) junction(std::integral_constant<uint32_t, kRevC>{}, t[ke + 1], t[n - 1]);
            old = old + D(po, t0);
#pragma unroll
            for (int r = 0; r < 7; ++r) v[r] = (v[r] + D(pc[r], t0)) - old;
        }
        const int64_t base = (((int64_t)i * N + j) * (N + 1) + k) * 8;
#pragma unroll
        for (int r = 0; r < 7; ++r)
            if (v[r] < best) { best = v[r]; key = base + r; }   // (a thread's keys only grow: the first of equals stays)
    };
    if constexpr (EXACT) {
        // chunk c of row i holds the row's entries 64 c .. 64 c + 63; lane l takes entry 64 c + l
        auto row_chunks = [&](int row) -> int64_t {
            const int64_t m = n - 1 - row;
            return (m * (m - 1) / 2 + (row > 0 ? m : 0) + kWave - 1) / kWave;
        };
        int i = 0;
        int64_t c = gw;
        while (i < n - 1 && c >= row_chunks(i)) { c -= row_chunks(i); ++i; }
        while (i < n - 1) {
            const int top = n + (i > 0 ? 1 : 0);                    // k < top: j's part of the row has top - 1 - j entries
            int j = i + 1;
            int64_t rem = c * kWave;                                // the chunk's first entry (it exists: c < row_chunks(i)) ..
            while (j < n && rem >= top - 1 - j) { rem -= top - 1 - j; ++j; }
            rem += lane;                                            // .. then this lane's; j = N: past the end of the row
            while (j < n && rem >= top - 1 - j) { rem -= top - 1 - j; ++j; }
            if (j < n) consider(i, j, j + 1 + (int)rem);
            c += nw;
            while (i < n - 1 && c >= row_chunks(i)) { c -= row_chunks(i); ++i; }
        }
    } else {
        // pair q is (i, i + 1 + off) with off counted inside row i (N - 1 - i pairs)
        int i = 0;
        int64_t off = gw;
        while (i < n - 1 && off >= n - 1 - i) { off -= n - 1 - i; ++i; }
        while (i < n - 1) {
            const int j = i + 1 + (int)off;
            const int top = n + (i > 0 ? 1 : 0);
            for (int k = j + 1 + lane; k < top; k += kWave) consider(i, j, k);
            off += nw;
            while (i < n - 1 && off >= n - 1 - i) { off -= n - 1 - i; ++i; }
        }
    }
#pragma unroll
    for (int m = 32; m >= 1; m >>= 1) {
        const double o = __shfl_xor(best, m, kWave);
        const int64_t ok = __shfl_xor(key, m, kWave);
        tsp3_merge(best, key, o, ok);
    }
    if (lane == 0) { rd[wib] = best; rk[wib] = key; }
    __syncthreads();
    if (tid == 0) {
        for (int w = 1; w < wpb; ++w) tsp3_merge(best, key, rd[w], rk[w]);
        const int64_t o = (int64_t)blockIdx.y * B + b;
        best_value[o] = key >= 0 ? best : (EXACT ? cur[b] : 0.0);
        if (gridDim.y == 1) {
            const int64_t q = key >> 3, q2 = q / (N + 1);
            best_i[o] = key >= 0 ? q2 / N : -1;
            best_j[o] = key >= 0 ? q2 % N : -1;
            best_k[o] = key >= 0 ? q % (N + 1) : -1;
            best_trial[o] = key >= 0 ? (key & 7) : -1;
        } else {
            best_i[o] = key;                                        // k_tsp_3opt_reduce splits the winner's
        }
    }
}

// rows 1 .. slices - 1 of the [slices, B] (best_value, best_i = key) folded into row 0, the key split into (i, j, k, trial)
__global__ void k_tsp_3opt_reduce(int64_t N, int64_t B, int64_t slices, int64_t* __restrict__ best_i, int64_t* __restrict__ best_j,
                                  int64_t* __restrict__ best_k, int64_t* __restrict__ best_trial, double* __restrict__ best_value) {
    const int64_t b = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (b >= B) return;
    double v = best_value[b];
    int64_t key = best_i[b];
    for (int64_t s = 1; s < slices; ++s) tsp3_merge(v, key, best_value[s * B + b], best_i[s * B + b]);
    const int64_t q = key >> 3, q2 = q / (N + 1);
    best_value[b] = v;
    best_i[b] = key >= 0 ? q2 / N : -1;
    best_j[b] = key >= 0 ? q2 % N : -1;
    best_k[b] = key >= 0 ? q % (N + 1) : -1;
    best_trial[b] = key >= 0 ? (key & 7) : -1;
}

}  // namespace rls

using namespace rls;

extern "C" {

int rls_tsp_3opt_launch_form(int64_t N, int32_t exact, rls_tsp_form* out) {
    RLS_REQUIRE(out != nullptr, RLS_EINVAL, "out is NULL");
    RLS_REQUIRE(N >= 3 && N < (1 << 20), RLS_EINVAL, "bad size N=%lld", (long long)N);
    const Tsp3Form f = tsp_plan_3opt_best(N, exact != 0);
    if (f.err != RLS_OK) *out = rls_tsp_form{0, 0, 0, 0, 0, 0, 0};
    else *out = rls_tsp_form{f.lds_d ? 1 : 0, 0, f.block, f.waves, (int64_t)f.lds, RLS_TSP_KERNEL_ONLY, 1};
    return RLS_OK;
}

int rls_tsp_3opt_best(const double* dist, int64_t N, const int64_t* perm, int64_t B, const double* cur_length, int32_t slices,
                      int64_t* best_i, int64_t* best_j, int64_t* best_k, int64_t* best_trial, double* best_value, void* stream) {
    RLS_REQUIRE(N >= 3 && N < (1 << 20) && B >= 0 && B < (1ll << 31), RLS_EINVAL, "bad sizes N=%lld B=%lld", (long long)N, (long long)B);
    RLS_REQUIRE(slices >= 1 && slices <= 65535, RLS_EINVAL, "slices=%d outside [1, 65535]", slices);
    if (B == 0) return RLS_OK;
    RLS_REQUIRE(dist && perm && best_i && best_j && best_k && best_trial && best_value, RLS_EINVAL, "NULL pointer");
    const bool exact = cur_length != nullptr;
    const Tsp3Form f = tsp_plan_3opt_best(N, exact);
    RLS_REQUIRE(f.err == RLS_OK, f.err, "N=%lld needs %zu B of LDS (max %d)", (long long)N, f.lds, kLdsBytes);
    const dim3 grid((unsigned)B, (unsigned)slices), block(f.block);
    with_bool(exact, [&](auto EX) {
        with_bool(f.lds_d, [&](auto LD) {
            auto kern = k_tsp_3opt_best<decltype(EX)::value, decltype(LD)::value>;
            ensure_dyn_lds((const void*)kern, f.lds);
            hipLaunchKernelGGL(kern, grid, block, f.lds, as_stream(stream), dist, N, perm, B, cur_length, best_i, best_j, best_k, best_trial,
                               best_value);
        });
    });
    if (slices > 1)
        hipLaunchKernelGGL(k_tsp_3opt_reduce, dim3((unsigned)ceil_div(B, 256)), dim3(256), 0, as_stream(stream), N, B, (int64_t)slices, best_i,
                           best_j, best_k, best_trial, best_value);
    return check_launch("k_tsp_3opt_best");
}

}  // extern "C"
