// The tour constructors of methods_problem_specific/TSP (nn.py, ins_n.py, ins_f.py, ins_c.py) for gfx950: the neighbour chain
// that fixes the order in which cities join a tour, and grow-and-converge -- a partial tour that takes the next city of its row
// of `order` at its end and is then 2-opted until a pass brings nothing, size after size, in ONE launch.
//
// k_tsp_neighbour_chain, a wave per start: c_0 = start, c_{k+1} = the nearest (farthest) city to c_k among those not yet in the
// chain -- nn.py:62-75 / ins_f.py:84-96, whose masking of visited rows, columns and the diagonal with +-inf leaves exactly those.
// A step is one coalesced read of row c_k and a fold of (value, city) through the lanes; among equal values the lowest city wins
// (numpy's first extremum).  The visited flags are bytes in LDS.
//
// k_tsp_grow_2opt, a persistent workgroup per row.  The matrix stride N and the tour length m are separate quantities: the tour
// t[0..m-1] grows from m_seed to m_end cities, and from m = first_m on every size ends with best-improvement passes of
// opt_2.py:27-57 on the closed m-city tour.  A pass is the EXACT ranking of k_tsp_2opt_best (rls_tsp.hip), bit for bit:
//   edges D[t[k], t[k+1]] load in parallel, one thread forms the running sums S[0..m] (float64, left to right, the closing edge
//   last) and S[m] is the seed's length; the m (m - 1) / 2 reversals [i..j] are one list in (i, j) order dealt round-robin over
//   the threads; a candidate resumes from S[i - 1] (the same additions in the same order) and walks the remaining edges with
//   plain float64 adds; values are compared, never differences; (value, i m + j) folds through lanes (shuffles) and waves (LDS)
//   so that the first of equals in (i, j) order wins; the reversal is applied in LDS and the loop repeats.
// The loop ends by itself (lengths strictly decrease); max_passes bounds one convergence all the same, so that the kernel returns
// whatever it is handed.  The tour, `order`, S and the reduction slots live in LDS, and so does the float64 matrix while it fits
// beside them (rls_tsp_grow_plan.h: N <= 141); above that it is read through L2.  No grid-wide barrier, no atomics, and in the
// staged form nothing inside the loop touches global memory.
#include "rls_ring.h"
#include "rls_tsp_grow_plan.h"

namespace rls {

// other (o, ok) replaces (v, key) when it is a candidate and better, or equal and earlier
__device__ __forceinline__ void grow_merge(double& v, int64_t& key, double o, int64_t ok) {
    if (ok >= 0 && (key < 0 || o < v || (o == v && ok < key))) { v = o; key = ok; }
}

__global__ __launch_bounds__(kWave) void k_tsp_neighbour_chain(const double* __restrict__ dist, int64_t N, const int64_t* __restrict__ start,
                                                                int32_t farthest, int64_t* __restrict__ chain, int32_t* __restrict__ status) {
    extern __shared__ __attribute__((aligned(16))) unsigned char smem[];
    unsigned char* visited = smem;                                          // [N]
    const int64_t s = blockIdx.x;
    const int lane = threadIdx.x;
    int64_t cur = start[s];
    if ((uint64_t)cur >= (uint64_t)N) {                                     // the row stays as it was
        if (lane == 0) status[s] = 2;
        return;
    }
    for (int64_t c = lane; c < N; c += kWave) visited[c] = 0;
    __syncthreads();
    for (int64_t step = 0; step < N; ++step) {
        if (lane == 0) {
            chain[s * N + step] = cur;
            visited[cur] = 1;
        }
        __syncthreads();
        if (step == N - 1) break;
        const double* row = dist + cur * N;
        double bv = 0.0;
        int64_t bc = -1;
        for (int64_t c = lane; c < N; c += kWave) {                         // a lane's cities only grow: the first of equals stays
            if (visited[c]) continue;
            const double v = row[c];
            if (bc < 0 || (farthest ? v > bv : v < bv)) { bv = v; bc = c; }
        }
#pragma unroll
        for (int m = 32; m >= 1; m >>= 1) {
            const double o = __shfl_xor(bv, m, kWave);
            const int64_t oc = __shfl_xor(bc, m, kWave);
            if (oc >= 0 && (bc < 0 || (farthest ? o > bv : o < bv) || (o == bv && oc < bc))) { bv = o; bc = oc; }
        }
        cur = __shfl(bc, 0, kWave);
        if ((uint64_t)cur >= (uint64_t)N) break;                            // (cannot happen: a city is left until step N - 1)
    }
    if (lane == 0) status[s] = 0;
}

template <bool LDS_D>
__global__ __launch_bounds__(kTspGrowWaves * kWave)
void k_tsp_grow_2opt(const double* __restrict__ dist, int64_t N, const int64_t* __restrict__ order, int32_t m_seed, int32_t m_end,
                     int32_t first_m, int64_t max_passes, int64_t* __restrict__ tours, double* __restrict__ length,
                     int64_t* __restrict__ passes, int32_t* __restrict__ status) {
    extern __shared__ __attribute__((aligned(16))) unsigned char smem[];
    const int n = (int)N;
    const int tid = threadIdx.x, lane = tid & 63, nthr = blockDim.x;
    const int wpb = nthr >> 6;
    const int wib = __builtin_amdgcn_readfirstlane(tid >> 6);
    double* Dl = reinterpret_cast<double*>(smem);                                           // [N, N] (staged form)
    double* S = reinterpret_cast<double*>(smem + (LDS_D ? (size_t)n * n * 8 : 0));          // [N + 1]
    double* rd = S + n + 1;                                                                 // [waves]
    int64_t* rk = reinterpret_cast<int64_t*>(rd + wpb);                                     // [waves]
    int32_t* t = reinterpret_cast<int32_t*>(rk + wpb);                                      // [N]
    int32_t* ord = t + n;                                                                   // [N]
    const int64_t s = blockIdx.x;

    if (tid == 0) rk[0] = 0;                                        // "an entry of the row is no city" (a slot of the reduction, not yet in use)
    __syncthreads();
    for (int k = tid; k < n; k += nthr) {
        const int64_t c = order[s * N + k];
        const bool in = (uint64_t)c < (uint64_t)N;
        if (!in) rk[0] = 1;
        ord[k] = in ? (int32_t)c : 0;
    }
    __syncthreads();
    if (rk[0] != 0) {                                               // nothing of this row is written but its status
        if (tid == 0) status[s] = 2;
        return;
    }
    if constexpr (LDS_D) {      // LDS-DMA of the matrix as dwords, 256 B per wave instruction, every chunk in flight at once
        const int ndw = 2 * n * n;
        const float* src = reinterpret_cast<const float*>(dist);
        float* dst = reinterpret_cast<float*>(Dl);
        for (int c = wib * kWave; c < ndw; c += nthr)
            if (c + lane < ndw) glds4(src + c + lane, dst + c);
        asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
    }
    for (int k = tid; k < m_seed; k += nthr) t[k] = ord[k];
    __syncthreads();
    auto D = [&](int a, int c) -> double {
        if constexpr (LDS_D) return Dl[a * n + c];
        else return dist[(int64_t)a * N + c];
    };
    // the edges of the closed m-city tour in parallel, then the one sequential sum: S[k] = the length of the first k edges
    auto running_sums = [&](int m) {
        for (int k = tid; k < m; k += nthr) S[k + 1] = D(t[k], t[k + 1 == m ? 0 : k + 1]);
        __syncthreads();
        if (tid == 0) {
            double acc = 0.0;
            S[0] = 0.0;
            for (int k = 0; k < m; ++k) {
                acc = acc + S[k + 1];
                S[k + 1] = acc;
            }
        }
        __syncthreads();
    };

    int64_t np = 0;
    int32_t st = 0;
    int m = m_seed;
    for (;; ++m) {
        if (m > m_seed) {
            if (tid == 0) t[m - 1] = ord[m - 1];
            __syncthreads();
        }
        if (m >= first_m) {
            const int64_t M = (int64_t)m * (m - 1) / 2;
            const double tm1 = (double)(2 * m - 1);
            for (int64_t conv = 0;;) {
                running_sums(m);
                double best = S[m];                                 // only strictly shorter candidates count
                int64_t key = -1;                                   // i * m + j of the best so far
                for (int64_t c = tid; c < M; c += nthr) {
                    // row i holds candidates off(i) .. off(i + 1) - 1, off(i) = i (2m - i - 1) / 2
                    int64_t i = (int64_t)((tm1 - sqrt(tm1 * tm1 - 8.0 * (double)c)) * 0.5);
                    if (i < 0) i = 0;
                    if (i > m - 2) i = m - 2;
                    while (i * (2 * (int64_t)m - i - 1) / 2 > c) --i;
                    while ((i + 1) * (2 * (int64_t)m - i - 2) / 2 <= c) ++i;
                    const int ii = (int)i, jj = (int)(i + 1 + (c - i * (2 * (int64_t)m - i - 1) / 2));
                    auto city = [&](int k) -> int {                 // the candidate tour, closed
                        if (k == m) k = 0;
                        return (k >= ii && k <= jj) ? t[ii + jj - k] : t[k];
                    };
                    const int k0 = ii >= 1 ? ii - 1 : 0;
                    double v = S[k0];
                    int c0 = city(k0);
#pragma unroll 4
                    for (int k = k0; k < m; ++k) {
                        const int c1 = city(k + 1);
                        v = v + D(c0, c1);
                        c0 = c1;
                    }
                    if (v < best) { best = v; key = i * m + jj; }   // (a thread's keys only grow: the first of equals stays)
                }
#pragma unroll
                for (int sh = 32; sh >= 1; sh >>= 1) {
                    const double o = __shfl_xor(best, sh, kWave);
                    const int64_t ok = __shfl_xor(key, sh, kWave);
                    grow_merge(best, key, o, ok);
                }
                if (lane == 0) { rd[wib] = best; rk[wib] = key; }
                __syncthreads();
                best = rd[0];                                       // every thread folds the waves' slots: the same winner everywhere
                key = rk[0];
                for (int w = 1; w < wpb; ++w) grow_merge(best, key, rd[w], rk[w]);
                ++np;
                if (key < 0) break;                                 // the fruitless pass that ends a convergence
                const int wi = (int)(key / m), wj = (int)(key % m);
                for (int k = tid; k < (wj - wi + 1) / 2; k += nthr) {
                    const int a = t[wi + k], b = t[wj - k];
                    t[wi + k] = b;
                    t[wj - k] = a;
                }
                __syncthreads();
                if (++conv == max_passes) { st = 1; break; }        // the guard: the state after max_passes passes is left
            }
        }
        if (st != 0 || m == m_end) break;
    }
    running_sums(m);
    for (int k = tid; k < n; k += nthr) tours[s * N + k] = k < m ? t[k] : ord[k];
    if (tid == 0) {
        length[s] = S[m];
        passes[s] = np;
        status[s] = st;
    }
}

}  // namespace rls

using namespace rls;

extern "C" {

int rls_tsp_grow_launch_form(int64_t N, rls_tsp_form* out) {
    RLS_REQUIRE(out != nullptr, RLS_EINVAL, "out is NULL");
    RLS_REQUIRE(N >= 2 && N < (1 << 20), RLS_EINVAL, "bad size N=%lld", (long long)N);
    const TspGrowForm f = tsp_plan_grow(N);
    if (f.err != RLS_OK) *out = rls_tsp_form{0, 0, 0, 0, 0, 0, 0};
    else *out = rls_tsp_form{f.lds_d ? 1 : 0, 0, f.block, f.waves, (int64_t)f.lds, RLS_TSP_KERNEL_ONLY, 1};
    return RLS_OK;
}

int rls_tsp_neighbour_chain(const double* dist, int64_t N, const int64_t* start, int64_t S, int32_t farthest, int64_t* chain,
                            int32_t* status, void* stream) {
    RLS_REQUIRE(N >= 2 && N < (1 << 20) && S >= 0 && S < (1ll << 31), RLS_EINVAL, "bad sizes N=%lld S=%lld", (long long)N, (long long)S);
    RLS_REQUIRE(farthest == 0 || farthest == 1, RLS_EINVAL, "farthest=%d must be 0 or 1", farthest);
    if (S == 0) return RLS_OK;
    RLS_REQUIRE(dist && start && chain && status, RLS_EINVAL, "NULL pointer");
    const size_t lds = ((size_t)N + 15) / 16 * 16;
    RLS_REQUIRE(lds <= (size_t)kLdsBytes, RLS_EUNSUPPORTED, "N=%lld needs %zu B of LDS (max %d)", (long long)N, lds, kLdsBytes);
    ensure_dyn_lds((const void*)k_tsp_neighbour_chain, lds);
    hipLaunchKernelGGL(k_tsp_neighbour_chain, dim3((unsigned)S), dim3(kWave), lds, as_stream(stream), dist, N, start, farthest, chain, status);
    return check_launch("k_tsp_neighbour_chain");
}

int rls_tsp_grow_2opt(const double* dist, int64_t N, const int64_t* order, int64_t S, int64_t m_seed, int64_t m_end, int64_t first_m,
                      int64_t max_passes, int64_t* tours, double* length, int64_t* passes, int32_t* status, void* stream) {
    RLS_REQUIRE(N >= 2 && N < (1 << 20) && S >= 0 && S < (1ll << 31), RLS_EINVAL, "bad sizes N=%lld S=%lld", (long long)N, (long long)S);
    RLS_REQUIRE(2 <= m_seed && m_seed <= m_end && m_end <= N, RLS_EINVAL, "need 2 <= m_seed=%lld <= m_end=%lld <= N=%lld", (long long)m_seed,
                (long long)m_end, (long long)N);
    RLS_REQUIRE(max_passes >= 1, RLS_EINVAL, "max_passes=%lld must be >= 1", (long long)max_passes);
    if (S == 0) return RLS_OK;
    RLS_REQUIRE(dist && order && tours && length && passes && status, RLS_EINVAL, "NULL pointer");
    const TspGrowForm f = tsp_plan_grow(N);
    RLS_REQUIRE(f.err == RLS_OK, f.err, "N=%lld needs %zu B of LDS (max %d)", (long long)N, f.lds, kLdsBytes);
    const int64_t cap = (int64_t)1 << 30;
    const int32_t fm = (int32_t)(first_m < 0 ? 0 : first_m > cap ? cap : first_m);          // (beyond m_end: no pass at all)
    with_bool(f.lds_d, [&](auto LD) {
        auto kern = k_tsp_grow_2opt<decltype(LD)::value>;
        ensure_dyn_lds((const void*)kern, f.lds);
        hipLaunchKernelGGL(kern, dim3((unsigned)S), dim3(f.block), f.lds, as_stream(stream), dist, N, order, (int32_t)m_seed, (int32_t)m_end, fm,
                           max_passes, tours, length, passes, status);
    });
    return check_launch("k_tsp_grow_2opt");
}

}  // extern "C"
