// ISCO sampler steps as single kernels (VERDICT r1 "missing" #7):
//   rls_isco_maxcut_step : ISCO_maxcut.step   rlsolver/envs/env_ISCO.py:26-49
//                          (get_local_dist :51-63, proposal :37-49, ll_y2x :65-77)
//   rls_isco_mis_step    : ISCO_MIS.step      rlsolver/envs/env_ISCO.py:111-174: the MaxCut step's kernels with the energy
//                          model (:162-170) as a template parameter
//   rls_pisco_step       : PISCO_maxcut.step  rlsolver/envs/env_ISCO.py:384-434: the same two bodies on f16 samples, the local
//                          distribution read from a row of the dense product
//   rls_isco_tsp_step    : ISCO_TSP.step      rlsolver/envs/env_ISCO.py:188-236 (opt_2 :238-335, switch :337-344)
// with the sampler helpers of rlsolver/methods/util.py:498-570 (gumbel, log1mexp,
// noreplacement_sampling_renormalize, multinomial, bernoulli_logp, mh_step) folded in.  The reference runs each
// step as ~25-40 torch ops on [B, N] tensors (log_softmax, two sorts, argsort, gathers, cumsum, scatter, where);
// here one wave owns one env and keeps its row in LDS from the first read to the accepted sample.
//
// What "Gumbel top-k without replacement" needs per env is only: which L entries have the largest perturbed
// log-probability, in which order, and the running sum of their probabilities in that order -- so the two full
// sorts of the reference become one radix select (32 ballot rounds) + a bitonic sort of the L selected entries.
//
// Floating point: f32 like the reference, libm-accurate expf / logf / log1pf / expm1f; sums over a row are wave
// tree reductions / scans, not torch's order: results agree with the reference to ~1e-6 relative (tests: 1e-5,
// the tolerance north_star states for floating-point results).
#include "rls_tile.h"
#include "rls_draw.h"
#include "rls_tsp_plan.h"
#include "rls_isco_plan.h"
#include <cmath>
#include <cstdlib>

namespace rls {

__device__ __forceinline__ float wave_max_f(float v) {
#pragma unroll
    for (int m = 32; m >= 1; m >>= 1) v = fmaxf(v, __shfl_xor(v, m, 64));
    return v;
}
__device__ __forceinline__ float wave_sum_f32x(float v) {
#pragma unroll
    for (int m = 32; m >= 1; m >>= 1) v += __shfl_xor(v, m, 64);
    return v;
}
__device__ __forceinline__ void lds_fence() {
    asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory");
    __builtin_amdgcn_wave_barrier();
}

// monotone map float -> uint32 (larger float <=> larger key)
__device__ __forceinline__ uint32_t fkey(float f) {
    const uint32_t u = __float_as_uint(f);
    return (u & 0x80000000u) ? ~u : (u | 0x80000000u);
}

// log(1 - exp(-|x|))   methods/util.py:502-505
__device__ __forceinline__ float log1mexp(float x) {
    x = -fabsf(x);
    return x > -0.693f ? logf(-expm1f(x)) : log1pf(-expf(x));
}

// sum over k of  min(ll_k - log1mexp(log(cum_k - p_k) + base), 0)   with p_k = exp(ll_k - base), cum = inclusive
// running sum of p in list order  (noreplacement_sampling_renormalize, methods/util.py:507-512, restricted to
// the entries that are summed afterwards).  ll(k) gives the k-th log-probability of the ordered list.
template <typename F>
__device__ __forceinline__ float noreplacement_ll_sum(int count, float base, int lane, F ll) {
    float carry = 0.0f, total = 0.0f;
    for (int k0 = 0; k0 < count; k0 += kWave) {
        const int k = k0 + lane;
        const bool in = k < count;
        const float l = in ? ll(k) : 0.0f;
        const float p = in ? expf(l - base) : 0.0f;
        float inc = p;                                   // inclusive scan across the wave
#pragma unroll
        for (int d = 1; d < kWave; d <<= 1) {
            const float o = __shfl_up(inc, d, 64);
            if (lane >= d) inc += o;
        }
        const float cum = carry + inc;
        const float ll_delta = logf(cum - p) + base;     // log(0) = -inf for the first entry -> log1mexp = 0
        const float out = fminf(l - log1mexp(ll_delta), 0.0f);
        total += in ? out : 0.0f;
        carry += __shfl(inc, kWave - 1, 64);
    }
    return wave_sum_f32x(total);
}

// ----------------------------------------------------------------------------------------------- the stages of a step
// A step on a graph or on a dense matrix is one pipeline: binarise the row | local distribution into lp[] | Gumbel perturbation
// into pert[] | the key of the L-th largest perturbed value | the selected set compacted into the LDS list | the list sorted (or,
// larger than the list, ordered by extraction) | ll_x2y, the flip, the backward distribution | ll_y2x | Metropolis-Hastings.
// Each stage is written once (the select and the compaction once per team shape: a wave, or a workgroup with its IscoWgScratch).

__device__ __forceinline__ float isco_block_max(float v, IscoWgScratch* sc, int lane, int w) {
    v = wave_max_f(v);
    __syncthreads();
    if (lane == 0) sc->f[w] = v;
    __syncthreads();
    float m = sc->f[0];
#pragma unroll
    for (int k = 1; k < kIscoWgWaves; ++k) m = fmaxf(m, sc->f[k]);
    return m;
}
__device__ __forceinline__ float isco_block_sum(float v, IscoWgScratch* sc, int lane, int w) {
    v = wave_sum_f32x(v);
    __syncthreads();
    if (lane == 0) sc->f[w] = v;
    __syncthreads();
    float m = 0.0f;
#pragma unroll
    for (int k = 0; k < kIscoWgWaves; ++k) m += sc->f[k];
    return m;
}
__device__ __forceinline__ int isco_block_sum_i(int v, IscoWgScratch* sc, int lane, int w) {
    v = wave_sum_i32(v);
    __syncthreads();
    if (lane == 0) sc->i[w] = v;
    __syncthreads();
    int m = 0;
#pragma unroll
    for (int k = 0; k < kIscoWgWaves; ++k) m += sc->i[k];
    return m;
}

// Threshold = the key of the `want`-th largest perturbed value (util.py:518-523): radix select on the monotone key.
// One wave: 32 one-bit passes.
__device__ __forceinline__ uint32_t isco_threshold_wave(const float* pert, int64_t N, int want, int lane) {
    uint32_t prefix = 0;
    if (N <= 32 * kWave) {
        // the lane's <= 32 keys in registers for the 32 bit passes (re-reading them from LDS put an LDS round trip on
        // every element of every pass); key 0 (out of range) has no bit set and is never counted
        uint32_t kk[32];
#pragma unroll
        for (int j = 0; j < 32; ++j) {
            const int64_t i = lane + (int64_t)j * kWave;
            kk[j] = i < N ? fkey(pert[i]) : 0u;
        }
        for (int bit = 31; bit >= 0; --bit) {
            const uint32_t hi_mask = bit == 31 ? 0u : (0xFFFFFFFFu << (bit + 1));
            int cnt = 0;
#pragma unroll
            for (int j = 0; j < 32; ++j) cnt += ((kk[j] & hi_mask) == prefix) && ((kk[j] >> bit) & 1u);
            cnt = wave_sum_i32(cnt);
            if (cnt >= want) prefix |= 1u << bit;              // the L-th largest has this bit set
            else want -= cnt;
        }
    } else {
        for (int bit = 31; bit >= 0; --bit) {
            const uint32_t hi_mask = bit == 31 ? 0u : (0xFFFFFFFFu << (bit + 1));
            int cnt = 0;
            for (int64_t i = lane; i < N; i += kWave) {
                const uint32_t k = fkey(pert[i]);
                cnt += ((k & hi_mask) == prefix) && ((k >> bit) & 1u);
            }
            cnt = wave_sum_i32(cnt);
            if (cnt >= want) prefix |= 1u << bit;              // the L-th largest has this bit set
            else want -= cnt;
        }
    }
    return prefix;
}

// ... a workgroup: four 8-bit histogram passes (LDS atomics); wave 0 reads each histogram
__device__ __forceinline__ uint32_t isco_threshold_wg(const float* pert, int64_t N, int want, IscoWgScratch* sc, int lane, int w, int tid) {
    constexpr int NT = kIscoWgWaves * kWave;
    uint32_t prefix = 0;
    for (int shift = 24; shift >= 0; shift -= 8) {
        const uint32_t hi_mask = shift == 24 ? 0u : (0xFFFFFFFFu << (shift + 8));
        for (int k = tid; k < 256; k += NT) sc->hist[k] = 0;
        __syncthreads();
        for (int64_t i = tid; i < N; i += NT) {
            const uint32_t k = fkey(pert[i]);
            if ((k & hi_mask) == prefix) atomicAdd(&sc->hist[(k >> shift) & 255u], 1);
        }
        __syncthreads();
        if (w == 0) {   // the largest byte value v whose suffix count (entries with byte >= v) reaches `want`
            int c[4], tot = 0;
#pragma unroll
            for (int q = 0; q < 4; ++q) { c[q] = sc->hist[lane * 4 + q]; tot += c[q]; }
            int suf = tot;                                        // inclusive suffix sum over lanes: lanes >= this one
#pragma unroll
            for (int d = 1; d < kWave; d <<= 1) {
                const int o = __shfl_down(suf, d, 64);
                if (lane + d < kWave) suf += o;
            }
            const int above = suf - tot;                          // entries in bins of higher lanes
            // inside this lane's four bins, from the top
            int byte_found = -1, want_left = 0, run = above;
#pragma unroll
            for (int q = 3; q >= 0; --q) {
                if (byte_found < 0 && run < want && run + c[q] >= want) { byte_found = lane * 4 + q; want_left = want - run; }
                run += c[q];
            }
            if (byte_found >= 0) { sc->prefix = prefix | ((uint32_t)byte_found << shift); sc->want = want_left; }
        }
        __syncthreads();
        prefix = sc->prefix;
        want = sc->want;
    }
    return prefix;
}

// The selected set (perturbed >= threshold) compacted into the list, as much of it as the list holds; returns its size.
// One wave: ballot / popcount, in node order.
__device__ __forceinline__ int isco_compact_wave(const float* pert, int64_t N, uint32_t prefix, float* skey, int32_t* sidx, int P,
                                                 int lane) {
    int count = 0;
    for (int64_t i0 = 0; i0 < N; i0 += kWave) {
        const int64_t i = i0 + lane;
        const bool sel = i < N && fkey(pert[i]) >= prefix;
        const uint64_t m = ballot64(sel);
        if (sel) {
            const int at = count + __popcll(m & ((1ull << lane) - 1ull));
            if (at < P) {
                skey[at] = pert[i];
                sidx[at] = (int)i;
            }
        }
        count += __popcll(m);
    }
    return count;
}

// ... a workgroup: a counter in LDS, any order (sorted next, equal keys by node id)
__device__ __forceinline__ int isco_compact_wg(const float* pert, int64_t N, uint32_t prefix, float* skey, int32_t* sidx, int P,
                                               IscoWgScratch* sc, int tid) {
    constexpr int NT = kIscoWgWaves * kWave;
    if (tid == 0) sc->count = 0;
    __syncthreads();
    for (int64_t i = tid; i < N; i += NT) {
        if (fkey(pert[i]) >= prefix) {
            const int at = atomicAdd(&sc->count, 1);
            if (at < P) {
                skey[at] = pert[i];
                sidx[at] = (int)i;
            }
        }
    }
    __syncthreads();
    return sc->count;
}

// The list sorted by perturbed value, descending, by ONE wave: padded to a power of two, bitonic.
// TIE: equal keys order by node id (lowest first, as the extraction), so that the result does not depend on the compaction order.
// A pad carries the key -inf and kIscoPadIdx, an index that orders after every node: a real entry's key is -inf too when its
// draw is u = 0 (isco_unit returns it once in 2^24 draws), and a pad in front of it would hand index arithmetic a node that
// does not exist.  Among keys of -inf the lower index goes first in both variants, so every pad ends up behind all `count`
// real entries; finite keys never compare equal to a pad's and order exactly as they did.
constexpr int32_t kIscoPadIdx = 0x7FFFFFFF;
template <bool TIE>
__device__ __forceinline__ void isco_sort_list(float* skey, int32_t* sidx, int count, int lane) {
    int P2 = 1;
    while (P2 < count) P2 <<= 1;
    for (int k = count + lane; k < P2; k += kWave) { skey[k] = -INFINITY; sidx[k] = kIscoPadIdx; }
    lds_fence();
    for (int size = 2; size <= P2; size <<= 1) {
        for (int stride = size >> 1; stride >= 1; stride >>= 1) {
            for (int t = lane; t < (P2 >> 1); t += kWave) {
                const int lo = ((t / stride) * (stride << 1)) + (t % stride);
                const int hi = lo + stride;
                const bool desc = ((lo & size) == 0);
                const float k0 = skey[lo], k1 = skey[hi];
                if constexpr (TIE) {
                    const int i0 = sidx[lo], i1 = sidx[hi];
                    const bool lt = (k0 < k1) || (k0 == k1 && i0 > i1);
                    if (lt == desc) {
                        skey[lo] = k1; skey[hi] = k0;
                        sidx[lo] = i1; sidx[hi] = i0;
                    }
                } else {
                    const bool lt = (k0 < k1) || (k1 == -INFINITY && k0 == k1 && sidx[lo] > sidx[hi]);
                    if (lt == desc) {
                        skey[lo] = k1; skey[hi] = k0;
                        const int t0 = sidx[lo]; sidx[lo] = sidx[hi]; sidx[hi] = t0;
                    }
                }
            }
            lds_fence();
        }
    }
}

// Order of a selection that does not fit the LDS list (count > capacity: path lengths in the thousands on a graph whose
// rows nearly fill LDS -- the reference draws Poisson(~10) path lengths, main_ISCO_maxcut.py:22-30): repeated extraction of
// the maximum, O(count N / 64) per sample, ONE wave.  The node ids leave in order into `ord` -- global scratch: for the graph
// models the sample's own f32 row of y_out reinterpreted (written last by the step), for the dense step (f16 rows: too short) a
// row of the caller's scratch -- `taken` is N bytes of LDS that are free at this point (yb).
// Equal keys: lowest node first.
__device__ __noinline__ void isco_order_by_extraction(const float* pert, uint8_t* taken, int64_t N, uint32_t prefix, int count,
                                                      int32_t* ord, int lane) {
    for (int64_t i = lane; i < N; i += kWave) taken[i] = 0;
    lds_fence();
    for (int k = 0; k < count; ++k) {
        uint32_t bk = 0;
        int bi = 0x7FFFFFFF;
        for (int64_t i = lane; i < N; i += kWave) {
            const uint32_t key = fkey(pert[i]);
            if (key >= prefix && !taken[i] && key > bk) { bk = key; bi = (int)i; }
        }
#pragma unroll
        for (int m = 32; m >= 1; m >>= 1) {
            const uint32_t ok = (uint32_t)__shfl_xor((int)bk, m, 64);
            const int oi = __shfl_xor(bi, m, 64);
            if (ok > bk || (ok == bk && oi < bi)) { bk = ok; bi = oi; }
        }
        if (lane == 0) { ord[k] = bi; taken[bi] = 1; }
        lds_fence();
    }
    __threadfence();      // the list is read back by every lane (and, in the workgroup kernel, by every wave after a barrier)
}

// ll_y2x: the log-probability of undoing the selection in reverse order under the backward distribution lp (env_ISCO.py:65-77);
// its ll_base is the maximum over the selected entries.  ONE wave.
template <typename S>
__device__ __forceinline__ float isco_reverse_ll(const float* lp, int count, S sel_at, int lane) {
    float bmax = -INFINITY;
    for (int k = lane; k < count; k += kWave) bmax = fmaxf(bmax, lp[sel_at(k)]);
    bmax = wave_max_f(bmax);
    return noreplacement_ll_sum(count, bmax, lane, [&](int k) { return lp[sel_at(count - 1 - k)]; });
}

// Metropolis-Hastings accept (env_ISCO.py:31-33, util.py:556-570) from the four terms and the clamped log-acceptance; lane 0
// publishes the energy, the acceptance probability and the five terms.  ONE wave; every lane returns the decision.
template <class A>
__device__ __forceinline__ bool isco_mh_accept(const A& a, int64_t b, float ll_x, float ll_x2y, float ll_y, float ll_y2x, float log_acc,
                                               int lane) {
    const float ua = a.u_accept ? a.u_accept[b] : isco_unit(isco_draw(a.seed, (uint64_t)(b + a.env_offset), 0xFFFFFFFFu, 0, 2));
    const bool accept = logf(ua + 1e-24f) < log_acc;
    if (lane == 0) {
        if (a.energy_out) a.energy_out[b] = ll_y * a.temperature;   // the reference returns ll_y * temperature of the PROPOSAL
        if (a.acc_out) a.acc_out[b] = expf(log_acc);
        if (a.terms_out) {
            float* t = a.terms_out + b * 5;
            t[0] = ll_x; t[1] = ll_x2y; t[2] = ll_y; t[3] = ll_y2x; t[4] = log_acc;
        }
    }
    return accept;
}

// ----------------------------------------------------------------------------------------------- MaxCut / MIS on a graph
// LDS per wave: xb[N] yb[N] bytes (padded to 8) | lp[N] f32 | pert[N] f32 | sel_key[P] f32 | sel_idx[P] i32,
// P = the list's capacity: the next power of two >= N while that fits LDS, else the largest power of two that does
// (N = 10^4, G70: 4096 entries).  A selection larger than P takes isco_order_by_extraction.
struct IscoMcArgs {
    const int32_t* rowptr; const int32_t* col;
    const int32_t* ell_ptr; const int32_t* ell;          // lane-per-node slabs of the symmetric CSR (rls_graph_ell) or NULL
    const float* x; float* y_out; int64_t B, N;
    const int64_t* path_length; float temperature;
    const float* u_gumbel; const float* u_accept; uint64_t seed; int64_t env_offset;
    float* energy_out; float* acc_out; float* terms_out; uint8_t* mask_out;
    int P;
    float lam;                                           // MIS: penalty weight of an edge inside the set (unread by MaxCut)
    float* rows;                                         // caller's scratch f32 [B, 2, N] (lp, pert) for rows past the LDS, else NULL
};

// The energy model of a step is the per-node epilogue after the neighbour loop, which counts d_i = the row entries of node i
// whose endpoint differs from s_i (deg_i = all row entries; a loop is listed twice in its row and never differs):
//   Acc        what a lane accumulates over its nodes
//   add        node i's contribution (the model reads s[i] itself if it needs it: MaxCut's code is then the code it was
//              before the model became a parameter, instruction for instruction)
//   score      (1 - 2 s_i) dE/ds_i / 2, the logit of flipping node i
//   ll         the energy / T from the accumulators, each summed over the sample by `sum` (the wave's or the workgroup's)
struct IscoMaxcut {       // energy = cut(s)  (env_ISCO.py:79-86): every cut edge differs at both of its ends
    using Acc = int;                                      // differing row entries
    __device__ static __forceinline__ Acc add(Acc a, const uint8_t*, int64_t, int, int d) { return a + d; }
    __device__ static __forceinline__ float score(const uint8_t*, int64_t, int deg, int d, float temperature, float) {
        return (float)(deg - 2 * d) / (2.0f * temperature);
    }
    template <class R>
    __device__ static __forceinline__ float ll(Acc a, float temperature, float, R sum) { return (float)(sum(a) >> 1) / temperature; }
};
struct IscoMis {          // energy = sum s_i - lam * #(edge entries with both ends set)  (env_ISCO.py:162-170)
    // set neighbours of i from d_i, NOT from a sum over s[nb]: the padding of a slab row holds the node itself, which never
    // differs from s_i but would count once per padding entry of a set node
    struct Acc { int ones = 0, pairs2 = 0; };
    __device__ static __forceinline__ int cnt(uint8_t si, int deg, int d) { return si ? deg - d : d; }
    __device__ static __forceinline__ Acc add(Acc a, const uint8_t* s, int64_t i, int deg, int d) {
        const uint8_t si = s[i];
        a.ones += si;
        a.pairs2 += si ? deg - d : 0;                     // every entry inside the set is seen from both of its ends
        return a;
    }
    __device__ static __forceinline__ float score(const uint8_t* s, int64_t i, int deg, int d, float temperature, float lam) {
        const uint8_t si = s[i];
        const float g = 1.0f - lam * (float)cnt(si, deg, d);
        return (si ? -g : g) / (2.0f * temperature);
    }
    template <class R>
    __device__ static __forceinline__ float ll(Acc a, float temperature, float lam, R sum) {
        const int ones = sum(a.ones), pairs2 = sum(a.pairs2);
        return ((float)ones - lam * (float)(pairs2 >> 1)) / temperature;
    }
};

// log-probabilities of the single-flip proposal distribution of state `s`: lp_i = log_softmax(gain_i / (2T)),
// gain_i = #same - #differing neighbours (the closed form of the reference's autograd, env_ISCO.py:51-63).
// Returns energy(s) / T (MaxCut: every edge counted from both ends -> / 2).  Other models (M): their score and energy.
template <class M>
__device__ __forceinline__ float isco_local_dist(const uint8_t* s, float* lp, int64_t N, const int32_t* __restrict__ rowptr,
                                                 const int32_t* __restrict__ col, const int32_t* __restrict__ ell_ptr,
                                                 const int32_t* __restrict__ ell, float temperature, float lam, int lane) {
    typename M::Acc acc{};
    float mx = -INFINITY;
    if (ell_ptr) {
        // neighbour ids from the lane-per-node slabs: round k of the 64 nodes of a group is one coalesced load that does
        // not depend on anything, eight rounds in flight -- walking col[rowptr[i] ..] per lane was a chain of ~deg L2 round
        // trips per node (155 of the step's 207 us for one sample on a G22-sized graph)
        const int64_t G = (N + 63) >> 6;
        int ep0 = 0, ep1 = 0;                                                // slab offsets of 64 groups at a time, one per lane
        for (int64_t g = 0; g < G; ++g) {
            if ((g & 63) == 0) {
                ep0 = ell_ptr[g + lane <= G ? g + lane : G];
                ep1 = ell_ptr[g + lane + 1 <= G ? g + lane + 1 : G];
            }
            const int64_t i = (g << 6) + lane;
            const bool in = i < N;
            const uint8_t si = in ? s[i] : 0;
            const int e0 = __builtin_amdgcn_readlane(ep0, (int)(g & 63)), e1 = __builtin_amdgcn_readlane(ep1, (int)(g & 63));
            const int deg = in ? rowptr[i + 1] - rowptr[i] : 0;             // requested before the rounds, used after them
            int d = 0;
            const int self = (int)(in ? i : 0);
            int nbn[8];                                                      // the next eight rounds, in flight while these are summed
#pragma unroll
            for (int q = 0; q < 8; ++q) nbn[q] = (e0 + q * kWave < e1) ? ell[e0 + q * kWave + lane] : self;
            for (int k = e0; k < e1; k += 8 * kWave) {
                int nb[8];
#pragma unroll
                for (int q = 0; q < 8; ++q) nb[q] = nbn[q];
                const int kn = k + 8 * kWave;
                if (kn < e1) {
#pragma unroll
                    for (int q = 0; q < 8; ++q) nbn[q] = (kn + q * kWave < e1) ? ell[kn + q * kWave + lane] : self;
                }
#pragma unroll
                for (int q = 0; q < 8; ++q) d += (s[nb[q]] != si);          // past a row's end the slab holds the node itself
            }
            if (in) {
                acc = M::add(acc, s, i, deg, d);
                const float sc = M::score(s, i, deg, d, temperature, lam);
                lp[i] = sc;
                mx = fmaxf(mx, sc);
            }
        }
    } else {
        for (int64_t i = lane; i < N; i += kWave) {
            const int r0 = rowptr[i], r1 = rowptr[i + 1];
            const uint8_t si = s[i];
            int d = 0;
            for (int j = r0; j < r1; ++j) d += (s[col[j]] != si);
            acc = M::add(acc, s, i, r1 - r0, d);
            const float sc = M::score(s, i, r1 - r0, d, temperature, lam);
            lp[i] = sc;
            mx = fmaxf(mx, sc);
        }
    }
    mx = wave_max_f(mx);
    float se = 0.0f;
    for (int64_t i = lane; i < N; i += kWave) se += expf(lp[i] - mx);
    const float lse = logf(wave_sum_f32x(se));
    for (int64_t i = lane; i < N; i += kWave) lp[i] = (lp[i] - mx) - lse;
    lds_fence();
    return M::ll(acc, temperature, lam, [](int v) { return wave_sum_i32(v); });
}

// isco_local_dist over the whole workgroup: wave w takes the 64-node groups w, w + W, ...
template <class M>
__device__ __forceinline__ float isco_local_dist_wg(const uint8_t* s, float* lp, int64_t N, const IscoMcArgs& a, float temperature,
                                                    IscoWgScratch* sc, int lane, int w) {
    typename M::Acc acc{};
    float mx = -INFINITY;
    const int64_t G = (N + 63) >> 6;
    for (int64_t g = w; g < G; g += kIscoWgWaves) {
        const int64_t i = (g << 6) + lane;
        const bool in = i < N;
        const uint8_t si = in ? s[i] : 0;
        int d = 0;
        const int deg = in ? a.rowptr[i + 1] - a.rowptr[i] : 0;
        if (a.ell_ptr) {
            const int e0 = a.ell_ptr[g], e1 = a.ell_ptr[g + 1];
            const int self = (int)(in ? i : 0);
            for (int k = e0; k < e1; k += 8 * kWave) {
                int nb[8];
#pragma unroll
                for (int q = 0; q < 8; ++q) nb[q] = (k + q * kWave < e1) ? a.ell[k + q * kWave + lane] : self;
#pragma unroll
                for (int q = 0; q < 8; ++q) d += (s[nb[q]] != si);
            }
        } else if (in) {
            for (int j = a.rowptr[i]; j < a.rowptr[i + 1]; ++j) d += (s[a.col[j]] != si);
        }
        if (in) {
            acc = M::add(acc, s, i, deg, d);
            const float v = M::score(s, i, deg, d, temperature, a.lam);
            lp[i] = v;
            mx = fmaxf(mx, v);
        }
    }
    mx = isco_block_max(mx, sc, lane, w);
    float se = 0.0f;
    for (int64_t g = w; g < G; g += kIscoWgWaves) {
        const int64_t i = (g << 6) + lane;
        if (i < N) se += expf(lp[i] - mx);
    }
    const float lse = logf(isco_block_sum(se, sc, lane, w));
    for (int64_t g = w; g < G; g += kIscoWgWaves) {
        const int64_t i = (g << 6) + lane;
        if (i < N) lp[i] = (lp[i] - mx) - lse;
    }
    return M::ll(acc, temperature, a.lam, [&](int v) { return isco_block_sum_i(v, sc, lane, w); });   // (its barriers also publish lp[])
}

// What the two step bodies below ask of a sample's source -- everything that differs between the graph steps and the dense one:
//   Args             the kernel's argument struct (the bodies read the fields the two share by name)
//   kWaveTie         whether the wave-per-sample body breaks ties of the sort by node id
//   bit(i)           the input element i as a bit
//   local_dist[_wg]  the proposal distribution of state s into lp, energy(s) / T returned, by a wave / by the workgroup
//   after_flip       between the flip and the backward distribution (the piece t of nt of the team)
//   ord()            where the order of a selection larger than the list lives
//   clamp0           the clamp of the log-acceptance at 0
//   put(i, v)        the output element i from a bit
// Graph steps, energy model M: f32 samples, the distribution from neighbour walks.
template <class M>
struct IscoGraph {
    using Args = IscoMcArgs;
    // false: what this kernel has always computed -- its compaction is in node order, only the sort's own order of equal keys differs
    static constexpr bool kWaveTie = false;
    const IscoMcArgs& a;
    const float* xr;
    float* yo;
    __device__ __forceinline__ IscoGraph(const IscoMcArgs& a_, int64_t b) : a(a_), xr(a_.x + b * a_.N), yo(a_.y_out + b * a_.N) {}
    __device__ __forceinline__ bool bit(int64_t i) const { return xr[i] > 0.0f; }
    __device__ __forceinline__ float local_dist(const uint8_t* s, float* lp, int lane) const {
        return isco_local_dist<M>(s, lp, a.N, a.rowptr, a.col, a.ell_ptr, a.ell, a.temperature, a.lam, lane);
    }
    __device__ __forceinline__ float local_dist_wg(const uint8_t* s, float* lp, IscoWgScratch* sc, int lane, int w, int) const {
        return isco_local_dist_wg<M>(s, lp, a.N, a, a.temperature, sc, lane, w);
    }
    template <typename S>
    __device__ __forceinline__ void after_flip(float*, const uint8_t*, int, S, int, int) {}
    __device__ __forceinline__ int32_t* ord() const { return reinterpret_cast<int32_t*>(yo); }   // this sample's output row, written last
    __device__ static __forceinline__ float clamp0(float v) { return fminf(v, 0.0f); }
    __device__ __forceinline__ void put(int64_t i, uint8_t v) const { yo[i] = (float)v; }
};

// ----------------------------------------------------------------------------------------------- PISCO (dense, weighted MaxCut)
// PISCO_maxcut.step (env_ISCO.py:384-434): the MaxCut step with the local distribution of a sample read from its row of the
// dense product r = delta . A (rls_pisco_product, rls_pisco.hip) instead of from neighbour walks:
//   score_k = delta_k r_k / (2T),  energy = -0.25 sum_k r_k delta_k / T   (tensor_core_energy :436-444 and its autograd)
// The proposal's row is the rank-L update r'_j = r_j - 2 sum_{k selected} delta_k A[k][j] (delta of x; contiguous f16 rows of the
// symmetric A), so a step runs one product.  half_rounding: r and sum_k r_k delta_k each rounded to f16 once, as the reference's
// half matmul and half sum do.  Samples are f16 in and out; all Np columns -- the padded ones too -- take part.
struct PiscoArgs {
    const uint16_t* adj; int64_t N;                       // f16 [N, N], N % 8 == 0
    const uint16_t* x; uint16_t* y_out; int64_t B;        // f16 [B, N]
    const int64_t* path_length; float temperature; int half_rounding;
    const float* u_gumbel; const float* u_accept; uint64_t seed; int64_t env_offset;
    float* energy_out; float* acc_out; float* terms_out; uint8_t* mask_out;
    int P;
    const float* r;                                       // f32 [B, N] from rls_pisco_product
    int32_t* ord;                                         // int32 [B, N]: the order of a selection larger than the list
};

__device__ __forceinline__ bool pisco_is_set(uint16_t h) { return __builtin_bit_cast(_Float16, h) > (_Float16)0; }
__device__ __forceinline__ float pisco_round_f16(float v) { return (float)(_Float16)v; }
// torch.clamp(v, max=0): a NaN stays a NaN (the f16 sum of a large instance overflows to -inf in the reference; -inf - -inf then
// rejects the proposal there, where fminf would return 0 and accept it)
__device__ __forceinline__ float pisco_clamp0(float v) { return v != v ? v : fminf(v, 0.0f); }
__device__ __forceinline__ float pisco_energy(float s, float temperature, bool half) {
    return (-0.25f * (half ? pisco_round_f16(s) : s)) / temperature;
}
// one column: the score into lp[i], the column's term of sum_k r_k delta_k returned
__device__ __forceinline__ float pisco_score(const uint8_t* s, const float* rrow, float* lp, int64_t i, float temperature, bool half,
                                             float& mx) {
    const float d = s[i] ? 1.0f : -1.0f;
    const float rv = half ? pisco_round_f16(rrow[i]) : rrow[i];
    const float sc = (d * rv) / (2.0f * temperature);
    lp[i] = sc;
    mx = fmaxf(mx, sc);
    return rv * d;
}

// r'[8c .. 8c + 7] = r[8c ..] - 2 sum_k delta_k A[sel_k][8c ..] in list order, for the 8-column pieces c = t, t + nt, ...
template <typename S>
__device__ __forceinline__ void pisco_rank_update(const PiscoArgs& a, const float* rrow, float* rnew, const uint8_t* xb, int count,
                                                  S sel_at, int t, int nt) {
    const int64_t N = a.N;
    for (int64_t c = t; c < (N >> 3); c += nt) {
        float v[8];
#pragma unroll
        for (int e = 0; e < 8; ++e) v[e] = rrow[c * 8 + e];
        for (int k = 0; k < count; ++k) {
            const int node = sel_at(k);
            const float two_d = xb[node] ? 2.0f : -2.0f;
            const u32x4 row = *reinterpret_cast<const u32x4*>(a.adj + (int64_t)node * N + c * 8);
            const uint32_t wd[4] = {row.x, row.y, row.z, row.w};
#pragma unroll
            for (int e = 0; e < 8; ++e)
                v[e] -= two_d * (float)__builtin_bit_cast(_Float16, (uint16_t)(wd[e >> 1] >> ((e & 1) * 16)));
        }
#pragma unroll
        for (int e = 0; e < 8; ++e) rnew[c * 8 + e] = v[e];
    }
}

__device__ __forceinline__ float pisco_local_dist(const uint8_t* s, const float* rrow, float* lp, int64_t N, float temperature,
                                                  bool half, int lane) {
    float sum = 0.0f, mx = -INFINITY;
    for (int64_t i = lane; i < N; i += kWave) sum += pisco_score(s, rrow, lp, i, temperature, half, mx);
    mx = wave_max_f(mx);
    float se = 0.0f;
    for (int64_t i = lane; i < N; i += kWave) se += expf(lp[i] - mx);
    const float lse = logf(wave_sum_f32x(se));
    for (int64_t i = lane; i < N; i += kWave) lp[i] = (lp[i] - mx) - lse;
    lds_fence();
    return pisco_energy(wave_sum_f32x(sum), temperature, half);
}

__device__ __forceinline__ float pisco_local_dist_wg(const uint8_t* s, const float* rrow, float* lp, int64_t N, float temperature,
                                                     bool half, IscoWgScratch* sc, int lane, int w, int tid) {
    constexpr int NT = kIscoWgWaves * kWave;
    float sum = 0.0f, mx = -INFINITY;
    for (int64_t i = tid; i < N; i += NT) sum += pisco_score(s, rrow, lp, i, temperature, half, mx);
    mx = isco_block_max(mx, sc, lane, w);
    float se = 0.0f;
    for (int64_t i = tid; i < N; i += NT) se += expf(lp[i] - mx);
    const float lse = logf(isco_block_sum(se, sc, lane, w));
    for (int64_t i = tid; i < N; i += NT) lp[i] = (lp[i] - mx) - lse;
    return pisco_energy(isco_block_sum(sum, sc, lane, w), temperature, half);      // (its barriers also publish lp[])
}

// The dense step's source: f16 samples, the distribution from `row` -- the sample's row of the product, then (after the flip)
// the proposal's row, which the rank-L update leaves in pert[] (free from there on).
struct IscoDense {
    using Args = PiscoArgs;
    static constexpr bool kWaveTie = true;
    const PiscoArgs& a;
    const uint16_t* xr;
    uint16_t* yo;
    const float* row;
    const bool half;
    int32_t* const ordp;
    __device__ __forceinline__ IscoDense(const PiscoArgs& a_, int64_t b)
        : a(a_), xr(a_.x + b * a_.N), yo(a_.y_out + b * a_.N), row(a_.r + b * a_.N), half(a_.half_rounding != 0), ordp(a_.ord + b * a_.N) {}
    __device__ __forceinline__ bool bit(int64_t i) const { return pisco_is_set(xr[i]); }
    __device__ __forceinline__ float local_dist(const uint8_t* s, float* lp, int lane) const {
        return pisco_local_dist(s, row, lp, a.N, a.temperature, half, lane);
    }
    __device__ __forceinline__ float local_dist_wg(const uint8_t* s, float* lp, IscoWgScratch* sc, int lane, int w, int tid) const {
        return pisco_local_dist_wg(s, row, lp, a.N, a.temperature, half, sc, lane, w, tid);
    }
    template <typename S>
    __device__ __forceinline__ void after_flip(float* pert, const uint8_t* xb, int count, S sel_at, int t, int nt) {
        pisco_rank_update(a, row, pert, xb, count, sel_at, t, nt);
        row = pert;
    }
    __device__ __forceinline__ int32_t* ord() const { return ordp; }   // an f16 output row is too short for it: the caller's scratch
    __device__ static __forceinline__ float clamp0(float v) { return pisco_clamp0(v); }
    __device__ __forceinline__ void put(int64_t i, uint8_t v) const { yo[i] = v ? 0x3C00 : 0; }
};

// ----------------------------------------------------------------------------------------------- the two step bodies
// A WAVE per sample, its rows in this wave's slice of LDS.
template <class S>
__device__ __forceinline__ void isco_step_wave(const typename S::Args& a) {
    extern __shared__ __attribute__((aligned(16))) unsigned char smem[];
    const int lane = threadIdx.x & (kWave - 1);
    const int wib = threadIdx.x / kWave;
    const int64_t b = (int64_t)blockIdx.x * (blockDim.x / kWave) + wib;
    if (b >= a.B) return;
    const int64_t N = a.N;
    const int P = a.P;
    const size_t nb8 = ((size_t)N + 7) & ~(size_t)7;
    const size_t per_wave = 2 * nb8 + (size_t)N * 8 + (size_t)P * 8;
    unsigned char* base = smem + (size_t)wib * per_wave;
    uint8_t* xb = base;
    uint8_t* yb = base + nb8;
    float* lp = reinterpret_cast<float*>(base + 2 * nb8);
    float* pert = lp + N;
    float* skey = pert + N;
    int32_t* sidx = reinterpret_cast<int32_t*>(skey + P);
    const uint64_t genv = (uint64_t)(b + a.env_offset);
    S src(a, b);

    for (int64_t i = lane; i < N; i += kWave) xb[i] = src.bit(i) ? 1 : 0;
    lds_fence();
    // ---- forward: ll_x, proposal distribution, Gumbel perturbation (env_ISCO.py:51-63, util.py:498-516)
    const float ll_x = src.local_dist(xb, lp, lane);
    float lmax = -INFINITY;
    for (int64_t i = lane; i < N; i += kWave) {
        const float u = a.u_gumbel ? a.u_gumbel[b * N + i] : isco_unit(isco_draw(a.seed, genv, (uint32_t)i, 0, 1));
        const float l = lp[i];
        pert[i] = l - logf(-logf(u));
        lmax = fmaxf(lmax, l);
    }
    lmax = wave_max_f(lmax);                                   // ll_base of the forward renormalisation: max over ALL entries
    lds_fence();
    // ---- the selected set: perturbed >= the L-th largest perturbed value, compacted then sorted by perturbed value, descending
    int64_t L = a.path_length[b];
    L = L < 1 ? 1 : (L > N ? N : L);
    const uint32_t prefix = isco_threshold_wave(pert, N, (int)L, lane);
    const int count = isco_compact_wave(pert, N, prefix, skey, sidx, P, lane);
    const bool big = count > P;                                  // (wave-uniform) the list does not hold the selection
    int32_t* ord = src.ord();                                    // its order then lives there until the end
    if (big) isco_order_by_extraction(pert, yb, N, prefix, count, ord, lane);
    else isco_sort_list<S::kWaveTie>(skey, sidx, count, lane);   // (graph steps: no tie-break, as ever -- see IscoGraph::kWaveTie)
    auto sel_at = [&](int k) -> int { return big ? ord[k] : sidx[k]; };
    // ---- ll_x2y: log-probability of drawing the selected set in that order (util.py:530-552)
    const float ll_x2y = noreplacement_ll_sum(count, lmax, lane, [&](int k) { return lp[sel_at(k)]; });
    // ---- y = x with the selected nodes flipped (env_ISCO.py:41-43)
    for (int64_t i = lane; i < N; i += kWave) yb[i] = xb[i];
    lds_fence();
    for (int k = lane; k < count; k += kWave) yb[sel_at(k)] ^= 1;
    src.after_flip(pert, xb, count, sel_at, lane, kWave);
    lds_fence();
    if (a.mask_out) {
        for (int64_t i = lane; i < N; i += kWave) a.mask_out[b * N + i] = xb[i] ^ yb[i];
    }
    // ---- backward: ll_y and the probability of undoing the selection in reverse order (env_ISCO.py:65-77)
    const float ll_y = src.local_dist(yb, lp, lane);
    const float ll_y2x = isco_reverse_ll(lp, count, sel_at, lane);
    const float log_acc = S::clamp0(((ll_y + ll_y2x) - ll_x) - ll_x2y);
    const bool accept = isco_mh_accept(a, b, ll_x, ll_x2y, ll_y, ll_y2x, log_acc, lane);
    for (int64_t i = lane; i < N; i += kWave) src.put(i, accept ? yb[i] : xb[i]);
}

// The same step with a WORKGROUP per sample, for the few-chain regime the reference's own configs run in (one chain:
// a lone wave is instruction-issue bound, ~155 us per step on a G22-sized graph).  The node loops are split over the
// kIscoWgWaves waves; maxima / sums meet through LDS; the L-th largest perturbed value comes from four 8-bit histogram
// passes (LDS atomics) instead of 32 one-bit passes; the <= L selected entries are sorted and their path
// log-probabilities summed by wave 0 as before.  Same arithmetic per element; row sums are reduced wave by wave.
// GROWS: the two f32 rows (lp, pert) live in the caller's scratch (global memory, L2-resident while a sample is worked on) and
// LDS holds the byte rows and the list only -- N past ~15 900, up to ~81 000.  The workgroup's barriers order its global
// stores and loads as they do the LDS ones (__syncthreads fences both at workgroup scope; the L1 is the CU's).
template <class S, bool GROWS>
__device__ __forceinline__ void isco_step_wg(const typename S::Args& a) {
    extern __shared__ __attribute__((aligned(16))) unsigned char smem[];
    const int lane = threadIdx.x & (kWave - 1);
    const int w = __builtin_amdgcn_readfirstlane((int)(threadIdx.x / kWave));
    const int tid = threadIdx.x, NT = kIscoWgWaves * kWave;
    const int64_t b = blockIdx.x;
    const int64_t N = a.N;
    const int P = a.P;
    const size_t nb8 = ((size_t)N + 7) & ~(size_t)7;
    uint8_t* xb = smem;
    uint8_t* yb = smem + nb8;
    float* lp;
    if constexpr (GROWS) lp = a.rows + b * 2 * N;
    else lp = reinterpret_cast<float*>(smem + 2 * nb8);
    float* pert = lp + N;
    float* skey = GROWS ? reinterpret_cast<float*>(smem + 2 * nb8) : pert + N;
    int32_t* sidx = reinterpret_cast<int32_t*>(skey + P);
    IscoWgScratch* sc = reinterpret_cast<IscoWgScratch*>(sidx + P);
    const uint64_t genv = (uint64_t)(b + a.env_offset);
    S src(a, b);

    for (int64_t i = tid; i < N; i += NT) xb[i] = src.bit(i) ? 1 : 0;
    __syncthreads();
    // ---- forward: ll_x, proposal distribution, Gumbel perturbation
    const float ll_x = src.local_dist_wg(xb, lp, sc, lane, w, tid);
    float lmax = -INFINITY;
    for (int64_t i = tid; i < N; i += NT) {
        const float u = a.u_gumbel ? a.u_gumbel[b * N + i] : isco_unit(isco_draw(a.seed, genv, (uint32_t)i, 0, 1));
        const float l = lp[i];
        pert[i] = l - logf(-logf(u));
        lmax = fmaxf(lmax, l);
    }
    lmax = isco_block_max(lmax, sc, lane, w);                  // ll_base of the forward renormalisation (also publishes pert[])
    // ---- the selected set: perturbed >= the L-th largest perturbed value, compacted, then ordered by wave 0
    int64_t L = a.path_length[b];
    L = L < 1 ? 1 : (L > N ? N : L);
    const uint32_t prefix = isco_threshold_wg(pert, N, (int)L, sc, lane, w, tid);
    const int count = isco_compact_wg(pert, N, prefix, skey, sidx, P, sc, tid);
    const bool big = count > P;                                  // the list does not hold the selection: order by extraction
    int32_t* ord = src.ord();
    auto sel_at = [&](int k) -> int { return big ? ord[k] : sidx[k]; };
    float ll_x2y = 0.0f;
    if (w == 0 && big) {
        isco_order_by_extraction(pert, yb, N, prefix, count, ord, lane);
        ll_x2y = noreplacement_ll_sum(count, lmax, lane, [&](int k) { return lp[ord[k]]; });
    } else if (w == 0) {
        isco_sort_list<true>(skey, sidx, count, lane);
        ll_x2y = noreplacement_ll_sum(count, lmax, lane, [&](int k) { return lp[sidx[k]]; });
    }
    // ---- y = x with the selected nodes flipped
    __syncthreads();                                              // (wave 0 may have used yb as the extraction's marks)
    for (int64_t i = tid; i < N; i += NT) yb[i] = xb[i];
    __syncthreads();
    for (int k = tid; k < count; k += NT) yb[sel_at(k)] ^= 1;
    src.after_flip(pert, xb, count, sel_at, tid, NT);
    __syncthreads();
    if (a.mask_out) {
        for (int64_t i = tid; i < N; i += NT) a.mask_out[b * N + i] = xb[i] ^ yb[i];
    }
    // ---- backward, the accept by wave 0
    const float ll_y = src.local_dist_wg(yb, lp, sc, lane, w, tid);
    if (w == 0) {
        const float ll_y2x = isco_reverse_ll(lp, count, sel_at, lane);
        const float log_acc = S::clamp0(((ll_y + ll_y2x) - ll_x) - ll_x2y);
        const bool accept = isco_mh_accept(a, b, ll_x, ll_x2y, ll_y, ll_y2x, log_acc, lane);
        if (lane == 0) sc->want = accept ? 1 : 0;
    }
    __syncthreads();
    const bool accept = sc->want != 0;
    for (int64_t i = tid; i < N; i += NT) src.put(i, accept ? yb[i] : xb[i]);
}

template <class M>
__global__ __launch_bounds__(512) void k_isco_maxcut_step(IscoMcArgs a) { isco_step_wave<IscoGraph<M>>(a); }
template <class M, bool GROWS>
__global__ __launch_bounds__(kIscoWgWaves * kWave) void k_isco_maxcut_step_wg(IscoMcArgs a) { isco_step_wg<IscoGraph<M>, GROWS>(a); }
__global__ __launch_bounds__(512) void k_pisco_step(PiscoArgs a) { isco_step_wave<IscoDense>(a); }
__global__ __launch_bounds__(kIscoWgWaves * kWave) void k_pisco_step_wg(PiscoArgs a) { isco_step_wg<IscoDense, false>(a); }

// ----------------------------------------------------------------------------------------------- TSP
struct IscoTspArgs {
    const float* dist; int64_t N; int32_t K; int32_t random_stride; float near_threshold;
    const int32_t* nearest; const int32_t* random;       // [N, K], [N, N-K-1]
    const int64_t* perm_in; int64_t* perm_out; int64_t B; int32_t path_length; float temperature;
    const float* u_partner; const int64_t* r_near; const int64_t* r_rand; const float* u_gumbel;   // [L, B, N] or NULL
    const float* u_accept;                                // [B] or NULL
    uint64_t seed; int64_t env_offset;
    float* log_acc_out; float* acc_out; int64_t* cur_out;
};

template <bool LDS_D>
__global__ __launch_bounds__(256) void k_isco_tsp_step(IscoTspArgs a) {
    extern __shared__ __attribute__((aligned(16))) unsigned char smem[];
    const int lane = threadIdx.x & (kWave - 1);
    const int wib = threadIdx.x / kWave;
    const int n = (int)a.N;
    float* dl = reinterpret_cast<float*>(smem);
    const float* D = a.dist;
    if constexpr (LDS_D) {
        for (int64_t c = threadIdx.x; c < a.N * a.N; c += blockDim.x) dl[c] = a.dist[c];
        __syncthreads();
        D = dl;
    }
    unsigned char* wbase = smem + (LDS_D ? (size_t)a.N * a.N * 4 : 0) + (size_t)wib * ((size_t)n * 16);
    int32_t* Pm = reinterpret_cast<int32_t*>(wbase);      // tour
    int32_t* INV = Pm + n;                                  // city -> position
    float* lg = reinterpret_cast<float*>(INV + n);          // logits of this iteration
    int32_t* jb = reinterpret_cast<int32_t*>(lg + n);       // partner position | banned << 31, per position
    const int64_t b = (int64_t)blockIdx.x * (blockDim.x / kWave) + wib;
    if (b >= a.B) return;
    const uint64_t genv = (uint64_t)(b + a.env_offset);
    const int K = a.K, NR = n - K - 1;
    const float T = a.temperature;
    const int64_t* pin = a.perm_in + b * a.N;
    for (int k = lane; k < n; k += kWave) {
        const int city = (int)pin[k];
        Pm[k] = city;
        INV[city] = k;
    }
    lds_fence();
    auto DD = [&](int u, int v) { return D[(int64_t)u * n + v]; };
    float s_delta = 0.0f, s_fwd = 0.0f, s_bwd = 0.0f;       // the three rows of `traj` (env_ISCO.py:190-196)
    for (int it = 0; it < a.path_length; ++it) {
        const int64_t row = ((int64_t)it * a.B + b) * a.N;
        // ---- opt_2 (env_ISCO.py:238-335): partner city per position, swap delta, ban mask; logits = logratio / 2
        float mx = -INFINITY;
        for (int i = lane; i < n; i += kWave) {
            const int city = Pm[i];
            float up;
            int rn, rr;
            if (a.u_partner) {
                up = a.u_partner[row + i];
                rn = (int)a.r_near[row + i];
                rr = (int)a.r_rand[row + i];
            } else {
                up = isco_unit(isco_draw(a.seed, genv, (uint32_t)i, (uint32_t)it, 3));
                rn = (int)(((uint64_t)isco_draw(a.seed, genv, (uint32_t)i, (uint32_t)it, 4) * (uint64_t)K) >> 32);
                rr = NR > 0 ? (int)(((uint64_t)isco_draw(a.seed, genv, (uint32_t)i, (uint32_t)it, 5) * (uint64_t)NR) >> 32) : 0;
            }
            const bool near = up < a.near_threshold;                              // rand < K / (K + 1)
            const int sel = near ? a.nearest[(int64_t)city * K + rn] : a.random[(int64_t)city * a.random_stride + rr];
            const int j = INV[sel];
            const int i0 = (i == 0) ? n - 1 : i - 1;
            const int i1 = (i + 1 == n) ? 0 : i + 1;
            const int i2 = (i1 + 1 == n) ? 0 : i1 + 1;
            const int j0 = (j == 0) ? n - 1 : j - 1;
            const int j1 = (j + 1 == n) ? 0 : j + 1;
            const int s_m1 = Pm[i1], s_m0 = Pm[i0];
            const bool banned = (s_m1 == sel) || (s_m0 == sel);
            const int s_i0 = Pm[j0], s_i1 = Pm[j1], s_i = sel;
            const bool c3 = (s_m1 == s_i0);
            const int nm = city, nm1 = s_m1, nm2 = Pm[i2];
            float delta;
            if (banned) delta = 0.0f;
            else if (c3) delta = -(DD(nm, nm1) + DD(s_i, s_i1)) + (DD(nm, s_i) + DD(s_i0, s_i1));
            else delta = -(((DD(nm, nm1) + DD(nm1, nm2)) + DD(s_i0, s_i)) + DD(s_i, s_i1)) +
                         (((DD(nm, s_i) + DD(s_i, nm2)) + DD(s_i0, nm1)) + DD(nm1, s_i1));
            const float logratio = banned ? -1e6f : (-delta) / T;                 // :197 logratio[ban_mask] = -1e6
            const float logit = logratio / 2.0f;                                  // apply_weight_function_logscale
            lg[i] = logit;
            jb[i] = j | (banned ? (int)0x80000000u : 0);
            mx = fmaxf(mx, logit);
        }
        lds_fence();
        mx = wave_max_f(mx);
        float se = 0.0f;
        for (int i = lane; i < n; i += kWave) se += expf(lg[i] - mx);
        const float lse = logf(wave_sum_f32x(se));
        // ---- multinomial with one draw: the position with the largest Gumbel-perturbed log-probability
        float best = -INFINITY;
        int bi = 0x7fffffff;
        for (int i = lane; i < n; i += kWave) {
            const float u = a.u_gumbel ? a.u_gumbel[row + i] : isco_unit(isco_draw(a.seed, genv, (uint32_t)i, (uint32_t)it, 6));
            const float pv = ((lg[i] - mx) - lse) - logf(-logf(u));
            if (pv > best) { best = pv; bi = i; }
        }
#pragma unroll
        for (int m = 32; m >= 1; m >>= 1) {
            const float ob = __shfl_xor(best, m, 64);
            const int oi = __shfl_xor(bi, m, 64);
            if (ob > best || (ob == best && oi < bi)) { best = ob; bi = oi; }
        }
        const int q = bi;
        const float lq = lg[q];
        const float ll_x2y = (lq - mx) - lse;                                      // first draw: no renormalisation term
        const uint32_t jq = (uint32_t)jb[q];
        const bool q_banned = jq >> 31;
        const float delta_yx = q_banned ? -1e6f : lq * 2.0f;                       // logratio of the selected position
        // ---- reverse move: log_softmax of the logits with the selected one negated, at the selected position (:214-226)
        const float nq = -lq;
        float mx2 = -INFINITY;
        for (int i = lane; i < n; i += kWave) mx2 = fmaxf(mx2, i == q ? nq : lg[i]);
        mx2 = wave_max_f(mx2);
        float se2 = 0.0f;
        for (int i = lane; i < n; i += kWave) se2 += expf((i == q ? nq : lg[i]) - mx2);
        const float ll_y2x = (nq - mx2) - logf(wave_sum_f32x(se2));
        s_delta += delta_yx;
        s_fwd += -ll_x2y;
        s_bwd += ll_y2x;
        // ---- switch (:337-344): swap the cities at positions q + 1 and j(q) unless banned
        lds_fence();
        if (!q_banned && lane == 0) {
            const int j = (int)(jq & 0x7fffffffu);
            const int p1 = (q + 1 == n) ? 0 : q + 1;
            const int c1 = Pm[p1], c2 = Pm[j];
            Pm[p1] = c2; Pm[j] = c1;
            INV[c2] = p1; INV[c1] = j;
        }
        lds_fence();
    }
    const float log_acc = fminf((s_delta + s_fwd) + s_bwd, 0.0f);
    const float ua = a.u_accept ? a.u_accept[b] : isco_unit(isco_draw(a.seed, genv, 0xFFFFFFFFu, 0, 7));
    const bool accept = logf(ua + 1e-24f) < log_acc;
    int64_t* po = a.perm_out + b * a.N;
    for (int k = lane; k < n; k += kWave) {
        const int64_t cur = Pm[k];
        if (a.cur_out) a.cur_out[b * a.N + k] = cur;
        po[k] = accept ? cur : pin[k];
    }
    if (lane == 0) {
        if (a.log_acc_out) a.log_acc_out[b] = log_acc;
        if (a.acc_out) a.acc_out[b] = expf(log_acc);
    }
}

// K10' evolutionary_replacement  methods/util.py:87-94, the row moves: xs[dst[k]] = xs[src[k]], vs likewise.
// The reference's  xs[replace_ids] = xs[low_ids]  gathers the right-hand side first; dst and src are disjoint
// by construction (top_ids vs low_ids), so the copy may run in place.  One wave per moved row, 16-byte lanes.
// dst and src come from device memory: a move with either index outside [0, B) is skipped (the unsigned compare also
// catches a negative index), so no index can turn into an address outside xs / vs.
__global__ __launch_bounds__(256) void k_copy_rows(uint8_t* __restrict__ xs, int64_t* __restrict__ vs, int64_t B, int64_t N,
                                                   const int64_t* __restrict__ dst, const int64_t* __restrict__ src,
                                                   int64_t K, int vec) {
    const int lane = threadIdx.x & (kWave - 1);
    const int64_t k = (int64_t)blockIdx.x * (blockDim.x / kWave) + threadIdx.x / kWave;
    if (k >= K) return;
    const int64_t d = dst[k], s = src[k];
    if ((uint64_t)d >= (uint64_t)B || (uint64_t)s >= (uint64_t)B) return;
    if (vec) {
        const u32x4* sp = reinterpret_cast<const u32x4*>(xs + s * N);
        u32x4* dp = reinterpret_cast<u32x4*>(xs + d * N);
        for (int64_t i = lane; i < N / 16; i += kWave) dp[i] = sp[i];
    } else {
        for (int64_t i = lane; i < N; i += kWave) xs[d * N + i] = xs[s * N + i];
    }
    if (lane == 0 && vs) vs[d] = vs[s];
}

}  // namespace rls

using namespace rls;

extern "C" {

int64_t rls_isco_maxcut_scratch_bytes(const rls_graph* g, int64_t B) {
    if (!g || B <= 0 || (isco_rows_fit_lds(isco_rows_bytes(g->num_nodes)) && !knob_on(KN_ISCO_GLOBAL_ROWS))) return 0;
    return B * g->num_nodes * 8;
}

}  // extern "C"

// One launcher for every energy model M of the step: validation, then what isco_plan_step answers (rls_isco_plan.h: the list's
// capacity, wave vs workgroup per sample, rows in LDS or in scratch) -- none of it depends on the model (the rows and the lists
// are the same).
template <class M>
static int isco_step_launch(const rls_graph* g, const float* x, float* y_out, int64_t B, const int64_t* path_length,
                            float temperature, float lam, const float* u_gumbel, const float* u_accept, uint64_t seed,
                            int64_t env_offset, float* energy_out, float* acc_out, float* terms_out, uint8_t* mask_out,
                            void* scratch, int64_t scratch_bytes, void* stream) {
    if (int rc = check_graph(g)) return rc;
    RLS_REQUIRE(B >= 0, RLS_EINVAL, "B < 0");
    if (B == 0) return RLS_OK;
    RLS_REQUIRE(x && y_out && path_length, RLS_EINVAL, "NULL pointer");
    RLS_REQUIRE((u_gumbel == nullptr) == (u_accept == nullptr), RLS_EINVAL, "u_gumbel and u_accept must both be given or both be NULL");
    RLS_REQUIRE(temperature > 0.0f, RLS_EINVAL, "temperature must be > 0");
    const int64_t N = g->num_nodes;
    RLS_REQUIRE((const void*)x != (const void*)y_out, RLS_EINVAL, "y_out must not alias x (a rejected proposal restores x; the row also serves as scratch)");
    const IscoPlan p = isco_plan_step(isco_rows_bytes(N), N, B, num_cus(), 1, true);
    RLS_REQUIRE(p.err == RLS_OK, p.err, "N=%lld: the two byte rows of a sample need %zu B of LDS (max %d)", (long long)N, p.need, kLdsBytes);
    if (p.grows)
        RLS_REQUIRE(scratch && scratch_bytes >= B * N * 8, RLS_EINVAL,
                    "N=%lld needs %lld B of scratch (rls_isco_maxcut_scratch_bytes), got %lld", (long long)N, (long long)(B * N * 8),
                    (long long)(scratch ? scratch_bytes : 0));
    const bool use_ell = g->ell_sym_ptr && g->ell_sym && !g->wgt;
    const IscoMcArgs a{g->rowptr, g->col, use_ell ? g->ell_sym_ptr : nullptr, use_ell ? g->ell_sym : nullptr, x, y_out, B, N,
                       path_length, temperature, u_gumbel, u_accept, seed, env_offset, energy_out, acc_out, terms_out, mask_out,
                       p.wg ? p.P : p.Pw, lam, p.grows ? static_cast<float*>(scratch) : nullptr};
    const dim3 wg_block(kIscoWgWaves * kWave);
    if (p.grows) {
        ensure_dyn_lds((const void*)(k_isco_maxcut_step_wg<M, true>), p.lds);
        hipLaunchKernelGGL((k_isco_maxcut_step_wg<M, true>), dim3((unsigned)B), wg_block, p.lds, as_stream(stream), a);
        return check_launch("k_isco_maxcut_step_wg<global rows>");
    }
    if (p.wg) {
        ensure_dyn_lds((const void*)(k_isco_maxcut_step_wg<M, false>), p.lds);
        hipLaunchKernelGGL((k_isco_maxcut_step_wg<M, false>), dim3((unsigned)B), wg_block, p.lds, as_stream(stream), a);
        return check_launch("k_isco_maxcut_step_wg");
    }
    ensure_dyn_lds((const void*)k_isco_maxcut_step<M>, p.lds);
    hipLaunchKernelGGL(k_isco_maxcut_step<M>, dim3((unsigned)ceil_div(B, p.waves)), dim3(p.waves * kWave), p.lds, as_stream(stream), a);
    return check_launch("k_isco_maxcut_step");
}

extern "C" {

int rls_isco_maxcut_step(const rls_graph* g, const float* x, float* y_out, int64_t B, const int64_t* path_length,
                         float temperature, const float* u_gumbel, const float* u_accept, uint64_t seed,
                         int64_t env_offset, float* energy_out, float* acc_out, float* terms_out, uint8_t* mask_out,
                         void* scratch, int64_t scratch_bytes, void* stream) {
    return isco_step_launch<IscoMaxcut>(g, x, y_out, B, path_length, temperature, 0.0f, u_gumbel, u_accept, seed, env_offset, energy_out,
                                        acc_out, terms_out, mask_out, scratch, scratch_bytes, stream);
}

int rls_isco_mis_step(const rls_graph* g, const float* x, float* y_out, int64_t B, const int64_t* path_length,
                      float temperature, float lam, const float* u_gumbel, const float* u_accept, uint64_t seed,
                      int64_t env_offset, float* energy_out, float* acc_out, float* terms_out, uint8_t* mask_out,
                      void* scratch, int64_t scratch_bytes, void* stream) {
    if (int rc = check_graph(g)) return rc;
    RLS_REQUIRE(std::isfinite(lam), RLS_EINVAL, "lam must be finite");
    return isco_step_launch<IscoMis>(g, x, y_out, B, path_length, temperature, lam, u_gumbel, u_accept, seed, env_offset, energy_out,
                                     acc_out, terms_out, mask_out, scratch, scratch_bytes, stream);
}

// The dense step: the product, then isco_plan_step's choices (list capacity -- at least 64 entries --, wave or workgroup per sample,
// the same knobs) with the rows in LDS only -- the rows-in-scratch form is not built for it (A alone would be 0.5 GB at its sizes).
// Every check comes before the first launch, and the checks that read no pointer (sizes, temperature, the LDS limit) before the
// pointer checks.
int rls_pisco_step(const uint16_t* adj, int64_t Np, const uint16_t* x, uint16_t* y_out, int64_t B, const int64_t* path_length,
                   float temperature, int32_t half_rounding, const float* u_gumbel, const float* u_accept, uint64_t seed,
                   int64_t env_offset, float* energy_out, float* acc_out, float* terms_out, uint8_t* mask_out, void* scratch,
                   int64_t scratch_bytes, void* stream) {
    RLS_REQUIRE(Np > 0 && Np % 8 == 0 && Np < (1ll << 31), RLS_EINVAL, "Np=%lld must be a positive multiple of 8", (long long)Np);
    RLS_REQUIRE(B >= 0, RLS_EINVAL, "B < 0");
    if (B == 0) return RLS_OK;
    RLS_REQUIRE(temperature > 0.0f, RLS_EINVAL, "temperature must be > 0");
    const IscoPlan p = isco_plan_step(isco_rows_bytes(Np), Np, B, num_cus(), kIscoMinList, false);
    RLS_REQUIRE(p.err == RLS_OK, p.err,
                "Np=%lld: a sample's rows and the smallest list need %zu B of LDS (max %d); the dense step has no rows-in-scratch form",
                (long long)Np, p.need, kLdsBytes);
    RLS_REQUIRE(adj && x && y_out && path_length, RLS_EINVAL, "NULL pointer");
    RLS_REQUIRE((u_gumbel == nullptr) == (u_accept == nullptr), RLS_EINVAL, "u_gumbel and u_accept must both be given or both be NULL");
    RLS_REQUIRE((const void*)x != (const void*)y_out, RLS_EINVAL, "y_out must not alias x (a rejected proposal restores x)");
    const int64_t need = rls_pisco_scratch_bytes(Np, B);
    RLS_REQUIRE(scratch && scratch_bytes >= need, RLS_EINVAL, "Np=%lld B=%lld need %lld B of scratch (rls_pisco_scratch_bytes), got %lld",
                (long long)Np, (long long)B, (long long)need, (long long)(scratch ? scratch_bytes : 0));
    RLS_REQUIRE((((uintptr_t)scratch) & 15) == 0, RLS_EINVAL, "scratch must be 16-byte aligned");
    float* r = static_cast<float*>(scratch);
    int32_t* ord = reinterpret_cast<int32_t*>(r + B * Np);
    if (int rc = rls_pisco_product(adj, Np, x, B, r, stream)) return rc;
    const PiscoArgs a{adj, Np, x, y_out, B, path_length, temperature, half_rounding, u_gumbel, u_accept, seed, env_offset,
                      energy_out, acc_out, terms_out, mask_out, p.wg ? p.P : p.Pw, r, ord};
    if (p.wg) {
        ensure_dyn_lds((const void*)k_pisco_step_wg, p.lds);
        hipLaunchKernelGGL(k_pisco_step_wg, dim3((unsigned)B), dim3(kIscoWgWaves * kWave), p.lds, as_stream(stream), a);
        return check_launch("k_pisco_step_wg");
    }
    ensure_dyn_lds((const void*)k_pisco_step, p.lds);
    hipLaunchKernelGGL(k_pisco_step, dim3((unsigned)ceil_div(B, p.waves)), dim3(p.waves * kWave), p.lds, as_stream(stream), a);
    return check_launch("k_pisco_step");
}

int rls_isco_tsp_step(const float* dist, int64_t N, const int32_t* nearest, int32_t K, float near_threshold, const int32_t* random,
                      int32_t random_stride,
                      const int64_t* perm_in, int64_t* perm_out, int64_t B, int32_t path_length, float temperature,
                      const float* u_partner, const int64_t* r_near, const int64_t* r_rand, const float* u_gumbel,
                      const float* u_accept, uint64_t seed, int64_t env_offset, float* log_acc_out, float* acc_out,
                      int64_t* cur_out, void* stream) {
    RLS_REQUIRE(N > 2 && N < (1 << 24) && B >= 0 && path_length >= 0, RLS_EINVAL, "bad sizes N=%lld B=%lld", (long long)N, (long long)B);
    RLS_REQUIRE(K >= 1 && K < N - 1, RLS_EINVAL, "K=%d outside [1, N-2]", K);
    RLS_REQUIRE(random_stride >= N - K - 1, RLS_EINVAL, "random_stride=%d < N - K - 1", random_stride);
    if (B == 0) return RLS_OK;
    RLS_REQUIRE(dist && nearest && random && perm_in && perm_out, RLS_EINVAL, "NULL pointer");
    RLS_REQUIRE(perm_in != perm_out, RLS_EINVAL, "perm_out must not alias perm_in (a rejected move restores it)");
    const bool test = u_partner || r_near || r_rand || u_gumbel || u_accept;
    RLS_REQUIRE(!test || (u_partner && r_near && r_rand && u_gumbel && u_accept), RLS_EINVAL,
                "test draws must be given all together");
    RLS_REQUIRE(temperature > 0.0f, RLS_EINVAL, "temperature must be > 0");
    const TspForm f = tsp_plan_step(N);
    RLS_REQUIRE(f.err == RLS_OK, f.err, "N=%lld too large for the per-env tour scratch", (long long)N);
    const bool lds_d = f.lds_d;
    const int waves = f.waves;
    const size_t lds = f.lds;
    IscoTspArgs a{dist, N, K, random_stride, near_threshold, nearest, random, perm_in, perm_out, B, path_length, temperature, u_partner, r_near, r_rand,
                  u_gumbel, u_accept, seed, env_offset, log_acc_out, acc_out, cur_out};
    const dim3 grid((unsigned)ceil_div(B, waves)), block(waves * kWave);
    if (lds_d) {
        if (lds > 64 * 1024) ensure_dyn_lds((const void*)k_isco_tsp_step<true>, lds);
        hipLaunchKernelGGL(k_isco_tsp_step<true>, grid, block, lds, as_stream(stream), a);
    } else {
        if (lds > 64 * 1024) ensure_dyn_lds((const void*)k_isco_tsp_step<false>, lds);
        hipLaunchKernelGGL(k_isco_tsp_step<false>, grid, block, lds, as_stream(stream), a);
    }
    return check_launch("k_isco_tsp_step");
}

int rls_copy_rows_bounded(uint8_t* xs, int64_t* vs, int64_t B, int64_t N, const int64_t* dst, const int64_t* src, int64_t K, void* stream) {
    RLS_REQUIRE(B >= 0 && N > 0 && K >= 0, RLS_EINVAL, "bad sizes B=%lld N=%lld K=%lld", (long long)B, (long long)N, (long long)K);
    RLS_REQUIRE(B <= INT64_MAX / N, RLS_EINVAL, "B * N = %lld * %lld does not fit int64", (long long)B, (long long)N);
    if (K == 0 || B == 0) return RLS_OK;
    RLS_REQUIRE(xs && dst && src, RLS_EINVAL, "NULL pointer");
    const int vec = ((((uintptr_t)xs) & 15) == 0 && N % 16 == 0) ? 1 : 0;
    hipLaunchKernelGGL(k_copy_rows, dim3((unsigned)ceil_div(K, 4)), dim3(256), 0, as_stream(stream), xs, vs, B, N, dst, src, K, vec);
    return check_launch("k_copy_rows");
}

// the first form: it is not told how many rows xs has, so only a negative index (or one past what int64 addresses) is skipped
int rls_copy_rows(uint8_t* xs, int64_t* vs, int64_t N, const int64_t* dst, const int64_t* src, int64_t K, void* stream) {
    RLS_REQUIRE(N > 0 && K >= 0, RLS_EINVAL, "bad sizes");
    return rls_copy_rows_bounded(xs, vs, INT64_MAX / N, N, dst, src, K, stream);
}

}  // extern "C"
