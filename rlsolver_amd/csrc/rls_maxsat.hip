// MaxSAT sampler of the MCPG package for gfx950: the node-sequential stochastic sweep of mcpg_sampling_maxsat
// (methods/MCPG/sampling.py:259-271) and its score (:272-274) in one kernel.
//
// One workgroup per 64-chain tile; the tile uint64 [nvar] (+ one zero word) sits in LDS.  The sweep runs on the level schedule
// of rls_maxsat_visit_levels (include/rlsolver_hip.h has the record format): lane = variable, a lane walks the stream of the
// clauses listed for its variable and every operation is 64 chains wide --
//     others |= x[v] ^ sign                         per literal of another variable        (1 LDS read, 2 ALU on 64-bit words)
//     crit = ~others; make += crit & ~own_true; break += crit & own_true                   per listed clause
//     x_i ^= [make > break] | ([make == break] & coin)                                     per variable
// make / break are bit-sliced vertical counters in registers, NP planes each (the schedule says how many a group needs).  The
// unweighted form adds a one-bit mask (a half-adder chain, 3 ops per plane); the weighted form adds the clause's constant
// weight gated by the mask (a full-adder chain) -- exact, and not the headline.
// The score: lane = clause, sat = OR of its literals over the tile; the 64 masks of a wave are summed per chain through
// readlane broadcasts (6 ops per clause and wave).
#include "rls_chains.h"
#include "rls_tile.h"

namespace rls {

constexpr int kMsWaves = 8;

template <int NP, bool WT>
__device__ __forceinline__ void ms_add(uint64_t (&cnt)[NP], uint64_t m, uint32_t wt) {
    uint64_t c = WT ? 0ull : m;
#pragma unroll
    for (int p = 0; p < NP; ++p) {
        if constexpr (WT) {
            const uint64_t a = ((wt >> p) & 1u) ? m : 0ull, s = cnt[p] ^ a;
            const uint64_t co = (cnt[p] & a) | (c & s);
            cnt[p] = s ^ c;
            c = co;
        } else {
            const uint64_t t = cnt[p] & c;
            cnt[p] ^= c;
            c = t;
        }
    }
}

// One group of <= 64 variables: this lane's stream of `blocks` blocks of 4 entries (first block in e / wt, the next one is
// requested while the current one is counted: the table ends in spare words).  Returns the flip mask of the lane's variable.
template <int NP, bool WT>
__device__ __forceinline__ uint64_t ms_group(const uint64_t* __restrict__ words, int64_t nvar, const int32_t* __restrict__ rec, int blocks,
                                             u32x4 e, u32x4 wt, uint64_t x, uint64_t coin, int lane) {
    constexpr int B = WT ? 512 : 256;
    uint64_t mk[NP], bk[NP];
#pragma unroll
    for (int p = 0; p < NP; ++p) mk[p] = bk[p] = 0;
    uint64_t others = 0;
    for (int b = 0; b < blocks; ++b) {
        const int32_t* nxt = rec + 128 + (int64_t)(b + 1) * B + 4 * lane;
        const u32x4 en = *reinterpret_cast<const u32x4*>(nxt);
        u32x4 wn = en;
        if constexpr (WT) wn = *reinterpret_cast<const u32x4*>(nxt + 256);
        const uint32_t ee[4] = {e.x, e.y, e.z, e.w}, ww[4] = {wt.x, wt.y, wt.z, wt.w};
#pragma unroll
        for (int r = 0; r < 4; ++r) {
            const uint32_t en_ = ee[r];
            uint32_t v = (en_ & 0x3FFF8u) >> 3;
            v = v < (uint32_t)nvar ? v : (uint32_t)nvar;                       // (the zero word; a table never points past it)
            others |= words[v] ^ (uint64_t)((int64_t)(int32_t)en_ >> 31);
            if (ballot64((en_ & 1u) != 0u)) {                                   // some lane's clause ends here (wave-uniform)
                const uint64_t ends = (en_ & 1u) ? ~0ull : 0ull;
                const uint32_t cls = (en_ >> 1) & 3u;
                const uint64_t crit = (cls == 3u) ? 0ull : (~others & ends);
                const uint64_t own_true = x ^ (cls == 2u ? ~0ull : 0ull);
                ms_add<NP, WT>(mk, crit & ~own_true, ww[r]);
                ms_add<NP, WT>(bk, crit & own_true, ww[r]);
                others &= ~ends;
            }
        }
        e = en;
        wt = wn;
    }
    uint64_t gt = 0, eq = ~0ull;
#pragma unroll
    for (int p = NP - 1; p >= 0; --p) {
        gt |= eq & mk[p] & ~bk[p];
        eq &= ~(mk[p] ^ bk[p]);
    }
    return gt | (eq & coin);
}

template <typename TO>
__global__ __launch_bounds__(kMsWaves * kWave) void k_maxsat_local_search(
    const uint64_t* xs_in, typename ChainStore<TO>::type* xs_out, int64_t nvar, int64_t C, int64_t tiles_in,
    const int32_t* __restrict__ lv_ptr, const int32_t* __restrict__ data, int64_t G, int64_t num_ls,
    const uint64_t* __restrict__ coins, uint64_t seed, const int32_t* __restrict__ clause_ptr, const int32_t* __restrict__ lit,
    const int32_t* __restrict__ weight, int64_t M, float* __restrict__ expected, ChainIds ids) {
    constexpr int W = kMsWaves;
    extern __shared__ __attribute__((aligned(16))) unsigned char smem[];
    uint64_t* words = reinterpret_cast<uint64_t*>(smem);                                          // [nvar + 1], word nvar = 0
    int* slots = reinterpret_cast<int*>(smem + (((size_t)(nvar + 1) * 8 + 15) & ~(size_t)15));     // [64] satisfied weight per chain, [64] = all weight
    const int lane = threadIdx.x & (kWave - 1);
    const int w = __builtin_amdgcn_readfirstlane((int)(threadIdx.x / kWave));
    const int64_t tile = mcpg_tile(), c0 = tile * kWave, c = c0 + lane;
    const int64_t CB = (C + kWave - 1) / kWave;
    if (threadIdx.x == 0) words[nvar] = 0;
    if (threadIdx.x <= kWave) slots[threadIdx.x] = 0;
    tile_load_packed(xs_in, nvar, C, tile, tiles_in, words, threadIdx.x, W * kWave);
    const uint32_t blk_key = k7_fmix32((uint32_t)seed ^ k7_fmix32((uint32_t)(seed >> 32) ^
                                                                  k7_fmix32((uint32_t)(ids(c0) >> 6) * 0x9E3779B1u + 0x632BE5ABu)));
    auto coin_word = [&](int64_t cnt, uint32_t pos) -> uint64_t {   // bit e: "u < 1/2" for chain c0 + e at (pass, pos); as K7's
        if (coins) return coins[(cnt * nvar + pos) * CB + tile];
        const uint32_t k = blk_key ^ (pos * 0x9E3779B1u) ^ ((uint32_t)cnt * 0x7FEB352Du + 0x165667B1u);
        return ((uint64_t)k7_fmix32(k ^ 0x4C4F4353u) << 32) | k7_fmix32(k + 0x27D4EB2Fu);
    };
    for (int64_t cnt = 0; cnt < num_ls; ++cnt) {
        for (int64_t k = 0; k < G; ++k) {
            const uint32_t lp = (uint32_t)lv_ptr[k];
            if (lp >> 31) __syncthreads();            // a new level (k = 0: the tile is loaded / the pass before is complete)
            if ((int)(k % W) != w) continue;
            const int64_t p0 = (int64_t)(lp & 0xFFFFFFu) * 64, p1 = (int64_t)((uint32_t)lv_ptr[k + 1] & 0xFFFFFFu) * 64;
            const bool wtd = (lp >> 30) & 1u;
            const int planes = (int)((lp >> 24) & 31u);
            const int blocks = (int)((p1 - p0 - 128) / (wtd ? 512 : 256));
            const int32_t* rec = data + p0;
            const uint2 hh = *reinterpret_cast<const uint2*>(rec + 2 * lane);
            const u32x4 e = *reinterpret_cast<const u32x4*>(rec + 128 + 4 * lane);
            const u32x4 wt = *reinterpret_cast<const u32x4*>(rec + 128 + (wtd ? 256 : 0) + 4 * lane);
            const bool live = hh.x < (uint32_t)nvar;
            const uint32_t var = live ? hh.x : (uint32_t)nvar;
            const uint64_t x = words[var];
            const uint64_t coin = coin_word(cnt, live ? hh.y : 0u);
            uint64_t flip;
            if (!wtd) {
                if (planes <= 3) flip = ms_group<3, false>(words, nvar, rec, blocks, e, wt, x, coin, lane);
                else if (planes <= 5) flip = ms_group<5, false>(words, nvar, rec, blocks, e, wt, x, coin, lane);
                else if (planes <= 8) flip = ms_group<8, false>(words, nvar, rec, blocks, e, wt, x, coin, lane);
                else if (planes <= 12) flip = ms_group<12, false>(words, nvar, rec, blocks, e, wt, x, coin, lane);
                else flip = ms_group<24, false>(words, nvar, rec, blocks, e, wt, x, coin, lane);
            } else {
                if (planes <= 8) flip = ms_group<8, true>(words, nvar, rec, blocks, e, wt, x, coin, lane);
                else if (planes <= 14) flip = ms_group<14, true>(words, nvar, rec, blocks, e, wt, x, coin, lane);
                else flip = ms_group<24, true>(words, nvar, rec, blocks, e, wt, x, coin, lane);
            }
            if (live) words[var] = x ^ flip;
        }
    }
    __syncthreads();
    if (C - c0 < kWave) {                             // a ragged last tile: the bits of chains past C stay zero (the layout's rule)
        const uint64_t keep = (1ull << (C - c0)) - 1ull;
        for (int64_t i = threadIdx.x; i < nvar; i += W * kWave) words[i] &= keep;
        __syncthreads();
    }
    // the score: expected[c] = -S[c] = (weight of the non-empty clauses) - 2 (weight of the satisfied ones)
    int acc = 0, all = 0;
    for (int64_t m0 = (int64_t)w * kWave; m0 < M; m0 += (int64_t)W * kWave) {
        const int64_t m = m0 + lane;
        uint64_t sat = 0;
        int wm = 0;
        if (m < M) {
            const int32_t a = clause_ptr[m], b = clause_ptr[m + 1];
            if (b > a) wm = weight ? weight[m] : 1;
            for (int32_t q = a; q < b; ++q) {
                const int32_t l = lit[q];
                const uint32_t v = (uint32_t)(l < 0 ? -l : l) - 1u;
                if (v < (uint32_t)nvar) sat |= words[v] ^ (uint64_t)((int64_t)l >> 63);
            }
        }
        const uint32_t lo = (uint32_t)sat, hi = (uint32_t)(sat >> 32);
#pragma unroll 8
        for (int j = 0; j < kWave; ++j) {
            const uint32_t sl = (uint32_t)__builtin_amdgcn_readlane((int)lo, j), sh = (uint32_t)__builtin_amdgcn_readlane((int)hi, j);
            const int wj = __builtin_amdgcn_readlane(wm, j);
            const uint32_t bit = ((lane < 32 ? sl : sh) >> (lane & 31)) & 1u;
            acc += bit ? wj : 0;
            all += wj;
        }
    }
    atomicAdd(&slots[lane], acc);
    if (lane == 0) atomicAdd(&slots[kWave], all);
    __syncthreads();
    if (w == 0 && c < C) expected[c] = (float)(slots[kWave] - 2 * slots[lane]);
    if constexpr (std::is_same<TO, Packed64>::value) {
        tile_store_packed(xs_out, nvar, tile, words, threadIdx.x, W * kWave);
    } else {
        if (c < C) {
            const uint32_t* w32 = reinterpret_cast<const uint32_t*>(smem);
            const int half = lane >> 5, sh = lane & 31;
            for (int64_t n = w; n < nvar; n += W) xs_out[n * C + c] = (float)((w32[(n << 1) + half] >> sh) & 1u);
        }
    }
}

}  // namespace rls

using namespace rls;

extern "C" {

int rls_maxsat_local_search(const void* xs_in, int64_t C_in, void* xs_out, int out_spin_bytes, int64_t C, int64_t nvar,
                            const int32_t* lv_ptr, const int32_t* lv_data, int64_t num_groups, int64_t num_ls,
                            const uint64_t* coins, uint64_t seed, const int32_t* clause_ptr, const int32_t* lit,
                            const int32_t* weight, int64_t M, float* expected, const rls_chain_ids* chain_ids, void* stream) {
    RLS_REQUIRE(C >= 0 && num_ls >= 0 && nvar >= 1 && M >= 0 && num_groups >= 1, RLS_EINVAL, "bad sizes");
    int64_t max_nvar = 0;
    RLS_REQUIRE(rls_maxsat_local_search_supported(nvar, 0, &max_nvar, nullptr), RLS_EUNSUPPORTED,
                "nvar=%lld: the 64-chain tile holds at most %lld variables in LDS", (long long)nvar, (long long)max_nvar);
    if (C == 0) return RLS_OK;
    ChainIds ids;
    dim3 grid;
    if (int rc = chain_ids_arg(chain_ids, C, ids, grid)) return rc;
    RLS_REQUIRE((ids.offset & (kWave - 1)) == 0 && (ids.skip & (kWave - 1)) == 0, RLS_EINVAL,
                "chain_ids: this kernel draws per 64-chain tile; offset, period and skip must be multiples of 64");
    RLS_REQUIRE(xs_in && xs_out && lv_ptr && lv_data && clause_ptr && expected && (lit || M == 0), RLS_EINVAL, "NULL pointer");
    RLS_REQUIRE(out_spin_bytes == 0 || out_spin_bytes == 4, RLS_EINVAL, "out_spin_bytes must be 0 (bit-packed) or 4 (float32)");
    if (C_in <= 0) C_in = C;
    RLS_REQUIRE(C_in == C || (C_in % kWave == 0 && C_in < C), RLS_EINVAL, "broadcast input (C_in != C) needs C_in a multiple of 64 below C");
    RLS_REQUIRE(xs_in != xs_out || (out_spin_bytes == 0 && C_in == C), RLS_EINVAL, "in-place needs a bit-packed output of C_in == C chains");
    const size_t lds = (((size_t)(nvar + 1) * 8 + 15) & ~(size_t)15) + 272;
    const int64_t tiles_in = ceil_div(C_in, kWave);
    hipStream_t s = as_stream(stream);
    with_bool(out_spin_bytes == 0, [&](auto packed) {
        using TO = std::conditional_t<decltype(packed)::value, Packed64, float>;
        auto kern = k_maxsat_local_search<TO>;
        ensure_dyn_lds((const void*)kern, lds);
        hipLaunchKernelGGL(kern, grid, dim3(kMsWaves * kWave), lds, s, (const uint64_t*)xs_in, (typename ChainStore<TO>::type*)xs_out, nvar, C,
                           tiles_in, lv_ptr, lv_data, num_groups, num_ls, coins, seed, clause_ptr, lit, weight, M, expected, ids);
    });
    return check_launch("k_maxsat_local_search");
}

}  // extern "C"
