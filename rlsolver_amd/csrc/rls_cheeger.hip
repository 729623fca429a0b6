// Cheeger-cut samplers of the MCPG package for gfx950: the node-sequential sweep and the score of mcpg_sampling_rcheegercut /
// mcpg_sampling_ncheegercut (methods/MCPG/sampling.py:181-250) in one kernel.
//
// Lane = chain.  A workgroup is ONE wave and owns one 64-chain tile, uint64 [N] node-major bit words in LDS (nothing else is kept
// there); cut, size and h of the lane's chain live in registers.  The decision at a node reads all three, and every earlier flip
// of the pass has changed them: the sweep is sequential per chain in visiting order, no level schedule applies.  The visited
// node and its neighbour list are wave-uniform -- they come from the flat visit stream through scalar loads -- and a neighbour's
// word is one broadcast LDS read of the 32-bit half the lane sits in, its bit one bit-field extract.  The 64 decisions of a visit
// go back into the node's word as one ballot.
#include "rls_chains.h"
#include "rls_tile.h"

namespace rls {

constexpr int64_t kCheegerMaxN = kLdsBytes / 8;          // the tile alone fills the LDS: 20 480 nodes
constexpr int64_t kCheegerExact = 1ll << 24;             // integers (and half-integers) below it are exact in float32

template <bool NORMALIZED>
__device__ __forceinline__ float cheeger_value(float cut, float size, float n) {
    const float rest = n - size;
    if constexpr (NORMALIZED) return cut * (1.0f / size + 1.0f / rest);                 // sampling.py:229, :237
    else return cut / (size < rest ? size : rest);                                       // sampling.py:193, :201
}

template <typename TO, bool NORMALIZED>
__global__ __launch_bounds__(kWave) void k_cheeger_local_search(
    const uint64_t* xs_in, typename ChainStore<TO>::type* xs_out, int64_t N, int64_t C, int64_t tiles_in,
    const int32_t* __restrict__ eu, const int32_t* __restrict__ ev, int64_t E, const int32_t* __restrict__ vs, int64_t vs_len,
    int64_t num_ls, float edge_weight_sum, float* __restrict__ h_out, float* __restrict__ cut_out, float* __restrict__ size_out) {
    extern __shared__ __attribute__((aligned(16))) unsigned char smem[];
    const int lane = threadIdx.x;
    const int64_t tile = blockIdx.x, c = tile * kWave + lane;
    tile_load_packed(xs_in, N, C, tile, tiles_in, reinterpret_cast<uint64_t*>(smem), lane, kWave);
    __syncthreads();
    uint32_t* w32 = reinterpret_cast<uint32_t*>(smem);     // word n of the tile = w32[2 n] (chains 0..31), w32[2 n + 1] (32..63)
    const int half = lane >> 5, sh = lane & 31;
    const uint32_t un = (uint32_t)N;
    // size = sum_v x_v; sum_e s_u s_v = E - 2 (cut edges), an integer pass over the stored edge list (a loop is never cut)
    int cnt = 0;
    for (uint32_t n = 0; n < un; ++n) cnt += (int)((w32[2 * n + half] >> sh) & 1u);
    int cut_edges = 0;
#pragma unroll 8
    for (int64_t e = 0; e < E; ++e) {                        // (endpoints clamped: a broken edge list reads inside the tile)
        uint32_t u = (uint32_t)eu[e], v = (uint32_t)ev[e];
        u = u < un ? u : un - 1u;
        v = v < un ? v : un - 1u;
        cut_edges += (int)(((w32[2 * u + half] ^ w32[2 * v + half]) >> sh) & 1u);
    }
    const float nf = (float)N;
    float size = (float)cnt;
    float cut = (edge_weight_sum - (float)((int)E - 2 * cut_edges)) / 2.0f;                // sampling.py:190-191
    float h = cheeger_value<NORMALIZED>(cut, size, nf);
    const bool live = c < C;                                 // chains past C stay zero: they never flip and write nothing
    for (int64_t pass = 0; pass < num_ls; ++pass) {
        int64_t p = 0;
        for (uint32_t k = 0; k < un && p + 3 <= vs_len; ++k) {
            const uint32_t node = (uint32_t)vs[p], deg = (uint32_t)vs[p + 1];
            const float wdeg = (float)vs[p + 2];
            if (node >= un || p + 3 + (int64_t)deg > vs_len) break;            // a stream that does not describe this graph
            const int32_t* nb = vs + p + 3;
            p += 3 + (int64_t)deg;
            int cn = 0;                                      // c = sum of x over the neighbour row, with multiplicity
#pragma unroll 4
            for (uint32_t j = 0; j < deg; ++j) {
                uint32_t v = (uint32_t)nb[j];
                v = v < un ? v : node;
                cn += (int)((w32[2 * v + half] >> sh) & 1u);
            }
            const uint32_t xw = w32[2 * node + half];
            const float s = ((xw >> sh) & 1u) ? 1.0f : -1.0f;                    // 2 x - 1
            const float ncut = cut - s * (wdeg - 2.0f * (float)cn);
            const float nsize = size - s;
            const float nh = cheeger_value<NORMALIZED>(ncut, nsize, nf);
            const float nrest = nf - nsize;
            const bool keep = (h < nh) || ((nsize < nrest ? nsize : nrest) < 0.0000001f);
            const bool flip = live && !keep;
            const uint64_t fm = ballot64(flip);
            if (fm != 0ull) {                                 // (wave-uniform)
                if (sh == 0) w32[2 * node + half] = xw ^ (uint32_t)(half ? fm >> 32 : fm);
                __builtin_amdgcn_wave_barrier();
            }
            cut = flip ? ncut : cut;
            size = flip ? nsize : size;
            h = flip ? nh : h;
        }
    }
    if (live) {
        h_out[c] = h;
        if (cut_out) cut_out[c] = cut;
        if (size_out) size_out[c] = size;
    }
    __syncthreads();
    if constexpr (std::is_same<TO, Packed64>::value) {
        tile_store_packed(xs_out, N, tile, reinterpret_cast<const uint64_t*>(smem), lane, kWave);
    } else {
        if (live)
            for (uint32_t n = 0; n < un; ++n) xs_out[(int64_t)n * C + c] = (float)((w32[2 * n + half] >> sh) & 1u);
    }
}

}  // namespace rls

using namespace rls;

extern "C" {

int rls_cheeger_local_search_supported(int64_t N, int64_t E, int64_t weight_abs_sum, int64_t* max_N) {
    if (max_N) *max_N = kCheegerMaxN;
    return N >= 1 && N <= kCheegerMaxN && N < kCheegerExact && E >= 0 && weight_abs_sum >= 0 && weight_abs_sum + 2 * E < kCheegerExact;
}

int rls_cheeger_local_search(const rls_graph* g, const void* xs_in, int64_t C_in, void* xs_out, int out_spin_bytes, int64_t C,
                             const int32_t* visit_stream, int64_t stream_len, int normalized, int64_t num_ls, float edge_weight_sum,
                             float* h, float* cut, float* size, void* stream) {
    if (int rc = check_graph(g)) return rc;
    const int64_t N = g->num_nodes, E = g->num_stored_edges;
    RLS_REQUIRE(C >= 0 && num_ls >= 0, RLS_EINVAL, "bad sizes");
    RLS_REQUIRE(normalized == 0 || normalized == 1, RLS_EINVAL, "normalized must be 0 (ratio) or 1 (normalised)");
    int64_t max_N = 0;
    const float aw = edge_weight_sum < 0 ? -edge_weight_sum : edge_weight_sum;
    RLS_REQUIRE(aw == aw && aw < (float)kCheegerExact, RLS_EUNSUPPORTED, "edge_weight_sum=%g is outside the exact float32 range (2^24)", (double)edge_weight_sum);
    RLS_REQUIRE(rls_cheeger_local_search_supported(N, E, (int64_t)aw, &max_N), RLS_EUNSUPPORTED,
                "N=%lld, E=%lld, |edge_weight_sum|=%lld: the 64-chain tile holds at most %lld nodes in LDS, and the weights' "
                "absolute sum + 2 E must stay below 2^24 (exact float32)", (long long)N, (long long)E, (long long)aw, (long long)max_N);
    RLS_REQUIRE(stream_len == 3 * N + g->nnz, RLS_EINVAL, "visit stream of %lld words, this graph's has 3 N + nnz = %lld",
                (long long)stream_len, (long long)(3 * N + g->nnz));
    if (C == 0) return RLS_OK;
    RLS_REQUIRE(xs_in && xs_out && visit_stream && h, RLS_EINVAL, "NULL pointer");
    RLS_REQUIRE(out_spin_bytes == 0 || out_spin_bytes == 4, RLS_EINVAL, "out_spin_bytes must be 0 (bit-packed) or 4 (float32)");
    if (C_in <= 0) C_in = C;
    RLS_REQUIRE(C_in == C || (C_in % kWave == 0 && C_in < C), RLS_EINVAL, "broadcast input (C_in != C) needs C_in a multiple of 64 below C");
    RLS_REQUIRE(xs_in != xs_out || (out_spin_bytes == 0 && C_in == C), RLS_EINVAL, "in-place needs a bit-packed output of C_in == C chains");
    const int64_t tiles = ceil_div(C, kWave), tiles_in = ceil_div(C_in, kWave);
    RLS_REQUIRE(tiles < (1ll << 31), RLS_EINVAL, "too many chains");
    const size_t lds = (((size_t)N * 8 + 15) & ~(size_t)15);
    hipStream_t s = as_stream(stream);
    with_bool(out_spin_bytes == 0, [&](auto packed) {
        using TO = std::conditional_t<decltype(packed)::value, Packed64, float>;
        with_bool(normalized != 0, [&](auto nrm) {
            auto kern = k_cheeger_local_search<TO, decltype(nrm)::value>;
            ensure_dyn_lds((const void*)kern, lds);
            hipLaunchKernelGGL(kern, dim3((unsigned)tiles), dim3(kWave), lds, s, (const uint64_t*)xs_in, (typename ChainStore<TO>::type*)xs_out, N, C,
                               tiles_in, g->eu, g->ev, E, visit_stream, stream_len, num_ls, edge_weight_sum, h, cut, size);
        });
    });
    return check_launch("k_cheeger_local_search");
}

}  // extern "C"
