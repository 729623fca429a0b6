// Edge-flip MaxCut sampler of the MCPG package for gfx950: the gauge fix, the edge-sequential sweep and the score of
// mcpg_sampling_maxcut_edge (methods/MCPG/sampling.py:141-172) in one kernel.
//
// Lane = chain.  A workgroup is ONE wave and owns one 64-chain tile, uint64 [N] node-major bit words in LDS; beside it sits a
// bitmap of the nodes a visit has written (the float32 output keeps the reference's -0.5 | 1.5 at a node that never was).  A
// visit sets both endpoints of an edge from the two neighbour sums, and every earlier visit has changed what those sums read:
// the sweep is sequential per chain in visiting order.  The visited edge, its three constants and both neighbour rows are
// wave-uniform -- they come from the flat visit stream through scalar loads -- and a neighbour's word is one broadcast LDS read
// of the 32-bit half the lane sits in, its bit one bit-field extract.  The sums are counted in integers (2 t = sum of
// w (fresh ? 4 x - 1 : 2 x)) and converted once; the noise and the `add` terms round as the reference's float32 expression
// does, one rounding per operation (the library is built without contraction).  The 64 decisions of a visit go back as one
// ballot per endpoint.
#include "rls_chains.h"
#include "rls_tile.h"

namespace rls {

constexpr int64_t kEdgeExact = 1ll << 24;               // integers (and half-integers) below it are exact in float32
constexpr int kEdgeHdr = 7;                             // r, c, len_r, len_c, add0, add1, add2

constexpr size_t edge_tile_bytes(int64_t N) { return ((size_t)N * 8 + 15) & ~(size_t)15; }
constexpr size_t edge_lds_bytes(int64_t N) { return edge_tile_bytes(N) + (size_t)((N + 31) / 32) * 4; }
constexpr int64_t edge_max_nodes() {                    // the largest N whose tile + bitmap fit
    int64_t n = kLdsBytes / 8;
    while (edge_lds_bytes(n) > (size_t)kLdsBytes) --n;
    return n;
}
constexpr int64_t kEdgeMaxN = edge_max_nodes();
static_assert(kEdgeMaxN == 20164, "include/rlsolver_hip.h: RLS_MAXCUT_EDGE_MAX_NODES");

template <typename TO>
__global__ __launch_bounds__(kWave) void k_maxcut_edge_local_search(
    const uint64_t* xs_in, typename ChainStore<TO>::type* xs_out, int64_t N, int64_t C, int64_t tiles_in,
    const int32_t* __restrict__ eu, const int32_t* __restrict__ ev, const int32_t* __restrict__ ew, int64_t E,
    const int32_t* __restrict__ vs, int64_t vs_len, int gauge_node, int64_t num_ls, const float* __restrict__ uniforms, uint64_t seed,
    float* __restrict__ expected, ChainIds ids) {
    extern __shared__ __attribute__((aligned(16))) unsigned char smem[];
    const int lane = threadIdx.x;
    const int64_t tile = mcpg_tile(), c = tile * kWave + lane;
    uint64_t* words = reinterpret_cast<uint64_t*>(smem);
    uint32_t* w32 = reinterpret_cast<uint32_t*>(smem);     // word n of the tile = w32[2 n] (chains 0..31), w32[2 n + 1] (32..63)
    uint32_t* written = reinterpret_cast<uint32_t*>(smem + edge_tile_bytes(N));
    const uint32_t un = (uint32_t)N;
    tile_load_packed(xs_in, N, C, tile, tiles_in, words, lane, kWave);
    for (uint32_t i = lane; i < (un + 31u) / 32u; i += kWave) written[i] = 0u;
    __syncthreads();
    if (gauge_node >= 0) {                                  // graph_probs = (graph_probs + graph_probs[hub]) % 2   (sampling.py:142-144)
        const uint64_t hub = words[gauge_node];
        __syncthreads();
        for (uint32_t n = lane; n < un; n += kWave) words[n] ^= hub;
        __syncthreads();
    }
    const int half = lane >> 5, sh = lane & 31;
    const bool live = c < C;                                // chains past C read as zero, stay zero and write nothing
    const int64_t gc = ids(c);                              // the chain's global id
    const uint32_t chain_key = k7_fmix32((uint32_t)seed ^ k7_fmix32((uint32_t)(seed >> 32) ^ k7_fmix32((uint32_t)gc) ^
                                                                    ((uint32_t)((uint64_t)gc >> 32) * 0x9E3779B1u)));
    for (int64_t pass = 0; pass < num_ls; ++pass) {
        const bool pass0 = pass == 0;
        int64_t p = 0;
        for (int64_t i = 0; i < E && p + kEdgeHdr <= vs_len; ++i) {
            const uint32_t r = (uint32_t)vs[p], cn = (uint32_t)vs[p + 1], len_r = (uint32_t)vs[p + 2], len_c = (uint32_t)vs[p + 3];
            const int64_t pairs = (int64_t)len_r + (int64_t)len_c;
            if (r >= un || cn >= un || p + kEdgeHdr + 2 * pairs > vs_len) break;      // a stream that does not describe this graph
            const float add0 = __int_as_float(vs[p + 4]), add1 = __int_as_float(vs[p + 5]), add2 = __int_as_float(vs[p + 6]);
            const int32_t* nb = vs + p + kEdgeHdr;
            p += kEdgeHdr + 2 * pairs;
            // 2 t = sum_k w_k (fresh_k ? 4 x_k - 1 : 2 x_k): a node holds 2 x - 0.5 until its first write (fresh: pass 0 only).  The
            // -w_k of the fresh entries are the same for every chain: they add up on the scalar side; a lane adds w_k << (1 + fresh)
            // where its bit is set (the bit sign-extended into a mask).
            auto twice_t = [&](auto p0, const int32_t* row, uint32_t len) -> int {   // p0: pass 0, the one that reads `fresh`
                int acc = 0, base = 0;
#pragma unroll 8
                for (uint32_t j = 0; j < len; ++j) {
                    const uint32_t e = (uint32_t)row[2 * j];
                    const int wj = row[2 * j + 1];
                    const uint32_t f = decltype(p0)::value ? e >> 31 : 0u;
                    uint32_t v = e & 0x7fffffffu;
                    v = v < un ? v : un - 1u;                                    // (clamped: a broken row reads inside the tile)
                    acc += __builtin_amdgcn_sbfe((int)w32[2 * v + half], sh, 1) & (wj << (1u + f));
                    base -= (int)f * wj;
                }
                return acc + base;
            };
            const int32_t* nb_c = nb + 2 * (int64_t)len_r;
            const int t2_r = pass0 ? twice_t(std::true_type{}, nb, len_r) : twice_t(std::false_type{}, nb, len_r);
            const int t2_c = pass0 ? twice_t(std::true_type{}, nb_c, len_c) : twice_t(std::false_type{}, nb_c, len_c);
            const float t_r = (float)t2_r * 0.5f, t_c = (float)t2_c * 0.5f;
            float u0, u1, u2;
            if (uniforms) {
                const float* up = uniforms + ((pass * E + i) * 3) * C + (live ? c : 0);
                u0 = up[0], u1 = up[C], u2 = up[2 * C];
            } else {
                const uint32_t k = chain_key ^ ((uint32_t)i * 0x9E3779B1u) ^ ((uint32_t)pass * 0x7FEB352Du + 0x165667B1u);
                u0 = u32_to_unit_float(k7_fmix32(k + 0x27D4EB2Fu));
                u1 = u32_to_unit_float(k7_fmix32(k + 2u * 0x27D4EB2Fu));
                u2 = u32_to_unit_float(k7_fmix32(k + 3u * 0x27D4EB2Fu));
            }
            const float a = (t_r + u0 * 0.1f) + add0;                            // temp[1]   sampling.py:163
            const float b = (t_c + u1 * 0.1f) + add1;                            // temp[2]   :164
            const float z = ((a + b) + u2 * 0.1f) - add2;                        // temp[0]   :165
            uint32_t k = 0;                                                      // first maximum of (z, a, b, 0)   :166
            float best = z;
            if (a > best) { best = a; k = 1; }
            if (b > best) { best = b; k = 2; }
            if (0.0f > best) k = 3;
            const uint64_t mr = ballot64(live && (k >> 1) != 0u), mc = ballot64(live && (k & 1u) != 0u);
            if (sh == 0) w32[2 * r + half] = (uint32_t)(half ? mr >> 32 : mr);   // graph_probs[node_r] = floor(k / 2)   :167
            __builtin_amdgcn_wave_barrier();
            if (sh == 0) w32[2 * cn + half] = (uint32_t)(half ? mc >> 32 : mc);  // graph_probs[node_c] = k % 2: wins on a loop   :168
            if (pass0 && lane == 0) {
                written[r >> 5] |= 1u << (r & 31u);
                written[cn >> 5] |= 1u << (cn & 31u);
            }
            __builtin_amdgcn_wave_barrier();
        }
    }
    __syncthreads();
    // expected = sum_e w_e (2 x_u - 1)(2 x_v - 1) over the stored edges   (:172)
    int total = 0;
#pragma unroll 4
    for (int64_t e = 0; e < E; ++e) {                       // (endpoints clamped: a broken edge list reads inside the tile)
        uint32_t u = (uint32_t)eu[e], v = (uint32_t)ev[e];
        u = u < un ? u : un - 1u;
        v = v < un ? v : un - 1u;
        const int we = ew[e];
        total += (((w32[2 * u + half] ^ w32[2 * v + half]) >> sh) & 1u) ? -we : we;
    }
    if (live) expected[c] = (float)total;
    if constexpr (std::is_same<TO, Packed64>::value) {
        tile_store_packed(xs_out, N, tile, words, lane, kWave);
    } else {
        if (live)
            for (uint32_t n = 0; n < un; ++n) {
                const float x = (float)((w32[2 * n + half] >> sh) & 1u);
                xs_out[(int64_t)n * C + c] = ((written[n >> 5] >> (n & 31u)) & 1u) ? x : 2.0f * x - 0.5f;   // (x - 0.5) * 2 + 0.5   :145
            }
    }
}

}  // namespace rls

using namespace rls;

extern "C" {

int rls_maxcut_edge_local_search_supported(int64_t N, int64_t E, int64_t max_abs_degree, int64_t weight_abs_sum, int64_t stream_len,
                                           int64_t* max_N) {
    if (max_N) *max_N = kEdgeMaxN;
    return N >= 1 && N <= kEdgeMaxN && E >= 0 && max_abs_degree >= 0 && max_abs_degree < kEdgeExact && 3 * max_abs_degree < kEdgeExact &&
           weight_abs_sum >= 0 && weight_abs_sum < kEdgeExact && stream_len >= 0 && stream_len < (1ll << 31);
}

int rls_maxcut_edge_local_search(const rls_graph* g, const int32_t* edge_weights, const void* xs_in, int64_t C_in, void* xs_out,
                                 int out_spin_bytes, int64_t C, const int32_t* visit_stream, int64_t stream_len, int64_t max_abs_degree,
                                 int64_t weight_abs_sum, int gauge_node, int64_t num_ls, const float* uniforms, uint64_t seed,
                                 float* expected, const rls_chain_ids* chain_ids, void* stream) {
    if (int rc = check_graph(g)) return rc;
    const int64_t N = g->num_nodes, E = g->num_stored_edges;
    RLS_REQUIRE(C >= 0 && num_ls >= 0, RLS_EINVAL, "bad sizes");
    int64_t max_N = 0;
    RLS_REQUIRE(rls_maxcut_edge_local_search_supported(N, E, max_abs_degree, weight_abs_sum, stream_len, &max_N), RLS_EUNSUPPORTED,
                "N=%lld, E=%lld, max |weighted degree|=%lld, |weights| sum=%lld, stream of %lld words: the 64-chain tile and its bitmap "
                "hold at most %lld nodes in LDS, 3 max |weighted degree| and the |weights| sum must stay below 2^24 (exact float32), the "
                "stream below 2^31 words", (long long)N, (long long)E, (long long)max_abs_degree, (long long)weight_abs_sum,
                (long long)stream_len, (long long)max_N);
    RLS_REQUIRE(stream_len >= kEdgeHdr * E, RLS_EINVAL, "visit stream of %lld words, this graph's has at least 7 E = %lld",
                (long long)stream_len, (long long)(kEdgeHdr * E));
    RLS_REQUIRE(gauge_node >= -1 && gauge_node < N, RLS_EINVAL, "gauge_node=%d must be a node or -1", gauge_node);
    if (C == 0) return RLS_OK;
    RLS_REQUIRE(xs_in && xs_out && expected && (visit_stream || stream_len == 0) && (edge_weights || E == 0), RLS_EINVAL, "NULL pointer");
    RLS_REQUIRE(out_spin_bytes == 0 || out_spin_bytes == 4, RLS_EINVAL, "out_spin_bytes must be 0 (bit-packed) or 4 (float32)");
    if (C_in <= 0) C_in = C;
    RLS_REQUIRE(C_in == C || (C_in % kWave == 0 && C_in < C), RLS_EINVAL, "broadcast input (C_in != C) needs C_in a multiple of 64 below C");
    RLS_REQUIRE(xs_in != xs_out || (out_spin_bytes == 0 && C_in == C), RLS_EINVAL, "in-place needs a bit-packed output of C_in == C chains");
    ChainIds ids;
    dim3 grid;
    if (int rc = chain_ids_arg(chain_ids, C, ids, grid)) return rc;
    const int64_t tiles_in = ceil_div(C_in, kWave);
    RLS_REQUIRE(ceil_div(C, kWave) < (1ll << 31), RLS_EINVAL, "too many chains");
    const size_t lds = edge_lds_bytes(N);
    hipStream_t s = as_stream(stream);
    with_bool(out_spin_bytes == 0, [&](auto packed) {
        using TO = std::conditional_t<decltype(packed)::value, Packed64, float>;
        auto kern = k_maxcut_edge_local_search<TO>;
        ensure_dyn_lds((const void*)kern, lds);
        hipLaunchKernelGGL(kern, grid, dim3(kWave), lds, s, (const uint64_t*)xs_in, (typename ChainStore<TO>::type*)xs_out, N, C, tiles_in, g->eu,
                           g->ev, edge_weights, E, visit_stream, stream_len, gauge_node, num_ls, uniforms, seed, expected, ids);
    });
    return check_launch("k_maxcut_edge_local_search");
}

}  // extern "C"
