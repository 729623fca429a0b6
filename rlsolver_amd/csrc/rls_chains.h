// Bit-packed chain tiles, the global chain ids of a shard and the counter hash of the production draws: what the MCPG kernels
// (rls_mcpg.hip) and the MaxSAT sampler (rls_maxsat.hip) share.  Internal; the layouts are those of include/rlsolver_hip.h.
#pragma once
#include "rls_common.h"

namespace rls {

// ---- bit-packed chains ("spin_bytes = 0"): tile-major uint64 [ceil(C / 64), N]; word (t, n) holds node n of the chains
// 64 t .. 64 t + 63 (bit e = chain 64 t + e).  A 64-chain tile is N CONSECUTIVE words: the LDS tile is a straight
// copy (16-byte lanes), 1/32 of the f32 node-major surface's bytes.  tiles_in < tiles broadcasts: tile t reads
// tile t % tiles_in (the reference's  xs_bool = temp_max_info.repeat(1, repeat_times)  without materialising it).
struct Packed64 {};
template <typename T> struct ChainStore { using type = T; };
template <> struct ChainStore<Packed64> { using type = uint64_t; };

__device__ __forceinline__ void tile_load_packed(const uint64_t* __restrict__ x, int64_t N, int64_t C, int64_t tile,
                                                 int64_t tiles_in, uint64_t* __restrict__ words, int tid, int nthreads) {
    const uint64_t* src = x + (tile % tiles_in) * N;
    const int64_t left = C - tile * kWave;
    const uint64_t live = left >= kWave ? ~0ull : ((1ull << left) - 1ull);   // chains past C read as 0
    if ((N & 1) == 0 && (((uintptr_t)src) & 15) == 0) {
        typedef uint64_t u64x2 __attribute__((ext_vector_type(2)));
        const u64x2* s2 = reinterpret_cast<const u64x2*>(src);
        u64x2* d2 = reinterpret_cast<u64x2*>(words);
        const u64x2 m{live, live};
#pragma unroll 4
        for (int64_t i = tid; i < N / 2; i += nthreads) d2[i] = s2[i] & m;
    } else {
        for (int64_t i = tid; i < N; i += nthreads) words[i] = src[i] & live;
    }
}

__device__ __forceinline__ void tile_store_packed(uint64_t* __restrict__ x, int64_t N, int64_t tile,
                                                  const uint64_t* __restrict__ words, int tid, int nthreads) {
    uint64_t* dst = x + tile * N;
    if ((N & 1) == 0 && (((uintptr_t)dst) & 15) == 0) {
        typedef uint64_t u64x2 __attribute__((ext_vector_type(2)));
        const u64x2* s2 = reinterpret_cast<const u64x2*>(words);
        u64x2* d2 = reinterpret_cast<u64x2*>(dst);
#pragma unroll 4
        for (int64_t i = tid; i < N / 2; i += nthreads) d2[i] = s2[i];
    } else {
        for (int64_t i = tid; i < N; i += nthreads) dst[i] = words[i];
    }
}

// murmur3's 32-bit finaliser: the counter-based generator of the production paths of K7 and K9 (two hashes
// per draw pair instead of a 10-round Philox, which was 70 % of a K9 round on its single walking wave)
__device__ __forceinline__ uint32_t k7_fmix32(uint32_t h) {
    h ^= h >> 16; h *= 0x85EBCA6Bu; h ^= h >> 13; h *= 0xC2B2AE35u; h ^= h >> 16;
    return h;
}

// Global id of local chain c (rls_chain_ids): the key of every counter-based draw, so that a rank's shard of the chains
// draws exactly what those chains draw in an unsharded run.  period > 0: the local batch is repeats of `period` kept
// chains (chain c = repeat c / period of kept chain c % period) cut out of a global batch whose repeats are period + skip
// chains apart.  No division in the kernels: in that mode the launch is TWO-dimensional -- blockIdx.y = the repeat,
// blockIdx.x = the 64-chain tile inside it (period a multiple of 64) -- and a kernel's linear tile index is mcpg_tile().
struct ChainIds {
    int64_t offset, skip;
    __device__ __forceinline__ int64_t operator()(int64_t c) const { return offset + c + (int64_t)blockIdx.y * skip; }
};
__device__ __forceinline__ int64_t mcpg_tile() { return (int64_t)blockIdx.y * gridDim.x + blockIdx.x; }

// rls_chain_ids -> the kernels' by-value form + the launch grid for C chains; NULL = the identity (a single-process run, 1-D grid)
inline int chain_ids_arg(const rls_chain_ids* in, int64_t C, ChainIds& out, dim3& grid) {
    out = ChainIds{0, 0};
    grid = dim3((unsigned)ceil_div(C, kWave));
    if (!in) return RLS_OK;
    RLS_REQUIRE(in->offset >= 0 && in->period >= 0 && in->skip >= 0, RLS_EINVAL, "chain_ids: negative offset / period / skip");
    out.offset = in->offset;
    if (in->period > 0 && in->skip > 0) {
        // repeats of `period` chains: one grid row per repeat (no division on the device)
        RLS_REQUIRE((in->period & (kWave - 1)) == 0 && C % in->period == 0 && C / in->period < 65536, RLS_EINVAL,
                    "chain_ids: period=%lld must be a multiple of 64 that divides C=%lld (fewer than 65536 repeats)", (long long)in->period,
                    (long long)C);
        out.skip = in->skip;
        grid = dim3((unsigned)(in->period / kWave), (unsigned)(C / in->period));
    }
    return RLS_OK;
}

}  // namespace rls
