// The 32-env "half tile": words32[n] is a 32-bit word whose bit e is the spin of node n in env (b0 + e) -- N * 4 bytes of
// LDS instead of N * 8, for graphs past the 64-env tile (20 224 < N <= ~40 000: rls_tile.h keeps one word per node in LDS) and
// as twice as many, half as long workgroups where a launch has few tiles per CU.  The loaders and stores use the building blocks of
// rls_tile.h: a wave still turns 64 x 64 bits at a time -- lanes 0..31 hold the 32 envs' bytes of one 64-node block, lanes 32..63
// the SAME envs' bytes of the next block, so the transpose leaves lane p with (r0 = the 32 envs of node p in the first block, r1 =
// in the second): two words32 per lane and transpose, nothing wasted.
// This file holds only what is about the tile's width: kHalf, narrow_tile and the byte <-> bit corner turns.  The cut counter
// (rls_cutcount.h) and the level-parallel sweep (rls_sweep.h) take these tiles' words as they take 64-bit ones, on 32-bit planes
// (rls_planes.h).
#pragma once
#include "rls_tile.h"

namespace rls {

constexpr int kHalf = 32;   // envs per half tile

// Load the half tile of envs [b0, b0 + 32) x nodes [0, N) into words32[0..N).  W waves share the job (wave w takes every W-th
// 128-node chunk); callers sync afterwards.  `stage` = this wave's kStageBytes of LDS (16-byte aligned) or nullptr.
// Byte spins whose rows are 16-byte multiples on a 16-byte base (VEC) go through the row-piece stage when there is one -- an
// instruction fetches 8 rows x 128 B, whole cache lines; the wave turns the corner through 4 KB of LDS: lane l = (env l & 31,
// block l >> 5) reads back the four 16-byte pieces of ITS 64 nodes -- else each lane reads its 64 bytes itself; anything else
// (float spins, ragged rows) takes one ballot per node.
// 16 bytes of a byte row at offset `off` (a multiple of 16) of a row whose start is 16- (a16) or only 8-byte aligned (rows of 8-byte
// multiples: every other row starts mid-vector -- the Gset sizes 1000 ... 9000): one 16-byte access or two 8-byte ones; bytes at and
// past N are neither read nor written (with N % 16 == 8 the last piece is half a piece)
typedef uint32_t u32x2_t32 __attribute__((ext_vector_type(2)));
__device__ __forceinline__ u32x4 row_ld16(const uint8_t* p, bool a16, int64_t off, int64_t N) {
    if (a16) return *reinterpret_cast<const u32x4*>(p);
    const u32x2_t32 lo = *reinterpret_cast<const u32x2_t32*>(p);
    const u32x2_t32 hi = (off + 8 < N) ? *reinterpret_cast<const u32x2_t32*>(p + 8) : u32x2_t32{0, 0};
    return u32x4{lo.x, lo.y, hi.x, hi.y};
}
__device__ __forceinline__ void row_st16(uint8_t* p, bool a16, int64_t off, int64_t N, u32x4 v) {
    if (a16) { *reinterpret_cast<u32x4*>(p) = v; return; }
    *reinterpret_cast<u32x2_t32*>(p) = u32x2_t32{v.x, v.y};
    if (off + 8 < N) *reinterpret_cast<u32x2_t32*>(p + 8) = u32x2_t32{v.z, v.w};
}

template <bool XORW> __device__ __forceinline__ void put_word32(uint32_t* words32, int64_t n, uint32_t v) {
    if constexpr (XORW) words32[n] ^= v;   // (x ^ mask without a second tile: the same lane of the same wave owns a word in both passes)
    else words32[n] = v;
}

template <typename T, bool VEC, bool XORW = false>
__device__ __forceinline__ void tile32_load_bits(const T* __restrict__ x, int64_t B, int64_t N, int64_t b0,
                                                 uint32_t* __restrict__ words32, int lane, int w, int W, unsigned char* stage) {
    const int env = lane & (kHalf - 1), blk = lane >> 5;
    const int64_t b = b0 + env;
    const bool valid = b < B;
    if constexpr (VEC && sizeof(T) == 1) {
        if ((N & 7) == 0) {
            const bool a16 = (N & 15) == 0;
            const uint8_t* xb = reinterpret_cast<const uint8_t*>(x);
            const int64_t nchunk = (N + 127) >> 7;                       // 128-node chunks = one transpose each
            const BitXpose xc = bit_xpose_consts(lane);
            const int node = xc.node;                                    // the column -> node map of pack_bits
            if (stage != nullptr) {
                const int r = lane & 7, j = lane >> 3;                   // row within the instruction's 8, piece 0..7 of the row's 128 B
                constexpr int DEPTH = 2;
                for (int64_t ch0 = w; ch0 < nchunk; ch0 += (int64_t)W * DEPTH) {
                    u32x4 g[DEPTH][4];
#pragma unroll
                    for (int d = 0; d < DEPTH; ++d) {
                        const int64_t off = ((ch0 + (int64_t)d * W) << 7) + j * 16;
#pragma unroll
                        for (int i = 0; i < 4; ++i) {
                            const int64_t rw = b0 + 8 * i + r;
                            g[d][i] = (rw < B && off < N) ? row_ld16(xb + rw * N + off, a16, off, N) : u32x4{0, 0, 0, 0};
                        }
                    }
#pragma unroll
                    for (int d = 0; d < DEPTH; ++d) {
                        const int64_t ch = ch0 + (int64_t)d * W;
                        if (ch < nchunk) {
#pragma unroll
                            for (int i = 0; i < 4; ++i) *reinterpret_cast<u32x4*>(stage + (j * 32 + 8 * i + r) * 16) = g[d][i];
                            asm volatile("" ::: "memory");               // LDS ops of one wave execute in order
                            u32x4 v[4];
#pragma unroll
                            for (int q = 0; q < 4; ++q) v[q] = *reinterpret_cast<const u32x4*>(stage + ((4 * blk + q) * 32 + env) * 16);
                            asm volatile("" ::: "memory");
                            uint32_t r0 = pack_bits(v[0], v[1]), r1 = pack_bits(v[2], v[3]);
                            bit_transpose64(r0, r1, xc);
                            const int64_t n = (ch << 7) + node;
                            if (n < N) put_word32<XORW>(words32, n, r0);
                            if (n + 64 < N) put_word32<XORW>(words32, n + 64, r1);
                        }
                    }
                }
                return;
            }
            const uint8_t* rowb = xb + (valid ? b : 0) * N;
            for (int64_t ch = w; ch < nchunk; ch += W) {
                u32x4 v[4];
#pragma unroll
                for (int q = 0; q < 4; ++q) {
                    const int64_t off = ((ch << 3) + 4 * blk + q) << 4;
                    v[q] = (valid && off < N) ? row_ld16(rowb + off, a16, off, N) : u32x4{0, 0, 0, 0};
                }
                uint32_t r0 = pack_bits(v[0], v[1]), r1 = pack_bits(v[2], v[3]);
                bit_transpose64(r0, r1, xc);
                const int64_t n = (ch << 7) + node;
                if (n < N) put_word32<XORW>(words32, n, r0);
                if (n + 64 < N) put_word32<XORW>(words32, n + 64, r1);
            }
            return;
        }
    }
    // one ballot per node: lanes 0..31 = the half tile's envs (lanes 32..63 vote 0)
    const T* row = x + (valid ? b : 0) * N;
    for (int64_t n0 = (int64_t)w * 64; n0 < N; n0 += (int64_t)W * 64) {
        uint32_t mine = 0;
        const int lim = (int)((N - n0) < 64 ? (N - n0) : 64);
        for (int k = 0; k < lim; ++k) {
            const T v = (valid && blk == 0) ? row[n0 + k] : T(0);
            const uint32_t wd = (uint32_t)ballot64(spin_is_set(v));
            if (lane == k) mine = wd;
        }
        if (lane < lim) put_word32<XORW>(words32, n0 + lane, mine);
    }
}

// Write the half tile back as env-major bytes (0 | 1); rows with store_row == false stay untouched.  Every lane of the wave
// takes part whatever it stores.
template <bool VEC>
__device__ __forceinline__ void tile32_store_bytes(uint8_t* __restrict__ x, int64_t B, int64_t N, int64_t b0,
                                                   const uint32_t* __restrict__ words32, int lane, int w, int W, bool store_row,
                                                   unsigned char* stage = nullptr) {
    const int env = lane & (kHalf - 1), blk = lane >> 5;
    const int64_t b = b0 + env;
    const bool valid = b < B && store_row;
    uint8_t* row = x + (b < B ? b : 0) * N;
    const bool a16 = (N & 15) == 0;
    if constexpr (VEC) {
        if ((N & 7) == 0 && stage != nullptr) {
            // through the row-piece stage (the loader's corner turn backwards): lane l = (env, block) parks its four 16-byte pieces,
            // instruction i then writes rows 8 i .. 8 i + 7 as 128-byte runs (lane -> row 8 i + (l & 7), piece l >> 3)
            const uint32_t rows_ok = (uint32_t)ballot64(valid && blk == 0);
            const int64_t nchunk = (N + 127) >> 7;
            const BitXpose xc = bit_xpose_consts(lane);
            const int r = lane & 7, j = lane >> 3;
            for (int64_t ch = w; ch < nchunk; ch += W) {
                const int64_t n = (ch << 7) + xc.node;
                uint32_t r0 = (n < N) ? words32[n] : 0u, r1 = (n + 64 < N) ? words32[n + 64] : 0u;
                bit_transpose64(r0, r1, xc);
                u32x4 v[4];
                unpack_bits(r0, v[0], v[1]);
                unpack_bits(r1, v[2], v[3]);
#pragma unroll
                for (int q = 0; q < 4; ++q) *reinterpret_cast<u32x4*>(stage + ((4 * blk + q) * 32 + env) * 16) = v[q];
                asm volatile("" ::: "memory");   // LDS ops of one wave execute in order
                const int64_t off = (ch << 7) + j * 16;
#pragma unroll
                for (int i = 0; i < 4; ++i) {
                    const int rr = 8 * i + r;
                    const u32x4 o = *reinterpret_cast<const u32x4*>(stage + (j * 32 + rr) * 16);
                    if (((rows_ok >> rr) & 1u) && off < N) row_st16(x + (b0 + rr) * N + off, a16, off, N, o);
                }
                asm volatile("" ::: "memory");
            }
            return;
        }
        if ((N & 7) == 0) {
            // inverse of the load: lane p fetches the two words of node p (blocks 2c, 2c + 1), the transpose hands lane l = (env,
            // block) that env's 64 bits of that block, unpacked to 64 bytes = four 16-byte stores
            const int64_t nchunk = (N + 127) >> 7;
            const BitXpose xc = bit_xpose_consts(lane);
            for (int64_t ch = w; ch < nchunk; ch += W) {
                const int64_t n = (ch << 7) + xc.node;
                uint32_t r0 = (n < N) ? words32[n] : 0u, r1 = (n + 64 < N) ? words32[n + 64] : 0u;
                bit_transpose64(r0, r1, xc);
                u32x4 v[4];
                unpack_bits(r0, v[0], v[1]);
                unpack_bits(r1, v[2], v[3]);
#pragma unroll
                for (int q = 0; q < 4; ++q) {
                    const int64_t off = ((ch << 3) + 4 * blk + q) << 4;
                    if (valid && off < N) row_st16(row + off, a16, off, N, v[q]);
                }
            }
            return;
        }
    }
    if (!valid || blk != 0) return;
    for (int64_t n = w; n < N; n += W) row[n] = (uint8_t)((words32[n] >> env) & 1u);
}

// ---- NARROW tiles (round 5): 16 or 8 envs per workgroup, words of 16 / 8 bits -- 2 N / N bytes of LDS, for graphs past the half tile
// (N > ~40 000: up to ~80 000 / ~160 000 nodes).  The schedules, the counters and the compare are the half tile's (planes in 32-bit
// registers whose upper bits stay zero); only the LDS word and the byte <-> bit corner turn differ: a wave still turns 64 x 64 bits
// at a time, row l of the transpose = env l % E of node block l / E (E = 16: four blocks of 64 nodes per turn), so lane p ends
// with the E-bit words of node p in 64 / E consecutive blocks.  Per env the work is 32 / E times the half tile's (the edge list and
// the schedule are walked once per E envs) -- against one env per WAVE on a byte row, which these sizes fell to before.
template <typename WT> struct narrow_tile {
    static constexpr int E = 8 * (int)sizeof(WT);       // envs per tile
    static constexpr int NB = 64 / E;                   // 64-node blocks per transpose
    static constexpr uint32_t MASK = sizeof(WT) == 4 ? 0xFFFFFFFFu : ((1u << (E & 31)) - 1u);
};

template <typename WT, bool XORW> __device__ __forceinline__ void put_word_n(WT* words, int64_t n, uint32_t v) {
    if constexpr (XORW) words[n] = (WT)((uint32_t)words[n] ^ v);
    else words[n] = (WT)v;
}

// env-major bytes -> narrow bit tile.  VEC: rows are 16-byte multiples on a 16-byte base (each lane reads the 64 bytes of its (env,
// block) itself); anything else takes one ballot per node.
template <typename T, typename WT, bool VEC, bool XORW = false>
__device__ __forceinline__ void tilen_load_bits(const T* __restrict__ x, int64_t B, int64_t N, int64_t b0, WT* __restrict__ words,
                                                int lane, int w, int W) {
    constexpr int E = narrow_tile<WT>::E, NB = narrow_tile<WT>::NB;
    const int env = lane % E, blk = lane / E;
    const int64_t b = b0 + env;
    const bool valid = b < B;
    if constexpr (VEC && sizeof(T) == 1) {
        if ((N & 7) == 0) {
            // rows of 16-byte multiples: 16-byte loads; of 8-byte multiples (every other row starts mid-vector -- the Gset sizes 1000,
            // 3000, 5000, 7000, 9000): the same 64 bytes as eight 8-byte loads
            typedef uint32_t u32x2 __attribute__((ext_vector_type(2)));
            const uint8_t* xb = reinterpret_cast<const uint8_t*>(x);
            const u32x4* rv = reinterpret_cast<const u32x4*>(xb + (valid ? b : 0) * N);
            const u32x2* r2 = reinterpret_cast<const u32x2*>(rv);
            const bool a16 = (N & 15) == 0;
            const int64_t nv = N >> 4, n8 = N >> 3;
            const int64_t nchunk = (N + 64 * NB - 1) / (64 * NB);        // chunk = NB blocks of 64 nodes = one transpose
            const BitXpose xc = bit_xpose_consts(lane);
            for (int64_t ch = w; ch < nchunk; ch += W) {
                u32x4 v[4];
#pragma unroll
                for (int q = 0; q < 4; ++q) {
                    const int64_t idx = (ch * NB + blk) * 4 + q;
                    if (a16) {
                        v[q] = (valid && idx < nv) ? rv[idx] : u32x4{0, 0, 0, 0};
                    } else {
                        const u32x2 lo = (valid && 2 * idx < n8) ? r2[2 * idx] : u32x2{0, 0};
                        const u32x2 hi = (valid && 2 * idx + 1 < n8) ? r2[2 * idx + 1] : u32x2{0, 0};
                        v[q] = u32x4{lo.x, lo.y, hi.x, hi.y};
                    }
                }
                uint32_t r0 = pack_bits(v[0], v[1]), r1 = pack_bits(v[2], v[3]);
                bit_transpose64(r0, r1, xc);
                // this lane: node xc.node of each of the NB blocks; rows k E .. k E + E - 1 of the turn = block k
#pragma unroll
                for (int k = 0; k < NB; ++k) {
                    const uint32_t half = (k * E) < 32 ? r0 : r1;
                    const uint32_t wd = (half >> ((k * E) & 31)) & narrow_tile<WT>::MASK;
                    const int64_t n = (ch * NB + k) * 64 + xc.node;
                    if (n < N) put_word_n<WT, XORW>(words, n, wd);
                }
            }
            return;
        }
    }
    const T* row = x + (valid ? b : 0) * N;
    for (int64_t n0 = (int64_t)w * 64; n0 < N; n0 += (int64_t)W * 64) {
        uint32_t mine = 0;
        const int lim = (int)((N - n0) < 64 ? (N - n0) : 64);
        for (int k = 0; k < lim; ++k) {
            const T v = (valid && blk == 0) ? row[n0 + k] : T(0);
            const uint32_t wd = (uint32_t)ballot64(spin_is_set(v)) & narrow_tile<WT>::MASK;
            if (lane == k) mine = wd;
        }
        if (lane < lim) put_word_n<WT, XORW>(words, n0 + lane, mine);
    }
}

// narrow bit tile -> env-major bytes (0 | 1); rows with store_row == false stay untouched (store_row: per lane, by lane % E)
template <typename WT, bool VEC>
__device__ __forceinline__ void tilen_store_bytes(uint8_t* __restrict__ x, int64_t B, int64_t N, int64_t b0, const WT* __restrict__ words,
                                                  int lane, int w, int W, bool store_row) {
    constexpr int E = narrow_tile<WT>::E, NB = narrow_tile<WT>::NB;
    const int env = lane % E, blk = lane / E;
    const int64_t b = b0 + env;
    const bool valid = b < B && store_row;
    uint8_t* row = x + (b < B ? b : 0) * N;
    if constexpr (VEC) {
        if ((N & 7) == 0) {      // (16-byte stores, or 8-byte ones for rows of 8-byte multiples: tilen_load_bits)
            typedef uint32_t u32x2 __attribute__((ext_vector_type(2)));
            u32x4* rv = reinterpret_cast<u32x4*>(row);
            u32x2* r2 = reinterpret_cast<u32x2*>(row);
            const bool a16 = (N & 15) == 0;
            const int64_t nv = N >> 4, n8 = N >> 3;
            const int64_t nchunk = (N + 64 * NB - 1) / (64 * NB);
            const BitXpose xc = bit_xpose_consts(lane);
            for (int64_t ch = w; ch < nchunk; ch += W) {
                uint32_t r0 = 0, r1 = 0;
#pragma unroll
                for (int k = 0; k < NB; ++k) {
                    const int64_t n = (ch * NB + k) * 64 + xc.node;
                    const uint32_t wd = (n < N) ? (uint32_t)words[n] : 0u;
                    if ((k * E) < 32) r0 |= wd << ((k * E) & 31);
                    else r1 |= wd << ((k * E) & 31);
                }
                bit_transpose64(r0, r1, xc);
                u32x4 v[4];
                unpack_bits(r0, v[0], v[1]);
                unpack_bits(r1, v[2], v[3]);
#pragma unroll
                for (int q = 0; q < 4; ++q) {
                    const int64_t idx = (ch * NB + blk) * 4 + q;
                    if (a16) {
                        if (valid && idx < nv) rv[idx] = v[q];
                    } else {
                        if (valid && 2 * idx < n8) r2[2 * idx] = u32x2{v[q].x, v[q].y};
                        if (valid && 2 * idx + 1 < n8) r2[2 * idx + 1] = u32x2{v[q].z, v[q].w};
                    }
                }
            }
            return;
        }
    }
    if (!valid || blk != 0) return;
    for (int64_t n = w; n < N; n += W) row[n] = (uint8_t)(((uint32_t)words[n] >> env) & 1u);
}

}  // namespace rls
