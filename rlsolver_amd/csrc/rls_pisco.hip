// PISCO_maxcut's dense product (rlsolver/envs/env_ISCO.py:436-444, tensor_core_energy):
//   rls_pisco_product : r[b][j] = sum_k delta(x)[b][k] * A[k][j],  delta = 2x - 1,  A f16 [Np, Np], x f16 [B, Np]
// on the f16 matrix instruction v_mfma_f32_16x16x32_f16 (f16 operands, f32 accumulate).  Energy and every flip gain of a
// sample come from its row of r; the step that consumes it is rls_pisco_step (rls_isco.hip).
//
// B > 64: one workgroup (4 waves) owns a [64 samples] x [64 columns] tile of r and walks K = Np in steps of 32 (B <= 64:
// k_pisco_product_few below, the same stage and fragments with the K walk split over the waves).  Per step it
// stages, through registers (the next step's loads are in flight while this one's MFMAs run):
//   Dl[m][k]  the sample tile as +1 / -1 (delta is made here from x > 0, never written to memory)
//   At[j][k]  the A tile TRANSPOSED, so that a lane's B fragment -- eight consecutive k of one column -- is one 16-byte read
// Operand lane maps (lane l, q = l >> 4, eight elements e): A fragment = Dl[l & 15][8q + e], B fragment = A[8q + e][l & 15];
// C/D: column l & 15, row 4q + register.
//
// Np is only a multiple of 8: neither the K-step nor the column block divides it.  A padded sample column is x = 0, delta = -1
// (not 0), so past Np it is the A tile that is zero-filled (rows k >= Np and columns j >= Np); the sample tile is zero-filled
// there too, and past B.  Every 16-byte piece lies wholly inside or wholly outside [0, Np) because Np % 8 == 0.
#include "rls_common.h"

namespace rls {

typedef _Float16 f16x8 __attribute__((ext_vector_type(8)));
typedef float f32x4 __attribute__((ext_vector_type(4)));
typedef uint32_t u32x4v __attribute__((ext_vector_type(4)));

constexpr int kPiscoBN = 64;        // columns of r per workgroup: 16 per wave
constexpr int kPiscoBK = 32;        // K per MFMA
constexpr int kPiscoFewMax = 64;    // batches up to this take k_pisco_product_few
constexpr int kPiscoLd = 40;        // f16 per LDS row: 32 + 8 of padding, rows stay 16-byte aligned

// eight f16 samples -> eight f16 deltas: x > 0 ? +1 : -1 (NaN and -0 read as 0, like the step)
__device__ __forceinline__ u32x4v pisco_delta8(u32x4v v) {
    u32x4v o;
#pragma unroll
    for (int i = 0; i < 4; ++i) {
        const uint32_t w = v[i];
        const _Float16 lo = __builtin_bit_cast(_Float16, (uint16_t)(w & 0xFFFFu));
        const _Float16 hi = __builtin_bit_cast(_Float16, (uint16_t)(w >> 16));
        o[i] = (lo > (_Float16)0 ? 0x3C00u : 0xBC00u) | ((hi > (_Float16)0 ? 0x3C00u : 0xBC00u) << 16);
    }
    return o;
}

constexpr int kPiscoBM = 64;        // samples of r per workgroup: four 16-row MFMA tiles per wave

__global__ __launch_bounds__(256) void k_pisco_product(const uint16_t* __restrict__ adj, int64_t Np, const uint16_t* __restrict__ x,
                                                       int64_t B, float* __restrict__ r_out) {
    constexpr int BM = kPiscoBM, MREP = BM / 16;
    __shared__ __attribute__((aligned(16))) uint16_t At[kPiscoBN * kPiscoLd + 32];
    __shared__ __attribute__((aligned(16))) uint16_t Dl[BM * kPiscoLd];
    const int tid = threadIdx.x, lane = tid & 63, w = tid >> 6;
    const int64_t col0 = (int64_t)blockIdx.x * kPiscoBN;
    const int64_t b0 = (int64_t)blockIdx.y * BM;
    // staging roles: the A tile is 32 rows x 8 pieces of 8 columns, the sample tile 64 rows x 4 pieces: one piece each per thread
    const int ak = tid >> 3, ac = (tid & 7) * 8;
    const int dm = tid >> 2, dk = (tid & 3) * 8;
    // The eight column pieces of a wave's transposing write are 8 LDS rows apart: 8 * kPiscoLd / 2 dwords, a multiple of 32
    // banks for any row length that keeps the rows 16-byte aligned -- an 8-way conflict on every 2-byte write (measured: 76 % of
    // the LDS-active cycles; 182 us at Np = 2000, B = 4096).  So the four 8-element k-blocks of row j are stored in the order
    // blk ^ ((j >> 3) & 3), which leaves rows 32 apart on one bank (2-way: 115 us), and rows 32 .. 63 start 16 dwords later.
    const int asw = (ac >> 3) & 3, askew = (ac >> 5) * 32;                    // rows ac .. ac + 7 share (row >> 3)
    const int bsw = ((w * 16 + (lane & 15)) >> 3) & 3, bskew = (w >> 1) * 32;
    const bool a_col_in = col0 + ac < Np;
    const bool d_row_in = b0 + dm < B;
    const u32x4v zero = {0u, 0u, 0u, 0u};
    auto load_a = [&](int64_t k0) -> u32x4v {
        return (a_col_in && k0 + ak < Np) ? *reinterpret_cast<const u32x4v*>(adj + (k0 + ak) * Np + col0 + ac) : zero;
    };
    auto load_d = [&](int64_t k0) -> u32x4v {
        return (d_row_in && k0 + dk < Np) ? pisco_delta8(*reinterpret_cast<const u32x4v*>(x + (b0 + dm) * Np + k0 + dk)) : zero;
    };
    f32x4 acc[MREP];
#pragma unroll
    for (int m = 0; m < MREP; ++m) acc[m] = f32x4{0.0f, 0.0f, 0.0f, 0.0f};
    u32x4v ra = load_a(0), rd = load_d(0);
    const int fr = lane & 15, fq = lane >> 4;
    for (int64_t k0 = 0; k0 < Np; k0 += kPiscoBK) {
        // transposing write of the A piece: element e of row ak goes to At[ac + e][ak]
#pragma unroll
        for (int e = 0; e < 8; ++e) At[(ac + e) * kPiscoLd + askew + ((((ak >> 3) ^ asw) << 3) | (ak & 7))] = (uint16_t)(ra[e >> 1] >> ((e & 1) * 16));
        *reinterpret_cast<u32x4v*>(&Dl[dm * kPiscoLd + dk]) = rd;
        __syncthreads();
        if (k0 + kPiscoBK < Np) { ra = load_a(k0 + kPiscoBK); rd = load_d(k0 + kPiscoBK); }
        const f16x8 bf = *reinterpret_cast<const f16x8*>(&At[(w * 16 + fr) * kPiscoLd + bskew + ((fq ^ bsw) << 3)]);
#pragma unroll
        for (int m = 0; m < MREP; ++m) {
            const f16x8 af = *reinterpret_cast<const f16x8*>(&Dl[(m * 16 + fr) * kPiscoLd + fq * 8]);
            acc[m] = __builtin_amdgcn_mfma_f32_16x16x32_f16(af, bf, acc[m], 0, 0, 0);
        }
        __syncthreads();
    }
    const int64_t j = col0 + w * 16 + fr;
    if (j < Np) {
#pragma unroll
        for (int m = 0; m < MREP; ++m) {
#pragma unroll
            for (int i = 0; i < 4; ++i) {
                const int64_t b = b0 + m * 16 + fq * 4 + i;
                if (b < B) r_out[b * Np + j] = acc[m][i];
            }
        }
    }
}

// B <= kPiscoFewMax (a chain or a few -- the reference's own BATCH_SIZE is 1): the product is close to a matrix-vector one and
// its time is the length of the K walk, so the walk is split.  A workgroup owns 16 samples x 16 columns only (A is re-read once per
// 16 samples, from L2: at most four times) and its four waves take
// the K-steps w, w + 4, ... each with a private LDS stage (no workgroup barrier inside the walk: LDS operations of one wave
// complete in order); the four accumulators meet in LDS at the end.
__device__ __forceinline__ void pisco_wave_lds_fence() {
    asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory");
    __builtin_amdgcn_wave_barrier();
}

__global__ __launch_bounds__(256) void k_pisco_product_few(const uint16_t* __restrict__ adj, int64_t Np, const uint16_t* __restrict__ x,
                                                           int64_t B, float* __restrict__ r_out) {
    __shared__ __attribute__((aligned(16))) uint16_t At[4][16 * kPiscoLd];
    __shared__ __attribute__((aligned(16))) uint16_t Dl[4][16 * kPiscoLd];
    __shared__ float red[4][256];
    const int tid = threadIdx.x, lane = tid & 63, w = tid >> 6;
    const int64_t col0 = (int64_t)blockIdx.x * 16;
    const int64_t b0 = (int64_t)blockIdx.y * 16;
    // staging roles inside a wave: the A tile is 32 rows x 2 pieces of 8 columns, the sample tile 16 rows x 4 pieces
    const int ak = lane >> 1, ac = (lane & 1) * 8;
    const int dm = lane >> 2, dk = (lane & 3) * 8;
    const bool a_col_in = col0 + ac < Np;
    const bool d_row_in = b0 + dm < B;
    const u32x4v zero = {0u, 0u, 0u, 0u};
    auto load_a = [&](int64_t k0) -> u32x4v {
        return (a_col_in && k0 + ak < Np) ? *reinterpret_cast<const u32x4v*>(adj + (k0 + ak) * Np + col0 + ac) : zero;
    };
    auto load_d = [&](int64_t k0) -> u32x4v {
        return (d_row_in && k0 + dk < Np) ? pisco_delta8(*reinterpret_cast<const u32x4v*>(x + (b0 + dm) * Np + k0 + dk)) : zero;
    };
    const int64_t nsteps = (Np + kPiscoBK - 1) / kPiscoBK;
    const int fr = lane & 15, fq = lane >> 4;
    f32x4 acc = {0.0f, 0.0f, 0.0f, 0.0f};
    u32x4v ra = zero, rd = zero;
    if (w < nsteps) { ra = load_a((int64_t)w * kPiscoBK); rd = load_d((int64_t)w * kPiscoBK); }
    for (int64_t s = w; s < nsteps; s += 4) {
#pragma unroll
        for (int e = 0; e < 8; ++e) At[w][(ac + e) * kPiscoLd + ak] = (uint16_t)(ra[e >> 1] >> ((e & 1) * 16));
        *reinterpret_cast<u32x4v*>(&Dl[w][dm * kPiscoLd + dk]) = rd;
        pisco_wave_lds_fence();
        if (s + 4 < nsteps) { ra = load_a((s + 4) * kPiscoBK); rd = load_d((s + 4) * kPiscoBK); }
        const f16x8 bf = *reinterpret_cast<const f16x8*>(&At[w][fr * kPiscoLd + fq * 8]);
        const f16x8 af = *reinterpret_cast<const f16x8*>(&Dl[w][fr * kPiscoLd + fq * 8]);
        acc = __builtin_amdgcn_mfma_f32_16x16x32_f16(af, bf, acc, 0, 0, 0);
        pisco_wave_lds_fence();
    }
#pragma unroll
    for (int i = 0; i < 4; ++i) red[w][lane * 4 + i] = acc[i];
    __syncthreads();
    if (w == 0) {
        const int64_t j = col0 + fr;
#pragma unroll
        for (int i = 0; i < 4; ++i) {
            const int64_t b = b0 + fq * 4 + i;
            const float v = ((red[0][lane * 4 + i] + red[1][lane * 4 + i]) + red[2][lane * 4 + i]) + red[3][lane * 4 + i];
            if (j < Np && b < B) r_out[b * Np + j] = v;
        }
    }
}

}  // namespace rls

using namespace rls;

extern "C" {

int64_t rls_pisco_scratch_bytes(int64_t Np, int64_t B) {
    if (Np <= 0 || Np % 8 != 0 || Np >= (1ll << 31) || B <= 0) return 0;
    return B * Np * 8;        // r f32 [B, Np] | ord int32 [B, Np]
}

int rls_pisco_product(const uint16_t* adj, int64_t Np, const uint16_t* x, int64_t B, float* r_out, void* stream) {
    RLS_REQUIRE(Np > 0 && Np % 8 == 0 && Np < (1ll << 31), RLS_EINVAL, "Np=%lld must be a positive multiple of 8", (long long)Np);
    RLS_REQUIRE(B >= 0, RLS_EINVAL, "B < 0");
    if (B == 0) return RLS_OK;
    RLS_REQUIRE(adj && x && r_out, RLS_EINVAL, "NULL pointer");
    RLS_REQUIRE((((uintptr_t)adj | (uintptr_t)x) & 15) == 0, RLS_EINVAL, "adj and x must be 16-byte aligned");
    const int64_t cb = ceil_div(Np, kPiscoBN);
    if (B <= kPiscoFewMax) {      // a chain or a few: 16-row tiles, 16 columns per workgroup, the K walk split over its waves
        hipLaunchKernelGGL(k_pisco_product_few, dim3((unsigned)ceil_div(Np, 16), (unsigned)ceil_div(B, 16)), dim3(256), 0, as_stream(stream),
                           adj, Np, x, B, r_out);
    } else {
        const int64_t rb = ceil_div(B, kPiscoBM);
        RLS_REQUIRE(rb <= 65535, RLS_EUNSUPPORTED, "B=%lld: more than 65535 sample tiles", (long long)B);
        hipLaunchKernelGGL(k_pisco_product, dim3((unsigned)cb, (unsigned)rb), dim3(256), 0, as_stream(stream), adj, Np, x, B, r_out);
    }
    return check_launch("k_pisco_product");
}

}  // extern "C"
