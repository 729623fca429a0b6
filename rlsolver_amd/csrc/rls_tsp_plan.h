// The launch policy of the TSP entry points (K12 rls_tsp_tour_length, K13 rls_tsp_swap_delta_all, rls_isco_tsp_step,
// rls_tsp_2opt_best, rls_rand_perms): which kernel form, how many waves per workgroup, how much LDS -- as pure functions of
// the sizes.  Plain C++ (no HIP): rls_tsp.hip and rls_isco.hip launch what these return, rls_tsp_launch_form of the C ABI answers
// with the same functions, so the answer cannot drift from the launch.
#pragma once
#include <stddef.h>
#include <stdint.h>
#include "rlsolver_hip.h"
#include "rls_host.h"

namespace rls {

constexpr int kTspBlock = 1024;     // launch bound; small tours use it whole (32 waves/CU hide the HBM round trip)
constexpr int kTspBlockSmall = 256;  // large N: the per-wave LDS tour scratch limits waves per workgroup
constexpr int kPermStride = 66;      // halfwords per position of k_rand_perms_lds' 64 tours (rls_tsp.hip)
constexpr int kTspStepWaves = 4;     // waves (= envs) per workgroup of the fused step while their scratch fits
constexpr size_t kTspLdsMargin = 1024;   // LDS left free beside a staged matrix

struct TspForm {
    bool lds_d, tab8;    // distance matrix staged in LDS; K13's byte tables in LDS
    int block, waves;    // threads / waves per workgroup
    size_t lds;          // dynamic LDS bytes
    size_t tabs;         // K13: bytes of the caller's tables8 block (0: none, or not usable at this N / K)
    int kernel;          // RLS_TSP_KERNEL_*
    int err;             // RLS_OK, or what the entry point returns without launching (RLS_EUNSUPPORTED)
};

constexpr size_t tsp_align16(size_t b) { return (b + 15) & ~(size_t)15; }

inline bool dist_fits_lds(int64_t N, size_t extra) { return (size_t)N * N * 4 + extra <= (size_t)kLdsBytes - kTspLdsMargin; }

inline int tsp_block(int64_t N) { return N <= 256 ? kTspBlock : kTspBlockSmall; }

// the byte form of the neighbour tables: ids < 256, and a far table to draw from (K <= N - 2: the reference's
// randint(0, N - K - 1) needs a non-empty range)
inline size_t tsp_tables8_size(int64_t N, int32_t K) {
    if (N < 3 || N > 256 || K < 1 || K > N - 2) return 0;
    return tsp_align16((size_t)N * K) + tsp_align16((size_t)N * (N - K - 1));
}

// K12: the matrix alone
inline TspForm tsp_plan_tour_length(int64_t N) {
    TspForm f{};
    f.block = tsp_block(N);
    f.waves = f.block / kWave;
    f.lds_d = dist_fits_lds(N, 0);
    f.lds = f.lds_d ? (size_t)N * N * 4 : 0;
    return f;
}

// K13: per wave the tour and its inverse (int32 each), then -- where they fit -- the byte tables (only the in-kernel draw reads
// them: `tables8` = drawn AND the caller gave the block) and the matrix
inline TspForm tsp_plan_swap_delta(int64_t N, int32_t K, bool tables8) {
    TspForm f{};
    f.block = tsp_block(N);
    f.waves = f.block / kWave;
    const size_t scratch = (size_t)f.waves * 2 * N * 4;
    f.tabs = (tables8 && N <= 256) ? tsp_tables8_size(N, K) : 0;
    if (scratch > (size_t)kLdsBytes - kTspLdsMargin) {
        f.err = RLS_EUNSUPPORTED;
        return f;
    }
    f.tab8 = f.tabs > 0 && dist_fits_lds(N, scratch + f.tabs);
    f.lds_d = dist_fits_lds(N, scratch + (f.tab8 ? f.tabs : 0));
    f.lds = (f.lds_d ? (size_t)N * N * 4 : 0) + scratch + (f.tab8 ? f.tabs : 0);
    return f;
}

// the fused step: 16 N bytes per wave (tour, inverse, logits, partner | ban), four waves beside the matrix or -- the matrix in
// global memory -- as many of 4 / 2 / 1 as the whole LDS holds
inline TspForm tsp_plan_step(int64_t N) {
    TspForm f{};
    const size_t per_wave = (size_t)N * 16;
    const size_t dbytes = (size_t)N * N * 4;
    f.lds_d = dbytes + kTspStepWaves * per_wave <= (size_t)kLdsBytes - kTspLdsMargin;
    f.waves = kTspStepWaves;
    if (!f.lds_d) {
        if (per_wave > (size_t)kLdsBytes) {
            f.err = RLS_EUNSUPPORTED;
            return f;
        }
        while (f.waves > 1 && per_wave * f.waves > (size_t)kLdsBytes) f.waves >>= 1;
    }
    f.block = f.waves * kWave;
    f.lds = (f.lds_d ? dbytes : 0) + per_wave * f.waves;
    return f;
}

// one 2-opt pass: the reduction's 256 (value, key) pairs, the seed's running sums (exact ranking) and the tour
inline TspForm tsp_plan_2opt_best(int64_t N, bool exact) {
    TspForm f{};
    f.block = 256;
    f.waves = f.block / kWave;
    f.lds = 256 * 16 + (exact ? (size_t)(N + 1) * 8 : 0) + (size_t)N * 4;
    if (f.lds > (size_t)kLdsBytes) f.err = RLS_EUNSUPPORTED;
    return f;
}

// the shuffle: a wave's 64 tours as uint16 in half the LDS (two workgroups per CU), else in place in global memory
inline TspForm tsp_plan_rand_perms(int64_t N) {
    TspForm f{};
    const size_t lds = (size_t)N * kPermStride * sizeof(uint16_t);
    if (N <= 65535 && lds <= (size_t)kLdsBytes / 2) {
        f.kernel = RLS_TSP_KERNEL_PERMS_LDS;
        f.block = kWave;
        f.lds = lds;
    } else {
        f.kernel = RLS_TSP_KERNEL_PERMS_GLOBAL;
        f.block = 256;
    }
    f.waves = f.block / kWave;
    return f;
}

}  // namespace rls
