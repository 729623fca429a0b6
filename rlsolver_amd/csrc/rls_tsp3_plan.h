// The launch policy of rls_tsp_3opt_best (rls_tsp3.hip): waves per workgroup, LDS bytes and whether the float64 distance matrix
// is staged in LDS -- a pure function of (N, exact).  Plain C++ (no HIP): the launcher launches what this returns and
// rls_tsp_3opt_launch_form of the C ABI answers with the same function, so the answer cannot drift from the launch.
//
// LDS of one workgroup, in this order (every offset a multiple of 8):
//   [ matrix  8 N^2      ]  staged form only
//   [ S       8 (N + 1)  ]  exact ranking only: running sums of the seed tour
//   [ red     16 waves   ]  one (value, key) pair per wave for the workgroup reduction
//   [ tour    4 N        ]  the tour as int32
// lds(N, exact, waves, staged) = staged * 8 N^2 + exact * 8 (N + 1) + 16 waves + 4 N.
// Staged (kTsp3WavesStaged = 16 waves share one copy of the matrix) while lds(.., 16, 1) <= kLdsBytes: N <= 142; else
// kTsp3WavesGlobal = 4 waves read the matrix through L2, refused (RLS_EUNSUPPORTED) once lds(.., 4, 0) > kLdsBytes.
#pragma once
#include <stddef.h>
#include <stdint.h>
#include "rlsolver_hip.h"
#include "rls_host.h"

namespace rls {

constexpr int kTsp3WavesStaged = 16;
constexpr int kTsp3WavesGlobal = 4;

struct Tsp3Form {
    bool lds_d;          // the matrix is staged in LDS
    int block, waves;    // threads / waves per workgroup
    size_t lds;          // dynamic LDS bytes
    int err;             // RLS_OK, or what the entry point returns without launching (RLS_EUNSUPPORTED)
};

constexpr size_t tsp3_lds(int64_t N, bool exact, int waves, bool staged) {
    return (staged ? (size_t)N * N * 8 : 0) + (exact ? (size_t)(N + 1) * 8 : 0) + (size_t)waves * 16 + (size_t)N * 4;
}

inline Tsp3Form tsp_plan_3opt_best(int64_t N, bool exact) {
    Tsp3Form f{};
    f.lds_d = N <= 1024 && tsp3_lds(N, exact, kTsp3WavesStaged, true) <= (size_t)kLdsBytes;
    f.waves = f.lds_d ? kTsp3WavesStaged : kTsp3WavesGlobal;
    f.block = f.waves * kWave;
    f.lds = tsp3_lds(N, exact, f.waves, f.lds_d);
    if (f.lds > (size_t)kLdsBytes) f.err = RLS_EUNSUPPORTED;
    return f;
}

}  // namespace rls
