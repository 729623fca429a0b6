// The launch policy of rls_tsp_grow_2opt (rls_tsp_grow.hip): waves per workgroup, LDS bytes and whether the float64 distance
// matrix is staged in LDS -- a pure function of N.  Plain C++ (no HIP): the launcher launches what this returns and
// rls_tsp_grow_launch_form of the C ABI answers with the same function, so the answer cannot drift from the launch.
//
// LDS of one workgroup, in this order (every offset a multiple of 8):
//   [ matrix  8 N^2      ]  staged form only
//   [ S       8 (N + 1)  ]  running sums of the pass's seed tour
//   [ red     16 waves   ]  one (value, key) pair per wave for the workgroup reduction
//   [ tour    4 N        ]  the partial tour as int32
//   [ order   4 N        ]  the row of `order` as int32
// lds(N, staged) = staged * 8 N^2 + 8 (N + 1) + 16 waves + 8 N, waves = kTspGrowWaves = 16 in both forms (one workgroup is all a
// row has: the candidates of a pass are dealt over its 1024 threads).  Staged while lds(N, 1) <= kLdsBytes: N <= 141; above that the
// matrix is read through L2, refused (RLS_EUNSUPPORTED) once lds(N, 0) > kLdsBytes: N >= 10224.
#pragma once
#include <stddef.h>
#include <stdint.h>
#include "rlsolver_hip.h"
#include "rls_host.h"

namespace rls {

constexpr int kTspGrowWaves = 16;

struct TspGrowForm {
    bool lds_d;          // the matrix is staged in LDS
    int block, waves;    // threads / waves per workgroup
    size_t lds;          // dynamic LDS bytes
    int err;             // RLS_OK, or what the entry point returns without launching (RLS_EUNSUPPORTED)
};

constexpr size_t tsp_grow_lds(int64_t N, bool staged) {
    return (staged ? (size_t)N * N * 8 : 0) + (size_t)(N + 1) * 8 + (size_t)kTspGrowWaves * 16 + (size_t)N * 8;
}

inline TspGrowForm tsp_plan_grow(int64_t N) {
    TspGrowForm f{};
    f.lds_d = N <= 1024 && tsp_grow_lds(N, true) <= (size_t)kLdsBytes;
    f.waves = kTspGrowWaves;
    f.block = f.waves * kWave;
    f.lds = tsp_grow_lds(N, f.lds_d);
    if (f.lds > (size_t)kLdsBytes) f.err = RLS_EUNSUPPORTED;
    return f;
}

}  // namespace rls
