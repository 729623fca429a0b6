// The launch policy of sub_set_sampling (rls_subset.hip): what the kernel keeps in LDS, the node limit that follows, the workgroup
// size and how many of the R repeats one workgroup writes -- as one pure function of the sizes and the CU count.  Plain C++ (no HIP):
// rls_sub_set_sampling launches what it returns and rls_sub_set_sampling_supported answers with its test, so the policy is
// written once (tools/host_sanitize.cpp runs it over random shapes).
#pragma once
#include <stddef.h>
#include <stdint.h>
#include "rlsolver_hip.h"
#include "rls_host.h"

namespace rls {

// what the waves of a workgroup share beside the rows (the first thing in its LDS)
struct SubsetScratch { int hist[256]; uint32_t digit; int want; int bin; int count; };

constexpr size_t subset_pad16(size_t b) { return (b + 15) & ~(size_t)15; }
constexpr size_t kSubsetFixed = subset_pad16(sizeof(SubsetScratch));
// one copy of the start row: N bytes rounded up to 16 + 16 (a 16-byte piece cut at any byte offset reads inside it)
constexpr size_t subset_row_bytes(int64_t N) { return subset_pad16((size_t)N) + 16; }
// scratch | det keys uint32 [N] | two copies of the row (a repeat patches one while the other leaves) | selected nodes uint16 [N]
constexpr size_t subset_lds_bytes(int64_t N) {
    return kSubsetFixed + subset_pad16((size_t)N * 4) + 2 * subset_row_bytes(N) + subset_pad16((size_t)N * 2);
}
constexpr int64_t subset_max_nodes() {                    // the largest N whose LDS layout fits
    int64_t n = kLdsBytes / 8;
    while (subset_lds_bytes(n) > (size_t)kLdsBytes) --n;
    return n;
}
constexpr int64_t kSubsetMaxN = subset_max_nodes();
static_assert(kSubsetMaxN == RLS_SUB_SET_SAMPLING_MAX_NODES, "include/rlsolver_hip.h: RLS_SUB_SET_SAMPLING_MAX_NODES");
static_assert(kSubsetMaxN < 65536, "the selected list holds uint16 node ids");

constexpr int64_t kSubsetMinRepeats = 4;    // repeats a workgroup writes at least (while R has them): its selection is paid once

// 1 when the kernel covers the shape: the row fits LDS, the repeat counter fits the generator's 32-bit counter and R S N an int64
inline bool subset_supported(int64_t S, int64_t N, int64_t R, int64_t top_k) {
    if (S < 0 || N < 1 || R < 1 || top_k < 0 || N > kSubsetMaxN || R >= (1ll << 31) || S >= (1ll << 31)) return false;
    return S == 0 || R <= INT64_MAX / N / S;
}

struct SubsetPlan {
    int err;            // RLS_OK, or what the entry point returns without launching (RLS_EUNSUPPORTED)
    int block;          // the form: threads of a workgroup, 256 | 512 | 1024 by the LDS a row takes
    int64_t repeats;    // repeats per workgroup: workgroup (s, c) writes repeats [c * repeats, min(R, (c + 1) * repeats)) of sim s
    int64_t chunks;     // workgroups per sim = ceil(R / repeats); the grid is S * chunks
    size_t lds;         // dynamic LDS bytes
};

inline SubsetPlan subset_plan(int64_t S, int64_t N, int64_t R, int64_t top_k, int cus) {
    SubsetPlan p{};
    if (!subset_supported(S, N, R, top_k)) {
        p.err = RLS_EUNSUPPORTED;
        return p;
    }
    p.lds = subset_lds_bytes(N);
    // the row bounds the workgroups a CU holds: the fewer of them, the more waves each brings (always 16 waves per CU or more)
    const int per_cu = (int)((size_t)kLdsBytes / p.lds) < 4 ? (int)((size_t)kLdsBytes / p.lds) : 4;
    p.block = per_cu >= 4 ? 256 : (per_cu >= 2 ? 512 : 1024);
    // as many workgroups as fill the chip once; each redoes its sim's selection (N values) and amortises it over its repeats
    const int64_t resident = (int64_t)(cus < 1 ? 1 : cus) * per_cu;
    int64_t chunks = S > 0 ? ceil_div(resident, S) : 1;
    if (chunks > R) chunks = R;
    int64_t repeats = ceil_div(R, chunks);
    if (repeats < kSubsetMinRepeats) repeats = R < kSubsetMinRepeats ? R : kSubsetMinRepeats;
    chunks = ceil_div(R, repeats);
    if (S > 0 && chunks > ((1ll << 31) - 1) / S) {       // (the grid is one dimension)
        chunks = ((1ll << 31) - 1) / S;
        repeats = ceil_div(R, chunks);
        chunks = ceil_div(R, repeats);
    }
    p.repeats = repeats;
    p.chunks = chunks;
    return p;
}

}  // namespace rls
