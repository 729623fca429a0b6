// The order in which the one-shot grid of K4's write-through form (rls_step.hip) walks the batch: a pure function
// (order, block, blocks of the grid) -> virtual block, the block of runs a workgroup works on.  No HIP include: the kernels call it,
// rls_maxcut_step_block of the C ABI answers with it, and a host-only program can include this file.
#pragma once
#include <stdint.h>

#if defined(__HIP__)
#define RLS_STEP_PLAN_FN __host__ __device__ inline
#else
#define RLS_STEP_PLAN_FN inline
#endif

namespace rls {

// kStepOrderFwd     workgroup b works on block b.
// kStepOrderXcdFwd  the workgroups with equal b % 8 -- one XCD under round-robin placement -- work on one contiguous range of blocks,
//                   in order: XCD x owns an eighth of the batch, the same eighth in every step, so a line of the ring, and every
//                   128-byte line of obj / reward, is written and read again through one L2.  Placement is a speed assumption only:
//                   the map is a bijection on [0, nblocks) for every nblocks (the first nblocks % 8 classes hold one block more), so
//                   every block is worked on exactly once wherever a workgroup runs.
//                   Measured (tools/ceilings/ring_step_ladder.hip, profiles/r10_step_ladder.txt, 2^16 envs x 2000 bytes): the bare
//                   copy 38.21 -> 37.26 us, the step's rung i 39.46 -> 38.99 (spreads 0.05).
enum : int { kStepOrderFwd = 0, kStepOrderXcdFwd = 1 };

RLS_STEP_PLAN_FN int64_t step_block(int order, int64_t b, int64_t nblocks) {
    if (order != kStepOrderXcdFwd) return b;
    const int64_t q = nblocks / 8, r = nblocks % 8, x = b % 8;
    return x * q + (x < r ? x : r) + b / 8;
}

}  // namespace rls
