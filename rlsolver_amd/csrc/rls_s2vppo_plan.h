// The launch policy of the S2V_PPO env kernels (rls_s2vppo.hip): which group of threads owns one env of a batch of DIFFERENT
// graphs, as one pure function of the batch size and the LARGEST graph of the batch.  Plain C++ (no HIP): rls_s2vppo_step and
// rls_s2vppo_reset launch what it returns and rls_s2vppo_launch_plan answers with it, so the policy is written once and the CPU
// suite pins it (tests/test_s2vppo_host.py).  The form never changes a result: every sum whose order could matter is taken in an
// order that does not depend on it (rls_s2vppo.hip).
#pragma once
#include <stdint.h>
#include "rlsolver_hip.h"
#include "rls_host.h"

namespace rls {

// One WAVE per env while a lane holds at most 4 of the env's nodes (a pass over the nodes is 4 loads in flight per lane and every
// reduction is cross-lane shuffles: no barrier, no LDS); 4 such envs share a workgroup of 256 threads.
constexpr int64_t kS2vWaveNodes = 4 * kWave;
constexpr int kS2vWaveEnvs = 4;
// Above that a WORKGROUP per env: 256 threads while a thread holds at most 16 nodes (more waves only add barrier cost to the two
// passes of a step), 1024 threads past it.  The reductions cross the waves through 128 bytes of LDS.
constexpr int64_t kS2vSmallGroupNodes = 16 * 256;

enum { S2V_FORM_WAVE = 0, S2V_FORM_GROUP = 1 };

struct S2vPlan {
    int err;        // RLS_OK or RLS_EINVAL
    int form;       // S2V_FORM_WAVE | S2V_FORM_GROUP
    int block;      // threads of a workgroup: 256 | 1024
    int envs;       // envs of a workgroup: 4 | 1
    int64_t grid;   // workgroups: ceil(B / envs)
};

inline S2vPlan s2vppo_plan(int64_t B, int64_t max_nodes) {
    S2vPlan p{};
    if (B < 0 || max_nodes < 0 || max_nodes >= (1ll << 31) || B >= (1ll << 31)) {
        p.err = RLS_EINVAL;
        return p;
    }
    if (max_nodes <= kS2vWaveNodes) {
        p.form = S2V_FORM_WAVE;
        p.block = kS2vWaveEnvs * kWave;
        p.envs = kS2vWaveEnvs;
    } else {
        p.form = S2V_FORM_GROUP;
        p.block = max_nodes <= kS2vSmallGroupNodes ? 256 : 1024;
        p.envs = 1;
    }
    p.grid = ceil_div(B, p.envs);
    return p;
}

}  // namespace rls
