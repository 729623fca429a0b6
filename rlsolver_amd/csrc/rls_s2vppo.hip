// The MaxCut env of S2V_PPO for gfx950 (rlsolver/methods/S2V_PPO/env.py): step() and reset() of a BATCH OF DIFFERENT GRAPHS as one
// launch each.  The reference keeps one Python object per env and steps them in a loop (train_ddp.py:117-139): about 25 small torch
// ops and four host reads per env-step.
//
// The batch is PyG-shaped: ptr[env] is the first node of an env in the concatenated node arrays, one CSR-by-source over all nodes
// holds the edge-list entries AS GIVEN (a line listed twice is two entries, a loop (u, u) an ordinary entry, a one-directional line
// stays one-directional), each row sorted by destination (stable), columns as global node ids.
//
// step (env.py:140-206), per env, for the action node a:
//   cut += delta[a];  z[a] = -z[a];  delta[dst] += 2 z[dst] z[a] w  over a's row (a loop sees the NEW z[a]: += 2 w);  THEN delta[a]
//   = -delta[a];  the tabu ring takes a;  last_flip[a] = step count;  the state hash takes key(a);  "new" = hash not among the last 50;
//   reward (float64) = improvement / (improvement + 0.1) if the cut beats the best, - stag_punishment if not new, + 0.01 if every
//   delta <= 0 and the state is no recorded basin;  THEN the hash joins the history;  x [N, 5] and the mask are rewritten.
// Entries of a row with the same destination are one run, adjacent because the row is sorted: the lane that holds a run's first
// entry adds the whole run in list order -- no lost update, no float atomic, the reference's index_add_ order.
// The state's identity is a 64-bit Zobrist hash (XOR of key(local node) over the nodes with z = +1), one XOR per flip.
//
// A group of threads owns an env: a wave (4 envs per workgroup) or a workgroup (rls_s2vppo_plan.h).  The per-node state stays in
// global memory (L2-resident between steps: 10 bytes per node); a step walks one row, then makes two passes over the env's nodes
// (count the positive deltas -- column 4, the basin verdict and so the reward need it first -- then write x and the mask).
// Nothing depends on the form: integer sums and XORs reduce in any order, float sums are taken per node / per run in list order,
// and reset's cut is summed by 64 lanes in either form.
#include "rls_draw.h"
#include "rls_s2vppo_plan.h"

namespace rls {

constexpr int kS2vHistory = 50;           // env.py:37  deque(maxlen=50)
constexpr int kS2vHashRow = kS2vHistory + 1;   // the ring + the current hash

__device__ __forceinline__ uint64_t s2v_key(uint32_t node) {          // splitmix64 of a constant + the local node index
    uint64_t x = 0x5332565F50504F31ull + (uint64_t)(node + 1u) * 0x9E3779B97F4A7C15ull;
    x = (x ^ (x >> 30)) * 0xBF58476D1CE4E5B9ull;
    x = (x ^ (x >> 27)) * 0x94D049BB133111EBull;
    return x ^ (x >> 31);
}

// what the threads of a group wrote to global memory is visible to the group after this
template <int FORM>
__device__ __forceinline__ void s2v_sync() {
    if constexpr (FORM == S2V_FORM_WAVE) {
        __builtin_amdgcn_fence(__ATOMIC_RELEASE, "workgroup");
        __builtin_amdgcn_wave_barrier();
        __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "workgroup");
    } else {
        __syncthreads();
    }
}

struct S2vAdd { __device__ uint64_t operator()(uint64_t a, uint64_t b) const { return a + b; } };
struct S2vMax { __device__ uint64_t operator()(uint64_t a, uint64_t b) const { return a > b ? a : b; } };
struct S2vXor { __device__ uint64_t operator()(uint64_t a, uint64_t b) const { return a ^ b; } };

// an associative, commutative op over the group; every thread gets the result.  Called by ALL threads of the group.
template <int FORM, typename Op>
__device__ __forceinline__ uint64_t s2v_reduce(uint64_t v, Op op, uint64_t* red) {
#pragma unroll
    for (int d = kWave / 2; d >= 1; d >>= 1) v = op(v, (uint64_t)__shfl_xor((unsigned long long)v, d, kWave));
    if constexpr (FORM == S2V_FORM_GROUP) {
        const int w = threadIdx.x >> 6, nw = blockDim.x >> 6;
        if ((threadIdx.x & (kWave - 1)) == 0) red[w] = v;
        __syncthreads();
        v = red[0];
        for (int k = 1; k < nw; ++k) v = op(v, red[k]);
        __syncthreads();
    }
    return v;
}

// (gain, node) as one key whose maximum is the largest gain at the LOWEST node index
__device__ __forceinline__ uint64_t s2v_gain_key(float v, int i) {
    uint32_t u = __float_as_uint(v);
    u ^= (u >> 31) ? 0xFFFFFFFFu : 0x80000000u;
    return ((uint64_t)u << 32) | (uint32_t)(0x7FFFFFFF - i);
}

// delta[dst] += 2 z[dst] za w over the row of global node ga, whose spin BECOMES za (not yet written).  A run of equal
// destinations is added by the thread that holds its first entry, in list order.  The loop entry (dst == ga): the reference's
// step adds 2 w before the negation that follows (env.py:204-206); EXACT (the greedy reset recomputes every gain instead,
// env.py:53: a loop's term w z_a z_a never changes) adds -2 w, so that the negation leaves +2 w.
// COST: one thread adds a whole run, because the sum is in list order; a row's time is bounded by its LONGEST run (all d entries
// when they share one destination), not by d / G.
template <bool EXACT>
__device__ __forceinline__ void s2v_flip_row(const rls_s2vppo_env& e, int64_t ga, float za, int t, int G) {
    const int64_t r0 = e.rowptr[ga], r1 = e.rowptr[ga + 1];
    for (int64_t k = r0 + t; k < r1; k += G) {
        const int32_t dst = e.col[k];
        if (k > r0 && e.col[k - 1] == dst) continue;
        float d = e.delta[dst];
        const float f = dst == ga ? (EXACT ? -2.0f : 2.0f) : 2.0f * (float)e.z[dst] * za;
        for (int64_t j = k; j < r1 && e.col[j] == dst; ++j) d += f * e.w[j];
        e.delta[dst] = d;
    }
}

// delta[i] = z_i * sum over i's row of w z[dst], float32 in list order (env.py:84-105)
__device__ __forceinline__ void s2v_all_deltas(const rls_s2vppo_env& e, int64_t n0, int N, int t, int G) {
    for (int i = t; i < N; i += G) {
        const int64_t g = n0 + i;
        float s = 0.0f;
        for (int64_t k = e.rowptr[g]; k < e.rowptr[g + 1]; ++k) s += e.w[k] * (float)e.z[e.col[k]];
        e.delta[g] = (float)e.z[g] * s;
    }
}

// x [N, 5] and the mask of one env (env.py:107-131); steps = the step count they describe; best_z takes z where `keep_best`
template <int FORM>
__device__ __forceinline__ void s2v_emit(const rls_s2vppo_env& e, int64_t env, int64_t n0, int N, int steps, int npos, bool keep_best,
                                         int t, int G) {
    const float wden = e.wtot[3 * env + 1];
    const float frac = (float)npos / (float)N;
    const float max_steps = (float)(e.multiplier * N);
    for (int i = t; i < N; i += G) {
        const int64_t g = n0 + i;
        const int8_t zi = e.z[g];
        float* xr = e.x + 5 * g;
        xr[0] = (float)zi;
        xr[1] = e.delta[g] / wden;
        xr[2] = 0.0f;
        xr[3] = (float)(steps - e.last_flip[g]) / max_steps;
        xr[4] = frac;
        e.mask[g] = 1;
        if (keep_best) e.best_z[g] = zi;
    }
    if (e.tenure > 0 && steps > 0) {
        s2v_sync<FORM>();
        const int held = steps < e.tenure ? steps : (int)e.tenure;      // the ring's live entries (any order; repeats allowed)
        const int32_t* ring = e.tabu + env * e.tenure;
        for (int j = t; j < held; j += G) {
            const int64_t g = n0 + ring[j];
            e.x[5 * g + 2] = 1.0f;
            if (e.delta[g] <= 0.0f) e.mask[g] = 0;
        }
    }
}

template <int FORM>
__global__ __launch_bounds__(1024) void k_s2vppo_step(rls_s2vppo_env e, const int64_t* __restrict__ action, double stag_punishment,
                                                      double* __restrict__ reward, uint8_t* __restrict__ done) {
    __shared__ uint64_t red[16];
    const int G = FORM == S2V_FORM_WAVE ? kWave : (int)blockDim.x;
    const int t = FORM == S2V_FORM_WAVE ? (int)(threadIdx.x & (kWave - 1)) : (int)threadIdx.x;
    const int64_t env = FORM == S2V_FORM_WAVE ? (int64_t)blockIdx.x * kS2vWaveEnvs + (threadIdx.x >> 6) : (int64_t)blockIdx.x;
    if (env >= e.num_envs) return;                                   // (a whole wave of the wave form: it meets no barrier)
    const int64_t n0 = e.ptr[env];
    const int N = (int)(e.ptr[env + 1] - n0);
    const int64_t a = action[env];
    int32_t* cnt = e.counters + 4 * env;
    const int sc = cnt[0], nb = cnt[1];
    const int64_t max_steps = e.multiplier * N;
    // as rls_maxcut_step: on an action outside [0, N) the env stays as it is and its reward is NaN; so does an env whose episode is
    // over (its basin table and the caller's step count hold one episode), whatever the caller's own count says
    if (a < 0 || a >= N || sc >= max_steps) {
        if (t == 0) {
            reward[env] = __longlong_as_double(0x7FF8000000000000ll);
            done[env] = sc >= max_steps;
        }
        return;
    }
    const double cut0 = e.cut[env], best0 = e.best_cut[env];
    uint64_t* hs = reinterpret_cast<uint64_t*>(e.hash) + (int64_t)kS2vHashRow * env;
    const uint64_t h_new = hs[kS2vHistory] ^ s2v_key((uint32_t)a);
    const int64_t ga = n0 + a;
    const float za = -(float)e.z[ga];
    const double cut1 = cut0 + (double)e.delta[ga];
    const bool improved = cut1 > best0;
    const int nh = sc < kS2vHistory ? sc : kS2vHistory;              // the history as it is BEFORE this state joins it
    uint64_t hit = 0;
    for (int i = t; i < nh; i += G) hit |= hs[i] == h_new;

    s2v_sync<FORM>();                                                // every thread has read delta[ga]: a loop entry of the row adds to it
    s2v_flip_row<false>(e, ga, za, t, G);
    s2v_sync<FORM>();
    if (t == 0) {
        e.delta[ga] = -e.delta[ga];                                  // after the row: a loop has added to it
        e.z[ga] = (int8_t)za;
        e.last_flip[ga] = sc + 1;
        if (e.tenure > 0) e.tabu[env * e.tenure + sc % e.tenure] = (int32_t)a;
    }
    s2v_sync<FORM>();

    uint64_t acc = hit << 40;
    for (int i = t; i < N; i += G) acc += e.delta[n0 + i] > 0.0f;
    acc = s2v_reduce<FORM>(acc, S2vAdd{}, red);
    const int npos = (int)(acc & ((1ull << 40) - 1));
    const bool revisit = (acc >> 40) != 0;
    bool new_basin = false;
    uint64_t* basins = reinterpret_cast<uint64_t*>(e.basins) + e.multiplier * n0;
    if (npos == 0) {                                                 // (uniform over the group)
        uint64_t seen = 0;
        for (int i = t; i < nb; i += G) seen |= basins[i] == h_new;
        new_basin = s2v_reduce<FORM>(seen, S2vAdd{}, red) == 0;
    }
    s2v_emit<FORM>(e, env, n0, N, sc + 1, npos, improved, t, G);

    if (t == 0) {
        double r = 0.0;
        if (improved) r = (cut1 - best0) / ((cut1 - best0) + 0.1);
        if (revisit) r -= stag_punishment;
        if (new_basin) r += 0.01;
        reward[env] = r;
        done[env] = sc + 1 >= max_steps;
        e.cut[env] = cut1;
        if (improved) e.best_cut[env] = cut1;
        hs[sc % kS2vHistory] = h_new;
        hs[kS2vHistory] = h_new;
        cnt[0] = sc + 1;
        if (new_basin && nb < max_steps) {                           // one slot per step of an episode
            basins[nb] = h_new;
            cnt[1] = nb + 1;
        }
    }
}

template <int FORM>
__global__ __launch_bounds__(1024) void k_s2vppo_reset(rls_s2vppo_env e, const int64_t* __restrict__ ids, int64_t num_ids,
                                                       const int8_t* __restrict__ z0, const uint8_t* __restrict__ greedy, uint64_t seed,
                                                       int64_t env_offset) {
    __shared__ uint64_t red[16];
    const int G = FORM == S2V_FORM_WAVE ? kWave : (int)blockDim.x;
    const int t = FORM == S2V_FORM_WAVE ? (int)(threadIdx.x & (kWave - 1)) : (int)threadIdx.x;
    const int64_t slot = FORM == S2V_FORM_WAVE ? (int64_t)blockIdx.x * kS2vWaveEnvs + (threadIdx.x >> 6) : (int64_t)blockIdx.x;
    if (slot >= num_ids) return;
    const int64_t env = ids ? ids[slot] : slot;
    if (env < 0 || env >= e.num_envs) return;                        // (uniform over the group)
    const int64_t n0 = e.ptr[env];
    const int N = (int)(e.ptr[env + 1] - n0);
    int32_t* cnt = e.counters + 4 * env;
    const uint32_t episode = (uint32_t)cnt[2];
    const uint64_t genv = (uint64_t)(env_offset + env);
    const uint32_t pos_key = isco_pos_key(isco_env_key(seed, genv), genv, episode);
    // where the start spins come from: 0 recorded, 1 random, 2 greedy from all-ones (env.py:48-57: random() < 0.5 is the random one)
    const int branch = z0 ? 0 : (greedy ? (greedy[env] ? 2 : 1) : ((isco_draw_at(pos_key, 0u, 1u) >> 31) ? 2 : 1));
    for (int i = t; i < N; i += G) {
        const int64_t g = n0 + i;
        e.z[g] = branch == 0 ? (z0[g] > 0 ? 1 : -1) : (branch == 1 ? ((isco_draw_at(pos_key, (uint32_t)i, 0u) >> 31) ? 1 : -1) : 1);
        e.last_flip[g] = 0;
    }
    s2v_sync<FORM>();
    s2v_all_deltas(e, n0, N, t, G);
    s2v_sync<FORM>();
    if (branch == 2) {
        const bool symmetric = e.wtot[3 * env + 2] != 0.0f;
        for (int it = 0; it < N / 2; ++it) {
            uint64_t key = 0;
            for (int i = t; i < N; i += G) {
                const uint64_t k = s2v_gain_key(e.delta[n0 + i], i);
                key = k > key ? k : key;
            }
            key = s2v_reduce<FORM>(key, S2vMax{}, red);
            uint32_t u = (uint32_t)(key >> 32);
            u ^= (u >> 31) ? 0x80000000u : 0xFFFFFFFFu;
            if (!(__uint_as_float(u) > 0.0f)) break;                 // (uniform)
            const int64_t gb = n0 + (0x7FFFFFFF - (int)(uint32_t)key);
            const float zb = -(float)e.z[gb];
            s2v_sync<FORM>();                                        // every thread has read z[gb] and its deltas
            if (symmetric) {                                         // (uniform) the node's own row is also what points at it
                s2v_flip_row<true>(e, gb, zb, t, G);
                s2v_sync<FORM>();
                if (t == 0) {
                    e.delta[gb] = -e.delta[gb];
                    e.z[gb] = (int8_t)zb;
                }
            } else {                                                 // a list that is not its own transpose: all gains again, as env.py:53
                if (t == 0) e.z[gb] = (int8_t)zb;
                s2v_sync<FORM>();
                s2v_all_deltas(e, n0, N, t, G);
            }
            s2v_sync<FORM>();
        }
        s2v_all_deltas(e, n0, N, t, G);                              // env.py:62 recomputes them after the search
        s2v_sync<FORM>();
    }
    // cut = W / 2 - sum(z nb) / 4 (env.py:93-96), the sum in float64 over 64 lanes in either form
    double same = 0.0;
    if (t < kWave) {
        for (int i = t; i < N; i += kWave) same += (double)e.delta[n0 + i];
#pragma unroll
        for (int d = kWave / 2; d >= 1; d >>= 1) same += __shfl_xor(same, d, kWave);
    }
    uint64_t h = 0, npos = 0;
    for (int i = t; i < N; i += G) {
        if (e.z[n0 + i] > 0) h ^= s2v_key((uint32_t)i);
        npos += e.delta[n0 + i] > 0.0f;
    }
    h = s2v_reduce<FORM>(h, S2vXor{}, red);
    npos = s2v_reduce<FORM>(npos, S2vAdd{}, red);
    s2v_emit<FORM>(e, env, n0, N, 0, (int)npos, true, t, G);
    if (t == 0) {
        const double cut = 0.5 * (double)e.wtot[3 * env] - 0.25 * same;
        e.cut[env] = cut;
        e.best_cut[env] = cut;
        reinterpret_cast<uint64_t*>(e.hash)[(int64_t)kS2vHashRow * env + kS2vHistory] = h;
        cnt[0] = 0;
        cnt[1] = 0;
        cnt[2] = (int32_t)(episode + 1u);
        cnt[3] = branch;
    }
}

static int s2v_check(const rls_s2vppo_env* e) {
    RLS_REQUIRE(e != nullptr, RLS_EINVAL, "env is NULL");
    RLS_REQUIRE(e->num_envs >= 0 && e->total_nodes >= 0 && e->total_nodes < (1ll << 31) && e->max_nodes >= 0 && e->max_nodes <= e->total_nodes &&
                    e->nnz >= 0,
                RLS_EINVAL, "bad sizes num_envs=%lld total_nodes=%lld max_nodes=%lld nnz=%lld", (long long)e->num_envs,
                (long long)e->total_nodes, (long long)e->max_nodes, (long long)e->nnz);
    RLS_REQUIRE(e->tenure >= 0 && e->tenure < (1ll << 31), RLS_EINVAL, "tabu_tenure must be in [0, 2^31), got %lld", (long long)e->tenure);
    RLS_REQUIRE(e->multiplier >= 1 && e->multiplier * e->total_nodes < (1ll << 31), RLS_EINVAL,
                "episode_length_multiplier must be >= 1 and multiplier * total_nodes < 2^31, got %lld", (long long)e->multiplier);
    if (e->num_envs == 0) return RLS_OK;
    RLS_REQUIRE(e->ptr && e->rowptr && e->wtot && e->counters && e->cut && e->best_cut && e->hash && e->tabu, RLS_EINVAL, "NULL pointer");
    RLS_REQUIRE(e->total_nodes == 0 || (e->z && e->delta && e->last_flip && e->best_z && e->basins && e->x && e->mask), RLS_EINVAL,
                "NULL pointer");
    RLS_REQUIRE(e->nnz == 0 || (e->col && e->w), RLS_EINVAL, "NULL pointer");
    return RLS_OK;
}

}  // namespace rls

using namespace rls;

extern "C" {

int rls_s2vppo_step(const rls_s2vppo_env* e, const int64_t* action, double stag_punishment, double* reward, uint8_t* done, void* stream) {
    if (int rc = s2v_check(e)) return rc;
    if (e->num_envs == 0) return RLS_OK;
    RLS_REQUIRE(action && reward && done, RLS_EINVAL, "action/reward/done is NULL");
    const S2vPlan p = s2vppo_plan(e->num_envs, e->max_nodes);
    if (p.err != RLS_OK) return fail(p.err, "s2vppo_step: no launch plan for B=%lld max_nodes=%lld", (long long)e->num_envs, (long long)e->max_nodes);
    if (p.form == S2V_FORM_WAVE)
        hipLaunchKernelGGL(k_s2vppo_step<S2V_FORM_WAVE>, dim3((unsigned)p.grid), dim3(p.block), 0, as_stream(stream), *e, action, stag_punishment,
                           reward, done);
    else
        hipLaunchKernelGGL(k_s2vppo_step<S2V_FORM_GROUP>, dim3((unsigned)p.grid), dim3(p.block), 0, as_stream(stream), *e, action, stag_punishment,
                           reward, done);
    return check_launch("k_s2vppo_step");
}

int rls_s2vppo_reset(const rls_s2vppo_env* e, const int64_t* ids, int64_t num_ids, const int8_t* z0, const uint8_t* greedy, uint64_t seed,
                     int64_t env_offset, void* stream) {
    if (int rc = s2v_check(e)) return rc;
    RLS_REQUIRE(env_offset >= 0, RLS_EINVAL, "env_offset must be >= 0, got %lld", (long long)env_offset);
    RLS_REQUIRE(ids ? num_ids >= 0 : num_ids == e->num_envs, RLS_EINVAL, "num_ids=%lld (without ids it is num_envs=%lld)", (long long)num_ids,
                (long long)e->num_envs);
    if (num_ids == 0 || e->num_envs == 0) return RLS_OK;
    const S2vPlan p = s2vppo_plan(num_ids, e->max_nodes);
    if (p.err != RLS_OK) return fail(p.err, "s2vppo_reset: no launch plan for %lld envs, max_nodes=%lld", (long long)num_ids, (long long)e->max_nodes);
    if (p.form == S2V_FORM_WAVE)
        hipLaunchKernelGGL(k_s2vppo_reset<S2V_FORM_WAVE>, dim3((unsigned)p.grid), dim3(p.block), 0, as_stream(stream), *e, ids, num_ids, z0, greedy,
                           seed, env_offset);
    else
        hipLaunchKernelGGL(k_s2vppo_reset<S2V_FORM_GROUP>, dim3((unsigned)p.grid), dim3(p.block), 0, as_stream(stream), *e, ids, num_ids, z0, greedy,
                           seed, env_offset);
    return check_launch("k_s2vppo_reset");
}

}  // extern "C"
