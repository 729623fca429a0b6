// A ladder from the chained-ring ceiling (ring_copy.hip, row `chained fwd nt sc1 one-shot`) up to K4's gym step: the same 8-slot ring,
// runs of EPW = 4 rows staged global -> LDS by nontemporal LDS-DMA on the global side's 128-byte lines, write-through (sc1) stores,
// one-shot grid of 4-wave workgroups -- and, rung by rung, the work K4 does on top of the copy:
//   a  copy only
//   b  + the action read (before the run is requested) and the reward write
//   c  + obj read-modify-write AFTER the run has landed
//   d  + the CSR chain rowptr[action] -> col[r0 + lane] and the neighbour gather from LDS AFTER the run has landed, one env after the
//        other, then the flipped byte patched in LDS: K4's order before round 8
//   e  the work of d in K4's order since round 8: obj requested before the run, all rowptr pairs in one batch and all col loads
//        beside the run, ONE wait, gather, obj written from the preloaded value
//   f  e with the per-env outputs leaving once per workgroup: every wave deposits obj_old + delta and reward in an LDS mailbox, the
//        wave that arrives last (LDS fetch-add, no wave waits for another) stores the workgroup's 64 bytes of each array
//   g  f with a shorter trip after landing: all 2 x EPW gather reads issued before one wait, the flip applied in registers in the
//        store loop (no LDS read-modify-write, no wait and wave barrier of its own)
//   h  g with the publisher's two stores write-through (sc1) as well: the launch leaves no dirty line in the L2s
//   i  e (per-wave outputs, no mailbox) with one wait for all 2 x EPW gather reads and the flip as ONE LDS write of the byte the
//        gather has read, no read-modify-write, no wait, no barrier: measured against e
//   j  i with the wave's obj / reward stores write-through (sc1)
//   k  i with the store loop reading 8 pieces of the run from LDS before it stores the first: measured against i
// Round 10 adds, each measured against the rung it is named after:
//   a / b / c / i  xcd-fwd   the same rung with the block order xcd-fwd (see xcd_fwd_block): under round-robin placement one XCD owns a
//                            contiguous eighth of the batch, so every obj / reward line is whole in one L2
//   i  aux A                 rung i with the LDS-DMA cache-policy immediate A (sc0 = 1, nt = 2, sc1 = 16; rung i itself is aux 2)
//   i  side-band nt          rung i with the wave's obj / reward stores nontemporal
// (rungs f - k are a kernel of their own, k_rung_wg; `vs below` of i is against e: the rungs a - e stay the code round 8 measured)
// The graph is synthetic: N nodes of degree 20, node i's row = i + 1 + 97 j mod N, j = 0..19 (N is refused where two of these
// coincide or one is i itself).  16 random action vectors, pass k takes vector k % 16.  All rungs interleaved in one process, 5 rounds
// of 200 passes; the spread of a rung is the max - min of its five rounds.  Before it is timed, every rung's pass 0 is checked against the host: the output slot is the input (rungs d, e: with
// each env's action byte flipped), reward and obj's change are what the rung is meant to compute -- a rung that dropped work fails.
// Build: hipcc --offload-arch=gfx950 -O3 -o /tmp/ring_step_ladder tools/ceilings/ring_step_ladder.hip
// Run:   /tmp/ring_step_ladder [B N [tags]]   (default: the G22 shape 65536 2000; B a multiple of 4, 4 N a multiple of 16; tags: a
//        comma-separated list of the rungs to run, by the tag in front of each row, e.g. a,i,i-sbnt -- the rung a row is measured
//        against is run with it)
#include <hip/hip_runtime.h>
#include <algorithm>
#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <string>
#include <vector>

typedef unsigned int u32x4 __attribute__((ext_vector_type(4)));
constexpr int kWave = 64, kWpb = 4, kPad = 128, kEpw = 4, kDeg = 20;

#define CK(x) do { hipError_t e_ = (x); if (e_ != hipSuccess) { fprintf(stderr, "%s: %s\n", #x, hipGetErrorString(e_)); exit(1); } } while (0)

__device__ __forceinline__ void store16_wt(u32x4* p, u32x4 v) {
    asm volatile("global_store_dwordx4 %0, %1, off sc1\n s_nop 1" :: "v"(p), "v"(v) : "memory");
}

// xcd-fwd: block b -> virtual block; blocks with equal b % 8 (one XCD under round-robin placement) get one contiguous range, in
// order.  A bijection on [0, nvb) for every nvb: the first nvb % 8 classes hold one block more.  Placement is a speed assumption only.
__host__ __device__ inline int64_t xcd_fwd_block(int64_t b, int64_t nvb) {
    const int64_t q = nvb / 8, r = nvb % 8, x = b % 8;
    return x * q + (x < r ? x : r) + b / 8;
}

template <int RUNG, int ORDER = 0>   // 0 .. 4 = a .. e; ORDER 1: xcd-fwd
__global__ __launch_bounds__(256) void k_rung(const unsigned char* __restrict__ xin, unsigned char* __restrict__ xout, int64_t B, int64_t N,
                                              const int32_t* __restrict__ rowptr, const int32_t* __restrict__ col,
                                              const int64_t* __restrict__ action, int32_t* __restrict__ obj, float* __restrict__ reward) {
    extern __shared__ __attribute__((aligned(16))) unsigned char smem[];
    const int lane = threadIdx.x & (kWave - 1);
    const int wib = __builtin_amdgcn_readfirstlane((int)(threadIdx.x / kWave));
    const int64_t vblock = ORDER ? xcd_fwd_block(blockIdx.x, gridDim.x) : (int64_t)blockIdx.x;
    const int64_t b0 = (vblock * kWpb + wib) * kEpw;
    if (b0 >= B) return;
    const int nenv = (int)((B - b0) < kEpw ? (B - b0) : kEpw);
    const int64_t nvec = (int64_t)nenv * N / 16;
    const u32x4* src = reinterpret_cast<const u32x4*>(xin + b0 * N);
    u32x4* dst = reinterpret_cast<u32x4*>(xout + b0 * N);
    const int h_in = (int)((reinterpret_cast<uintptr_t>(src) >> 4) & 7), h_out = (int)((reinterpret_cast<uintptr_t>(dst) >> 4) & 7);
    u32x4* region = reinterpret_cast<u32x4*>(smem + (size_t)wib * ((size_t)kEpw * N + kPad));
    u32x4* stage_v = region + h_in;
    unsigned char* stage = reinterpret_cast<unsigned char*>(stage_v);

    int64_t act[kEpw];
#pragma unroll
    for (int k = 0; k < kEpw; ++k) {
        act[k] = -1;
        if constexpr (RUNG >= 1) {
            const int64_t a = (k < nenv) ? action[b0 + k] : -1;
            act[k] = ((uint64_t)a < (uint64_t)N) ? a : -1;
        }
    }
    int obj_old = 0;
    if constexpr (RUNG == 4) {
        const int32_t* po = obj + b0 + (lane < nenv ? lane : 0);
        asm volatile("global_load_dword %0, %1, off" : "=v"(obj_old) : "v"(po) : "memory");
    }
    for (int64_t s0 = 0; s0 < nvec + h_in; s0 += kWave) {
        const int64_t i = s0 + lane - h_in;
        if (i >= 0 && i < nvec)
            __builtin_amdgcn_global_load_lds((const __attribute__((address_space(1))) void*)(src + i),
                                             (__attribute__((address_space(3))) void*)(region + s0), 16, 0, 2);
    }
    int r0[kEpw], deg[kEpw], nb[kEpw];
#pragma unroll
    for (int k = 0; k < kEpw; ++k) { r0[k] = 0; deg[k] = 0; nb[k] = 0; }
    if constexpr (RUNG == 4) {
#pragma unroll
        for (int k = 0; k < kEpw; ++k) {
            const int64_t ai = act[k] < 0 ? 0 : act[k];
            r0[k] = rowptr[ai];
            deg[k] = rowptr[ai + 1];
        }
        __builtin_amdgcn_sched_barrier(0);
#pragma unroll
        for (int k = 0; k < kEpw; ++k) {
            deg[k] -= r0[k];
            if (act[k] >= 0 && deg[k] > 0) {
                const int32_t* pn = col + r0[k] + (lane < deg[k] ? lane : 0);
                asm volatile("global_load_dword %0, %1, off" : "=v"(nb[k]) : "v"(pn) : "memory");
            }
        }
    }
    asm volatile("s_waitcnt vmcnt(0) lgkmcnt(0)" ::: "memory");     // the run has landed (rung e: and every operand with it)
    __builtin_amdgcn_wave_barrier();
    if constexpr (RUNG == 3) {
#pragma unroll
        for (int k = 0; k < kEpw; ++k)
            if (act[k] >= 0) {
                r0[k] = rowptr[act[k]];
                deg[k] = rowptr[act[k] + 1] - r0[k];
                if (lane < deg[k]) nb[k] = col[r0[k] + lane];
            }
        asm volatile("s_waitcnt vmcnt(0) lgkmcnt(0)" ::: "memory");
    }
    int my_delta = 0;
    if constexpr (RUNG >= 3) {
        if constexpr (RUNG == 4) {
            asm volatile("" : "+v"(obj_old) :: "memory");
#pragma unroll
            for (int k = 0; k < kEpw; ++k) asm volatile("" : "+v"(nb[k]) :: "memory");
        }
#pragma unroll
        for (int k = 0; k < kEpw; ++k)
            if (act[k] >= 0) {
                const unsigned char* row = stage + (int64_t)k * N;
                const bool xa = row[act[k]] != 0;
                const bool on = lane < deg[k];
                const bool xn = on ? row[nb[k]] != 0 : xa;
                const int d = deg[k] - 2 * __popcll(__builtin_amdgcn_ballot_w64(xn != xa));
                if (lane == k) my_delta = d;
            }
    }
    if constexpr (RUNG >= 1) {
        if (lane < nenv) {
            const int64_t b = b0 + lane;
            int64_t a = -1;
#pragma unroll
            for (int k = 0; k < kEpw; ++k) if (lane == k) a = act[k];
            if constexpr (RUNG <= 2) my_delta = (int)(a & 1) * 2 - 1;
            if constexpr (RUNG == 2 || RUNG == 3) obj[b] = obj[b] + my_delta;
            if constexpr (RUNG == 4) obj[b] = obj_old + my_delta;
            reward[b] = a >= 0 ? (float)my_delta : __builtin_nanf("");
            if constexpr (RUNG >= 3) {
                if (a >= 0) {
                    unsigned char* p = stage + (int64_t)lane * N + a;
                    *p = *p == 0 ? 1 : 0;
                }
            }
        }
        asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory");
        __builtin_amdgcn_wave_barrier();
    }
    for (int64_t s0 = 0; s0 < nvec + h_out; s0 += kWave) {
        const int64_t i = s0 + lane - h_out;
        if (i >= 0 && i < nvec) store16_wt(dst + i, stage_v[i]);
    }
}

__device__ __forceinline__ u32x4 flip_byte(u32x4 v, int word, int sh) {   // logical_not of the byte at bit `sh` of dword `word`
#pragma unroll
    for (int q = 0; q < 4; ++q) {
        const uint32_t d = v[q];
        const uint32_t nb = (((d >> sh) & 0xffu) == 0) ? 1u : 0u;
        const uint32_t nd = (d & ~(0xffu << sh)) | (nb << sh);
        v[q] = (q == word) ? nd : d;
    }
    return v;
}

// bytes of the workgroup's mailbox behind its kWpb stages: obj and reward of kWpb * kEpw envs, the arrival counter
constexpr int kMailbox = kWpb * kEpw * 8 + 16;
constexpr int kStoreBatch = 8;   // rung k: 1 KB pieces read from LDS before the first is stored

template <int RUNG, int AUX = 2, int ORDER = 0, bool SBNT = false>   // 5 .. 10 = f .. k; AUX: LDS-DMA policy; ORDER 1: xcd-fwd; SBNT: obj / reward stored nt
__global__ __launch_bounds__(256) void k_rung_wg(const unsigned char* __restrict__ xin, unsigned char* __restrict__ xout, int64_t B, int64_t N,
                                                 const int32_t* __restrict__ rowptr, const int32_t* __restrict__ col,
                                                 const int64_t* __restrict__ action, int32_t* __restrict__ obj, float* __restrict__ reward) {
    extern __shared__ __attribute__((aligned(16))) unsigned char smem[];
    const int lane = threadIdx.x & (kWave - 1);
    const int wib = __builtin_amdgcn_readfirstlane((int)(threadIdx.x / kWave));
    int* mb_obj = reinterpret_cast<int*>(smem + (size_t)kWpb * ((size_t)kEpw * N + kPad));
    float* mb_rew = reinterpret_cast<float*>(mb_obj + kWpb * kEpw);
    unsigned* mb_arrived = reinterpret_cast<unsigned*>(mb_rew + kWpb * kEpw);
    constexpr bool MAILBOX = RUNG <= 7;                 // f, g, h: outputs once per workgroup; i, j: per wave, as in e
    constexpr bool REGFLIP = RUNG == 6 || RUNG == 7;    // g, h: flip in registers in the store loop
    constexpr bool BLINDFLIP = RUNG >= 8;               // i, j: flip written to LDS from the byte the gather has read
    constexpr bool SC1 = RUNG == 7 || RUNG == 9;        // h, j: obj / reward stored write-through
    if constexpr (MAILBOX) {
        if (threadIdx.x == 0) *mb_arrived = 0;
        __syncthreads();                  // before any load is issued; a wave without a run leaves only behind it
    }
    const int64_t wg_b0 = (ORDER ? xcd_fwd_block(blockIdx.x, gridDim.x) : (int64_t)blockIdx.x) * kWpb * kEpw;
    const int64_t b0 = wg_b0 + (int64_t)wib * kEpw;
    if (b0 >= B) return;
    const int64_t wg_runs = (B - wg_b0 + kEpw - 1) / kEpw;
    const unsigned expected = (unsigned)(wg_runs < kWpb ? wg_runs : kWpb);      // the waves of this workgroup that have a run
    const int nenv = (int)((B - b0) < kEpw ? (B - b0) : kEpw);
    const int64_t nvec = (int64_t)nenv * N / 16;
    const u32x4* src = reinterpret_cast<const u32x4*>(xin + b0 * N);
    u32x4* dst = reinterpret_cast<u32x4*>(xout + b0 * N);
    const int h_in = (int)((reinterpret_cast<uintptr_t>(src) >> 4) & 7), h_out = (int)((reinterpret_cast<uintptr_t>(dst) >> 4) & 7);
    u32x4* region = reinterpret_cast<u32x4*>(smem + (size_t)wib * ((size_t)kEpw * N + kPad));
    u32x4* stage_v = region + h_in;
    unsigned char* stage = reinterpret_cast<unsigned char*>(stage_v);

    int64_t act[kEpw];
#pragma unroll
    for (int k = 0; k < kEpw; ++k) {
        const int64_t a = (k < nenv) ? action[b0 + k] : -1;
        act[k] = ((uint64_t)a < (uint64_t)N) ? a : -1;
    }
    // where the flips fall in the run (rungs g, h), worked out while the run is in flight: piece of the store loop, lane, dword, bit (a run is < 2^31 bytes)
    int fj[kEpw], fl[kEpw], fq[kEpw], fsh[kEpw];
#pragma unroll
    for (int k = 0; k < kEpw; ++k) {
        const int rel = act[k] < 0 ? 0 : k * (int)N + (int)act[k];
        const int slot = (rel >> 4) + (int)((reinterpret_cast<uintptr_t>(xout + b0 * N) >> 4) & 7);      // + h_out
        fj[k] = act[k] < 0 ? -1 : slot >> 6; fl[k] = slot & 63; fq[k] = (rel >> 2) & 3; fsh[k] = (rel & 3) * 8;
    }
    int obj_old;
    {
        const int32_t* po = obj + b0 + (lane < nenv ? lane : 0);
        asm volatile("global_load_dword %0, %1, off" : "=v"(obj_old) : "v"(po) : "memory");
    }
    for (int64_t s0 = 0; s0 < nvec + h_in; s0 += kWave) {
        const int64_t i = s0 + lane - h_in;
        if (i >= 0 && i < nvec)
            __builtin_amdgcn_global_load_lds((const __attribute__((address_space(1))) void*)(src + i),
                                             (__attribute__((address_space(3))) void*)(region + s0), 16, 0, AUX);
    }
    int r0[kEpw], deg[kEpw], nb[kEpw];
#pragma unroll
    for (int k = 0; k < kEpw; ++k) {
        const int64_t ai = act[k] < 0 ? 0 : act[k];
        r0[k] = rowptr[ai];
        deg[k] = rowptr[ai + 1];
    }
    __builtin_amdgcn_sched_barrier(0);
#pragma unroll
    for (int k = 0; k < kEpw; ++k) {
        nb[k] = 0;
        deg[k] -= r0[k];
        if (act[k] >= 0 && deg[k] > 0) {
            const int32_t* pn = col + r0[k] + (lane < deg[k] ? lane : 0);
            asm volatile("global_load_dword %0, %1, off" : "=v"(nb[k]) : "v"(pn) : "memory");
        }
    }
    if constexpr (REGFLIP) {
#pragma unroll
        for (int k = 0; k < kEpw; ++k) asm volatile("" : "+s"(fj[k]), "+s"(fl[k]), "+s"(fq[k]), "+s"(fsh[k]));    // (computed HERE, not sunk behind the wait)
    }
    asm volatile("s_waitcnt vmcnt(0) lgkmcnt(0)" ::: "memory");     // the run has landed, and every operand with it
    __builtin_amdgcn_wave_barrier();
    asm volatile("" : "+v"(obj_old) :: "memory");
#pragma unroll
    for (int k = 0; k < kEpw; ++k) asm volatile("" : "+v"(nb[k]) :: "memory");
    int my_delta = 0;
    unsigned char ba[kEpw], bn[kEpw];
    if constexpr (RUNG == 5) {
#pragma unroll
        for (int k = 0; k < kEpw; ++k)
            if (act[k] >= 0) {
                const unsigned char* row = stage + (int64_t)k * N;
                const bool xa = row[act[k]] != 0;
                const bool on = lane < deg[k];
                const bool xn = on ? row[nb[k]] != 0 : xa;
                const int d = deg[k] - 2 * __popcll(__builtin_amdgcn_ballot_w64(xn != xa));
                if (lane == k) my_delta = d;
            }
    } else {
        // every read of the gather before one wait: the indices are in bounds whatever the action (an invalid one reads byte 0 of
        // its row; a lane past the row's end holds the row's first neighbour, a node without neighbours 0)
#pragma unroll
        for (int k = 0; k < kEpw; ++k) {
            const unsigned char* row = stage + (int64_t)k * N;
            ba[k] = row[act[k] < 0 ? 0 : act[k]];
            bn[k] = row[nb[k]];
        }
#pragma unroll
        for (int k = 0; k < kEpw; ++k) {
            const bool xa = ba[k] != 0, xn = bn[k] != 0;
            const int d = deg[k] - 2 * __popcll(__builtin_amdgcn_ballot_w64(lane < deg[k] && xn != xa));
            if (lane == k && act[k] >= 0) my_delta = d;
        }
    }
    int64_t a = -1;
#pragma unroll
    for (int k = 0; k < kEpw; ++k) if (lane == k) a = act[k];
    if constexpr (!MAILBOX) {
        // i, j: the wave publishes its own entries as in e; the flip is ONE LDS write of the byte the gather has read already (lane k
        // holds env k's), with no read, no wait and no barrier of its own -- a wave's LDS instructions execute in order, so the store
        // loop's reads, issued later, see it
        if (lane < nenv) {
            const int v = obj_old + my_delta;
            const float r = a >= 0 ? (float)my_delta : __builtin_nanf("");
            if constexpr (SC1) {
                asm volatile("global_store_dword %0, %1, off sc1" :: "v"(obj + b0 + lane), "v"(v) : "memory");
                asm volatile("global_store_dword %0, %1, off sc1" :: "v"(reward + b0 + lane), "v"(r) : "memory");
            } else if constexpr (SBNT) {
                __builtin_nontemporal_store(v, obj + b0 + lane);
                __builtin_nontemporal_store(r, reward + b0 + lane);
            } else {
                obj[b0 + lane] = v;
                reward[b0 + lane] = r;
            }
            unsigned char old = 0;
#pragma unroll
            for (int k = 0; k < kEpw; ++k) if (lane == k) old = ba[k];
            if (a >= 0) stage[(int64_t)lane * N + a] = old == 0 ? 1 : 0;
        }
        __builtin_amdgcn_wave_barrier();
        if constexpr (RUNG >= 10) {
            // k: the store loop reads kStoreBatch pieces from LDS before it stores the first (an LDS read of a clamped index needs no
            // branch): the reads' latencies overlap instead of one round trip per 1 KB piece
            const int nv = (int)nvec;
            for (int s0 = 0; s0 < nv + h_out; s0 += kStoreBatch * kWave) {
                u32x4 v[kStoreBatch];
#pragma unroll
                for (int q = 0; q < kStoreBatch; ++q) {
                    const int i = s0 + q * kWave + lane - h_out;
                    v[q] = stage_v[i < 0 ? 0 : (i < nv ? i : nv - 1)];
                }
#pragma unroll
                for (int q = 0; q < kStoreBatch; ++q) {
                    const int i = s0 + q * kWave + lane - h_out;
                    if (i >= 0 && i < nv) store16_wt(dst + i, v[q]);
                }
            }
            return;
        }
        for (int64_t s0 = 0; s0 < nvec + h_out; s0 += kWave) {
            const int64_t i = s0 + lane - h_out;
            if (i >= 0 && i < nvec) store16_wt(dst + i, stage_v[i]);
        }
        return;
    }
    if (lane < nenv) {
        mb_obj[wib * kEpw + lane] = obj_old + my_delta;
        mb_rew[wib * kEpw + lane] = a >= 0 ? (float)my_delta : __builtin_nanf("");
        if constexpr (RUNG == 5) {
            if (a >= 0) {
                unsigned char* p = stage + (int64_t)lane * N + a;
                *p = *p == 0 ? 1 : 0;
            }
        }
    }
    // arrive: this wave's deposits are released (nothing is outstanding on the vector counter here, so the fence costs the LDS wait
    // that rung e has at this point anyway); the fetch-add's answer is not looked at before the run's stores have been issued
    __builtin_amdgcn_fence(__ATOMIC_RELEASE, "workgroup");
    unsigned before = 0;
    if (lane == 0) before = __hip_atomic_fetch_add(mb_arrived, 1u, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_WORKGROUP);
    if constexpr (RUNG == 5) __builtin_amdgcn_wave_barrier();
    if constexpr (RUNG == 5) {
        for (int64_t s0 = 0; s0 < nvec + h_out; s0 += kWave) {
            const int64_t i = s0 + lane - h_out;
            if (i >= 0 && i < nvec) store16_wt(dst + i, stage_v[i]);
        }
    } else {
        // (piece j of the store loop holds vector fv at lane fl of piece fj: a scalar compare per env and piece, the lane compare and
        // the flip only in the one piece that holds it -- a per-lane `i == fv[k]` costs the loop a vector compare and a branch per env)
        const int nv = (int)nvec;
        for (int j = 0; j * kWave < nv + h_out; ++j) {
            const int i = j * kWave + lane - h_out;
            if (i >= 0 && i < nv) {
                u32x4 v = stage_v[i];
#pragma unroll
                for (int k = 0; k < kEpw; ++k)
                    if (j == fj[k]) {
                        if (lane == fl[k]) v = flip_byte(v, fq[k], fsh[k]);
                    }
                store16_wt(dst + i, v);
            }
        }
    }
    before = (unsigned)__builtin_amdgcn_readfirstlane((int)before);
    if (before + 1 == expected) {        // wave-uniform: the last arriver publishes the workgroup's entries, one store per array
        __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "workgroup");     // (this wave only: the others wait for nothing)
        const int64_t left = B - wg_b0;
        const int n_wg = (int)(left < kWpb * kEpw ? left : kWpb * kEpw);
        if (lane < n_wg) {
            const int v = mb_obj[lane];
            const float r = mb_rew[lane];
            if constexpr (SC1) {
                asm volatile("global_store_dword %0, %1, off sc1" :: "v"(obj + wg_b0 + lane), "v"(v) : "memory");
                asm volatile("global_store_dword %0, %1, off sc1" :: "v"(reward + wg_b0 + lane), "v"(r) : "memory");
            } else {
                obj[wg_b0 + lane] = v;
                reward[wg_b0 + lane] = r;
            }
        }
    }
}

typedef void (*KernFn)(const unsigned char*, unsigned char*, int64_t, int64_t, const int32_t*, const int32_t*, const int64_t*, int32_t*, float*);

int main(int argc, char** argv) {
    const int64_t B = argc >= 3 ? atoll(argv[1]) : 65536, N = argc >= 3 ? atoll(argv[2]) : 2000;
    const size_t lds = (size_t)kWpb * (kEpw * N + kPad);
    bool rows_ok = N > kDeg;
    for (int j = 0; j < kDeg && rows_ok; ++j) {
        rows_ok = (1 + 97 * j) % N != 0;                                              // never the node itself
        for (int j2 = 0; j2 < j && rows_ok; ++j2) rows_ok = (97 * (j - j2)) % N != 0;  // 20 distinct neighbours
    }
    if (B <= 0 || B % kEpw || (kEpw * N) % 16 || !rows_ok || lds + kMailbox > 160 * 1024) {
        fprintf(stderr, "need B a multiple of 4, 4 N a multiple of 16, an N at which i + 1 + 97 j mod N (j < 20) are 20 nodes other "
                        "than i, and 4 staged runs within 160 KB of LDS\n");
        return 1;
    }
    // kind: what pass 0 must have computed -- 0 copy, 1 + reward, 2 + obj, 3 the gain and the flip
    struct Rung { const char* tag; const char* name; KernFn fn; int kind; bool mailbox; const char* below; };
    const std::vector<Rung> ALL = {
        {"a", "a  copy only", k_rung<0>, 0, false, "a"},
        {"b", "b  + action read, reward write", k_rung<1>, 1, false, "a"},
        {"c", "c  + obj read-modify-write after the run", k_rung<2>, 2, false, "b"},
        {"d", "d  + rowptr -> col chain, gather, flip after the run (serial per env)", k_rung<3>, 3, false, "c"},
        {"e", "e  the work of d, operands requested beside the run", k_rung<4>, 3, false, "d"},
        {"f", "f  e, obj / reward leave once per workgroup (LDS mailbox, last arriver stores)", k_rung_wg<5>, 3, true, "e"},
        {"g", "g  f, one wait for all gather reads, flip in registers in the store loop", k_rung_wg<6>, 3, true, "f"},
        {"h", "h  g, the publisher's stores write-through (sc1)", k_rung_wg<7>, 3, true, "g"},
        {"i", "i  e, one wait for all gather reads, flip = one LDS write of the byte read (vs e)", k_rung_wg<8>, 3, false, "e"},
        {"j", "j  i, the wave's obj / reward stores write-through (sc1)", k_rung_wg<9>, 3, false, "i"},
        {"k", "k  i, the store loop reads 8 pieces from LDS before it stores the first (vs i)", k_rung_wg<10>, 3, false, "i"},
        {"a-x", "a  xcd-fwd (vs a)", k_rung<0, 1>, 0, false, "a"},
        {"b-x", "b  xcd-fwd (vs b)", k_rung<1, 1>, 1, false, "b"},
        {"c-x", "c  xcd-fwd (vs c)", k_rung<2, 1>, 2, false, "c"},
        {"i-x", "i  xcd-fwd (vs i)", k_rung_wg<8, 2, 1>, 3, false, "i"},
        {"i-aux0", "i  aux 0: default policy (vs i)", k_rung_wg<8, 0>, 3, false, "i"},
        {"i-aux1", "i  aux 1: sc0 (vs i)", k_rung_wg<8, 1>, 3, false, "i"},
        {"i-aux3", "i  aux 3: sc0 nt (vs i)", k_rung_wg<8, 3>, 3, false, "i"},
        {"i-aux16", "i  aux 16: sc1 (vs i)", k_rung_wg<8, 16>, 3, false, "i"},
        {"i-aux17", "i  aux 17: sc0 sc1 (vs i)", k_rung_wg<8, 17>, 3, false, "i"},
        {"i-aux18", "i  aux 18: nt sc1 (vs i)", k_rung_wg<8, 18>, 3, false, "i"},
        {"i-aux19", "i  aux 19: sc0 nt sc1 (vs i)", k_rung_wg<8, 19>, 3, false, "i"},
        {"i-sbnt", "i  side-band nt: obj / reward stored nontemporal (vs i)", k_rung_wg<8, 2, 0, true>, 3, false, "i"},
    };
    std::vector<Rung> R;
    {
        const std::string want = argc >= 4 ? std::string(",") + argv[3] + "," : "";
        auto asked = [&](const char* tag) { return want.empty() || want.find(std::string(",") + tag + ",") != std::string::npos; };
        for (const Rung& r : ALL) {
            bool take = asked(r.tag);
            for (const Rung& o : ALL) take = take || (asked(o.tag) && std::string(o.below) == r.tag);
            if (take) R.push_back(r);
        }
        if (R.empty()) { fprintf(stderr, "no rung has one of the tags %s\n", argv[3]); return 1; }
    }
    const int NR = (int)R.size();
    auto lds_of = [&](int r) { return R[r].mailbox ? lds + kMailbox : lds; };
    auto below_of = [&](int r) { for (int o = 0; o < NR; ++o) if (std::string(R[o].tag) == R[r].below) return o; return r; };
    for (const Rung& r : R) CK(hipFuncSetAttribute((const void*)r.fn, hipFuncAttributeMaxDynamicSharedMemorySize, 160 * 1024));

    // graph: node i's row = i + 1 + 97 j mod N, j = 0..19 (distinct and never i itself: checked above)
    std::vector<int32_t> h_rowptr(N + 1), h_col((size_t)N * kDeg);
    for (int64_t i = 0; i <= N; ++i) h_rowptr[i] = (int32_t)(i * kDeg);
    for (int64_t i = 0; i < N; ++i)
        for (int j = 0; j < kDeg; ++j) h_col[i * kDeg + j] = (int32_t)((i + 1 + 97 * j) % N);
    const int NA = 16;
    std::vector<int64_t> h_act((size_t)NA * B);
    uint64_t s = 0x9E3779B97F4A7C15ull;
    for (auto& a : h_act) { s = s * 6364136223846793005ull + 1442695040888963407ull; a = (int64_t)((s >> 33) % (uint64_t)N); }
    int32_t *rowptr, *col, *obj; int64_t* action; float* reward;
    CK(hipMalloc(&rowptr, h_rowptr.size() * 4)); CK(hipMalloc(&col, h_col.size() * 4)); CK(hipMalloc(&action, h_act.size() * 8));
    CK(hipMalloc(&obj, B * 4)); CK(hipMalloc(&reward, B * 4));
    CK(hipMemcpy(rowptr, h_rowptr.data(), h_rowptr.size() * 4, hipMemcpyHostToDevice));
    CK(hipMemcpy(col, h_col.data(), h_col.size() * 4, hipMemcpyHostToDevice));
    CK(hipMemcpy(action, h_act.data(), h_act.size() * 8, hipMemcpyHostToDevice));
    CK(hipMemset(obj, 0, B * 4));

    const size_t bytes = (size_t)B * N;
    const int S = 8;
    unsigned char* slot[S];
    for (int i = 0; i < S; ++i) { CK(hipMalloc(&slot[i], bytes)); CK(hipMemset(slot[i], 0, bytes)); }
    std::vector<unsigned char> h_in(bytes), h_out(bytes);
    for (auto& v : h_in) { s = s * 6364136223846793005ull + 1442695040888963407ull; v = (unsigned char)((s >> 40) & 1); }
    CK(hipMemcpy(slot[0], h_in.data(), bytes, hipMemcpyHostToDevice));   // every later slot derives from this one
    const unsigned grid = (unsigned)((B / kEpw + kWpb - 1) / kWpb);
    {   // pass 0 of every rung against the host
        std::vector<int32_t> h_obj(B);
        std::vector<float> h_rew(B);
        for (int r = 0; r < NR; ++r) {
            CK(hipMemset(obj, 0, B * 4)); CK(hipMemset(reward, 0xff, B * 4)); CK(hipMemset(slot[1], 2, bytes));
            hipLaunchKernelGGL(R[r].fn, dim3(grid), dim3(kWpb * kWave), lds_of(r), 0, slot[0], slot[1], B, N, rowptr, col, action, obj, reward);
            CK(hipDeviceSynchronize());
            CK(hipMemcpy(h_out.data(), slot[1], bytes, hipMemcpyDeviceToHost));
            CK(hipMemcpy(h_obj.data(), obj, B * 4, hipMemcpyDeviceToHost));
            CK(hipMemcpy(h_rew.data(), reward, B * 4, hipMemcpyDeviceToHost));
            long long bad_bytes = 0, bad_env = 0;
            for (int64_t b = 0; b < B; ++b) {
                const int64_t a = h_act[b];
                const unsigned char* row = &h_in[b * N];
                int want = 0;
                const int kind = R[r].kind;
                if (kind >= 3) {
                    int cut = 0;
                    for (int j = 0; j < kDeg; ++j) cut += row[h_col[a * kDeg + j]] != row[a];
                    want = kDeg - 2 * cut;
                } else if (kind >= 1) {
                    want = (int)(a & 1) * 2 - 1;
                }
                for (int64_t i = 0; i < N; ++i) {
                    const unsigned char w = (kind >= 3 && i == a) ? (row[i] == 0 ? 1 : 0) : row[i];
                    bad_bytes += h_out[b * N + i] != w;
                }
                if (kind >= 1 && h_rew[b] != (float)want) ++bad_env;
                if (h_obj[b] != (kind >= 2 ? want : 0)) ++bad_env;
            }
            if (bad_bytes || bad_env) { fprintf(stderr, "rung %s: %lld wrong output bytes, %lld wrong reward / obj entries\n", R[r].tag, bad_bytes, bad_env); return 1; }
        }
        printf("pass 0 of every rung equals the host's result (output slot, reward, obj)\n");
        CK(hipMemset(obj, 0, B * 4));
    }
    const int passes = 200;
    hipEvent_t e0, e1; CK(hipEventCreate(&e0)); CK(hipEventCreate(&e1));
    std::vector<std::vector<float>> us(NR);
    for (int rep = 0; rep < 5; ++rep)
        for (int r = 0; r < NR; ++r) {
            auto pass = [&](int k) {
                hipLaunchKernelGGL(R[r].fn, dim3(grid), dim3(kWpb * kWave), lds_of(r), 0, slot[k % S], slot[(k + 1) % S], B, N, rowptr, col,
                                   action + (size_t)(k % NA) * B, obj, reward);
            };
            for (int k = 0; k < 16; ++k) pass(k);
            CK(hipEventRecord(e0));
            for (int k = 0; k < passes; ++k) pass(k);
            CK(hipEventRecord(e1));
            CK(hipEventSynchronize(e1));
            CK(hipGetLastError());
            float ms; CK(hipEventElapsedTime(&ms, e0, e1));
            us[r].push_back(ms * 1e3f / passes);
        }
    printf("B = %lld, N = %lld bytes, EPW = %d, degree %d: slot %.1f MB, %u workgroups; %d passes per timing, 5 interleaved rounds\n",
           (long long)B, (long long)N, kEpw, kDeg, bytes / 1e6, grid, passes);
    printf("%-8s %-78s %8s %8s %8s %9s %9s %7s %8s\n", "tag", "rung", "us min", "us med", "us max", "vs below", "vs a", "spread", "wg / CU");
    std::vector<float> med(NR, 0.f);
    float base = 0;
    for (int r = 0; r < NR; ++r) { auto t = us[r]; std::sort(t.begin(), t.end()); med[r] = t[2]; }
    for (int r = 0; r < NR; ++r) {
        auto t = us[r];
        std::sort(t.begin(), t.end());
        if (r == 0) base = t[2];
        int per_cu = 0;     // resident workgroups per CU at this rung's LDS size
        CK(hipOccupancyMaxActiveBlocksPerMultiprocessor(&per_cu, (const void*)R[r].fn, kWpb * kWave, lds_of(r)));
        printf("%-8s %-78s %8.2f %8.2f %8.2f %+9.2f %+9.2f %7.2f %8d\n", R[r].tag, R[r].name, t[0], t[2], t[4], t[2] - med[below_of(r)],
               t[2] - base, t[4] - t[0], per_cu);
    }
    return 0;
}
