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
// The graph is synthetic: N nodes of degree 20, node i's row = i + 1 + 97 j mod N, j = 0..19 (N is refused where two of these
// coincide or one is i itself).  16 random action vectors, pass k takes vector k % 16.  All rungs interleaved in one process, 5 rounds
// of 200 passes.  Before it is timed, every rung's pass 0 is checked against the host: the output slot is the input (rungs d, e: with
// each env's action byte flipped), reward and obj's change are what the rung is meant to compute -- a rung that dropped work fails.
// Build: hipcc --offload-arch=gfx950 -O3 -o /tmp/ring_step_ladder tools/ceilings/ring_step_ladder.hip
// Run:   /tmp/ring_step_ladder [B N]     (default: the G22 shape 65536 2000; B a multiple of 4, 4 N a multiple of 16)
#include <hip/hip_runtime.h>
#include <algorithm>
#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <vector>

typedef unsigned int u32x4 __attribute__((ext_vector_type(4)));
constexpr int kWave = 64, kWpb = 4, kPad = 128, kEpw = 4, kDeg = 20;

#define CK(x) do { hipError_t e_ = (x); if (e_ != hipSuccess) { fprintf(stderr, "%s: %s\n", #x, hipGetErrorString(e_)); exit(1); } } while (0)

__device__ __forceinline__ void store16_wt(u32x4* p, u32x4 v) {
    asm volatile("global_store_dwordx4 %0, %1, off sc1\n s_nop 1" :: "v"(p), "v"(v) : "memory");
}

template <int RUNG>   // 0 .. 4 = a .. e
__global__ __launch_bounds__(256) void k_rung(const unsigned char* __restrict__ xin, unsigned char* __restrict__ xout, int64_t B, int64_t N,
                                              const int32_t* __restrict__ rowptr, const int32_t* __restrict__ col,
                                              const int64_t* __restrict__ action, int32_t* __restrict__ obj, float* __restrict__ reward) {
    extern __shared__ __attribute__((aligned(16))) unsigned char smem[];
    const int lane = threadIdx.x & (kWave - 1);
    const int wib = __builtin_amdgcn_readfirstlane((int)(threadIdx.x / kWave));
    const int64_t b0 = ((int64_t)blockIdx.x * kWpb + wib) * kEpw;
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

typedef void (*KernFn)(const unsigned char*, unsigned char*, int64_t, int64_t, const int32_t*, const int32_t*, const int64_t*, int32_t*, float*);

int main(int argc, char** argv) {
    const int64_t B = argc >= 3 ? atoll(argv[1]) : 65536, N = argc >= 3 ? atoll(argv[2]) : 2000;
    const size_t lds = (size_t)kWpb * (kEpw * N + kPad);
    bool rows_ok = N > kDeg;
    for (int j = 0; j < kDeg && rows_ok; ++j) {
        rows_ok = (1 + 97 * j) % N != 0;                                              // never the node itself
        for (int j2 = 0; j2 < j && rows_ok; ++j2) rows_ok = (97 * (j - j2)) % N != 0;  // 20 distinct neighbours
    }
    if (B <= 0 || B % kEpw || (kEpw * N) % 16 || !rows_ok || lds > 160 * 1024) {
        fprintf(stderr, "need B a multiple of 4, 4 N a multiple of 16, an N at which i + 1 + 97 j mod N (j < 20) are 20 nodes other "
                        "than i, and 4 staged runs within 160 KB of LDS\n");
        return 1;
    }
    const KernFn K[5] = {k_rung<0>, k_rung<1>, k_rung<2>, k_rung<3>, k_rung<4>};
    const char* NAME[5] = {"a  copy only", "b  + action read, reward write", "c  + obj read-modify-write after the run",
                           "d  + rowptr -> col chain, gather, flip after the run (serial per env)", "e  the work of d, operands requested beside the run"};
    for (auto k : K) CK(hipFuncSetAttribute((const void*)k, hipFuncAttributeMaxDynamicSharedMemorySize, 160 * 1024));

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
        for (int r = 0; r < 5; ++r) {
            CK(hipMemset(obj, 0, B * 4)); CK(hipMemset(reward, 0xff, B * 4)); CK(hipMemset(slot[1], 2, bytes));
            hipLaunchKernelGGL(K[r], dim3(grid), dim3(kWpb * kWave), lds, 0, slot[0], slot[1], B, N, rowptr, col, action, obj, reward);
            CK(hipDeviceSynchronize());
            CK(hipMemcpy(h_out.data(), slot[1], bytes, hipMemcpyDeviceToHost));
            CK(hipMemcpy(h_obj.data(), obj, B * 4, hipMemcpyDeviceToHost));
            CK(hipMemcpy(h_rew.data(), reward, B * 4, hipMemcpyDeviceToHost));
            long long bad_bytes = 0, bad_env = 0;
            for (int64_t b = 0; b < B; ++b) {
                const int64_t a = h_act[b];
                const unsigned char* row = &h_in[b * N];
                int want = 0;
                if (r >= 3) {
                    int cut = 0;
                    for (int j = 0; j < kDeg; ++j) cut += row[h_col[a * kDeg + j]] != row[a];
                    want = kDeg - 2 * cut;
                } else if (r >= 1) {
                    want = (int)(a & 1) * 2 - 1;
                }
                for (int64_t i = 0; i < N; ++i) {
                    const unsigned char w = (r >= 3 && i == a) ? (row[i] == 0 ? 1 : 0) : row[i];
                    bad_bytes += h_out[b * N + i] != w;
                }
                if (r >= 1 && h_rew[b] != (float)want) ++bad_env;
                if (h_obj[b] != (r >= 2 ? want : 0)) ++bad_env;
            }
            if (bad_bytes || bad_env) { fprintf(stderr, "rung %c: %lld wrong output bytes, %lld wrong reward / obj entries\n", 'a' + r, bad_bytes, bad_env); return 1; }
        }
        printf("pass 0 of every rung equals the host's result (output slot, reward, obj)\n");
        CK(hipMemset(obj, 0, B * 4));
    }
    const int passes = 200;
    hipEvent_t e0, e1; CK(hipEventCreate(&e0)); CK(hipEventCreate(&e1));
    std::vector<float> us[5];
    for (int rep = 0; rep < 5; ++rep)
        for (int r = 0; r < 5; ++r) {
            auto pass = [&](int k) {
                hipLaunchKernelGGL(K[r], dim3(grid), dim3(kWpb * kWave), lds, 0, slot[k % S], slot[(k + 1) % S], B, N, rowptr, col,
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
    printf("%-78s %8s %8s %8s %9s %9s\n", "rung", "us min", "us med", "us max", "vs prev", "vs a");
    float prev = 0, base = 0;
    for (int r = 0; r < 5; ++r) {
        auto t = us[r];
        std::sort(t.begin(), t.end());
        if (r == 0) base = t[2];
        printf("%-78s %8.2f %8.2f %8.2f %+9.2f %+9.2f\n", NAME[r], t[0], t[2], t[4], r ? t[2] - prev : 0.f, t[2] - base);
        prev = t[2];
    }
    return 0;
}
