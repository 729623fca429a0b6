// Chained-ring ceiling: K4's exact memory pattern without the gain.  8 slots of B*N bytes; pass k reads slot k % 8 and writes
// slot (k + 1) % 8, so every pass reads what the previous pass has just written (the rollout ring of bench.py).  One wave owns
// EPW consecutive rows (a run of EPW*N bytes), staged global -> LDS by LDS-DMA with 16-byte lanes and streamed LDS -> global,
// instruction boundaries on the global side's 128-byte lines (K4 MODE 2).  Variants:
//   order   fwd       every pass walks the runs from run 0 up (K4 before round 7)
//           alt       odd passes walk them from the last run down (virtual block vb -> nvb - 1 - vb)
//           alt-xcd   odd passes reversed in groups of 8 blocks: vb -> 8 (nvb/8 - 1 - vb/8) + vb % 8 (forward remainder), so that
//                     under round-robin placement a run is read on the XCD that wrote it
//   load    nt (aux = 2) | def (aux = 0)
//   store   plain | nt | sc1 | sc0sc1
//   grid    one-shot (one run per wave) | persist (resident workgroups, waves loop over runs)
// plus `indep`: the same kernel over 8 independent (src, dst) pairs -- nothing a pass reads was written by the pass before.
// Build: hipcc --offload-arch=gfx950 -O3 -o /tmp/ring_copy tools/ceilings/ring_copy.hip
// Run:   /tmp/ring_copy [B N EPW] ...   (default: the G22 shape 65536 2000 4 and the G70 shard 131072 10000 1)
#include <hip/hip_runtime.h>
#include <algorithm>
#include <cstdio>
#include <cstdlib>
#include <vector>

typedef unsigned int u32x4 __attribute__((ext_vector_type(4)));
constexpr int kWave = 64, kWpb = 4, kPad = 128;

#define CK(x) do { hipError_t e_ = (x); if (e_ != hipSuccess) { fprintf(stderr, "%s: %s\n", #x, hipGetErrorString(e_)); exit(1); } } while (0)

__device__ __forceinline__ int64_t map_vblock(int64_t vb, int64_t nvb, int order) {
    if (order == 1) return nvb - 1 - vb;
    if (order == 2) {
        const int64_t g = nvb / 8;
        return vb < 8 * g ? 8 * (g - 1 - vb / 8) + vb % 8 : vb;
    }
    return vb;
}

template <int ST> __device__ __forceinline__ void store16(u32x4* p, u32x4 v) {
    if constexpr (ST == 0) *p = v;
    else if constexpr (ST == 1) __builtin_nontemporal_store(v, p);
    else if constexpr (ST == 2) asm volatile("global_store_dwordx4 %0, %1, off sc1\n s_nop 1" :: "v"(p), "v"(v) : "memory");
    else asm volatile("global_store_dwordx4 %0, %1, off sc0 sc1\n s_nop 1" :: "v"(p), "v"(v) : "memory");
}

template <int AUX, int ST>
__global__ __launch_bounds__(256) void k_ring(const unsigned char* __restrict__ xin, unsigned char* __restrict__ xout, int64_t B,
                                              int64_t N, int epw, int order) {
    extern __shared__ __attribute__((aligned(16))) unsigned char smem[];
    const int lane = threadIdx.x & (kWave - 1);
    const int wib = __builtin_amdgcn_readfirstlane((int)(threadIdx.x / kWave));
    const int64_t run_bytes = (int64_t)epw * N;
    const int64_t nruns = (B + epw - 1) / epw, nvb = (nruns + kWpb - 1) / kWpb;
    u32x4* region = reinterpret_cast<u32x4*>(smem + (size_t)wib * (run_bytes + kPad));
    for (int64_t vb = blockIdx.x; vb < nvb; vb += gridDim.x) {
        const int64_t run = map_vblock(vb, nvb, order) * kWpb + wib;
        if (run >= nruns) continue;
        const int64_t b0 = run * epw;
        const int64_t nvec = ((B - b0) < epw ? (B - b0) : epw) * N / 16;
        const u32x4* src = reinterpret_cast<const u32x4*>(xin + b0 * N);
        u32x4* dst = reinterpret_cast<u32x4*>(xout + b0 * N);
        const int h_in = (int)((reinterpret_cast<uintptr_t>(src) >> 4) & 7), h_out = (int)((reinterpret_cast<uintptr_t>(dst) >> 4) & 7);
        for (int64_t s0 = 0; s0 < nvec + h_in; s0 += kWave) {
            const int64_t i = s0 + lane - h_in;
            if (i >= 0 && i < nvec)
                __builtin_amdgcn_global_load_lds((const __attribute__((address_space(1))) void*)(src + i),
                                                 (__attribute__((address_space(3))) void*)(region + s0), 16, 0, AUX);
        }
        asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
        __builtin_amdgcn_wave_barrier();
        const u32x4* stage = region + h_in;
        for (int64_t s0 = 0; s0 < nvec + h_out; s0 += kWave) {
            const int64_t i = s0 + lane - h_out;
            if (i >= 0 && i < nvec) store16<ST>(dst + i, stage[i]);
        }
        asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory");
        __builtin_amdgcn_wave_barrier();   // the stage is refilled by the next trip's LDS-DMA
    }
}

__global__ void k_xcc(int* out) {
    if (threadIdx.x == 0) {
        int id;
        asm volatile("s_getreg_b32 %0, hwreg(HW_REG_XCC_ID)" : "=s"(id));
        out[blockIdx.x] = id & 15;
    }
}

typedef void (*KernFn)(const unsigned char*, unsigned char*, int64_t, int64_t, int, int);
struct Variant { const char* order; int ord; const char* load; const char* store; KernFn fn; bool persist; bool indep; };

int main(int argc, char** argv) {
    std::vector<int64_t> shapes = {65536, 2000, 4, 131072, 10000, 1};
    if (argc >= 4) { shapes.clear(); for (int i = 1; i + 2 < argc; i += 3) for (int k = 0; k < 3; ++k) shapes.push_back(atoll(argv[i + k])); }
    int dev_cus = 0;
    CK(hipDeviceGetAttribute(&dev_cus, hipDeviceAttributeMultiprocessorCount, 0));

    {   // placement check (speed only): is block b on the XCD of block b % 8?
        const int nb = 4096;
        int* d; CK(hipMalloc(&d, nb * sizeof(int)));
        hipLaunchKernelGGL(k_xcc, dim3(nb), dim3(256), 0, 0, d);
        std::vector<int> h(nb);
        CK(hipMemcpy(h.data(), d, nb * sizeof(int), hipMemcpyDeviceToHost));
        int same = 0;
        for (int b = 0; b < nb; ++b) same += h[b] == h[b % 8];
        printf("placement: %d of %d blocks on the XCD of block b %% 8 (block 0..7 on XCC %d %d %d %d %d %d %d %d)\n", same, nb,
               h[0], h[1], h[2], h[3], h[4], h[5], h[6], h[7]);
        CK(hipFree(d));
    }

    const KernFn K[2][4] = {{k_ring<2, 0>, k_ring<2, 1>, k_ring<2, 2>, k_ring<2, 3>}, {k_ring<0, 0>, k_ring<0, 1>, k_ring<0, 2>, k_ring<0, 3>}};
    const char* LD[2] = {"nt", "def"};
    const char* STN[4] = {"plain", "nt", "sc1", "sc0sc1"};
    const char* ORN[3] = {"fwd", "alt", "alt-xcd"};
    std::vector<Variant> vs;
    for (int p = 0; p < 2; ++p)
        for (int o = 0; o < 3; ++o)
            for (int l = 0; l < 2; ++l)
                for (int s = 0; s < 4; ++s) vs.push_back({ORN[o], o, LD[l], STN[s], K[l][s], p == 1, false});
    vs.push_back({"fwd", 0, "nt", "plain", K[0][0], false, true});
    vs.push_back({"fwd", 0, "nt", "nt", K[0][1], false, true});
    for (auto& v : vs) CK(hipFuncSetAttribute((const void*)v.fn, hipFuncAttributeMaxDynamicSharedMemorySize, 160 * 1024));

    for (size_t si = 0; si < shapes.size(); si += 3) {
        const int64_t B = shapes[si], N = shapes[si + 1];
        const int epw = (int)shapes[si + 2];
        const size_t bytes = (size_t)B * N;
        if (((size_t)epw * N) % 16) { fprintf(stderr, "EPW*N must be a multiple of 16\n"); return 1; }
        const int S = 8;
        unsigned char* slot[S];
        unsigned char* other[S];   // indep: pass k reads slot[k % 8], writes other[k % 8]
        for (int i = 0; i < S; ++i) { CK(hipMalloc(&slot[i], bytes)); CK(hipMalloc(&other[i], bytes)); CK(hipMemset(slot[i], i, bytes)); CK(hipMemset(other[i], 0, bytes)); }
        const size_t lds = (size_t)kWpb * (epw * N + kPad);
        const int64_t nruns = (B + epw - 1) / epw, nvb = (nruns + kWpb - 1) / kWpb;
        const int64_t per_cu = std::min<int64_t>(8, (160 * 1024) / lds);
        const int64_t resident = (int64_t)dev_cus * per_cu;
        const int passes = 200;   // even: the alternating orders end where they started
        hipEvent_t e0, e1; CK(hipEventCreate(&e0)); CK(hipEventCreate(&e1));
        std::vector<std::vector<float>> us(vs.size());
        for (int rep = 0; rep < 5; ++rep)
            for (size_t vi = 0; vi < vs.size(); ++vi) {
                const Variant& v = vs[vi];
                const unsigned grid = (unsigned)(v.persist ? std::min(nvb, resident) : nvb);
                auto pass = [&](int k) {
                    const int ord = (k & 1) ? v.ord : 0;
                    const unsigned char* in = slot[k % S];
                    unsigned char* out = v.indep ? other[k % S] : slot[(k + 1) % S];
                    hipLaunchKernelGGL(v.fn, dim3(grid), dim3(kWpb * kWave), lds, 0, in, out, B, N, epw, ord);
                };
                for (int k = 0; k < 16; ++k) pass(k);
                CK(hipEventRecord(e0));
                for (int k = 0; k < passes; ++k) pass(k);
                CK(hipEventRecord(e1));
                CK(hipEventSynchronize(e1));
                CK(hipGetLastError());
                float ms; CK(hipEventElapsedTime(&ms, e0, e1));
                us[vi].push_back(ms * 1e3f / passes);
            }
        printf("\nB = %lld, N = %lld bytes, EPW = %d: slot %.1f MB, %lld runs, %lld workgroups one-shot / %lld persistent (%d CUs); "
               "%d passes per timing, 5 interleaved rounds\n",
               (long long)B, (long long)N, epw, bytes / 1e6, (long long)nruns, (long long)nvb, (long long)std::min(nvb, resident), dev_cus, passes);
        printf("%-8s %-8s %-5s %-7s %-8s %9s %9s %9s %8s %8s\n", "pattern", "order", "load", "store", "grid", "us min", "us med", "us max",
               "TB/s", "vs base");
        float base = 0;
        for (size_t vi = 0; vi < vs.size(); ++vi) {
            auto t = us[vi];
            std::sort(t.begin(), t.end());
            if (vi == 0) base = t[2];
            const Variant& v = vs[vi];
            printf("%-8s %-8s %-5s %-7s %-8s %9.2f %9.2f %9.2f %8.2f %+7.1f%%\n", v.indep ? "indep" : "chained", v.order, v.load, v.store,
                   v.persist ? "persist" : "one-shot", t[0], t[2], t[4], 2.0 * bytes / t[2] / 1e6, (base / t[2] - 1) * 100);
        }
        for (int i = 0; i < S; ++i) { CK(hipFree(slot[i])); CK(hipFree(other[i])); }
        CK(hipEventDestroy(e0)); CK(hipEventDestroy(e1));
    }
    return 0;
}
