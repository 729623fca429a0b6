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
//        /tmp/ring_copy axes [B N EPW]  the round 10 axes (see k_axes): data pattern of the ring x {chained copy, read only, write
//                                       only}, all eight LDS-DMA load policies x {sc1, plain} stores, block order xcd-fwd, a share of
//                                       the runs stored nontemporal, and the slot size from 0.5 to 1.25 x the shape's
#include <hip/hip_runtime.h>
#include <algorithm>
#include <cstdio>
#include <cstdlib>
#include <string>
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

// ---- round 10 axes: data pattern, load policy, block order xcd-fwd, residency edge, split store policy (run: ring_copy axes) ----
// The ring's content is a pure function of (pattern, run, vector in the run), so the device fills it, the write-only passes produce
// it and the host checks it: dword q of vector i of run r is rotr(mix(((r * 64 + (i & 63)) * 4 + q)), 8 * ((i >> 6) & 3)) & andm | orm.
// (andm, orm) = (0, 0): all 0x00; (0, 0x01010101): all 0x01; (0x01010101, 0): random 0/1 bytes; (~0, 0): random bytes.  The byte
// rotation keeps a lane's value one v_alignbit per dword and piece away from its last: a hash per dword would make the write-only
// pass VALU-bound.
__host__ __device__ inline uint32_t mix32(uint32_t z) {
    z *= 0x9E3779B1u; z ^= z >> 15; z *= 0x85EBCA77u; z ^= z >> 13; z *= 0xC2B2AE3Du; z ^= z >> 16;
    return z;
}
__host__ __device__ inline uint32_t rotr8(uint32_t v, int k) { k &= 3; return k ? (v >> (8 * k)) | (v << (32 - 8 * k)) : v; }
__host__ __device__ inline uint32_t pat_dword(int64_t run, int64_t i, int q, uint32_t andm, uint32_t orm) {
    return (rotr8(mix32((uint32_t)((run * 64 + (i & 63)) * 4 + q)), (int)((i >> 6) & 3)) & andm) | orm;
}

// xcd-fwd: block b -> virtual block; blocks with equal b % 8 (one XCD under round-robin placement) get one contiguous range, in
// order.  A bijection on [0, nvb) for every nvb: the first nvb % 8 classes hold one block more.
__host__ __device__ inline int64_t xcd_fwd_block(int64_t b, int64_t nvb) {
    const int64_t q = nvb / 8, r = nvb % 8, x = b % 8;
    return x * q + (x < r ? x : r) + b / 8;
}

// OP 0 copy | 1 read only (LDS-DMA, nothing stored; `csum` non-null: the wave's xor over its landed run, for the check) |
// 2 write only, the pattern from registers | 3 write only, the pattern written to LDS first and stored from there.
// order 0 fwd | 3 xcd-fwd.  Runs with (run & 7) >= nt_from are stored nontemporal instead of ST (8: none).
template <int AUX, int ST, int OP>
__global__ __launch_bounds__(256) void k_axes(const unsigned char* __restrict__ xin, unsigned char* __restrict__ xout, int64_t B, int64_t N,
                                              int epw, int order, int nt_from, uint32_t andm, uint32_t orm, uint32_t* __restrict__ csum) {
    extern __shared__ __attribute__((aligned(16))) unsigned char smem[];
    const int lane = threadIdx.x & (kWave - 1);
    const int wib = __builtin_amdgcn_readfirstlane((int)(threadIdx.x / kWave));
    const int64_t run_bytes = (int64_t)epw * N;
    const int64_t nruns = (B + epw - 1) / epw, nvb = (nruns + kWpb - 1) / kWpb;
    u32x4* region = reinterpret_cast<u32x4*>(smem + (size_t)wib * (run_bytes + kPad));
    const int64_t vb = order == 3 ? xcd_fwd_block(blockIdx.x, nvb) : (int64_t)blockIdx.x;
    const int64_t run = vb * kWpb + wib;
    if (vb >= nvb || run >= nruns) return;
    const int64_t b0 = run * epw;
    const int64_t nvec = ((B - b0) < epw ? (B - b0) : epw) * N / 16;
    const u32x4* src = reinterpret_cast<const u32x4*>(xin + b0 * N);
    u32x4* dst = reinterpret_cast<u32x4*>(xout + b0 * N);
    const int h_in = (OP <= 1) ? (int)((reinterpret_cast<uintptr_t>(src) >> 4) & 7) : 0;
    const int h_out = (int)((reinterpret_cast<uintptr_t>(dst) >> 4) & 7);
    const bool nt_run = nt_from < 8 && (int)(run & 7) >= nt_from;        // wave-uniform
    if constexpr (OP <= 1) {
        for (int64_t s0 = 0; s0 < nvec + h_in; s0 += kWave) {
            const int64_t i = s0 + lane - h_in;
            if (i >= 0 && i < nvec)
                __builtin_amdgcn_global_load_lds((const __attribute__((address_space(1))) void*)(src + i),
                                                 (__attribute__((address_space(3))) void*)(region + s0), 16, 0, AUX);
        }
        asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
        __builtin_amdgcn_wave_barrier();
    }
    const u32x4* stage = region + h_in;
    if constexpr (OP == 1) {
        if (csum) {
            uint32_t x = 0;
            for (int64_t i = lane; i < nvec; i += kWave) { const u32x4 v = stage[i]; x ^= v[0] ^ v[1] ^ v[2] ^ v[3]; }
            for (int o = 32; o; o >>= 1) x ^= __shfl_xor(x, o);
            if (lane == 0) csum[run] = x;
        }
        return;
    }
    if constexpr (OP == 3) {
        u32x4 v;
        for (int q = 0; q < 4; ++q) v[q] = mix32((uint32_t)((run * 64 + lane) * 4 + q));
        for (int64_t i = lane; i < nvec; i += kWave) {
            u32x4 w;
            for (int q = 0; q < 4; ++q) w[q] = (v[q] & andm) | orm;
            region[i] = w;
            for (int q = 0; q < 4; ++q) v[q] = rotr8(v[q], 1);
        }
        asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory");
        __builtin_amdgcn_wave_barrier();
    }
    u32x4 v{};
    if constexpr (OP == 2) {                                             // lane's vector i = s0 + lane - h_out: (i & 63) is fixed
        const int64_t i0 = (int64_t)lane - h_out;
        for (int q = 0; q < 4; ++q) v[q] = rotr8(mix32((uint32_t)((run * 64 + (i0 & 63)) * 4 + q)), (int)((i0 >> 6) & 3));
    }
    for (int64_t s0 = 0; s0 < nvec + h_out; s0 += kWave) {
        const int64_t i = s0 + lane - h_out;
        u32x4 w;
        if constexpr (OP == 2) {
            for (int q = 0; q < 4; ++q) { w[q] = (v[q] & andm) | orm; v[q] = rotr8(v[q], 1); }
        }
        if (i >= 0 && i < nvec) {
            if constexpr (OP != 2) w = stage[i];
            if (nt_run) store16<1>(dst + i, w); else store16<ST>(dst + i, w);
        }
    }
}

typedef void (*AxFn)(const unsigned char*, unsigned char*, int64_t, int64_t, int, int, int, uint32_t, uint32_t, uint32_t*);
struct AxVariant {
    const char* section; char name[96];
    AxFn fn; int op; int pat; int order; int nt_from; bool same_slot; int64_t B;
};

static void fill_host(std::vector<uint32_t>& h, int64_t B, int64_t N, int epw, uint32_t andm, uint32_t orm) {
    const int64_t run_vec = (int64_t)epw * N / 16, nruns = B / epw;
    h.resize((size_t)B * N / 4);
    for (int64_t r = 0; r < nruns; ++r)
        for (int64_t i = 0; i < run_vec; ++i)
            for (int q = 0; q < 4; ++q) h[(size_t)(r * run_vec + i) * 4 + q] = pat_dword(r, i, q, andm, orm);
}

// The round 10 tables at the shape (B, N, epw); B a multiple of 16 * epw so that every scaled batch keeps whole runs.
static int run_axes(int64_t B0, int64_t N, int epw) {
    const uint32_t ANDM[4] = {0u, 0u, 0x01010101u, 0xffffffffu}, ORM[4] = {0u, 0x01010101u, 0u, 0u};
    const char* PAT[4] = {"0x00", "0x01", "rand01", "randbyte"};
    const int AUXV[8] = {0, 1, 2, 3, 16, 17, 18, 19};
    const char* AUXN[8] = {"-", "sc0", "nt", "sc0 nt", "sc1", "sc0 sc1", "nt sc1", "sc0 nt sc1"};
    const AxFn COPY[8][2] = {{k_axes<0, 2, 0>, k_axes<0, 0, 0>},   {k_axes<1, 2, 0>, k_axes<1, 0, 0>},   {k_axes<2, 2, 0>, k_axes<2, 0, 0>},
                             {k_axes<3, 2, 0>, k_axes<3, 0, 0>},   {k_axes<16, 2, 0>, k_axes<16, 0, 0>}, {k_axes<17, 2, 0>, k_axes<17, 0, 0>},
                             {k_axes<18, 2, 0>, k_axes<18, 0, 0>}, {k_axes<19, 2, 0>, k_axes<19, 0, 0>}};
    const AxFn READ = k_axes<2, 2, 1>, WREG = k_axes<2, 2, 2>, WLDS = k_axes<2, 2, 3>, FILL = k_axes<2, 0, 2>;
    const double SCALE[7] = {0.5, 0.75, 0.9, 1.0, 1.02, 1.1, 1.25};
    auto scaled = [&](double f) { const int64_t g = 16 * epw; return (int64_t)(B0 * f / g + 0.5) * g; };
    const int64_t Bmax = scaled(1.25);
    std::vector<AxVariant> vs;
    auto add = [&](const char* sec, AxFn fn, int op, int pat, int order, int nt_from, bool same, int64_t B, const char* fmt, auto... a) {
        AxVariant v{sec, {0}, fn, op, pat, order, nt_from, same, B};
        snprintf(v.name, sizeof v.name, fmt, a...);
        vs.push_back(v);
    };
    for (int p = 0; p < 4; ++p) {
        add("pattern", COPY[2][0], 0, p, 0, 8, false, B0, "%-8s chained copy, nt loads, sc1 stores", PAT[p]);
        add("pattern", READ, 1, p, 0, 8, false, B0, "%-8s read only, the 8 slots in turn (nt)", PAT[p]);
        add("pattern", READ, 1, p, 0, 8, true, B0, "%-8s read only, one slot again and again (nt)", PAT[p]);
        add("pattern", WREG, 2, p, 0, 8, false, B0, "%-8s write only, sc1, from registers", PAT[p]);
        add("pattern", WLDS, 3, p, 0, 8, false, B0, "%-8s write only, sc1, from LDS", PAT[p]);
    }
    for (int s = 0; s < 2; ++s)
        for (int a = 0; a < 8; ++a)
            add("policy", COPY[a][s], 0, 2, 0, 8, false, B0, "rand01   chained copy, load aux %2d (%s), store %s", AUXV[a], AUXN[a], s ? "plain" : "sc1");
    add("order", COPY[2][0], 0, 2, 0, 8, false, B0, "rand01   chained copy, nt / sc1, order fwd");
    add("order", COPY[2][0], 0, 2, 3, 8, false, B0, "rand01   chained copy, nt / sc1, order xcd-fwd");
    const int NTF[3] = {4, 6, 7};
    const char* NTN[3] = {"1/2", "3/4", "7/8"};
    for (int k = 0; k < 3; ++k)
        add("split", COPY[2][0], 0, 2, 0, NTF[k], false, B0, "rand01   chained copy, %s of the runs sc1, the rest nt", NTN[k]);
    for (int k = 0; k < 7; ++k)
        add("size", COPY[2][0], 0, 2, 0, 8, false, scaled(SCALE[k]), "rand01   chained copy, nt / sc1, slot x %.2f", SCALE[k]);
    for (auto& v : vs) CK(hipFuncSetAttribute((const void*)v.fn, hipFuncAttributeMaxDynamicSharedMemorySize, 160 * 1024));
    CK(hipFuncSetAttribute((const void*)FILL, hipFuncAttributeMaxDynamicSharedMemorySize, 160 * 1024));

    const int S = 8;
    const size_t max_bytes = (size_t)Bmax * N;
    unsigned char* slot[S];
    for (int i = 0; i < S; ++i) CK(hipMalloc(&slot[i], max_bytes));
    uint32_t* csum; CK(hipMalloc(&csum, (size_t)(Bmax / epw) * 4));
    const size_t lds = (size_t)kWpb * (epw * N + kPad);
    auto grid_of = [&](int64_t B) { return (unsigned)((B / epw + kWpb - 1) / kWpb); };
    int cur_pat = -1; int64_t cur_B = -1;
    auto set_ring = [&](int pat, int64_t B) {          // every slot holds the pattern
        if (pat == cur_pat && B == cur_B) return;
        for (int i = 0; i < S; ++i)
            hipLaunchKernelGGL(FILL, dim3(grid_of(B)), dim3(kWpb * kWave), lds, 0, nullptr, slot[i], B, N, epw, 0, 8, ANDM[pat], ORM[pat], nullptr);
        cur_pat = pat; cur_B = B;
    };
    auto pass = [&](const AxVariant& v, int k, uint32_t* cs) {
        const unsigned char* in = slot[v.same_slot ? 0 : k % S];
        unsigned char* out = slot[(k + 1) % S];
        hipLaunchKernelGGL(v.fn, dim3(grid_of(v.B)), dim3(kWpb * kWave), lds, 0, in, out, v.B, N, epw, v.order, v.nt_from, ANDM[v.pat],
                           ORM[v.pat], cs);
    };
    {   // pass 0 of every variant against the host
        std::vector<uint32_t> want, got, hcs;
        int want_pat = -1; int64_t want_B = -1;
        for (auto& v : vs) {
            if (v.pat != want_pat || v.B != want_B) { fill_host(want, v.B, N, epw, ANDM[v.pat], ORM[v.pat]); want_pat = v.pat; want_B = v.B; }
            const size_t bytes = (size_t)v.B * N;
            set_ring(v.pat, v.B);
            CK(hipMemset(slot[1], 0xEE, bytes));
            CK(hipMemset(csum, 0, (size_t)(v.B / epw) * 4));
            pass(v, 0, v.op == 1 ? csum : nullptr);
            CK(hipDeviceSynchronize());
            long long bad = 0;
            if (v.op == 1) {
                const int64_t nruns = v.B / epw, run_dw = (int64_t)epw * N / 4;
                hcs.resize(nruns);
                CK(hipMemcpy(hcs.data(), csum, nruns * 4, hipMemcpyDeviceToHost));
                for (int64_t r = 0; r < nruns; ++r) {
                    uint32_t x = 0;
                    for (int64_t d = 0; d < run_dw; ++d) x ^= want[(size_t)(r * run_dw + d)];
                    bad += x != hcs[r];
                }
            } else {
                got.resize(bytes / 4);
                CK(hipMemcpy(got.data(), slot[1], bytes, hipMemcpyDeviceToHost));
                for (size_t d = 0; d < bytes / 4; ++d) bad += got[d] != want[d];
            }
            if (bad) { fprintf(stderr, "%s: %lld wrong %s in pass 0\n", v.name, bad, v.op == 1 ? "run checksums" : "output dwords"); return 1; }
            cur_pat = -1;                         // (slot 1 holds 0xEE bytes after a read-only check: the ring is set again)
        }
        printf("\npass 0 of every variant of the axes equals the host's pattern (output slot; read only: every run's xor)\n");
    }
    const int passes = 200;
    hipEvent_t e0, e1; CK(hipEventCreate(&e0)); CK(hipEventCreate(&e1));
    std::vector<std::vector<float>> us(vs.size());
    for (int rep = 0; rep < 5; ++rep)
        for (size_t vi = 0; vi < vs.size(); ++vi) {
            const AxVariant& v = vs[vi];
            set_ring(v.pat, v.B);
            for (int k = 0; k < 16; ++k) pass(v, k, nullptr);
            CK(hipEventRecord(e0));
            for (int k = 0; k < passes; ++k) pass(v, k, nullptr);
            CK(hipEventRecord(e1));
            CK(hipEventSynchronize(e1));
            CK(hipGetLastError());
            float ms; CK(hipEventElapsedTime(&ms, e0, e1));
            us[vi].push_back(ms * 1e3f / passes);
        }
    printf("axes at B = %lld, N = %lld bytes, EPW = %d (slot %.2f MB; `size` rows scale B); one-shot grid; %d passes per timing, 5 interleaved "
           "rounds over all rows; spread = max - min; TB/s counts the bytes the row moves (copy: read + written)\n",
           (long long)B0, (long long)N, epw, (double)B0 * N / 1e6, passes);
    printf("%-8s %-64s %8s %8s %8s %7s %8s %9s\n", "axis", "variant", "us min", "us med", "us max", "spread", "TB/s", "us / MB");
    for (size_t vi = 0; vi < vs.size(); ++vi) {
        auto t = us[vi];
        std::sort(t.begin(), t.end());
        const AxVariant& v = vs[vi];
        const double mb = (double)v.B * N / 1e6;
        printf("%-8s %-64s %8.2f %8.2f %8.2f %7.2f %8.2f %9.4f\n", v.section, v.name, t[0], t[2], t[4], t[4] - t[0],
               (v.op == 0 ? 2.0 : 1.0) * mb / t[2], t[2] / mb);
    }
    for (int i = 0; i < S; ++i) CK(hipFree(slot[i]));
    CK(hipFree(csum));
    CK(hipEventDestroy(e0)); CK(hipEventDestroy(e1));
    return 0;
}

int main(int argc, char** argv) {
    if (argc >= 2 && std::string(argv[1]) == "axes")
        return argc >= 5 ? run_axes(atoll(argv[2]), atoll(argv[3]), atoi(argv[4])) : run_axes(65536, 2000, 4);
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
