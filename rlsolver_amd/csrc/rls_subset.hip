// sub_set_sampling of the L2A policy step for gfx950 (methods/L2A/transformer.py:335-353; the first box of the loop body of
// L2A/demo_instance.py:141-165): both topk calls, the gather / scatter, start_xs.repeat and the Python loop over top_k columns
// in one kernel.
//
// The rule, quirks included (they are the reference's; keep them): det = |probs - 0.5| (one float32 subtraction); the min(top_k, N)
// nodes of a sim with the smallest det are selected; row r S + s of xs is start_xs[s] except at the selected nodes, where it is
// u < det[s, node] with a fresh uniform per (row, node) -- the Bernoulli parameter is the determinism, not the probability --;
// the returned probs keep the input at the selected nodes and are (p < 0.5 ? 1 : 0) elsewhere.  det >= 0, so its bit pattern
// orders as an unsigned integer with NaN (one canonical pattern) on top, where torch.topk puts it.  TIES at the selection
// boundary go to the LOWER node index (our rule: torch.topk does not specify it).
//
// A workgroup owns one sim and a chunk of its repeats (rls_subset_plan.h).  It keeps the sim's det keys in LDS, finds the k-th
// smallest by four 8-bit histogram passes (two more over the node ids when the boundary value is shared and not all of its nodes are
// taken), compacts the selected nodes into a list once, and then writes its repeats: the start row sits in LDS twice, a repeat
// draws and compares at the k listed nodes only, patches one copy while the other is on its way out in 16-byte stores (cut on the
// destination's alignment, whatever N is), one barrier per repeat.  Every workgroup redoes its sim's selection -- N values -- rather
// than paying a second launch; the chunk-0 workgroup of a sim also writes its probs row.
#include "rls_draw.h"
#include "rls_subset_plan.h"
#include "rls_tile.h"

namespace rls {

struct SubsetBin { uint32_t digit; int want; int bin; };

// One histogram pass of the select: digit(i) = the 8-bit digit of entry i, or -1 when the entry is out of play.  -> the smallest
// digit whose bin, with the bins below it, holds `want` entries; how many of that bin are wanted; the bin's size.
// Determinism rows are lopsided (a softmax sits near 0 | 1: every key shares its high bytes), so a wave first adds up the lanes
// that hold its first lane's digit, twice, and only the rest go to the LDS atomics one by one.
template <typename Digit>
__device__ __forceinline__ SubsetBin subset_hist_pass(int n, int tid, int NT, int lane, int w, SubsetScratch* sc, int want, Digit digit) {
    for (int b = tid; b < 256; b += NT) sc->hist[b] = 0;
    __syncthreads();
    for (int base = w * kWave; base < n; base += NT) {      // (wave-uniform trip count)
        const int i = base + lane;
        const int d = i < n ? digit(i) : -1;
        bool act = d >= 0;
#pragma unroll
        for (int peel = 0; peel < 2; ++peel) {
            const uint64_t m_act = ballot64(act);
            if (m_act == 0) break;
            const int leader = __builtin_ctzll(m_act);
            const int dl = __shfl(d, leader, 64);
            const bool same = act && d == dl;
            const uint64_t m = ballot64(same);
            if (lane == leader) atomicAdd(&sc->hist[dl], __popcll(m));
            act = act && !same;
        }
        if (act) atomicAdd(&sc->hist[d], 1);
    }
    __syncthreads();
    if (w == 0) {
        int c[4], tot = 0;
#pragma unroll
        for (int q = 0; q < 4; ++q) { c[q] = sc->hist[lane * 4 + q]; tot += c[q]; }
        int pre = tot;                                        // inclusive prefix sum over lanes: lanes <= this one
#pragma unroll
        for (int d = 1; d < kWave; d <<= 1) {
            const int o = __shfl_up(pre, d, 64);
            if (lane >= d) pre += o;
        }
        int run = pre - tot;                                  // entries in bins of lower lanes
#pragma unroll
        for (int q = 0; q < 4; ++q) {
            if (run < want && run + c[q] >= want) { sc->digit = (uint32_t)(lane * 4 + q); sc->want = want - run; sc->bin = c[q]; }
            run += c[q];
        }
    }
    __syncthreads();
    return SubsetBin{sc->digit, sc->want, sc->bin};
}

// n bytes of an LDS row to dst (any alignment): 16-byte stores on dst's alignment, the row read as aligned dwords and shifted
// into place; the up to 15 bytes before and after go one by one.
__device__ __forceinline__ void subset_store_row(uint8_t* __restrict__ dst, const uint8_t* buf, int n, int tid, int NT) {
    const int mis = (int)(reinterpret_cast<uintptr_t>(dst) & 15);
    int head = (16 - mis) & 15;
    if (head > n) head = n;
    const int pieces = (n - head) >> 4, tail0 = head + (pieces << 4);
    if (head == 0) {
        for (int p = tid; p < pieces; p += NT) *reinterpret_cast<uint4*>(dst + (p << 4)) = *reinterpret_cast<const uint4*>(buf + (p << 4));
    } else {
        const uint32_t sh = (uint32_t)head & 3u;
        for (int p = tid; p < pieces; p += NT) {
            const int o = head + (p << 4);
            const uint32_t* src = reinterpret_cast<const uint32_t*>(buf + (o & ~3));   // (src[4] lies inside the row's 16 spare bytes)
            const uint32_t w0 = src[0], w1 = src[1], w2 = src[2], w3 = src[3], w4 = src[4];
            uint4 v;
            v.x = __builtin_amdgcn_alignbyte(w1, w0, sh);
            v.y = __builtin_amdgcn_alignbyte(w2, w1, sh);
            v.z = __builtin_amdgcn_alignbyte(w3, w2, sh);
            v.w = __builtin_amdgcn_alignbyte(w4, w3, sh);
            *reinterpret_cast<uint4*>(dst + o) = v;
        }
    }
    const int loose = head + (n - tail0);
    for (int b = tid; b < loose; b += NT) {
        const int o = b < head ? b : tail0 + (b - head);
        dst[o] = buf[o];
    }
}

__global__ __launch_bounds__(1024) void k_sub_set_sampling(const float* __restrict__ probs, const uint8_t* __restrict__ start_xs, int64_t S,
                                                           int64_t N, int64_t R, int k, int64_t repeats,
                                                           const float* __restrict__ uniforms, uint64_t seed, int64_t env_offset,
                                                           uint8_t* __restrict__ xs_out, float* __restrict__ probs_out) {
    extern __shared__ __attribute__((aligned(16))) unsigned char smem[];
    SubsetScratch* sc = reinterpret_cast<SubsetScratch*>(smem);
    uint32_t* keys = reinterpret_cast<uint32_t*>(smem + kSubsetFixed);
    uint8_t* row0 = smem + kSubsetFixed + subset_pad16((size_t)N * 4);
    uint8_t* row1 = row0 + subset_row_bytes(N);
    uint16_t* list = reinterpret_cast<uint16_t*>(row1 + subset_row_bytes(N));
    const int tid = threadIdx.x, NT = blockDim.x, lane = tid & (kWave - 1), w = tid >> 6;
    const int n = (int)N;
    const int64_t s = (int64_t)blockIdx.x % S, chunk = (int64_t)blockIdx.x / S;
    const float* prow = probs + s * N;
    const uint8_t* srow = start_xs + s * N;
    for (int i = tid; i < n; i += NT) {
        const float d = fabsf(prow[i] - 0.5f);
        keys[i] = d != d ? 0x7FC00000u : __float_as_uint(d);     // every NaN is the same key, above +inf
        const uint8_t b = srow[i];
        row0[i] = b;
        row1[i] = b;
    }
    for (int i = n + tid; i < (int)subset_row_bytes(N); i += NT) row0[i] = row1[i] = 0;
    __syncthreads();

    // ---- the k-th smallest key T; of the nodes that hold T, those with ids <= id_cut are selected
    uint32_t T = 0, id_cut = 0xFFFFFFFFu;
    if (k > 0) {
        int want = k, bin = 0;
        for (int shift = 24; shift >= 0; shift -= 8) {
            const uint32_t hi_mask = shift == 24 ? 0u : (0xFFFFFFFFu << (shift + 8));
            const SubsetBin r = subset_hist_pass(n, tid, NT, lane, w, sc, want, [&](int i) {
                const uint32_t key = keys[i];
                return (key & hi_mask) == T ? (int)((key >> shift) & 255u) : -1;
            });
            T |= r.digit << shift;
            want = r.want;
            bin = r.bin;
        }
        if (want < bin) {                                     // (workgroup-uniform) a shared boundary value: the `want` lowest ids
            const SubsetBin hi = subset_hist_pass(n, tid, NT, lane, w, sc, want, [&](int i) { return keys[i] == T ? i >> 8 : -1; });
            const SubsetBin lo = subset_hist_pass(n, tid, NT, lane, w, sc, hi.want,
                                                  [&](int i) { return keys[i] == T && (uint32_t)(i >> 8) == hi.digit ? i & 255 : -1; });
            id_cut = (hi.digit << 8) | lo.digit;
        }
    }

    // ---- the selected nodes, compacted once (any order: a draw is keyed by its node); chunk 0 writes the sim's probs row
    if (tid == 0) sc->count = 0;
    __syncthreads();
    float* pout = (probs_out && chunk == 0) ? probs_out + s * N : nullptr;
    for (int base = w * kWave; base < n; base += NT) {
        const int i = base + lane;
        const uint32_t key = i < n ? keys[i] : 0u;
        const bool sel = i < n && k > 0 && (key < T || (key == T && (uint32_t)i <= id_cut));
        const uint64_t m = ballot64(sel);
        if (m) {
            int at = 0;
            if (lane == 0) at = atomicAdd(&sc->count, __popcll(m));
            at = __shfl(at, 0, 64);
            if (sel) list[at + __popcll(m & ((1ull << lane) - 1ull))] = (uint16_t)i;
        }
        if (pout && i < n) {
            const float p = prow[i];
            pout[i] = sel ? p : (p < 0.5f ? 1.0f : 0.0f);
        }
    }
    __syncthreads();
    const int count = sc->count;                              // == k

    // ---- the repeats of this chunk: patch one copy of the row at the listed nodes, send it off, one barrier each
    const int64_t r0 = chunk * repeats, r1 = r0 + repeats < R ? r0 + repeats : R;
    const uint64_t env = (uint64_t)(env_offset + s);
    const uint32_t env_key = isco_env_key(seed, env);
    for (int64_t r = r0; r < r1; ++r) {
        uint8_t* buf = ((r - r0) & 1) ? row1 : row0;
        const int64_t row = r * S + s;
        if (uniforms) {
            const float* urow = uniforms + row * N;
            for (int j = tid; j < count; j += NT) {
                const int node = list[j];
                buf[node] = urow[node] < __uint_as_float(keys[node]);
            }
        } else {
            const uint32_t pos_key = isco_pos_key(env_key, env, (uint32_t)r);
            for (int j = tid; j < count; j += NT) {
                const int node = list[j];
                buf[node] = isco_unit(isco_draw_at(pos_key, (uint32_t)node, 0u)) < __uint_as_float(keys[node]);
            }
        }
        __syncthreads();
        subset_store_row(xs_out + row * N, buf, n, tid, NT);
    }
}

}  // namespace rls

using namespace rls;

extern "C" {

int rls_sub_set_sampling(const float* probs, const uint8_t* start_xs, int64_t S, int64_t N, int64_t R, int64_t top_k,
                         const float* uniforms, uint64_t seed, int64_t env_offset, uint8_t* xs_out, float* probs_out, void* stream) {
    RLS_REQUIRE(S >= 0 && N >= 1 && R >= 1 && top_k >= 0 && env_offset >= 0, RLS_EINVAL, "bad sizes S=%lld N=%lld R=%lld top_k=%lld env_offset=%lld",
                (long long)S, (long long)N, (long long)R, (long long)top_k, (long long)env_offset);
    RLS_REQUIRE(rls_sub_set_sampling_supported(S, N, R, top_k), RLS_EUNSUPPORTED,
                "S=%lld, N=%lld, R=%lld: a sim's determinism row, two copies of its start row and its selected nodes stay in LDS (%zu bytes "
                "here), N <= %lld; R and S stay below 2^31 and R S N within int64", (long long)S, (long long)N, (long long)R,
                subset_lds_bytes(N < (1ll << 40) ? N : (1ll << 40)), (long long)kSubsetMaxN);
    if (S == 0) return RLS_OK;
    RLS_REQUIRE(probs && start_xs && xs_out, RLS_EINVAL, "NULL pointer");
    const SubsetPlan p = subset_plan(S, N, R, top_k, num_cus());
    if (p.err != RLS_OK) return fail(p.err, "sub_set_sampling: no launch plan for S=%lld N=%lld R=%lld", (long long)S, (long long)N, (long long)R);
    ensure_dyn_lds((const void*)k_sub_set_sampling, p.lds);
    hipLaunchKernelGGL(k_sub_set_sampling, dim3((unsigned)(S * p.chunks)), dim3(p.block), p.lds, as_stream(stream), probs, start_xs, S, N, R,
                       (int)(top_k < N ? top_k : N), p.repeats, uniforms, seed, env_offset, xs_out, probs_out);
    return check_launch("k_sub_set_sampling");
}

}  // extern "C"
