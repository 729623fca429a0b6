// The launch policy of the local-search entry points (rls_maxcut_local_search, _ls_threshold, _ls_propose, _ls_rounds): which tile class
// an N falls in, which kernels run in which order with which template arguments, grid, LDS and runtime ints -- as pure functions of
// the shape, the tuning knobs and the CU count.  Plain C++ (no HIP): rls_localsearch.hip launches what these return, the four host
// queries (_local_search_supported, _ls_rounds_supported, _ls_scratch_bytes, _ls_slices) and rls_maxcut_ls_launch_plan answer with the
// same functions, and a host-only program can include this file.  Limits in the comments: at 256 CUs (tests/golden/ls_launch_plans.json.gz).
#pragma once
#include "rls_maxcut_plan.h"

namespace rls {
constexpr int kLsMergeWaves = 4;   // waves that own the top-k merge and the batched sweep; a fused tile runs on 4 or 8 waves
constexpr int kLsRoundWaves = 8;   // waves of the round kernels (threshold, mask, propose, apply)
constexpr int kTopCap = 16;        // num_spin + 1 <= kTopCap
constexpr int kPlanRingMaxRun = kPlanRing / 8;   // what rls_ring.h calls kRingMaxRun (rls_localsearch.hip asserts that they agree)
constexpr size_t kLsMaxMaskBytes = (size_t)1 << 30;   // all rounds' mask words at once only while they stay under 1 GiB

struct LsShape {
    int64_t N, B, E, G, ws_pitch;   // nodes, envs, stored edges, sweep groups, entries between two rows of ws (never 0 here)
    int ws_bytes, num_spin, num_draws, max_degree, cus;
    bool weighted, has_levels, has_batches;   // rls_graph.wgt, sweep_lv_*, sweep_rowptr / _stream
    bool x_aligned, noise16, pitch_ok;   // tile_rows_aligned of x; noise on a 16-byte base; ws rows a multiple of 16 bytes apart on one
    bool scratch_ok;   // scratch present and 16-byte aligned
    size_t scratch_bytes;
};
// which kernels an N's proposal rounds take: k_ls_propose's tile with its stages (N <= 15 872; the fused kernel covers the lower part
// of that range), else through the mask words -- the bare 4-wave 64-env tile, half tiles, K6 on narrow tiles -- or nothing
enum LsClass { LS_PROPOSE, LS_BIG64, LS_HALF, LS_NARROW, LS_NONE };
enum LsKernel { LSK_FUSED, LSK_THRESHOLD, LSK_THRESHOLD_MERGE, LSK_MASK, LSK_PROPOSE, LSK_APPLY, LSK_APPLY32, LSK_K6 };
struct LsTile {
    int cls, slices;                // LsClass; workgroups per tile of the noise passes.  (Fused-capable, on 8 or 4 waves: ls_fused_waves -- by N, B and the CUs)
    bool propose_sd_lds;            // k_ls_propose keeps rd_std in LDS (N <= 10 580)
    bool sd_lds, passes_fit;        // the threshold and mask kernels do (N <= 24 576); past it the passes fit only with N % 4 == 0
};
typedef rls_ls_launch LsLaunch;   // include/rlsolver_hip.h: kernel (LsKernel), template arguments, grid, block, LDS, the kernel's runtime ints
struct LsPlan {   // the launches of one call: l[0 .. n), `repeat` times over, the draw advancing by `per_launch` each time
    int err, n, repeat, per_launch;   // err: RLS_OK, or what the entry point returns with `msg`
    LsLaunch l[2];
    char msg[288];
};
constexpr size_t ls_sd_bytes(int64_t N) { return (size_t)((N + 3) & ~3ll) * 4; }   // rd_std, whole quads
inline int64_t ls_chunks(int64_t N, int ws_bytes) { return (N * ws_bytes + 63) >> 6; }   // ls_num_chunks of the kernels: 64 bytes of a ws row
inline size_t ls_apply32_lds(int64_t N, bool stage) { return tile_lds(N, 4, kLsRoundWaves, stage ? stages(kLsRoundWaves) : 0); }
inline size_t ls_apply_lds(int64_t N, int W, bool stage) { return tile_lds((N + 1) & ~1ll, 8, W, stage ? stages(W) : 0); }
inline size_t ls_propose_lds(int64_t N, bool sd_lds) { return ls_apply_lds(N, kLsRoundWaves, true) + (sd_lds ? ls_sd_bytes(N) : 0); }
// rd_std beside the lists and the stages (sd_lds), or read from global memory where 4 N bytes do not fit (needs N % 4 == 0).  (The
// lane = node mask kernel keeps nothing in LDS -- rd_std in registers, ws read as it lies -- and takes its SD_LDS from here.)
inline size_t ls_threshold_lds(int64_t N, bool sd_lds) { return (size_t)kLsRoundWaves * kTopCap * kWave * 4 + stages(kLsRoundWaves) + (sd_lds ? ls_sd_bytes(N) : 0); }
// LDS bytes of the fused kernel's W-wave layout (W = 4: compact, the sweep offsets reuse the proposal tile; W = 8: separate tables)
inline size_t ls_fused_lds(int64_t N, int W) {
#ifdef RLS_LS_ROUND_LANE_ENV
    const size_t sd4 = ls_sd_bytes(N);
#else
    const size_t sd4 = 0;   // (the compact layout keeps rd_std in the proposal tile)
#endif
    const size_t tiles = (size_t)(N + 2) * 8 + (size_t)N * 8 + (size_t)kPlanRing * 4 + (size_t)W * kWave * 8;
    return W == kLsMergeWaves ? sd4 + tiles : ls_sd_bytes(N) + tiles + (size_t)kLsMergeWaves * kTopCap * kWave * 4;
}
// Waves per fused tile.  What counts is waves per SIMD (the VALU issues a wave's stream at ~5 cycles per instruction and two or more
// waves' at ~2.6: tools/ceilings/valu_issue.hip): 8 waves when a CU holds one tile anyway -- at most one tile per CU in the launch, or
// rows so long that two 4-wave layouts do not fit LDS (N > 3172) -- else 4 waves and two tiles per CU.  Measured
// (tools/timing/ls_waves.py): G22-sized 2^14 envs 0.53 -> 0.46 ms with 8, 2^15 0.83 -> 0.72 with 4; G(5000, 20000) 2^16 4.02 -> 3.13
// with 8.  The 8-wave layout fits up to N = 6348, the 4-wave one up to 7268.  0 = neither layout fits.
inline int ls_fused_waves(int64_t N, int64_t B, int cus) {
    const int force_w = (int)knob(KN_LS_WAVES, 0);   // dev knob
    // (which graphs the fused kernel takes, and from where two 4-wave tiles share a CU, is decided on the layout WITH rd_std's own
    // 4N bytes, as until round 6: the compact layout now keeps rd_std inside the proposal tile and launches with less, but the
    // rows that gains -- N ~ 6500 .. 9000, one tile per CU -- are rows the round kernels win on (envs/env_L2A.py))
    auto fit = [&](int w) { return ls_fused_lds(N, w) + (w == kLsMergeWaves ? ls_sd_bytes(N) : 0); };
    int W = force_w == 4 || force_w == 8 ? force_w : (ceil_div(B, kWave) <= (int64_t)cus || !fits_lds(2 * fit(4)) ? 8 : 4);
    if (W == 8 && !fits_lds(fit(8))) W = 4;
    return fits_lds(fit(W)) ? W : 0;
}
// workgroups per tile for the noise passes: 1 once the tiles alone fill the chip, else up to 8 slices of the rows
inline int ls_slices(int64_t B, int64_t nchunks, int cus) {
    const int force = (int)knob(KN_LS_SLICES, 0);   // dev knob
    const int64_t tiles = ceil_div(B, kWave);
    int S = force > 0 ? force : (int)(cus / (tiles > 0 ? tiles : 1));
    if (S > 8) S = 8;
    if ((int64_t)S * 2 * kLsRoundWaves > nchunks) S = (int)(nchunks / (2 * kLsRoundWaves));   // a slice keeps every wave busy
    return S < 1 ? 1 : S;
}
inline LsTile ls_tile(const LsShape& s) {
    const int64_t N = s.N;
    LsTile t{};
    // N beyond the proposal kernel's tile + stages but within the bare tile (15 872 < N <= 20 224): mask kernels + the 4-wave apply kernel
    // (rows of 16- or 8-byte multiples take half tiles there instead: their loader keeps 64-byte runs, the bare tile's reads 16 B per
    // env).  N past the 64-env tile altogether but within the half tile (20 224 < N <= 39 936): mask kernels + the apply kernel on half
    // tiles.  N past the half tile too, within the narrow tiles (rls_tile32.h: 16 / 8 envs per workgroup; 39 936 < N <= 159 740): mask
    // kernels, then every round's proposal through K6 on narrow tiles with the mask words as its bit-packed mask (round 5; such
    // graphs ran the search as torch ops on [B, N] float tensors around K6: 16.6 ms for 4096 envs at N = 44 000)
    t.cls = fits_lds(ls_propose_lds(N, false))                                ? LS_PROPOSE
            : fits_lds(ls_apply_lds(N, 4, false)) && (N & 7) != 0             ? LS_BIG64
            : fits_lds(ls_apply32_lds(N, false))                              ? LS_HALF
            : fits_lds(tile_lds(N + 2, 1, 8)) && knob(KN_NARROW_TILE, 1) != 0 ? LS_NARROW
                                                                              : LS_NONE;
    t.propose_sd_lds = !knob_on(KN_LS_SD_GLOBAL) && fits_lds(ls_propose_lds(N, true));   // (dev knob: rd_std from global memory even where it fits)
    t.sd_lds = fits_lds(ls_threshold_lds(N, true));   // (the threshold kernel is the larger)
    t.passes_fit = t.sd_lds || (N & 3) == 0;
    t.slices = ls_slices(s.B, ls_chunks(N, s.ws_bytes), s.cus);
    return t;
}
inline bool ls_masked(int cls) { return cls == LS_BIG64 || cls == LS_HALF || cls == LS_NARROW; }   // the rounds run through the mask words
inline size_t ls_round_bytes(const LsShape& s) { return (size_t)ceil_div(s.B, kWave) * (size_t)s.N * 8; }   // one round's mask words
// scratch for S slices: the partial top-k lists, and the mask words of `rounds` rounds at once
inline size_t ls_scratch_need(const LsShape& s, int S, int rounds = 1) {
    const size_t one = ls_round_bytes(s), all = one * (size_t)(rounds > 1 ? rounds : 1);
    const size_t lists = S > 1 ? (size_t)ceil_div(s.B, kWave) * S * kTopCap * kWave * 4 : 0;
    // one round's words when the noise pass is split (S > 1); every round's whenever more than one is asked for and they fit
    const size_t masks = rounds > 1 ? (all <= kLsMaxMaskBytes ? all : (S > 1 ? one : 0)) : (S > 1 ? all : 0);
    return lists > masks ? lists : masks;
}
// what rls_maxcut_ls_scratch_bytes answers: where the mask words are how the rounds run at all, at least one round's
inline size_t ls_scratch_bytes(const LsShape& s) {
    const LsTile t = ls_tile(s);
    const size_t need = ls_scratch_need(s, t.slices, s.num_draws), one = ls_round_bytes(s);
    return ls_masked(t.cls) && one > need ? one : need;
}
inline int ls_slices_with(const LsShape& s, int S) { return !s.scratch_ok || s.scratch_bytes < ls_scratch_need(s, S) ? 1 : S; }   // without the scratch: one workgroup per tile
template <typename... A>
inline LsPlan ls_refuse(const char* fmt, A... args) { LsPlan p; p.err = RLS_EUNSUPPORTED; p.n = p.repeat = 0; p.per_launch = 1; snprintf(p.msg, sizeof(p.msg), fmt, args...); return p; }
inline LsPlan ls_refuse_pitch(const LsShape& s) { return ls_refuse("ws rows must start 16-byte aligned: pitch %lld entries of %d bytes (N=%lld)", (long long)s.ws_pitch, s.ws_bytes, (long long)s.N); }
inline LsPlan ls_refuse_spin(const LsShape& s) { return ls_refuse("num_spin=%d outside [0, %d] (and < N)", s.num_spin, kTopCap - 1); }
inline bool ls_spin_ok(const LsShape& s) { return s.num_spin >= 0 && s.num_spin + 1 <= kTopCap && s.num_spin < s.N; }
inline LsLaunch ls_launch(int kernel, const LsShape& s, int width, int waves, size_t lds, int gy = 1, int gz = 1) {
    LsLaunch l{};
    l.kernel = kernel; l.waves = waves; l.lds = (int64_t)lds; l.x_aligned = s.x_aligned; l.block = (uint32_t)(waves * kWave);
    l.grid[0] = (uint32_t)ceil_div(s.B, width); l.grid[1] = (uint32_t)gy; l.grid[2] = (uint32_t)gz;
    return l;
}
// (a plan is built on every call of a launcher: nothing of it is zeroed that is not read)
inline LsPlan ls_plan_of(const LsLaunch& a, int repeat = 1, int per_launch = 1) { LsPlan p; p.err = RLS_OK; p.n = 1; p.repeat = repeat; p.per_launch = per_launch; p.l[0] = a; p.msg[0] = 0; return p; }
inline LsPlan ls_plan_of(const LsLaunch& a, const LsLaunch& b, int repeat = 1, int per_launch = 1) { LsPlan p = ls_plan_of(a, repeat, per_launch); p.n = 2; p.l[1] = b; return p; }

// ---- rls_maxcut_local_search ----
inline LsPlan plan_ls_fused(const LsShape& s) {
    const int64_t N = s.N;
    if (!ls_spin_ok(s)) return ls_refuse_spin(s);
    if (s.weighted || s.max_degree >= kPlanRingMaxRun) return ls_refuse("fused local search needs an unweighted graph with max degree < %d", kPlanRingMaxRun);
    // x and noise: rows that start 4-byte aligned on 16-byte bases (N % 4 == 0).  ws is read in 16-byte pieces, the last piece
    // of a row included: its rows sit ws_pitch entries apart, a multiple of 16 bytes (rls_maxcut_ls_weights writes that layout),
    // so no piece leaves its row -- an exactly sized [B, N] array whose rows are not 16-byte multiples is refused, not over-read
    if (!s.pitch_ok)
        return ls_refuse("fused local search reads ws in 16-byte pieces: rows must sit a multiple of 16 bytes apart on a 16-byte base "
                         "(ws_pitch=%lld entries of %d bytes, N=%lld)", (long long)s.ws_pitch, s.ws_bytes, (long long)N);
    // (an element-wise form for rows that are not dword-aligned existed until round 3: 180 - 300 KB per instantiation, and slower
    // there than the round kernels, which read the weights on a padded pitch -- so the kernel's ALIGNED is always true)
    if (!(s.x_aligned && s.noise16))
        return ls_refuse("fused local search needs rows of x and noise that start 4-byte aligned on 16-byte bases "
                         "(N=%lld): rls_maxcut_ls_threshold / rls_maxcut_ls_rounds take any layout", (long long)N);
    const int W = ls_fused_waves(N, s.B, s.cus), P = plan_planes(s.E);
    if (W == 0) return ls_refuse("N=%lld needs %zu B of LDS (max %d)", (long long)N, ls_fused_lds(N, 4), kLdsBytes);
    if (P == 0) return ls_refuse("E'=%lld too large", (long long)s.E);
    LsLaunch l = ls_launch(LSK_FUSED, s, kWave, W, ls_fused_lds(N, W));
    // two counter widths (the 12- and 20-plane forms of the edge counter save a few carry steps per 1024 edges: not worth
    // a second pair of 190 KB kernels each)
    l.ws_bytes = s.ws_bytes; l.planes = P == 12 || P == 16 ? 16 : 24;
    // sweep schedule: 2 level groups (lane = node) | 1 level schedule stream (lane = env) | 0 the CSR as it is
    const bool levels = !knob_on(KN_SWEEP_NO_LEVELS) && s.has_levels && s.G > 0 && s.G <= N;   // (SWEEP_NO_LEVELS: dev knob)
    l.batched = levels ? 2 : (s.has_batches ? 1 : 0);
    return ls_plan_of(l);
}
// what rls_maxcut_local_search_supported answers: the plan for well-laid-out arguments (rows that are not dword-aligned take the round
// kernels: any N, and faster there than an element-wise fused form was)
inline bool ls_fused_supported(LsShape s) { s.pitch_ok = s.noise16 = true; s.x_aligned = (s.N & 3) == 0; return plan_ls_fused(s).err == RLS_OK; }

// ---- rls_maxcut_ls_threshold ----
inline LsPlan plan_ls_threshold(const LsShape& s) {
    if (!ls_spin_ok(s)) return ls_refuse_spin(s);
    if (!s.pitch_ok) return ls_refuse_pitch(s);
    const LsTile t = ls_tile(s);
    if (!t.passes_fit) return ls_refuse("N=%lld: rd_std does not fit LDS and N is not a multiple of 4", (long long)s.N);
    const int S = ls_slices_with(s, t.slices);
    LsLaunch th = ls_launch(LSK_THRESHOLD, s, kWave, kLsRoundWaves, ls_threshold_lds(s.N, t.sd_lds), S);
    th.ws_bytes = s.ws_bytes; th.sd_lds = t.sd_lds;
    if (S == 1) return ls_plan_of(th);
    LsLaunch merge = ls_launch(LSK_THRESHOLD_MERGE, s, kWave, 1, 0);   // (reads the threshold off the S slices' lists)
    merge.rounds = S;
    return ls_plan_of(th, merge);
}

// ---- rls_maxcut_ls_rounds: num_draws proposal rounds.  One round per k_ls_propose launch (behind a k_ls_mask launch when the scratch lets the noise pass split), or -- a batch with
// scratch for all rounds' mask words, and every N past the propose tile -- the mask words of `per_launch` rounds from one launch
// (blockIdx.z = round), applied on one load of the tile.  Same result either way.
inline LsPlan plan_ls_rounds(const LsShape& s) {
    const int64_t N = s.N;
    const LsTile t = ls_tile(s);
    const bool masked = ls_masked(t.cls);
    if ((t.cls == LS_HALF || t.cls == LS_NARROW) && !t.passes_fit) return ls_refuse("N=%lld: rd_std does not fit LDS and N is not a multiple of 4", (long long)N);
    const size_t one_round = ls_round_bytes(s);
    const int P = plan_planes(s.E);
    const bool scratch_ok = s.scratch_ok && s.pitch_ok && P != 0;
    if (masked && !(scratch_ok && s.scratch_bytes >= one_round))
        return ls_refuse("N=%lld: the proposal rounds need %zu bytes of scratch (rls_maxcut_ls_scratch_bytes) and ws rows on a 16-byte pitch", (long long)N, one_round);
    const bool per_round = knob_on(KN_LS_PER_ROUND);   // dev knob: one propose launch per round
    const bool all_at_once = !per_round && s.num_draws > 1 && scratch_ok && s.scratch_bytes >= one_round * (size_t)s.num_draws && t.cls != LS_NONE;
    if (!all_at_once && !masked) {
        if (!s.pitch_ok) return ls_refuse_pitch(s);
        if (t.cls == LS_NONE) return ls_refuse("N=%lld needs %zu B of LDS (max %d)", (long long)N, ls_propose_lds(N, false), kLdsBytes);
        if (P == 0) return ls_refuse("E'=%lld too large", (long long)s.E);
        const int S = ls_slices_with(s, t.slices);
        // (one counter width: the round is bound by its noise generation, the few carry steps a narrower counter saves per 1024
        // edges do not show, and every instantiation is ~40 KB)
        const bool sd_lds = S == 1 && t.propose_sd_lds;
        LsLaunch pr = ls_launch(LSK_PROPOSE, s, kWave, kLsRoundWaves, ls_propose_lds(N, sd_lds));
        pr.planes = 24; pr.sd_lds = sd_lds; pr.premask = S > 1;
        pr.ws_bytes = S > 1 ? 1 : s.ws_bytes;   // (WT and SD_LDS play no part once the mask is given)
        if (S == 1) return ls_plan_of(pr, s.num_draws);
        LsLaunch mk = ls_launch(LSK_MASK, s, kWave, kLsRoundWaves, 0, S);   // the mask words first, S workgroups per tile
        mk.ws_bytes = s.ws_bytes; mk.sd_lds = 1; mk.rounds = 1;
        return ls_plan_of(mk, pr, s.num_draws);
    }
    const int per_launch = all_at_once ? s.num_draws : 1;   // rounds whose mask words are in the scratch at once
    LsLaunch mk = ls_launch(LSK_MASK, s, kWave, kLsRoundWaves, 0, t.slices, per_launch), ap;
    mk.ws_bytes = s.ws_bytes; mk.sd_lds = t.sd_lds; mk.rounds = per_launch; mk.round_words = (int64_t)mk.grid[0] * N;
    // half tiles (twice the workgroups, the same mask words): past the 64-env tile, and for batches that leave half the CUs
    // without a 64-env tile (whole local_search_inplace calls, 4096 envs: G22-sized 0.324 -> 0.305 ms, BA n = 10^4 0.893 -> 0.816,
    // G70-sized 0.689 -> 0.642; at 16 384 envs no gain).  Dev knob RLS_LS_APPLY32 = 0 | 1 forces the choice.  Their row-piece stages
    // (rows of 8-byte multiples on an aligned base) fit up to N = 31 744.
    const int knob32 = (int)knob(KN_LS_APPLY32, -1);
    const bool fast32 = s.x_aligned && (N & 7) == 0 && fits_lds(ls_apply32_lds(N, true));
    const bool few32 = knob32 >= 0 ? knob32 != 0 : 2 * (int64_t)mk.grid[0] <= (int64_t)s.cus;
    if (t.cls == LS_NARROW) ap = ls_launch(LSK_K6, s, kWave, 0, 0);   // each round's mask words are K6's bit-packed mask (narrow tiles there: rls_maxcut_plan.h)
    else if (t.cls == LS_HALF || (few32 && fast32)) ap = ls_launch(LSK_APPLY32, s, kPlanHalf, kLsRoundWaves, ls_apply32_lds(N, fast32));
    else if (t.cls == LS_BIG64) ap = ls_launch(LSK_APPLY, s, kWave, 4, ls_apply_lds(N, 4, false));   // the bare tile: 4 waves, lane-per-env loads and stores
    else ap = ls_launch(LSK_APPLY, s, kWave, kLsRoundWaves, ls_apply_lds(N, kLsRoundWaves, true));
    ap.stage = ap.kernel == LSK_APPLY32 ? fast32 : ap.kernel == LSK_APPLY && ap.waves == kLsRoundWaves;   // row-piece stages: not beside the bare tile
    ap.planes = t.cls == LS_NARROW ? 0 : 24; ap.rounds = per_launch;
    return ls_plan_of(mk, ap, s.num_draws / per_launch, per_launch);
}
// rls_maxcut_ls_propose is one round of the above (it names the pitch first)
inline LsPlan plan_ls_propose(LsShape s) { s.num_draws = 1; return s.pitch_ok ? plan_ls_rounds(s) : ls_refuse_pitch(s); }
// what rls_maxcut_ls_rounds_supported answers: with the scratch rls_maxcut_ls_scratch_bytes asks for, on well-laid-out arguments
inline bool ls_rounds_supported(LsShape s) {
    s.pitch_ok = s.scratch_ok = true; s.num_draws = 1; s.scratch_bytes = ls_scratch_bytes(s);
    return ls_spin_ok(s) && plan_ls_rounds(s).err == RLS_OK;
}

}  // namespace rls
