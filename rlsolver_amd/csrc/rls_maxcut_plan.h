// The launch policy of the MaxCut tile entry points (K1 rls_maxcut_obj, K6 _propose_accept, K5 _greedy_sweep, K2 _node_cutdeg,
// K3 _delta_all, the local-search weights): which tile width, how many waves, which stages, how much LDS, which grid -- as pure
// functions of the shape, the tuning knobs and the CU count.  Plain C++ (no HIP): rls_maxcut.hip launches what these return,
// rls_maxcut_launch_plan of the C ABI answers with the same functions, and a host-only program can include this file.
// Every threshold carries the measurement it came from.
#pragma once
#include <stdarg.h>
#include <stddef.h>
#include <stdint.h>
#include <stdio.h>
#include "rls_host.h"

namespace rls {

constexpr int kTileWaves = 4;   // waves cooperating on one 64-env tile (one per SIMD)
constexpr int kTileWavesMax = 8;   // K1 / K6 take 8 when the tile is so large that only one workgroup fits a CU
constexpr int kNarrowWaves = 8;   // waves of a narrow (16- / 8-env) tile
constexpr int kNsWaves = 8;   // waves of a bit-sliced node-stats tile
constexpr int kSweepLoadWaves = 4;   // waves that move the tile (the ring holds 4 row-piece stages)
// what the kernels' headers call kStageBytes, kHalf, kRing, kSweepMaxDeg (rls_maxcut.hip asserts that they agree)
constexpr int kPlanStageBytes = 4096, kPlanHalf = 32, kPlanRing = 4096, kPlanSweepMaxDeg = 512;

enum PlanForm {
    PF_TILE64, PF_TILE32, PF_NARROW16, PF_NARROW8,   // bit tiles of 64 / 32 / 16 / 8 envs per workgroup
    PF_ROWS,                                         // one env per wave on a byte row
    PF_SWEEP_BATCHED, PF_SWEEP_FAST, PF_SWEEP_GENERIC,   // K5's stream forms (64-env tiles)
    PF_NS_TILE, PF_NS_ELEM,                          // K2 / K3 / weights: lane = env tile, element-parallel
    PF_UNSUPPORTED
};

struct TileShape {
    int64_t N, B, E, G, nnz;   // nodes, envs, stored edges, sweep groups, CSR entries
    int spin_bytes;
    bool rows_aligned;   // tile_rows_aligned of x (and of a byte mask)
    bool out16;          // output base 16-byte aligned (K2 / K3 row staging)
    bool mask_bits, minmax, weighted;   // K6's mask is bit-packed; the weights fold min / max; rls_graph.wgt
    int32_t max_degree;
    bool has_levels, has_batches, has_ell, col4;   // sweep_lv_*, sweep_rowptr / _stream, the entry's ELL slabs, col 4-byte aligned
    int cus;
};

struct LaunchPlan {
    int form, waves, planes;
    bool vec, wide;
    int stage;   // the int the kernel receives: a stage offset (K1 / K6), has-stage (K5), stage flags (node stats)
    uint32_t grid, block;
    size_t lds;
    int err;         // PF_UNSUPPORTED: what the entry point returns
    char msg[96];
};

inline int plan_width(int form) { return form == PF_TILE32 ? kPlanHalf : form == PF_NARROW16 ? 16 : form == PF_NARROW8 ? 8 : kWave; }
constexpr size_t align16(size_t b) { return (b + 15) & ~(size_t)15; }
inline bool fits_lds(size_t b) { return b <= (size_t)kLdsBytes; }

// LDS of a bit tile: one word of `word_bytes` (8 / 4 / 2 / 1 for 64 / 32 / 16 / 8 envs) per node -- 16-byte aligned but for the 64-env
// tiles' whole 8-byte words --, 512 bytes of reduction scratch per wave, and `extra` (a level table, row-piece stages)
constexpr size_t tile_lds(int64_t nodes, int word_bytes, int waves, size_t extra = 0) {
    return (word_bytes == 8 ? (size_t)nodes * 8 : align16((size_t)nodes * word_bytes)) + (size_t)waves * kWave * 8 + extra;
}
inline size_t stages(int waves) { return (size_t)waves * kPlanStageBytes; }
inline size_t level_table(int64_t G) { return align16((size_t)(G + 1) * 4); }

inline int plan_planes(int64_t E) {   // bit planes of the cut counters (pick_planes of rls_cutcount.h)
    if (E < (1 << 12)) return 12;
    if (E < (1 << 16)) return 16;
    if (E < (1 << 20)) return 20;
    if (E < (1 << 24)) return 24;
    return 0;
}
inline int narrow_planes(int64_t E) { return plan_planes(E) == 12 ? 16 : plan_planes(E); }   // (the narrow kernels come in 16 / 20 / 24)

// the half and narrow tiles' fast loaders: byte rows of 16- or 8-byte multiples on a 16-byte base (rls_tile32.h)
inline bool fast_loader(const TileShape& s) { return s.rows_aligned && (s.N & 7) == 0; }

// Append W row-piece stages to a tile's LDS when they fit; returns their byte offset or -1 (tile_stage_offset of rls_tile.h).
inline int plan_stage_offset(size_t* lds_bytes, int W, bool wanted) {
    const bool off = knob_on(KN_TILE_NOSTAGE);   // dev knob: lane-per-env global access
    const size_t base = align16(*lds_bytes);
    if (!wanted || off || !fits_lds(base + stages(W))) return -1;
    *lds_bytes = base + stages(W);
    return (int)base;
}

inline LaunchPlan tile_plan(int form, const TileShape& s, int waves, int planes, bool vec, size_t lds, int stage = 0) {
    LaunchPlan p{};
    p.form = form; p.waves = waves; p.planes = planes; p.vec = vec; p.stage = stage; p.lds = lds;
    p.grid = (uint32_t)ceil_div(s.B, plan_width(form));
    p.block = (uint32_t)(waves * kWave);
    return p;
}

#if defined(__GNUC__)
__attribute__((format(printf, 2, 3)))
#endif
inline LaunchPlan unsupported(int code, const char* fmt, ...) {
    LaunchPlan p{};
    p.form = PF_UNSUPPORTED;
    p.err = code;
    va_list ap;
    va_start(ap, fmt);
    vsnprintf(p.msg, sizeof(p.msg), fmt, ap);
    va_end(ap);
    return p;
}

// Which tile a launch of B envs should take when several fit: a tile's load / sweep / store is a chain of its own whatever it holds,
// so a batch of few tiles wants NARROWER ones until the chip is full -- 4096 envs are 64 / 128 / 256 / 512 tiles of 64 / 32 / 16 / 8
// envs on 256 CUs.  Returns 0 (the wide tiles), 16 or 8.  RLS_NARROW_TILE: 0 never, 1 automatic, 2 / 3 force 16 / 8 where they fit.
inline int narrow_policy(const TileShape& s, Knob wide_knob) {
    const int64_t k = knob(KN_NARROW_TILE, 1);
    if (k == 0 || (k == 1 && knob(wide_knob, -1) >= 0)) return 0;      // (a forced 64-env / half-tile form is honoured)
    if (k == 2) return 16;
    if (k == 3) return 8;
    // automatic (tools/timing/narrow_policy.py, K1 / K6 / K5 in us, wide -> narrow): N = 10^4, 4096 envs 21.8 / 31.6 / 47.6 -> 11.7 /
    // 22.4 / 39.2 (16 envs), 256 envs 19.4 / 27.8 / 42.4 -> 7.6 / 13.2 / 24.9 (8 envs); N = 39 936, 4096 envs 47 / 120 / 356 -> 36 / 86 /
    // 135; N = 2000, 4096 envs 10.4 / 11.6 / 47 -> 7.1 / 9.1 / 46; N = 800: nothing.  From 16 384 envs on the wide tiles win
    // (N = 10^4: 29.7 / 77.5 / 69.8 vs 32.8 / 89.6 / 110) -- the chip is full and a narrow tile walks the edge list / schedule per 16 envs.
    if (!fast_loader(s) || s.N < 1536) return 0;      // (the narrow loader's fast path: byte rows of 16- or 8-byte multiples)
    if (ceil_div(s.B, 8) <= s.cus) return 8;
    if (ceil_div(s.B, 16) <= s.cus) return 16;
    return 0;
}

// A narrow tile (16 or 8 envs per workgroup: rls_tile32.h).  `want`: 0 = the widest that fits, 16 / 8 = that one (8: never 16).
// False: not applicable here (no planes for E, or not even the 8-env words fit).
inline bool plan_narrow(const TileShape& s, int want, int planes, int scratch_waves, size_t extra, bool vec, LaunchPlan* p) {
    const size_t l16 = tile_lds(s.N + 2, 2, scratch_waves, extra), l8 = tile_lds(s.N + 2, 1, scratch_waves, extra);
    if (planes == 0 || !fits_lds(l8)) return false;
    const bool w16 = want != 8 && fits_lds(l16);
    *p = tile_plan(w16 ? PF_NARROW16 : PF_NARROW8, s, kNarrowWaves, planes, vec, w16 ? l16 : l8);
    return true;
}

// one env per wave on a byte row: up to 4 waves (= envs) per workgroup
inline LaunchPlan plan_rows(const TileShape& s, bool say_bytes) {
    const size_t per = align16((size_t)s.N);
    if (!fits_lds(per))
        return say_bytes ? unsupported(RLS_EUNSUPPORTED, "N=%lld: a row of %lld bytes does not fit LDS (max %d)", (long long)s.N, (long long)s.N, kLdsBytes)
                         : unsupported(RLS_EUNSUPPORTED, "N=%lld: a row does not fit LDS (max %d)", (long long)s.N, kLdsBytes);
    int w = (int)((size_t)kLdsBytes / per);
    w = w > 4 ? 4 : w;
    LaunchPlan p{};
    p.form = PF_ROWS; p.waves = w; p.lds = (size_t)w * per;
    p.grid = (uint32_t)ceil_div(s.B, w);
    p.block = (uint32_t)(w * kWave);
    return p;
}

// waves of K1's / K6's 64-env tile: with one workgroup per CU, 4 waves cannot keep enough loads in flight
inline int tile_waves_for(int64_t N) { return (size_t)N * 8 + 4 * 4096 + 4096 > 80 * 1024 ? kTileWavesMax : kTileWaves; }
// ... and the tile itself: 8 or 4 waves by size; where only the tile alone still fits (N <= 20 224: Gset's 20 000-node G81) 4 waves, no
// row-piece stage (lane-per-env loads at ~2.5 TB/s) -- an order of magnitude ahead of the one-env-per-wave form
inline size_t tile64_lds(int64_t N, int* tw) {
    *tw = tile_waves_for(N);
    if (!fits_lds(tile_lds(N, 8, *tw)) && fits_lds(tile_lds(N, 8, kTileWaves))) *tw = kTileWaves;
    return tile_lds(N, 8, *tw);
}

// ---- K1 ---------------------------------------------------------------------------------------------------------------
inline LaunchPlan plan_obj(const TileShape& s) {
    const int64_t N = s.N;
    const bool bytes = s.spin_bytes == 1, vec = s.rows_aligned;
    LaunchPlan p;
    if (const int nw = narrow_policy(s, KN_K1_TILE32))
        if (plan_narrow(s, nw, narrow_planes(s.E), kNarrowWaves, 0, vec && bytes, &p)) return p;
    int tw;
    size_t lds = tile64_lds(N, &tw);
    // Half tiles (32 envs, 32-bit words: rls_tile32.h).  Where the 64-env tile does not fit but N * 4 bytes do (20 224 < N <=
    // 40 448) -- and, for byte rows of 16-byte multiples (their fast loader), where they measure faster (tools/timing/k1_tile32.py):
    // rows past 8192 nodes, whose 64-env tile leaves one workgroup per CU or no room for the row-piece stage (G70-sized 2^17:
    // 280 -> 262 us, N = 20 000 2^16: 374 -> 282), and launches of at most two 64-env tiles per CU (G22-sized 2^14: 14.8 -> 13.4 us;
    // at 2^16 the half tiles LOSE, 34.4 -> 36.3: twice the edge-list reads per env).  Dev knob RLS_K1_TILE32 = 0 | 1 forces the choice.
    const int knob32 = (int)knob(KN_K1_TILE32, -1);
    // 8 waves once two 4-wave workgroups (with their stages) no longer share a CU: one 4-wave workgroup per CU cannot keep
    // enough loads in flight (N = 15 984 .. 16 384 ran at 0.43 of HBM beside 0.61 at 15 872, where two still fit)
    int w32 = 2 * (tile_lds(N, 4, kTileWaves) + stages(kTileWaves)) > (size_t)kLdsBytes ? kTileWavesMax : kTileWaves;
    if (!fits_lds(tile_lds(N, 4, w32))) w32 = kTileWaves;
    size_t l32 = tile_lds(N, 4, w32);
    const int P = plan_planes(s.E);
    const bool fast32 = bytes && fast_loader(s);      // (rows of 16- or 8-byte multiples: rls_tile32.h)
    const bool want32 = knob32 >= 0 ? knob32 != 0 : fast32 && (N >= 3000 || ceil_div(s.B, kWave) <= 2 * (int64_t)s.cus);
    // (N >= 3000, round 5: until then "rows past 8192 nodes" -- at 2^16 envs the half tile also wins from 3000 nodes on, K1 N = 3008 /
    // 5008 / 7008: 42.6 / 77.5 / 103.8 -> 38.6 / 75.1 / 102.2 us, rows of 8-byte multiples 49.8 / 89.4 / 124.0 -> 43.1 / 83.1 / 116.3;
    // at G22's 2000 it loses, 36.3 vs 34.4: tools/sweeps/align_sweep.py with RLS_K1_TILE32 = 1)
    if ((want32 || !fits_lds(lds)) && fits_lds(l32) && P != 0) {
        const int st_off = plan_stage_offset(&l32, w32, fast32);
        return tile_plan(PF_TILE32, s, w32, P, vec && bytes, l32, st_off);
    }
    if (!fits_lds(lds) && knob(KN_NARROW_TILE, 1) != 0)      // neither the 64-env nor the half tile fits: 16 or 8 envs per workgroup
        if (plan_narrow(s, 0, narrow_planes(s.E), kNarrowWaves, 0, vec && bytes, &p)) return p;
    if (!fits_lds(lds)) return plan_rows(s, true);   // neither tile fits: one env per wave on a byte row
    if (P == 0) return unsupported(RLS_EUNSUPPORTED, "E'=%lld too large", (long long)s.E);
    const int stage_off = plan_stage_offset(&lds, tw, bytes);   // (unaligned byte rows use it too)
    // dev knob: ask for more LDS than the tile needs, i.e. fewer resident workgroups per CU and a second round of them whose loads
    // could hide the first round's counting (RLS_K1_LDS_KB = kilobytes per workgroup)
    const int pad_kb = (int)knob(KN_K1_LDS_KB, 0);
    if (pad_kb > 0 && (size_t)pad_kb * 1024 > lds && fits_lds((size_t)pad_kb * 1024)) lds = (size_t)pad_kb * 1024;
    return tile_plan(PF_TILE64, s, tw, P, vec, lds, stage_off);
}

// ---- K6 ---------------------------------------------------------------------------------------------------------------
inline LaunchPlan plan_propose_accept(const TileShape& s) {
    const int64_t N = s.N;
    const bool vec = s.rows_aligned;   // (x and a byte mask)
    LaunchPlan p;
    if (const int nw = narrow_policy(s, KN_K6_TILE32))
        if (plan_narrow(s, nw, narrow_planes(s.E), kNarrowWaves, 0, vec, &p)) return p;
    int tw;
    size_t lds = tile64_lds(N, &tw);
    // Half tiles (rls_tile32.h): where the 64-env tile does not fit and N * 4 bytes do, for rows past 8192 nodes (G70-sized 2^17,
    // byte mask: 608 -> 481 us; N = 20 000 2^15, where the 64-env tile has no room for its stage: 387 -> 299), and in launches of
    // at most one 64-env tile per CU (G22-sized 2^12: 21.8 -> 11.4 us, 2^14: 26.8 -> 20.9; at 2^16 they lose, 63.6 -> 67.3).
    // tools/timing/k5_tile32.py.
    const int knob32 = (int)knob(KN_K6_TILE32, -1);   // dev knob: 0 | 1 forces the choice
    const bool no_stage64 = !fits_lds(lds + stages(tw));
    // (the half tile's fast loader wants byte rows of 16-byte multiples on a 16-byte base; other rows keep the 64-env forms)
    const bool fast32 = fast_loader(s);
    const bool want32 = knob32 >= 0 ? knob32 != 0 : fast32 && (no_stage64 || N >= 3000 || ceil_div(s.B, kWave) <= (int64_t)s.cus);
    // (N >= 3000, round 5, as for K1: K6 with a byte mask at 2^16 envs, N = 3008 / 5008 / 7008: 101 / 173 / 236 -> 95 / 158 / 212 us,
    // rows of 8-byte multiples 116 / 194 / 271 -> 101 / 165 / 236)
    const int P = plan_planes(s.E);
    if (want32 || !fits_lds(lds)) {
        const int w32 = fits_lds(tile_lds(N, 4, kTileWavesMax)) ? kTileWavesMax : kTileWaves;
        size_t l32 = tile_lds(N, 4, w32);
        if (fits_lds(l32) && P != 0) {
            const int st32 = plan_stage_offset(&l32, w32, fast32);    // (row-piece stages when they fit beside the tile)
            return tile_plan(PF_TILE32, s, w32, P, vec, l32, st32);
        }
    }
    if (!fits_lds(lds) && knob(KN_NARROW_TILE, 1) != 0)      // neither the 64-env nor the half tile fits: 16 or 8 envs per workgroup
        if (plan_narrow(s, 0, narrow_planes(s.E), kNarrowWaves, 0, vec, &p)) return p;
    if (!fits_lds(lds)) {   // neither tile fits: one env per wave on a byte row
        p = plan_rows(s, false);
        if (p.form == PF_ROWS && s.mask_bits)
            return unsupported(RLS_EUNSUPPORTED, "N=%lld: beyond the tiles the mask must be bytes [B, N]", (long long)N);
        return p;
    }
    if (P == 0) return unsupported(RLS_EUNSUPPORTED, "E'=%lld too large", (long long)s.E);
    const int stage_off = plan_stage_offset(&lds, tw, true);
    return tile_plan(PF_TILE64, s, tw, P, vec, lds, stage_off);
}

// ---- K5 ---------------------------------------------------------------------------------------------------------------
inline LaunchPlan plan_greedy_sweep(const TileShape& s) {
    const int64_t N = s.N, G = s.G;
    const bool vec = s.rows_aligned;
    const int P = plan_planes(s.E);
    // level-parallel sweep: needs the lane-per-node schedule (N < 2^20, degrees < 256) and the tile in LDS
    const bool levels = !knob_on(KN_SWEEP_NO_LEVELS) && !s.weighted && s.has_levels && G > 0 && P != 0;   // (SWEEP_NO_LEVELS: dev knob)
    const size_t lv = level_table(G);
    LaunchPlan p;
    if (const int nw = narrow_policy(s, KN_K5_TILE32))
        if (levels && plan_narrow(s, nw, narrow_planes(s.E), kNarrowWaves, lv, vec, &p)) return p;
    if (levels) {
        const int force_lw = (int)knob(KN_SWEEP_WAVES, 0);
        // one group per level (G22: 44 nodes per group): a level is ONE wave's pass and the others only prefetch -- few
        // waves, more tiles per CU; well-filled groups (G70: 9 levels of ~17 groups): 8 waves share a level
        int sw = force_lw == 2 || force_lw == 4 || force_lw == 8 || force_lw == 16 ? force_lw : (N >= 56 * G ? 8 : 4);
        auto lds_of = [&](int word_bytes, int waves, bool stage) { return tile_lds(N + 2, word_bytes, waves, lv + (stage ? stages(kSweepLoadWaves) : 0)); };
        int has_stage = 1;
        if (!fits_lds(lds_of(8, sw, true))) {   // the tile nearly fills LDS (N ~ 20 000): no row-piece stage, fewer waves
            has_stage = 0;
            if (!fits_lds(lds_of(8, sw, false))) sw = 4;
            if (!fits_lds(lds_of(8, sw, false))) sw = 2;
        }
        const size_t lds_l = lds_of(8, sw, has_stage != 0);
        // half tiles (rls_tile32.h) where the 64-env tile does not fit (dev knob RLS_K5_TILE32 = 1: at any size)
        const int knob32 = (int)knob(KN_K5_TILE32, -1);
        // ... and, for byte rows of 16-byte multiples (the half tile's staged loader / store), where they measure faster
        // (tools/timing/k5_tile32.py): rows past 8192 nodes (G70-sized 2^17: 780 -> 705 us; N = 20 000, where the 64-env tile has no
        // room for its stage, 4096 envs: 171 -> 100) and launches of at most one 64-env tile per CU (G22-sized 2^14: 63 -> 53 us;
        // at 2^16 the half tiles lose, 113 -> 128: twice the schedule reads per env)
        const bool prefer32 = knob32 < 0 && fast_loader(s) && (!has_stage || (size_t)N * 8 > 64 * 1024 || ceil_div(s.B, kWave) <= (int64_t)s.cus);
        if (knob32 > 0 || prefer32 || !fits_lds(lds_l)) {
            int sw32 = force_lw == 2 || force_lw == 4 || force_lw == 8 ? force_lw : (N >= 56 * G ? 8 : 4);
            int stage32 = fast_loader(s) ? 1 : 0;
            if (stage32 && !fits_lds(lds_of(4, sw32, true))) stage32 = 0;
            if (!fits_lds(lds_of(4, sw32, stage32 != 0))) sw32 = 4;
            if (!fits_lds(lds_of(4, sw32, stage32 != 0))) sw32 = 2;
            // a half tile that leaves room for two waves only (N ~ 40 000: the words fill LDS) sweeps slower than 16-env tiles with
            // eight at every batch size (N = 39 936: 2^12 envs 356 -> 135 us, 2^16 3779 -> 2332)
            if (sw32 == 2 && knob(KN_NARROW_TILE, 1) == 1 && knob32 < 0)
                if (plan_narrow(s, 16, narrow_planes(s.E), kNarrowWaves, lv, vec, &p)) return p;
            const size_t l32 = lds_of(4, sw32, stage32 != 0);
            if (fits_lds(l32)) return tile_plan(PF_TILE32, s, sw32, P, vec, l32, stage32);
            // the half tile does not fit either: 16 or 8 envs per workgroup (the same level schedule)
            if (knob(KN_NARROW_TILE, 1) != 0)
                if (plan_narrow(s, 0, narrow_planes(s.E), kNarrowWaves, lv, vec, &p)) return p;
        }
        if (fits_lds(lds_l)) return tile_plan(PF_TILE64, s, sw, P, vec, lds_l, has_stage);
    }
    // the stream forms: 64-env tile, the schedule through the LDS ring
    const size_t lds_fast = (size_t)(N + 2) * 8 + (size_t)((N + 1 + 3) & ~3ll) * 4 + (size_t)kPlanRing * 4;
    const bool fast = !s.weighted && s.max_degree < kPlanSweepMaxDeg && fits_lds(lds_fast) && s.col4;
    const bool unbatched = knob_on(KN_SWEEP_UNBATCHED);   // dev knob
    if (fast && s.has_batches && !unbatched) {
        const int force_sw = (int)knob(KN_SWEEP_WAVES, 0);   // dev knob
        const int sw = force_sw == 4 || force_sw == 8 || force_sw == 16 ? force_sw : (ceil_div(s.B, kWave) <= (int64_t)s.cus ? 16 : 8);
        const size_t lds_b = lds_fast + (size_t)sw * kWave * 8;
        if (fits_lds(lds_b)) return tile_plan(PF_SWEEP_BATCHED, s, sw, 0, vec, lds_b);
    }
    if (fast) return tile_plan(PF_SWEEP_FAST, s, 1, 0, vec, lds_fast);
    const size_t lds = (size_t)N * 8;
    if (!fits_lds(lds)) return plan_rows(s, false);   // the 64-env bit tile does not fit: one env per wave on a byte row
    return tile_plan(PF_SWEEP_GENERIC, s, 1, 0, vec, lds);
}

// ---- K2 / K3 / the local-search weights (mode 0 / 1 / 2) ---------------------------------------------------------------
inline size_t ns_bits_lds(int64_t N, int word_bytes, bool with_stage, int waves = kNsWaves) {   // (no reduction scratch)
    return align16(tile_lds(N, word_bytes, 0)) + (with_stage ? stages(waves) : 0);
}
// the bit-sliced kernel needs the slabs, an unweighted graph, byte-sized counters and a tile that fits.  A tile costs about
// 0.011 us per node however few envs it holds, the element-parallel kernels about 2e-6 us per (env, node + entry): K3 on a
// G22-sized graph 28 us flat vs 9 / 21 / 68 us at 64 / 256 / 1024 envs, N = 10^4 with 10^4 edges 88 flat vs 7 / 17 / 70
// (tools/sweeps/node_stats_forms.py) -- so small batches go element-parallel
inline bool node_stats_batch_fills_tiles(const TileShape& s) {
    const int64_t force = (int64_t)knob(KN_NODE_STATS_MIN_B, -1);   // dev knob
    if (force >= 0) return s.B >= force;
    return (double)s.B * (double)(s.N + s.nnz) > 4000.0 * (double)s.N;
}
inline bool node_stats_use_bits(const TileShape& s) {
    const bool off = knob_on(KN_NODE_STATS_LANE_ENV);   // dev knob: the lane = env kernels
    return !off && s.has_ell && !s.weighted && s.max_degree < 65536 && node_stats_batch_fills_tiles(s) &&
           fits_lds(knob(KN_NARROW_TILE, 1) != 0 ? tile_lds(s.N + 2, 1, 0)              // (half tiles without the row-piece stage if
                                                 : ns_bits_lds(s.N, 4, false));        // need be, narrow ones past them)
}
inline size_t node_stats_tile_lds(int64_t N) { return (size_t)(N + 2) * 8 + (size_t)kTileWaves * kWave * 144; }
// the lane = env tile kernels (weighted graphs, degrees >= 65536) walk every node and entry of the graph once per tile, 0.10 us
// per node + 0.008 us per entry whatever the batch (K3 on a +-1-weighted G22-sized graph: 530 us from 2048 to 16 384 envs), the
// element-parallel kernels 2.75e-6 us per (env, node + entry) (250 / 480 / 1890 us at 2048 / 4096 / 16 384): the tile form from
// the batch where it is the cheaper one (tools/sweeps/node_stats_forms.py)
inline bool node_stats_use_tile(const TileShape& s) {
    const bool off = knob_on(KN_NODE_STATS_NO_TILE);   // dev knob
    return !off && fits_lds(node_stats_tile_lds(s.N)) &&
           2.75e-6 * (double)s.B * (double)(s.N + s.nnz) > 0.103 * (double)s.N + 0.008 * (double)s.nnz;
}

inline LaunchPlan plan_node_stats_bits(const TileShape& s, int mode) {
    const int64_t N = s.N, cus = s.cus;
    const bool vec = s.rows_aligned, fast = fast_loader(s);
    const bool wide = s.max_degree >= 256;
    const int knob32 = (int)knob(KN_NS_TILE32, -1);   // dev knob: half tiles at any size
    LaunchPlan p;
    // Half tiles: past the 64-env tile; and, for byte rows of 16-byte multiples whose half tile has room for its stage, where they
    // measure faster (this round's GPU runs): batches of few tiles -- a tile costs the same however few envs it holds, so twice
    // as many half as long workgroups win while CUs are idle: K3 / K2 up to 8192 envs (G22-sized 4096: 31 -> 23 us, BA n = 10^4
    // 135 -> 101, G70-sized 88 -> 62), the weights pre-pass up to 2048 (its 64-env kernel has the dword stores) --, K3 on short
    // rows at full batches (G22-sized 2^16: 166 -> 154 us), and -- few tiles again -- rows whose 64-env tile has no room for its
    // stage (N > ~15 800: K3 at N = 20 000, 4096 envs 278 -> 186 us)
    const int64_t t64 = ceil_div(s.B, kWave);
    const bool few = mode == 2 ? 8 * t64 <= cus : 2 * t64 <= cus;
    // (round 6: from two 64-env tiles per CU on -- N = 3008, 2^15 envs: 121 us on 64-env tiles, 109-112 on half tiles)
    const bool full_k3 = mode == 1 && t64 >= 2 * cus && (size_t)N * 8 <= 64 * 1024;
    const bool prefer32 = knob32 < 0 && fast && fits_lds(ns_bits_lds(N, 4, true)) &&
                          (few || full_k3 || (!fits_lds(ns_bits_lds(N, 8, true)) && 2 * t64 <= cus));
    // Narrow tiles (16 / 8 envs, rls_tile32.h) where the half tile is past the LDS (N > 40 960): the rows these took before went
    // element-parallel -- one L2 gather per (env, entry)
    // -- and, like K1 / K6 / K5 (narrow_policy), for batches of few tiles on rows the narrow loader's fast path takes: a tile's load,
    // count and stores are one chain whatever it holds, so 256 CUs want 256+ tiles (tools/timing/narrow_ns_ab.py, K3 / K2 / weights in us,
    // wide -> narrow: N = 10^4, 4096 envs 62 / 83 / 95 -> 44 / 74 / 91 (16 envs); N = 20 000, 1024 envs 128 / 102 / 148 -> 75 / 55 / 114
    // (8 envs); G22-sized, 256 envs 18.4 / 15.3 / 25.5 -> 11.9 / 9.5 / 22.5).  The weights' 8-env tiles only up to 512 envs (every tile
    // folds its min / max into the table with atomics: G22-sized 1024 envs 27.8 -> 32.6)
    const int64_t nk = knob(KN_NARROW_TILE, 1);
    int auto_n = 0;
    if (nk == 1 && knob32 < 0 && fast) {
        if (mode == 2) {    // (G22-sized, 4096 envs on 16-env tiles: 31 -> 57 us -- 256 tiles' worth of min / max atomics per node)
            if (ceil_div(s.B, 8) <= cus / 4) auto_n = 8;
            else if (N >= 8192 && ceil_div(s.B, 16) <= cus / 4) auto_n = 16;
        } else {
            if (ceil_div(s.B, 8) <= cus) auto_n = 8;
            else if (ceil_div(s.B, 16) <= cus) auto_n = 16;
        }
    }
    if (nk != 0 && (nk >= 2 || auto_n || !fits_lds(ns_bits_lds(N, 4, false))))
        if (plan_narrow(s, nk == 3 || auto_n == 8 ? 8 : 0, -1, 0, 0, vec, &p)) { p.wide = wide; p.planes = 0; return p; }
    if (knob32 > 0 || prefer32 || !fits_lds(ns_bits_lds(N, 8, false))) {   // half tiles (rls_tile32.h)
        int st32 = (fast && fits_lds(ns_bits_lds(N, 4, true))) ? 1 : 0;
        size_t l32 = ns_bits_lds(N, 4, st32 != 0);
        // K3's row staging on full half tiles (the kernel's comment): 16-byte-aligned output, rows of 4-node multiples
        const int rk = (int)knob(KN_NS_ROWS, -1);
        const size_t lrows = ns_bits_lds(N, 4, false) + (size_t)kNsWaves * kPlanHalf * 132;
        // measured (tools/timing/k3_rows.py, half tiles per group -> rows): N = 3008 112 -> 109 us, G70-sized 1603 -> 1527, BA n = 10^4
        // 1093 -> 1043; G22-sized 162 -> 167 (sixteen 512-byte pieces per pair are too few stores to pay for the staging): from 3000 nodes
        if (mode == 1 && st32 && (N & 3) == 0 && s.out16 && (rk < 0 ? N >= 3000 : rk != 0) && fits_lds(lrows)) {
            st32 |= 4;
            if (lrows > l32) l32 = lrows;
        }
        p = tile_plan(PF_TILE32, s, kNsWaves, 0, vec, l32, st32);
        p.wide = wide;
        return p;
    }
    const int has_stage = fits_lds(ns_bits_lds(N, 8, true)) ? 1 : 0;
    // 8 waves per tile, or 4 where that turns a launch of one-and-a-bit rounds of workgroups into ONE round: a G22-sized tile
    // is 16 KB + 4 KB of row-piece stage per wave -- 3 eight-wave workgroups per CU (768 resident: 1024 tiles = a full round
    // and a third of one), 5 four-wave ones (every tile resident at once)
    const int force_w = (int)knob(KN_NS_WAVES, 0);     // dev knob
    // measured (tools/timing/k7_packed.py, ls_parts.py with RLS_NS_WAVES=4 | 8; G22 2^16): K3 171 vs 167 us, weights 156 vs 139 us,
    // G70 2^17 K3 1889 vs 1656 -- the single round does not pay for halving a tile's waves: 8 stays, 4 is a knob
    const bool four = force_w == 4 && !wide && has_stage;
    const int waves = four ? 4 : kNsWaves;
    size_t lds = ns_bits_lds(N, 8, has_stage != 0, waves);
    // MODE 2's parked min / max folds (the kernel's comment): 4 N bytes behind the tile, over the stages' bytes -- where they fit
    // without costing the CU a workgroup
    int stage_flags = has_stage;
    const int seeds = (int)knob(KN_NS_PARK, 16);       // dev knob: 0 = every tile folds as it goes
    if (mode == 2 && s.minmax && seeds > 0 && t64 > seeds) {
        const size_t with_stash = ns_bits_lds(N, 8, false) + (size_t)N * 4;
        const size_t need = with_stash > lds ? with_stash : lds;
        if (fits_lds(need) && (size_t)kLdsBytes / need == (size_t)kLdsBytes / lds) { lds = need; stage_flags |= 2 | (seeds << 8); }
    }
    // K2 / K3 of full tiles through row staging (the kernel's comment): 16-byte-aligned output rows of 4-node multiples, 8 KB + of
    // LDS per wave behind the tile (where the row-piece stages are: the hub groups' cooperative pass needs those)
    const int rows_knob = (int)knob(KN_NS_ROWS, -1);
    const size_t lds_rows = ns_bits_lds(N, 8, false) + (size_t)kNsWaves * kWave * 132;
    // measured (tools/timing/k3_rows.py, per group -> rows): K3 G70-sized 2^17 1648 -> 1574 us, BA n = 10^4 2^16 1136 -> 1032; G22-sized
    // 2^16 169 -> 178 and N = 3008 117 -> 123 (the 64 KB of staging cost the CU a workgroup there); K2's int64 rows lose everywhere
    // (G70 2274 -> 2361): K3, on tiles that leave one workgroup per CU either way
    const bool rows_auto = mode == 1 && 2 * ns_bits_lds(N, 8, true, waves) > (size_t)kLdsBytes;
    if (mode != 2 && waves == kNsWaves && has_stage && (N & 3) == 0 && s.out16 && (rows_knob < 0 ? rows_auto : rows_knob != 0) &&
        fits_lds(lds_rows)) {
        stage_flags |= 4;
        if (lds_rows > lds) lds = lds_rows;
    }
    p = tile_plan(PF_TILE64, s, waves, 0, vec, lds, stage_flags);
    p.wide = wide && !four;
    return p;
}

// which kernel family K2 / K3 / the weights take: the bit-sliced tiles, the lane = env tile (K2 / K3 only), element-parallel
inline LaunchPlan plan_node_stats(const TileShape& s, int mode) {
    if (node_stats_use_bits(s)) return plan_node_stats_bits(s, mode);
    // (for the weights a lane = env tile kernel used to take the small batches: 850 us per call on a G22-sized graph at any batch size,
    // against 30 us for the bit-sliced one and 20 - 100 us for the element-parallel one: tools/sweeps/ls_weights_forms.py)
    if (mode != 2 && node_stats_use_tile(s)) return tile_plan(PF_NS_TILE, s, kTileWaves, 0, s.rows_aligned, node_stats_tile_lds(s.N));
    LaunchPlan p{};
    p.form = PF_NS_ELEM;
    p.grid = (uint32_t)grid_for(s.B * s.N, 256);
    p.block = 256;
    return p;
}

}  // namespace rls
