// The launch policy of the ISCO sampler steps on a graph or a dense matrix (rls_isco_maxcut_step, rls_isco_mis_step,
// rls_pisco_step): the capacity of the selected-set list, a wave or a workgroup per sample, rows in LDS or in the caller's
// scratch, how many samples share a workgroup, how much LDS -- as one pure function of the sizes, the CU count and the dev knobs.
// Plain C++ (no HIP): rls_isco.hip launches what it returns, for every energy model and both sample formats, so the policy is
// written once.
#pragma once
#include <stddef.h>
#include <stdint.h>
#include "rlsolver_hip.h"
#include "rls_host.h"

namespace rls {

constexpr int kIscoWgWaves = 16;     // waves of the workgroup-per-sample kernels

// what the waves of a workgroup-per-sample kernel share beside the rows and the list (the last thing in its LDS)
struct IscoWgScratch { float f[kIscoWgWaves]; int i[kIscoWgWaves]; int hist[256]; int count; uint32_t prefix; int want; };

constexpr size_t kIscoLdsFixed = sizeof(IscoWgScratch) + 16;
constexpr int kIscoMinList = 64;     // entries of the smallest list a plan shrinks to by itself

// bytes of a sample's rows: two byte rows (padded to 8) and two f32 rows (lp, pert)
inline size_t isco_byte_rows(int64_t N) { return 2 * (((size_t)N + 7) & ~(size_t)7); }
inline size_t isco_rows_bytes(int64_t N) { return isco_byte_rows(N) + (size_t)N * 8; }

// the rows and the smallest list fit LDS
inline bool isco_rows_fit_lds(size_t rows) { return rows + kIscoMinList * 8 + kIscoLdsFixed <= (size_t)kLdsBytes; }

struct IscoPlan {
    bool wg;        // a workgroup per sample (kIscoWgWaves waves), else a wave per sample
    bool grows;     // workgroup per sample with the two f32 rows in the caller's scratch
    int P;          // the list's capacity, workgroup per sample
    int Pw;         // ... and wave per sample (it gives up capacity for resident samples)
    int waves;      // samples (= waves) per workgroup of the wave-per-sample kernel
    size_t lds;     // dynamic LDS bytes of the chosen form
    int err;        // RLS_OK, or what the entry point returns without launching (RLS_EUNSUPPORTED)
    size_t need;    // the refusal: the LDS bytes the smallest form would take
};

// rows: isco_rows_bytes(N).  min_cap: a floor on the list's capacity before it is fitted to LDS (the dense step keeps 64 entries
// at any N).  has_grows: the rows-in-scratch form exists for this step (the graph steps), else rows past LDS are refused.
inline IscoPlan isco_plan_step(size_t rows, int64_t N, int64_t B, int cus, int min_cap, bool has_grows) {
    IscoPlan p{};
    const size_t lds_max = (size_t)kLdsBytes, fixed = kIscoLdsFixed;
    const int force_cap = (int)knob(KN_ISCO_SEL_CAP, 0);   // dev / test knob
    auto forced = [&](int cap) { return force_cap >= 2 && force_cap < cap && (force_cap & (force_cap - 1)) == 0 ? force_cap : cap; };
    if (has_grows && (!isco_rows_fit_lds(rows) || knob_on(KN_ISCO_GLOBAL_ROWS))) {
        // rows past the LDS: a workgroup per sample with lp / pert in the caller's scratch (rls_isco_maxcut_scratch_bytes), the byte
        // rows and a list of up to 4096 entries in LDS
        const size_t brow = rows - (size_t)N * 8;
        p.wg = p.grows = true;
        p.waves = 1;
        p.need = brow + kIscoMinList * 8 + fixed;
        if (p.need > lds_max) {
            p.err = RLS_EUNSUPPORTED;
            return p;
        }
        int Pg = kIscoMinList;
        while (Pg < 4096 && Pg < N && brow + (size_t)Pg * 16 + fixed <= lds_max) Pg <<= 1;
        p.P = p.Pw = forced(Pg);
        p.lds = brow + (size_t)p.P * 8 + fixed;
        return p;
    }
    p.need = rows + kIscoMinList * 8 + fixed;
    if (!isco_rows_fit_lds(rows)) {
        p.err = RLS_EUNSUPPORTED;
        return p;
    }
    // capacity of the selected-set list in LDS: a power of two >= N while that fits (N <= 4096: as before), else the largest
    // power of two the rows leave room for, at least 64 (N = 10^4: 4096; N = 15 000: 1024; N = 15 500: 512) -- a larger selection takes the
    // extraction path.  The rows themselves (two byte rows, two f32 rows) bound N at ~15 900.  (The smallest list fits, checked
    // above, so the list this leaves always does.)
    int P = 1;
    while (P < N) P <<= 1;
    if (P < min_cap) P = min_cap;
    while (P > kIscoMinList && rows + (size_t)P * 8 + fixed > lds_max) P >>= 1;
    P = forced(P);
    const int force_wg = (int)knob(KN_ISCO_FORCE_WG, -1);      // dev knob: 0 wave per sample, 1 workgroup per sample
    // few chains (the reference's configs run one): a workgroup per sample; from ~4 samples per CU on the wave-per-sample
    // kernel has the throughput.
    // The workgroup kernel (8-bit radix passes, node loops over 16 waves) also wins at LARGE batches from ~1500 nodes on: a wave's
    // select is 32 one-bit passes over all its keys (from LDS past 2048 nodes) and its rows leave a CU ever fewer samples -- 4096
    // samples (tools/timing/isco_kernels.py): N = 2000 485 vs 427 us, N = 4000 2121 vs 527, G70's 10^4 8410 vs 852, N = 15 000 14 526
    // vs 1320; at N = 800 the wave kernel keeps the large batches (163 vs 301)
    p.wg = force_wg >= 0 ? (force_wg != 0 && N >= 4 * kWave) : (B <= (int64_t)2 * cus || N >= 1536) && N >= 4 * kWave;
    // wave-per-sample kernel: one wave per SIMD is latency-bound (round 3: 4 samples per CU), so the list gives up capacity for
    // resident samples while it stays >= 512 entries -- the reference draws Poisson(~10) path lengths, a longer selection takes
    // the extraction path -- G22-sized rows: 2048 entries x 4 samples -> 512 x 6 per CU, 4096 samples 606 -> 508 us
    const int max_waves = (int)knob(KN_ISCO_WAVES, 8);     // dev knob (<= 8)
    auto waves_for = [&](int cap) {
        int wv = (int)(lds_max / (rows + (size_t)cap * 8));
        return wv > max_waves ? max_waves : wv;
    };
    int Pw = P;
    if (!p.wg && force_cap == 0)
        while (Pw > 512 && waves_for(Pw >> 1) > waves_for(Pw)) Pw >>= 1;
    p.P = P;
    p.Pw = Pw;
    p.waves = waves_for(Pw) < 1 ? 1 : waves_for(Pw);
    p.lds = p.wg ? rows + (size_t)P * 8 + fixed : (rows + (size_t)Pw * 8) * p.waves;
    return p;
}

}  // namespace rls
