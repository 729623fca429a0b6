// Bit-sliced ("vertical") counters: plane p holds bit p of one independent count per bit of the plane word.  Every primitive is
// written once for both plane words PW: uint64_t (the 64-env tile of rls_tile.h) and uint32_t (the half tile, and the narrow tiles
// of 16 / 8 envs whose planes simply leave the upper bits of the 32-bit registers zero: rls_tile32.h).
#pragma once
#include "rls_common.h"

namespace rls {

// the plane word of a tile whose LDS word is WT
template <typename WT> struct plane_word { typedef uint32_t type; };
template <> struct plane_word<uint64_t> { typedef uint64_t type; };
template <typename WT> using plane_word_t = typename plane_word<WT>::type;

// (an argument of this type takes no part in template deduction: the planes decide PW, a mask such as `0ull - flag` converts)
template <typename T> struct plane_same { typedef T type; };

// carry-save adder on every counter at once; gfx950's v_bitop3 does a 3-input majority / parity in one op
__device__ __forceinline__ void csa(uint32_t& hi, uint32_t& lo, uint32_t a, uint32_t b, uint32_t c) {
    const uint32_t h = __builtin_amdgcn_bitop3_b32(a, b, c, 0xE8), l = __builtin_amdgcn_bitop3_b32(a, b, c, 0x96);
    hi = h;
    lo = l;
}
__device__ __forceinline__ void csa(uint64_t& hi, uint64_t& lo, uint64_t a, uint64_t b, uint64_t c) {
    const uint32_t a0 = (uint32_t)a, a1 = (uint32_t)(a >> 32), b0 = (uint32_t)b, b1 = (uint32_t)(b >> 32),
                   c0 = (uint32_t)c, c1 = (uint32_t)(c >> 32);
    const uint32_t h0 = __builtin_amdgcn_bitop3_b32(a0, b0, c0, 0xE8), h1 = __builtin_amdgcn_bitop3_b32(a1, b1, c1, 0xE8);
    const uint32_t l0 = __builtin_amdgcn_bitop3_b32(a0, b0, c0, 0x96), l1 = __builtin_amdgcn_bitop3_b32(a1, b1, c1, 0x96);
    hi = ((uint64_t)h1 << 32) | h0;
    lo = ((uint64_t)l1 << 32) | l0;
}

// carry into c[LO], rippling up to c[HI - 1] (a carry out of the last plane is dropped: the caller sizes the counter)
template <int LO, int HI, typename PW, int CAP>
__device__ __forceinline__ void ripple(PW (&c)[CAP], PW carry) {
    static_assert(HI <= CAP, "planes");
#pragma unroll
    for (int p = LO; p < HI; ++p) {
        const PW t = c[p] & carry;
        c[p] ^= carry;
        carry = t;
    }
}

// 8 words into a (ones, twos, fours) vertical counter: seven carry-save adders; returns the carry into the eights plane
template <typename PW>
__device__ __forceinline__ PW add8(const PW (&d)[8], PW& ones, PW& twos, PW& fours) {
    PW twosA, twosB, foursA, foursB, carry;
    csa(twosA, ones, ones, d[0], d[1]);
    csa(twosB, ones, ones, d[2], d[3]);
    csa(foursA, twos, twos, twosA, twosB);
    csa(twosA, ones, ones, d[4], d[5]);
    csa(twosB, ones, ones, d[6], d[7]);
    csa(foursB, twos, twos, twosA, twosB);
    csa(carry, fours, fours, foursA, foursB);
    return carry;
}
// ... and on into c[0 .. NC) = planes 3 ..  NC follows the number of words the counter can take (a count <= 7 never carries out of
// `fours`, <= 15 needs one more plane, ...): the ripple is 4 VALU per plane and half.
// (The node-stats kernels of rls_maxcut.hip keep this block written out, three times, with a run-time number of planes in the ripple:
// with a helper in its place the compiler orders their loops' phi nodes differently and the kernels' register numbering changes.)
template <int NC, typename PW, int CAP>
__device__ __forceinline__ void add8(const PW (&d)[8], PW& ones, PW& twos, PW& fours, PW (&c)[CAP]) {
    ripple<0, NC>(c, add8(d, ones, twos, fours));
}

// lane exchange of a plane with lane ^ 1, ^ 2 (DPP quad_perm 0xB1 / 0x4E) or ^ 4 (ds_swizzle bit mode: and 0x1F, or 0, xor 4), no memory
template <int X>
__device__ __forceinline__ uint32_t lv_lane_xor(uint32_t v) {
    if constexpr (X == 4) return (uint32_t)__builtin_amdgcn_ds_swizzle((int)v, 0x101F);
    else return (uint32_t)__builtin_amdgcn_update_dpp(0, (int)v, X == 1 ? 0xB1 : 0x4E, 0xF, 0xF, false);
}
template <int X>
__device__ __forceinline__ uint64_t lv_lane_xor(uint64_t v) {
    const uint32_t lo = lv_lane_xor<X>((uint32_t)v), hi = lv_lane_xor<X>((uint32_t)(v >> 32));
    return ((uint64_t)hi << 32) | lo;
}

// pl[0 .. NPL) += lane ^ X's pl[0 .. NPL) where `take` is all-ones (bit-sliced ripple-carry add; the sum must fit the NPL planes)
template <int X, typename PW, int NPL>
__device__ __forceinline__ void lv_merge_planes(PW (&pl)[NPL], typename plane_same<PW>::type take) {
    PW carry = 0;
#pragma unroll
    for (int p = 0; p < NPL; ++p) csa(carry, pl[p], pl[p], lv_lane_xor<X>(pl[p]) & take, carry);
}

// Bit-sliced compare of the vertical counters (planes pl[0 .. NP), plane p = bit p of every count) with a per-LANE constant
// thr < 2^NP:   c <= thr  <=>  c + (2^NP - 1 - thr) < 2^NP  <=>  adding ~thr (NP bits) to c carries nothing out of plane
// NP - 1.  Only the carry chain is needed -- one 3-input majority (v_bitop3) per plane and half, one v_bfe_i32 per plane for
// the constant's bit -- where the scan from the top plane down ("smaller so far / equal so far") took four operations per
// plane and half.  Returns the mask of counters that are <= thr.
template <int NP, int CAP>
__device__ __forceinline__ uint32_t lv_le_const(const uint32_t (&pl)[CAP], uint32_t thr) {
    static_assert(NP <= CAP, "planes");
    const int nt = (int)~thr;
    uint32_t c0 = 0;
#pragma unroll
    for (int p = 0; p < NP; ++p) c0 = __builtin_amdgcn_bitop3_b32(pl[p], (uint32_t)__builtin_amdgcn_sbfe(nt, p, 1), c0, 0xE8);
    return ~c0;
}
template <int NP, int CAP>
__device__ __forceinline__ uint64_t lv_le_const(const uint64_t (&pl)[CAP], uint32_t thr) {
    static_assert(NP <= CAP, "planes");
    const int nt = (int)~thr;
    uint32_t c0 = 0, c1 = 0;
#pragma unroll
    for (int p = 0; p < NP; ++p) {
        const uint32_t kb = (uint32_t)__builtin_amdgcn_sbfe(nt, p, 1);      // all ones where thr has bit p CLEAR
        c0 = __builtin_amdgcn_bitop3_b32((uint32_t)pl[p], kb, c0, 0xE8);
        c1 = __builtin_amdgcn_bitop3_b32((uint32_t)(pl[p] >> 32), kb, c1, 0xE8);
    }
    return ~(((uint64_t)c1 << 32) | c0);
}

// The same with one more plane below: mask of [2 c + low <= thr2], `low` a 0 | 1 bit per counter (a 64-bit word), thr2 < 2^(NP+1).
template <int NP, int CAP>
__device__ __forceinline__ uint64_t lv_le_const_x2(const uint64_t (&pl)[CAP], uint64_t low, uint32_t thr2) {
    static_assert(NP <= CAP, "planes");
    const int nt = (int)~thr2;
    const uint32_t k0 = (uint32_t)__builtin_amdgcn_sbfe(nt, 0, 1);
    uint32_t c0 = (uint32_t)low & k0, c1 = (uint32_t)(low >> 32) & k0;       // majority with carry-in 0
#pragma unroll
    for (int p = 0; p < NP; ++p) {
        const uint32_t kb = (uint32_t)__builtin_amdgcn_sbfe(nt, p + 1, 1);
        c0 = __builtin_amdgcn_bitop3_b32((uint32_t)pl[p], kb, c0, 0xE8);
        c1 = __builtin_amdgcn_bitop3_b32((uint32_t)(pl[p] >> 32), kb, c1, 0xE8);
    }
    return ~(((uint64_t)c1 << 32) | c0);
}

}  // namespace rls
