// What more than one of the per-tile stages uses — the depth sort of each 8x8 tile's list (fr_tile_sort.hip), the
// front-to-back alpha blend (fr_blend_fwd.hip) and the back-to-front gradient pass (fr_blend_bwd.hip) — and nothing else:
// a helper with a single user lives in that user's file.
//
// Execution model of all three: 8x8-pixel tiles = one 64-lane wavefront, one pixel per lane.  The sort leaves, per tile, the
// Gaussian ids of its list in blend order; the list is cut into UNITS of 64 instances (kUnit), the independent work items
// of the blend kernels, which gather each instance's 48-byte splat RECORD through the sorted ids (RecSrc).
#pragma once
#include "fr_common.hpp"

namespace fr {

// 48-byte record = 3 x float4:
//   q0 = (x, y, conic_a', conic_b')   q1 = (conic_c', opacity, r, g)   q2 = (b, id_bits, depth, 0)
// (GeomView::rec_tmpl; staged in LDS, the blend kernels keep a unit's footprint masks or pair slots in q2's last words)
constexpr int kRecQuads = 3;
constexpr int kGroup = 4;   // records per step of the all-pairs loops (blend_unit_dense_local, bwd_unit_all_pairs)

#ifndef FR_UNIT_WAVES
#define FR_UNIT_WAVES 4
#endif
constexpr int kWavesPerWG = FR_UNIT_WAVES;   // the unit kernels run 4 independent waves per workgroup (workgroup dispatch rate, not work,
                                 // bounded the one-wave-per-workgroup version)

typedef unsigned long long u64;

// ---- lane exchange by a compile-time xor mask without going through LDS addressing where the
// hardware offers it: DPP (quad_perm, row mirrors, row rotate) inside 16-lane rows, ds_swizzle bit-mode
// inside 32 lanes, v_permlane32_swap across the halves.
template <int MASK>
__device__ __forceinline__ int lane_xor_i32(int x, int lane)
{
    if constexpr (MASK == 1) return __builtin_amdgcn_mov_dpp(x, 0xB1, 0xF, 0xF, true);        // quad_perm [1,0,3,2]
    else if constexpr (MASK == 2) return __builtin_amdgcn_mov_dpp(x, 0x4E, 0xF, 0xF, true);   // quad_perm [2,3,0,1]
    else if constexpr (MASK == 3) return __builtin_amdgcn_mov_dpp(x, 0x1B, 0xF, 0xF, true);   // quad_perm [3,2,1,0]
    else if constexpr (MASK == 4) {
        const int t = __builtin_amdgcn_update_dpp(x, x, 0x104, 0xF, 0x5, false);              // row_shl:4 -> banks 0,2
        return __builtin_amdgcn_update_dpp(t, x, 0x114, 0xF, 0xA, false);                     // row_shr:4 -> banks 1,3
    } else if constexpr (MASK == 7) return __builtin_amdgcn_mov_dpp(x, 0x141, 0xF, 0xF, true);  // row_half_mirror
    else if constexpr (MASK == 8) return __builtin_amdgcn_mov_dpp(x, 0x128, 0xF, 0xF, true);   // row_ror:8
    else if constexpr (MASK == 15) return __builtin_amdgcn_mov_dpp(x, 0x140, 0xF, 0xF, true);  // row_mirror
    else if constexpr (MASK == 16) return __builtin_amdgcn_ds_swizzle(x, 0x401F);              // xor 16 within 32 lanes
    else if constexpr (MASK == 31) return __builtin_amdgcn_ds_swizzle(x, 0x7C1F);              // xor 31 within 32 lanes
    else if constexpr (MASK == 32) {
        auto r = __builtin_amdgcn_permlane32_swap((unsigned)x, (unsigned)x, false, false);   // r[0]=[lo,lo] r[1]=[hi,hi]
        return (lane < 32) ? (int)r[1] : (int)r[0];
    } else if constexpr (MASK == 63) return lane_xor_i32<32>(lane_xor_i32<31>(x, lane), lane);
    else {
        static_assert(MASK == 1, "unsupported xor mask");
        return x;
    }
}
template <int MASK>
__device__ __forceinline__ u64 lane_xor_u64(u64 v, int lane)
{
    const uint32_t lo = (uint32_t)lane_xor_i32<MASK>((int)(uint32_t)v, lane);
    const uint32_t hi = (uint32_t)lane_xor_i32<MASK>((int)(uint32_t)(v >> 32), lane);
    return ((u64)hi << 32) | lo;
}

// inclusive prefix sum over the 64 lanes with DPP only (no LDS round trips): shifts inside the 16-lane rows, then the
// row totals broadcast into the following rows (row_bcast:15 into rows 1 and 3, row_bcast:31 into rows 2 and 3)
__device__ __forceinline__ uint32_t wave_incl_scan_u32(uint32_t x)
{
#define FR_DPP_SHR_ADD(CTRL, ROWS) x += (uint32_t)__builtin_amdgcn_update_dpp(0, (int)x, (CTRL), (ROWS), 0xF, false)
    FR_DPP_SHR_ADD(0x111, 0xF);  // row_shr:1
    FR_DPP_SHR_ADD(0x112, 0xF);  // row_shr:2
    FR_DPP_SHR_ADD(0x114, 0xF);  // row_shr:4
    FR_DPP_SHR_ADD(0x118, 0xF);  // row_shr:8
    FR_DPP_SHR_ADD(0x142, 0xA);  // row_bcast:15
    FR_DPP_SHR_ADD(0x143, 0xC);  // row_bcast:31
#undef FR_DPP_SHR_ADD
    return x;
}

// Index of the lowest set bit of a 64-bit mask — and SOME index in 0 .. 63 for an empty mask, without a select: v_ffbl_b32
// returns -1 for 0, so the unsigned minimum over the two halves (the other half's count + 32, which wraps to 31) stays in
// range.  The blend walks let an idle lane read a valid record or pixel and mask what it does with it (__builtin_ctzll(0) is
// undefined, and the guarded form costs a v_cndmask per pair).
__device__ __forceinline__ int low_bit_or_any(u64 m)
{
    uint32_t a, b;
    asm("v_ffbl_b32 %0, %1" : "=v"(a) : "v"((uint32_t)m));
    asm("v_ffbl_b32 %0, %1" : "=v"(b) : "v"((uint32_t)(m >> 32)));
    const uint32_t r = min(a, b + 32u);
    __builtin_assume(r < 64u);
    return (int)r;
}

// The exponent of the Gaussian falloff of one (pixel, record) pair from the record's conic — the reference's
// power = -0.5 (a dx^2 + c dy^2) - b dx dy (forward.cu:340) — with the conic stored as (-0.5 a, -b, -0.5 c): scalings by powers of
// two, so the record holds the reference's conic EXACTLY (the blend backward combines it with (dx, dy) per pixel, where an
// extra rounding of a against b would be amplified by the cancellation of the two products).  G = exp2(power * log2(e)).
constexpr float kLog2e = 1.4426950408889634f;
__device__ __forceinline__ float pair_power(float a2, float b2, float c2, float dx, float dy)
{
    float p = (a2 * dx) * dx;
    p = fmaf(c2 * dy, dy, p);
    return fmaf(b2 * dx, dy, p);
}

}  // namespace fr
