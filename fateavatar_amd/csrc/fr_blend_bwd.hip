// Back-to-front gradient pass over every 8x8 tile's sorted list for gfx950 (reference: renderCUDA, backward.cu:399-557).
// Per (pixel, Gaussian) pair the arithmetic is the reference's.
//
// Execution model: the forward has left every UNIT of 64 records with the state behind it, so every unit is an
// independent wavefront-sized work item, one pixel per lane (k_unit_blend_bwd_sparse strides over the forward's work
// list, BwdUnit).  A unit walks only the (pixel, record) pairs its footprint masks name and sums each record's gradient
// moments without a cross-lane reduction (see "sparse blend backward" below); a unit in which most pairs are named takes
// the all-pairs form instead (bwd_unit_all_pairs).  Either way the 64 pixels of the tile are reduced inside the wavefront
// before anything goes to memory, instead of the reference's 9 global atomics per contributing PAIR.
#include "fr_tile.hpp"
#include "fr_diag.hpp"
#include <hip/hip_ext.h>
#include <type_traits>

namespace fr {

// ------------------------------------------------------------------ all-pairs form
// Four Gaussians are processed per step: their 4 x 9 per-lane partial gradients go through a reduce-scatter butterfly
// (v_permlane32_swap / v_permlane16_swap across the four 16-lane rows, DPP inside a row) that leaves each of the 36 totals
// in a different lane, and ONE global_atomic_add_f32 instruction with 36 active lanes adds them to the per-Gaussian
// accumulators.
#define FR_DPP_ADD(v, ctrl) ((v) + __builtin_bit_cast(float, __builtin_amdgcn_mov_dpp(__builtin_bit_cast(int, (v)), (ctrl), 0xF, 0xF, true)))

__device__ __forceinline__ float swap16_add(float a, float b)
{
    // even rows: a.r(2i) + a.r(2i+1) ; odd rows: b.r(2i) + b.r(2i+1)
    auto r = __builtin_amdgcn_permlane16_swap(__builtin_bit_cast(unsigned, a), __builtin_bit_cast(unsigned, b), false, false);
    return __builtin_bit_cast(float, (unsigned)r[0]) + __builtin_bit_cast(float, (unsigned)r[1]);
}

// Reduce 36 per-lane values across the 64 lanes; on return lane l holds the wave total of value
// bitrev6(l) (for bitrev6(l) < 36; other lanes hold junk).
__device__ __forceinline__ float reduce_scatter_36(const float (&r)[36], int lane)
{
    float a[18], b[9], c[5], d[3], e[2];
    // the swaps exchange halves (quarters) of two registers in place; the additions that follow are independent,
    // so two of them go into one packed v_pk_add_f32
    typedef float v2f __attribute__((ext_vector_type(2)));
#pragma unroll
    for (int i = 0; i < 18; i += 2) {                                        // lane bit 5 <- value bit 0
        auto p0 = __builtin_amdgcn_permlane32_swap(__builtin_bit_cast(unsigned, r[2 * i]), __builtin_bit_cast(unsigned, r[2 * i + 1]), false, false);
        auto p1 = __builtin_amdgcn_permlane32_swap(__builtin_bit_cast(unsigned, r[2 * i + 2]), __builtin_bit_cast(unsigned, r[2 * i + 3]), false, false);
        const v2f x = {__builtin_bit_cast(float, (unsigned)p0[0]), __builtin_bit_cast(float, (unsigned)p1[0])};
        const v2f y = {__builtin_bit_cast(float, (unsigned)p0[1]), __builtin_bit_cast(float, (unsigned)p1[1])};
        const v2f z = x + y;
        a[i] = z.x, a[i + 1] = z.y;
    }
#pragma unroll
    for (int i = 0; i < 9; i++) b[i] = swap16_add(a[2 * i], a[2 * i + 1]);   // lane bit 4 <- value bit 1 (pairing these
                                                                             // for packed adds costs more moves than it saves)
    const bool b3 = (lane & 8) != 0, b2 = (lane & 4) != 0, b1 = (lane & 2) != 0, b0 = (lane & 1) != 0;
#pragma unroll
    for (int i = 0; i < 4; i++) {                                            // lane bit 3 <- value bit 2
        const float lo = FR_DPP_ADD(b[2 * i], 0x128), hi = FR_DPP_ADD(b[2 * i + 1], 0x128);  // row_ror:8
        c[i] = b3 ? hi : lo;
    }
    c[4] = FR_DPP_ADD(b[8], 0x128);
#pragma unroll
    for (int i = 0; i < 2; i++) {                                            // lane bit 2 <- value bit 3
        const float lo = FR_DPP_ADD(c[2 * i], 0x141), hi = FR_DPP_ADD(c[2 * i + 1], 0x141);  // row_half_mirror
        d[i] = b2 ? hi : lo;
    }
    d[2] = FR_DPP_ADD(c[4], 0x141);
    {                                                                        // lane bit 1 <- value bit 4
        const float lo = FR_DPP_ADD(d[0], 0x4E), hi = FR_DPP_ADD(d[1], 0x4E);  // quad_perm [2,3,0,1]
        e[0] = b1 ? hi : lo;
        e[1] = FR_DPP_ADD(d[2], 0x4E);
    }
    const float lo = FR_DPP_ADD(e[0], 0xB1), hi = FR_DPP_ADD(e[1], 0xB1);      // quad_perm [1,0,3,2]; lane bit 0 <- value bit 5
    return b0 ? hi : lo;
}

// reduce_scatter_36 for 40 values (four records x 10 components: the blend backward of a frame with depth and alpha planes):
// lane l holds the wave total of value bitrev6(l) for bitrev6(l) < 40.  The same butterfly; only the first three levels
// have more registers to pair (and level 3 no value left over).
__device__ __forceinline__ float reduce_scatter_40(const float (&r)[40], int lane)
{
    float a[20], b[10], c[5], d[3], e[2];
    typedef float v2f __attribute__((ext_vector_type(2)));
#pragma unroll
    for (int i = 0; i < 20; i += 2) {                                        // lane bit 5 <- value bit 0
        auto p0 = __builtin_amdgcn_permlane32_swap(__builtin_bit_cast(unsigned, r[2 * i]), __builtin_bit_cast(unsigned, r[2 * i + 1]), false, false);
        auto p1 = __builtin_amdgcn_permlane32_swap(__builtin_bit_cast(unsigned, r[2 * i + 2]), __builtin_bit_cast(unsigned, r[2 * i + 3]), false, false);
        const v2f x = {__builtin_bit_cast(float, (unsigned)p0[0]), __builtin_bit_cast(float, (unsigned)p1[0])};
        const v2f y = {__builtin_bit_cast(float, (unsigned)p0[1]), __builtin_bit_cast(float, (unsigned)p1[1])};
        const v2f z = x + y;
        a[i] = z.x, a[i + 1] = z.y;
    }
#pragma unroll
    for (int i = 0; i < 10; i++) b[i] = swap16_add(a[2 * i], a[2 * i + 1]);  // lane bit 4 <- value bit 1
    const bool b3 = (lane & 8) != 0, b2 = (lane & 4) != 0, b1 = (lane & 2) != 0, b0 = (lane & 1) != 0;
#pragma unroll
    for (int i = 0; i < 5; i++) {                                            // lane bit 3 <- value bit 2
        const float lo = FR_DPP_ADD(b[2 * i], 0x128), hi = FR_DPP_ADD(b[2 * i + 1], 0x128);  // row_ror:8
        c[i] = b3 ? hi : lo;
    }
#pragma unroll
    for (int i = 0; i < 2; i++) {                                            // lane bit 2 <- value bit 3
        const float lo = FR_DPP_ADD(c[2 * i], 0x141), hi = FR_DPP_ADD(c[2 * i + 1], 0x141);  // row_half_mirror
        d[i] = b2 ? hi : lo;
    }
    d[2] = FR_DPP_ADD(c[4], 0x141);
    {                                                                        // lane bit 1 <- value bit 4
        const float lo = FR_DPP_ADD(d[0], 0x4E), hi = FR_DPP_ADD(d[1], 0x4E);  // quad_perm [2,3,0,1]
        e[0] = b1 ? hi : lo;
        e[1] = FR_DPP_ADD(d[2], 0x4E);
    }
    const float lo = FR_DPP_ADD(e[0], 0xB1), hi = FR_DPP_ADD(e[1], 0xB1);      // quad_perm [1,0,3,2]; lane bit 0 <- value bit 5
    return b0 ? hi : lo;
}

__device__ __forceinline__ int bitrev6(int l)
{
    return ((l & 1) << 5) | ((l & 2) << 3) | ((l & 4) << 1) | ((l & 8) >> 1) | ((l & 16) >> 3) | ((l & 32) >> 5);
}

// All 64 x 64 pairs of one staged unit, back to front, four records at a time: every lane (= pixel) evaluates the four
// records, the 36 partial sums are reduce-scattered over the wave and 36 lanes issue one atomic each.  T / A enter as
// the state behind the unit (see k_unit_blend_bwd_sparse); lanes with lim <= 0 carry T = A = 0.  PLANES (FR_FLAG_DEPTH_ALPHA):
// the records' view-space depths s_z are a fourth colour channel with dL/dpixel dpz (A and bg_dot_dpixel carry it), and a
// tenth component, ACC_Z = alpha T dpz, goes with the nine: 40 partial sums, 40 lanes.
template <bool PLANES>
__device__ __forceinline__ void bwd_unit_all_pairs(const float4* __restrict__ s_rec, const float* __restrict__ s_z, int m, int lim,
                                                   float fx, float fy, float T, float A, float T_final, float bg_dot_dpixel,
                                                   float dpr, float dpg, float dpb, float dpz, float* __restrict__ accum, int lane,
                                                   int vv, int own_u, int own_c)
{
    constexpr int NC = PLANES ? 10 : 9;   // components per record
    for (int j = ((m + kGroup - 1) & ~(kGroup - 1)) - kGroup; j >= 0; j -= kGroup) {
        float araw[kGroup], cd[kGroup], dx[kGroup], dy[kGroup], gx[kGroup], gy[kGroup];
        bool ok[kGroup];
        bool any_ok = false;
#pragma unroll
        for (int k = 0; k < kGroup; k++) {
            const float4 q0 = s_rec[(j + k) * kRecQuads + 0];
            const float4 q1 = s_rec[(j + k) * kRecQuads + 1];
            const float q2x = s_rec[(j + k) * kRecQuads + 2].x;
            dx[k] = q0.x - fx, dy[k] = q0.y - fy;
            // -(a dx + b dy), -(b dx + c dy): the pair's dG/d(centre) / G, from the record's conic (-0.5 a, -b, -0.5 c)
            gx[k] = fmaf(2.f * q0.z, dx[k], q0.w * dy[k]);
            gy[k] = fmaf(2.f * q1.x, dy[k], q0.w * dx[k]);
            const float power = pair_power(q0.z, q0.w, q1.x, dx[k], dy[k]);
            araw[k] = q1.y * __builtin_amdgcn_exp2f(power * kLog2e);  // opacity * G: alpha before the 0.99 clamp (1/255 < 0.99: same test)
            ok[k] = (j + k < lim) && !(power > 0.0f) && !(araw[k] < 1.0f / 255.0f);
            any_ok = any_ok || ok[k];
            cd[k] = (q1.z * dpr + q1.w * dpg) + q2x * dpb;  // colour . dL_dpixel
            if (PLANES) cd[k] += s_z[j + k] * dpz;          // (+ depth . dL_ddepth)
        }
        if (!__any(any_ok)) continue;

        float s[kGroup * NC];
#pragma unroll
        for (int k = kGroup - 1; k >= 0; k--) {  // back to front
            // Lanes that fail the tests take alpha = G = 0: every state update below is then the identity and
            // every partial gradient is zero, so nothing needs a per-lane select.
            const float ar_e = ok[k] ? araw[k] : 0.f;   // opacity * G, or 0
            const float a_e = __builtin_amdgcn_fmed3f(ar_e, 0.f, 0.99f);  // alpha = min(0.99, .), or 0 (ar_e >= 0)
            const float inv = __builtin_amdgcn_rcpf(1.f - a_e);
            T *= inv;  // transmittance in front of this Gaussian (backward.cu:503)
            const float e = cd[k] - A;                   // (colour - accum_rec) . dL_dpixel
            const float dL_dalpha = e * T + (-T_final * inv) * bg_dot_dpixel;  // backward.cu:525-534
            A += a_e * e;                                // accum_rec for the next (closer) Gaussian
            const float wgt = a_e * T;                   // dchannel_dcolor
            // q = dL_dG * G = (opacity * dL_dalpha) * G: the gradient ignores the 0.99 clamp, as the reference
            // does.  The reference's per-pair updates are all q times a monomial of (dx, dy); their
            // combination with the conic / opacity happens once per Gaussian in k_preprocess_bwd.
            const float q = dL_dalpha * ar_e;
            const float qdx = q * dx[k], qdy = q * dy[k];
            float* su = s + k * NC;
            su[ACC_MX] = q * gx[k];   // combined with the conic per PIXEL, as backward.cu:540-546 does (see ACC_MX)
            su[ACC_MY] = q * gy[k];
            su[ACC_CA] = qdx * dx[k];
            su[ACC_CB] = qdx * dy[k];
            su[ACC_CC] = qdy * dy[k];
            su[ACC_OP] = q;
            su[ACC_R] = wgt * dpr;
            su[ACC_G] = wgt * dpg;
            su[ACC_B] = wgt * dpb;
            if (PLANES) su[ACC_Z] = wgt * dpz;
        }
        float total;
        if constexpr (PLANES) total = reduce_scatter_40(s, lane);
        else total = reduce_scatter_36(s, lane);
        if (vv < kGroup * NC && (j + own_u) < m) {
            const uint32_t id = __float_as_uint(s_rec[(j + own_u) * kRecQuads + 2].y);
            atomic_add_f32(accum + (size_t)id * kAccumStride + own_c, total);
        }
    }
}

// ================================================================== sparse blend backward
// Only ~1 in 7 (pixel, record) pairs of an 8x8 tile passes the alpha test at BASELINE config 2 (splats a few pixels
// wide); the all-pairs form above evaluates all 64 x 64 of a unit and reduces 36 mostly-zero values across the
// wave for every four records.  This kernel only touches the pairs the records' footprint masks name
// (footprint_mask() of the forward, a superset of the pairs that pass; the exact tests are applied to each), in two phases per unit:
//   A  lane = PIXEL: walks the records whose mask holds the pixel, back to front (the reference's order), carrying
//      T and accum_rec . dL_dpixel in registers, and leaves (q = dL_dG G, w = alpha T) of every pair in LDS;
//   B  lane = RECORD: walks the pixels of its own mask, picks the pairs up and sums its nine gradient moments in
//      registers — no cross-lane reduction at all;
// then the 64 x 9 sums are re-laid through LDS so that the lanes of one global_atomic_add_f32 cover 7 records x 9
// components (lanes of an instruction that fall into the same 64-byte line merge into one L2 request).
// The pixel-major view of the masks (which records does pixel p touch) is the 64 x 64 bit-matrix transpose of the
// record-major one; the forward has stored both (BinningView::masks, walks).
// LDS per wave decides how many units are in flight per CU (the kernel is latency-bound: a unit is a chain of
// dependent LDS round trips): 9.25 KB -> 16 waves per CU, enough for every unit of BASELINE config 2 to be resident.
constexpr int kPairCap = 640;      // (q, w) slots per wave; denser units are processed in several record ranges
constexpr int kARecs = 2;         // records per phase-A iteration (3 and 4 measured: no faster, the T / accum_rec chain is the iteration)

struct SparseLds {
    float4 rec[kUnit * kRecQuads];  // the unit's records: (x, y, a', b') (c', opacity, r, g) (b, first pair slot, mask lo, hi)   3 KB
    float4 pix[64];                   // per pixel: dL_dpixel (r, g, b, -)                                     1 KB
    float2 pair[kPairCap + 64];       // (q, w) of every pair, RECORD-major: a record's pairs are consecutive  5.5 KB
                                      // (+ 64: one scratch slot per lane, where a lane without a pair reads and writes)
};

// maximum over the 64 lanes, in every lane's SGPR-able form (result is wave-uniform); read by the FR_DIAG_STATS accounting only
__device__ __forceinline__ uint32_t wave_max_u32(uint32_t x)
{
#define FR_DPP_MAX(CTRL) x = max(x, (uint32_t)__builtin_amdgcn_update_dpp((int)x, (int)x, (CTRL), 0xF, 0xF, false))
    FR_DPP_MAX(0xB1);   // quad_perm [1,0,3,2]
    FR_DPP_MAX(0x4E);   // quad_perm [2,3,0,1]
    FR_DPP_MAX(0x141);  // row_half_mirror
    FR_DPP_MAX(0x140);  // row_mirror
#undef FR_DPP_MAX
    // every lane now holds its 16-lane row's maximum
    const uint32_t a = (uint32_t)__builtin_amdgcn_readlane((int)x, 0), b = (uint32_t)__builtin_amdgcn_readlane((int)x, 16);
    const uint32_t c = (uint32_t)__builtin_amdgcn_readlane((int)x, 32), d = (uint32_t)__builtin_amdgcn_readlane((int)x, 48);
    return max(max(a, b), max(c, d));
}

// low_bit_or_any's mirror for phase A's back-to-front walk: the HIGHEST set bit, SOME index in 0 .. 63 for an empty mask
__device__ __forceinline__ int high_bit_or_any(u64 m)
{
    uint32_t a, b;
    asm("v_ffbh_u32 %0, %1" : "=v"(a) : "v"((uint32_t)(m >> 32)));
    asm("v_ffbh_u32 %0, %1" : "=v"(b) : "v"((uint32_t)m));
    const uint32_t r = min(a, b + 32u);
    __builtin_assume(r < 64u);
    return 63 - (int)r;
}

struct BlendBwdArgs {
    const DeviceCounts* counts;
    ImageView v;
    const float4* rec_tmpl;   // GeomView::rec_tmpl: the records are gathered through the sorted ids
    void* binning;
    int W, H;
    const float* bg;
    const float* dL_dpix;
    float* accum;
    uint32_t dense_pairs;
};

// What the blend backward of a frame with depth and alpha planes reads besides (FR_FLAG_DEPTH_ALPHA): the planes' upstream
// gradients (either may be null: zero) and the depth part of the units' entry state.
struct BwdPlaneArgs {
    const float* dL_ddepth;
    const float* dL_dalpha;
    const float* depth_state;
};
// the staged records' view-space depths next to the plain form's LDS (PLANES only)
struct SparseLdsPlanes : SparseLds {
    float z[kUnit];
};

// PLANES (FR_FLAG_DEPTH_ALPHA): the depth plane is a fourth colour channel whose colour is the record's view-space depth and
// whose background is 0 (A, the per-pair colour dot and phase B's tenth sum, ACC_Z = dL/dz), and the alpha plane
// 1 - T_final enters through the background term: dL/dT_final = bg . dL_dpixel - dL_dalpha.
template <bool PLANES>
__device__ __forceinline__ void unit_blend_bwd_sparse_body(const BlendBwdArgs& a, const BwdPlaneArgs& pl)
{
    constexpr int NC = PLANES ? 10 : 9;     // gradient components per record
    constexpr int RPF = PLANES ? 6 : 7;     // records per flush atomic (NC * RPF <= 63 lanes)
    const DeviceCounts* __restrict__ counts = a.counts;
    const ImageView v = a.v;
    void* binning = a.binning;
    const int W = a.W, H = a.H;
    const float* __restrict__ bg = a.bg;
    const float* __restrict__ dL_dpix = a.dL_dpix;
    float* __restrict__ accum = a.accum;
    const uint32_t dense_pairs = a.dense_pairs;
    __shared__ std::conditional_t<PLANES, SparseLdsPlanes, SparseLds> s_all[kWavesPerWG];
    const int lane = threadIdx.x & 63;
    const int wave_in_wg = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
    // The first unit's descriptor is requested BEFORE the counts are known (one round trip less in front of every
    // wave's first loads): the descriptors sit at the head of the binning buffer whatever its capacity, and there are at
    // least T + 1 of them (BinningView::units_for), so index min(u, T) is always inside the buffer.
    const uint32_t n_tiles = (uint32_t)v.tiles_x * (uint32_t)v.tiles_y;
    const uint32_t w_first = blockIdx.x * kWavesPerWG + wave_in_wg;   // slot of the work list (BwdUnit)
    const uint32_t nu = counts->num_units, capacity = counts->capacity;
    const BwdUnit* __restrict__ work = BinningView::make(binning, 0, (size_t)n_tiles).bwd_units;
    const uint4 d_first = work[min(w_first, n_tiles)].d;
    const uint32_t u_of_first = work[min(w_first, n_tiles)].u;
    // (pinned together: the descriptor load is issued before anything waits for the counts — without this the compiler
    // parks it behind the loop's entry test, i.e. behind the counts' round trip)
    asm volatile("" ::"v"(d_first.x), "v"(u_of_first), "s"(nu), "s"(capacity));
    const BinningView b = BinningView::make(binning, (size_t)capacity, (size_t)n_tiles);
    auto& S = s_all[wave_in_wg];
    const uint32_t wave_stride = gridDim.x * kWavesPerWG;
    const float bg0 = bg[0], bg1 = bg[1], bg2 = bg[2];
    // flush: lanes 0..62 = 7 records x 9 components; lane l of a septet starting at record r0 reads word r0 * 9 + l of
    // the [record][9] sums and adds it to component l % 9 of record r0 + l / 9 (PLANES: 6 records x 10 components)
    const int fl_rec = lane / NC, fl_c = lane - fl_rec * NC;
    float* const accum_c = accum + fl_c;
    // the same for the all-pairs form (bwd_unit_all_pairs): 4 records x 9 (10) components after its reduce-scatter
    const int vv = bitrev6(lane);
    const int own_u = vv / NC, own_c = vv - own_u * NC;
    const size_t HW = (size_t)H * W;
    for (uint32_t w = w_first; w < nu; w += wave_stride) {
        // ---- every load below depends on the descriptor only: all of them are in flight together (clamped indices keep
        // them unconditional; the compiler serialises loads that sit behind exec-masked branches)
        FR_TR_DECL;
        uint4 d = d_first;
        uint32_t u = u_of_first;
        if (w != w_first || w > n_tiles) d = work[w].d, u = work[w].u;
        const uint32_t base = d.y * kUnit, start = d.z, n = d.w;
        const uint32_t m = min((uint32_t)kUnit, n - base);
        const int tx0 = (int)(d.x & 0xFFFFu) * kTile, ty0 = (int)(d.x >> 16) * kTile;
        const int px = tx0 + (lane & 7), py = ty0 + (lane >> 3);
        const bool inside = px < W && py < H;
        const size_t pix = inside ? (size_t)py * W + px : 0;
        const uint32_t ridx = min(base + (uint32_t)lane, n - 1u);
        const RecSrc recsrc = {b.ids, a.rec_tmpl};
        const float4* rsrc = recsrc.at((size_t)start + ridx);
        const uint32_t last_raw = v.n_contrib[pix];
        const float4 rq0 = rsrc[0], rq1 = rsrc[1];
        const float2 rq2 = *reinterpret_cast<const float2*>(rsrc + 2);         // (colour b, id)
        const uint2 mraw = b.masks[(size_t)start + ridx];
        const uint2 bt = b.walks[(size_t)u * kUnit + lane];   // the unit's footprint masks, pixel-major
        const float Tf_raw = v.final_T[pix];
        // entry state (colour behind the unit / T_out, T_out).  A tile's last unit has nothing behind it and leaves with
        // final_T: the forward does not store that row (gather_tile)
        float4 st = make_float4(0.f, 0.f, 0.f, 0.f);
        const bool last_unit = base + (uint32_t)kUnit >= n;
        if (!last_unit) st = b.unit_state[(size_t)u * kUnit + lane];
        const float d0 = dL_dpix[pix], d1 = dL_dpix[HW + pix], d2 = dL_dpix[2 * HW + pix];
        // (PLANES: the record's depth, the two plane gradients and the depth entry state, with the other loads)
        float rz = 0.f, dz_raw = 0.f, da_raw = 0.f, sd = 0.f;
        if (PLANES) {
            rz = reinterpret_cast<const float*>(rsrc + 2)[2];
            if (pl.dL_ddepth) dz_raw = pl.dL_ddepth[pix];
            if (pl.dL_dalpha) da_raw = pl.dL_dalpha[pix];
            if (pl.dL_ddepth && !last_unit) sd = pl.depth_state[(size_t)u * kUnit + lane];   // (only ever multiplied by dL_ddepth)
            asm volatile("" ::"v"(rz), "v"(dz_raw), "v"(da_raw), "v"(sd));
        }
        // (pinned: otherwise everything but n_contrib is sunk below the early exit, a second round trip)
        asm volatile("" ::"v"(last_raw), "v"(rq0.x), "v"(rq1.x), "v"(rq2.x), "v"(mraw.x), "v"(bt.x), "v"(st.x), "v"(Tf_raw), "v"(d0), "v"(d1), "v"(d2));
        const uint32_t last = inside ? last_raw : 0u;
        FR_TR(0);   // the unit's loads have landed
        // nothing at or behind the deepest contributor of any pixel of the tile can matter
        if (!__any(last > base)) continue;

        // ---- lane = record: stage the records; this lane keeps what phase B needs of its own
        const bool valid_rec = base + (uint32_t)lane < n;
        const uint2 mj = valid_rec ? mraw : make_uint2(0u, 0u);
        const u64 Mj = ((u64)mj.y << 32) | mj.x;
        const uint32_t cnt = (uint32_t)__popcll(Mj);
        const uint32_t cum = wave_incl_scan_u32(cnt);             // pairs of records [0, lane]
        const uint32_t npairs = (uint32_t)__builtin_amdgcn_readlane((int)cum, 63);
        // A unit in which a large share of the 64 x 64 pairs is named is cheaper in the all-pairs form (wave-uniform
        // record reads, four independent alpha evaluations in flight, no divergent walk, no pair slots).
        const bool dense = npairs > dense_pairs;
        const uint32_t my_id = __float_as_uint(rq2.y);
        // (padding: opacity 0 -> alpha 0.  Component-wise on purpose: a select between two float4 goes through scratch)
        S.rec[lane * kRecQuads + 0] = make_float4(valid_rec ? rq0.x : 0.f, valid_rec ? rq0.y : 0.f, valid_rec ? rq0.z : 0.f, valid_rec ? rq0.w : 0.f);
        S.rec[lane * kRecQuads + 1] = make_float4(valid_rec ? rq1.x : 0.f, valid_rec ? rq1.y : 0.f, valid_rec ? rq1.z : 0.f, valid_rec ? rq1.w : 0.f);
        // the walks read (colour b, first pair slot, mask) from the third quad, the all-pairs form (colour b, id)
        S.rec[lane * kRecQuads + 2] = make_float4(rq2.x, dense ? rq2.y : __uint_as_float(cum - cnt), __uint_as_float(mj.x), __uint_as_float(mj.y));
        if constexpr (PLANES) S.z[lane] = valid_rec ? rz : 0.f;
        // the pixel's walk set, limited to the records in front of its last contributor
        const int lim = (int)last - (int)base;      // records [0, lim) of this unit can contribute to this pixel
        u64 Bp = ((u64)bt.y << 32) | bt.x;
        Bp = lim <= 0 ? 0ull : (lim >= 64 ? Bp : (Bp & ((1ull << lim) - 1ull)));

        const float T_final = inside ? Tf_raw : 0.f;
        const float dpr = inside ? d0 : 0.f, dpg = inside ? d1 : 0.f, dpb = inside ? d2 : 0.f;
        const float fx = (float)px, fy = (float)py;
        const float dpz = inside ? dz_raw : 0.f, dpa = inside ? da_raw : 0.f;   // (PLANES; 0 otherwise)
        float bgd = (bg0 * dpr + bg1 * dpg) + bg2 * dpb;
        if (PLANES) bgd -= dpa;                                                // alpha = 1 - T_final
        const float tfb = -T_final * bgd;                                      // -T_final * (bg . dL_dpixel)
        float T = lim > 0 ? (last_unit ? Tf_raw : st.w) : 0.f;
        float A = lim > 0 ? (st.x * dpr + st.y * dpg) + st.z * dpb : 0.f;     // accum_rec . dL_dpixel: the recurrence is linear, one scalar is carried
        if (PLANES) A += lim > 0 ? sd * dpz : 0.f;
        const float* s_z = nullptr;
        if constexpr (PLANES) s_z = S.z;
        if (dense) {
            __builtin_amdgcn_fence(__ATOMIC_ACQ_REL, "wavefront");
            __builtin_amdgcn_wave_barrier();
            bwd_unit_all_pairs<PLANES>(S.rec, s_z, (int)m, lim, fx, fy, T, A, T_final, bgd, dpr, dpg, dpb, dpz, accum, lane, vv, own_u,
                                       own_c);
            __builtin_amdgcn_wave_barrier();   // (S.rec is restaged by the next unit)
            continue;
        }
        S.pix[lane] = make_float4(dpr, dpg, dpb, PLANES ? dpz : 0.f);
        const float rxl = rq0.x - (float)tx0, ryl = rq0.y - (float)ty0;           // own record centre, tile-local
        // own record's conic as stored, (a', b', c') = (-0.5 a, -b, -0.5 c) EXACTLY: phase B combines a pair's (dx, dy) with it
        // per PIXEL — (2 a' dx + b' dy, b' dx + 2 c' dy) = -(a dx + b dy, b dx + c dy) = dG/d(centre) / G — as backward.cu:540-546 does
        const float ca2 = 2.f * rq0.z, cc2 = 2.f * rq1.x, cb1 = rq0.w;

        // ---- record ranges [lo, hi), from the back, each with at most kPairCap mask bits
        int hi = (int)m;
        FR_TR(1);   // staged
        while (hi > 0) {
            const uint32_t cum_hi = (uint32_t)__builtin_amdgcn_readlane((int)cum, hi - 1);
            int lo = 0;
            if (cum_hi > (uint32_t)kPairCap) {   // (rare: the whole unit normally fits)
                // smallest lo with pairs[lo, hi) <= kPairCap: lanes are monotone in that predicate
                const bool fits = (lane < hi) && (cum_hi - (cum - cnt) <= (uint32_t)kPairCap);
                lo = (int)__builtin_ctzll(__ballot(fits));   // hi - 1 always fits (a record has <= 64 bits)
            }
            const u64 range = (hi >= 64 ? ~0ull : ((1ull << hi) - 1ull)) & ~((1ull << lo) - 1ull);
            const uint32_t slot0 = (uint32_t)__builtin_amdgcn_readlane((int)(cum - cnt), lo);   // first slot of the range
            const uint32_t np = cum_hi - slot0;
            // pairs no pixel walks (record behind the pixel's last contributor, pixel outside the image) must read as
            // zero in phase B: only then is anything left unwritten by phase A
            if (!__all(inside && lim >= hi))
                for (uint32_t z = (uint32_t)lane; z * 2u < np; z += 64u)
                    reinterpret_cast<float4*>(S.pair)[z] = make_float4(0.f, 0.f, 0.f, 0.f);
            __builtin_amdgcn_fence(__ATOMIC_ACQ_REL, "wavefront");
            __builtin_amdgcn_wave_barrier();

            // ---- phase A: lane = pixel, back to front over the records its mask column names.  Two records per
            // iteration: their alpha evaluations and slot computations are independent instruction streams; only the
            // T / accum_rec recurrence is serial
            u64 Bg = Bp & range;
#ifdef FR_DIAG_STATS
            const uint32_t stat_a = (wave_max_u32((uint32_t)__popcll(Bg)) + 1u) >> 1;
            const uint32_t stat_b = (wave_max_u32((lane >= lo && lane < hi) ? cnt : 0u) + 1u) >> 1;
#endif
            FR_STAT_ADD(counts, 0, 1u);       // record ranges
            FR_STAT_ADD(counts, 1, stat_a);   // phase A trips (two records each)
            FR_STAT_ADD(counts, 3, np);       // pair slots
            FR_STAT_ADD(counts, 4, stat_b);   // phase B trips (two pixels each)
            FR_TR(3);   // range set up, slots zeroed
            if (__any(Bg != 0ull) && !FR_ABLATE(2)) do {   // (do-while: as a while loop the compiler copies the loop-carried registers every trip)
                bool act[kARecs];
                int j[kARecs];
#pragma unroll
                for (int k = 0; k < kARecs; k++) {
                    act[k] = Bg != 0ull;
                    j[k] = high_bit_or_any(Bg);
                    Bg &= ~(1ull << j[k]);       // (no bits set: stays 0)
                }
                float ar_e[kARecs], cd[kARecs];
                uint32_t slot[kARecs];
#pragma unroll
                for (int k = 0; k < kARecs; k++) {
                    const float4 q0 = S.rec[j[k] * kRecQuads + 0];
                    const float4 q1 = S.rec[j[k] * kRecQuads + 1];
                    const float4 q2 = S.rec[j[k] * kRecQuads + 2];
                    const float dx = q0.x - fx, dy = q0.y - fy;
                    const float power = pair_power(q0.z, q0.w, q1.x, dx, dy);
                    const float araw = q1.y * __builtin_amdgcn_exp2f(power * kLog2e);   // opacity * G (alpha before the 0.99 clamp)
                    const bool ok = act[k] && !(power > 0.0f) && !(araw < 1.0f / 255.0f);
                    cd[k] = (q1.z * dpr + q1.w * dpg) + q2.x * dpb;              // colour . dL_dpixel
                    if (PLANES) cd[k] += s_z[j[k]] * dpz;                       // (+ depth . dL_ddepth)
                    ar_e[k] = ok ? araw : 0.f;                                  // failed pair: alpha = 0, every update is the identity
                    // rank of this pixel among the record's pixels: mask bits below this lane (v_mbcnt: popcount of
                    // (operand & lanes-below-mine) + accumulator, two instructions for the 64 bits)
                    slot[k] = __builtin_amdgcn_mbcnt_hi(__float_as_uint(q2.w),
                                                        __builtin_amdgcn_mbcnt_lo(__float_as_uint(q2.z), __float_as_uint(q2.y) - slot0));
                    slot[k] = act[k] ? slot[k] : (uint32_t)kPairCap + (uint32_t)lane;   // (idle lane: its own scratch slot, no exec games)
                }
#pragma unroll
                for (int k = 0; k < kARecs; k++) {
                    const float a_e = __builtin_amdgcn_fmed3f(ar_e[k], 0.f, 0.99f);
                    const float inv = __builtin_amdgcn_rcpf(1.f - a_e);
                    T *= inv;                                                   // backward.cu:503
                    const float e = cd[k] - A;
                    const float dL_dalpha = e * T + tfb * inv;                  // backward.cu:525-534
                    A += a_e * e;
                    S.pair[slot[k]] = make_float2(dL_dalpha * ar_e[k], a_e * T);   // (q = dL_dG G, w = dchannel_dcolor)
                }
            } while (__any(Bg != 0ull));
            __builtin_amdgcn_fence(__ATOMIC_ACQ_REL, "wavefront");
            __builtin_amdgcn_wave_barrier();
            FR_TR(4);   // phase A

            // ---- phase B: lane = record, over its own pixels (two per iteration); its pairs are consecutive slots
            typedef float v2f __attribute__((ext_vector_type(2)));
            v2f s_m = {0.f, 0.f}, s_ab = {0.f, 0.f}, s_rg = {0.f, 0.f};   // (MX, MY) (CA, CB) (R, G)
            float s_cc = 0.f, s_op = 0.f, s_b = 0.f, s_z_sum = 0.f;
            u64 Mg = (lane >= lo && lane < hi) ? Mj : 0ull;
            uint32_t slot = (cum - cnt) - slot0;
            if (__any(Mg != 0ull) && !FR_ABLATE(3)) do {
#pragma unroll
                for (int k = 0; k < 2; k++) {
                    const bool act = Mg != 0ull;
                    const int p = low_bit_or_any(Mg);
                    Mg &= Mg - 1ull;
                    float2 qw = S.pair[act ? slot : (uint32_t)kPairCap + (uint32_t)lane];
                    const float q = act ? qw.x : 0.f, wgt = act ? qw.y : 0.f;
                    slot += act ? 1u : 0u;
                    const float4 dp = S.pix[p];
                    const v2f dd = {rxl - (float)(p & 7), ryl - (float)(p >> 3)};
                    const v2f qd = q * dd;
                    // q (2a' dx + b' dy), q (2c' dy + b' dx): the pixel's two products go into the sums one behind the other
                    // (the running sum stays as small as the combined value: what matters for the rounding)
                    s_m += (v2f){ca2, cc2} * qd;
                    s_m += cb1 * (v2f){qd.y, qd.x};
                    s_ab += qd.x * dd;
                    s_cc += qd.y * dd.y;
                    s_op += q;
                    s_rg += wgt * (v2f){dp.x, dp.y};
                    s_b += wgt * dp.z;
                    if (PLANES) s_z_sum += wgt * dp.w;
                }
            } while (__any(Mg != 0ull));
            __builtin_amdgcn_fence(__ATOMIC_ACQ_REL, "wavefront");
            __builtin_amdgcn_wave_barrier();
            FR_TR(5);   // phase B
            // ---- flush: [record][9] through LDS (the pair slots are dead now), then 7 records x 9 components per atomic
            // (PLANES: [record][10], 6 records x 10 components)
            float* fl = reinterpret_cast<float*>(S.pair);
            {
                float* o = fl + lane * NC;
                o[ACC_MX] = s_m.x, o[ACC_MY] = s_m.y, o[ACC_CA] = s_ab.x, o[ACC_CB] = s_ab.y, o[ACC_CC] = s_cc, o[ACC_OP] = s_op;
                o[ACC_R] = s_rg.x, o[ACC_G] = s_rg.y, o[ACC_B] = s_b;
                if (PLANES) o[ACC_Z] = s_z_sum;
            }
            __builtin_amdgcn_fence(__ATOMIC_ACQ_REL, "wavefront");
            __builtin_amdgcn_wave_barrier();
            for (int r0 = lo; r0 < hi; r0 += RPF) {
                const int rj = r0 + fl_rec;
                const uint32_t id = (uint32_t)__builtin_amdgcn_ds_bpermute(min(rj, 63) << 2, (int)my_id);
                const float val = fl[r0 * NC + lane];
                if (lane < RPF * NC && rj < hi && val != 0.f && !FR_ABLATE(4)) {
                    if (FR_ABLATE(5)) accum_c[(size_t)id * kAccumStride] = val;   // (timing experiment: plain stores)
                    else atomic_add_f32(accum_c + (size_t)id * kAccumStride, val);
                }
            }
            __builtin_amdgcn_fence(__ATOMIC_ACQ_REL, "wavefront");
            __builtin_amdgcn_wave_barrier();
            FR_TR(6);   // flush
            hi = lo;
        }
        FR_TR_STORE(u);
    }
}

__global__ void __launch_bounds__(256) k_unit_blend_bwd_sparse(BlendBwdArgs a) { unit_blend_bwd_sparse_body<false>(a, BwdPlaneArgs{}); }
__global__ void __launch_bounds__(256) k_unit_blend_bwd_sparse_batch(BatchOf<BlendBwdArgs> b)
{
    unit_blend_bwd_sparse_body<false>(b.v[blockIdx.y], BwdPlaneArgs{});
}
// frames with depth and alpha planes (FR_FLAG_DEPTH_ALPHA) whose backward is handed a plane gradient
struct BlendBwdPlanesArgs {
    BlendBwdArgs b;
    BwdPlaneArgs p;
};
__global__ void __launch_bounds__(256) k_unit_blend_bwd_sparse_planes(BlendBwdPlanesArgs a) { unit_blend_bwd_sparse_body<true>(a.b, a.p); }
__global__ void __launch_bounds__(256) k_unit_blend_bwd_sparse_planes_batch(BatchOf<BlendBwdPlanesArgs> b)
{
    unit_blend_bwd_sparse_body<true>(b.v[blockIdx.y].b, b.v[blockIdx.y].p);
}

// test hook: run the 36-value reduce-scatter on in[lane*36 + k] and return each lane's result
__global__ void __launch_bounds__(64) k_selftest_reduce(const float* in, float* out)
{
    float r[36];
    for (int k = 0; k < 36; k++) r[k] = in[threadIdx.x * 36 + k];
    out[threadIdx.x] = reduce_scatter_36(r, threadIdx.x);
}

int launch_selftest_reduce(const float* in, float* out, hipStream_t s)
{
    hipLaunchKernelGGL(k_selftest_reduce, dim3(1), dim3(64), 0, s, in, out);
    FR_HIP(hipGetLastError());
    return FR_OK;
}

constexpr uint32_t kUnitGrid = 8192;  // most workgroups (of 4 waves) of the blend backward, which strides over the work list beyond that
                                      // (config 5, ~30 k units: 8192 workgroups 70.6 us, 2048: 73.4, 1024: 75.4 — the dispatcher balances better than the stride)

int launch_blend_backward(int n, const BackwardCall* calls, const GeomView* g, const ImageView* v, bool planes, hipStream_t s, bool debug)
{
    // The unit count lives on the device: grid-stride loop over the units, whatever the grid.  The grid follows the unit
    // count of the handle's most recent frame whose counts have reached the host (+ 1/8), between 256 and kUnitGrid
    // workgroups: waves that find no unit still cost a dispatch slot and a round trip for the counts.
    uint32_t unit_grid = 256;
    for (int k = 0; k < n; k++) {
        const fr_handle_impl* h = calls[k].h;
        const uint32_t seen = h->counts_seen ? reinterpret_cast<const uint32_t*>(h->host_counts)[5] : ~0u;
        const uint32_t want = seen > 4u * kUnitGrid ? kUnitGrid : (seen + seen / 8 + kWavesPerWG - 1) / kWavesPerWG;
        unit_grid = min(kUnitGrid, max(unit_grid, want));
    }
    BlendBwdArgs a[kMaxBatch];
    for (int k = 0; k < n; k++) {
        a[k].counts = v[k].counts, a[k].v = v[k], a[k].binning = const_cast<void*>(calls[k].binning);
        a[k].rec_tmpl = g[k].rec_tmpl;
        a[k].W = calls[k].prm->W, a[k].H = calls[k].prm->H, a[k].bg = calls[k].in->background;
        a[k].dL_dpix = calls[k].dL_dpix, a[k].accum = g[k].accum, a[k].dense_pairs = calls[k].h->dense_pairs_bwd;
    }
    if (planes) {   // (a plane gradient, FR_FLAG_DEPTH_ALPHA: checked by fr_backward)
        BlendBwdPlanesArgs ap[kMaxBatch];
        for (int k = 0; k < n; k++) {
            const fr_aux* aux = calls[k].prm->aux;
            ap[k] = BlendBwdPlanesArgs{a[k], BwdPlaneArgs{aux ? aux->dL_ddepth : nullptr, aux ? aux->dL_dalpha : nullptr,
                                                          aux && aux->planes ? PlaneView::make(aux->planes, 0, 0).depth_state : nullptr}};
        }
        StageScope sc(calls[0].h, ST_BLEND_BWD, s);
        launch_views(k_unit_blend_bwd_sparse_planes, k_unit_blend_bwd_sparse_planes_batch, n, ap, unit_grid, 64 * kWavesPerWG, 0, s);
        FR_HIP(hipGetLastError());
        return debug_sync(debug, s, "blend_bwd");
    }
    hipEvent_t ev_a, ev_b;
    if (n == 1 && next_stage_events(calls[0].h, ST_BLEND_BWD, &ev_a, &ev_b)) {
        // the graded kernel, timed the way a profiler times it: events taken from the dispatch itself
        hipExtLaunchKernelGGL(k_unit_blend_bwd_sparse, dim3(unit_grid), dim3(64 * kWavesPerWG), 0, s, ev_a, ev_b, 0, a[0]);
    } else {
        StageScope sc(n > 1 ? calls[0].h : nullptr, ST_BLEND_BWD, s);
        launch_views(k_unit_blend_bwd_sparse, k_unit_blend_bwd_sparse_batch, n, a, unit_grid, 64 * kWavesPerWG, 0, s);
    }
    FR_HIP(hipGetLastError());
    return debug_sync(debug, s, "blend_bwd");
}

}  // namespace fr
