// Front-to-back alpha blend of every 8x8 tile's sorted list for gfx950 (reference: renderCUDA, forward.cu:263-389), in ONE
// launch per frame, and the gather of the image as a launch of its own (FR_BLEND_FWD=gather).
//
// Execution model: a tile's sorted list is cut into UNITS of 64 records, and every unit is an independent wavefront-sized
// work item, one pixel per lane, so the serial instruction stream of a wave is bounded by 64 records no matter how long a
// tile's list is.  k_unit_blend_chained walks only the (pixel, record) pairs the records' footprint masks name
// (footprint_mask; an all-pairs loop, blend_unit_dense_local, for the units in which most pairs are named), and walks them
// ONCE: compositing is linear in the transmittance entering a unit, so every unit first blends its records LOCALLY (T starts
// at 1, no termination test: partial colour, product of (1 - alpha), last blended record), then learns the transmittance
// entering it from the products of the units in front of it and scales.  Only a pixel whose transmittance crosses the
// reference's 1e-4 threshold INSIDE the unit (T_in >= 1e-4 > T_in * product; at most one unit per pixel) is walked again,
// from T_in, with the reference's termination test.  The tile's last unit gathers the image; the forward leaves, per unit
// and pixel, the state the backward starts from (masks, walks, unit_state, the BwdUnit work list), so that the backward
// runs every unit independently.  See "the blend with the unit chain resolved INSIDE the unit kernel" below for how the
// units of a tile talk to each other inside one launch.
// Tried on the way here and dropped: one workgroup per tile with barriers between the phases (30.7 us at config 2, bound
// by the latency chain of its heaviest tiles); local blend + a per-tile finishing kernel that chains the units and
// re-walks the crossing ones itself (25 us at config 2 in two launches, but a serial string of re-walks per tile behind
// an opaque surface: 64 us at opacity 0.9 against 33 us now).
#include "fr_tile.hpp"

//   -DFR_DIAG_FWD_TRACE   per-unit time stamps of k_unit_blend_chained's phases (development only: tools/diag/fwd_trace.py)
#ifdef FR_DIAG_FWD_TRACE
namespace fr {
__device__ unsigned long long g_fwd_trace[16384 * 16];
}
extern "C" int fr_debug_read_fwd_trace(void* dst, size_t bytes)
{
    return (int)hipMemcpyFromSymbol(dst, HIP_SYMBOL(fr::g_fwd_trace), bytes < sizeof(fr::g_fwd_trace) ? bytes : sizeof(fr::g_fwd_trace));
}
#define FW_STAMP(K) do { if (lane == 0 && u < 16384u) ::fr::g_fwd_trace[(size_t)u * 16 + (K)] = __builtin_readcyclecounter(); } while (0)
#define FW_STAMPV(K, V) do { if (lane == 0 && u < 16384u) ::fr::g_fwd_trace[(size_t)u * 16 + (K)] = (unsigned long long)(V); } while (0)
#else
#define FW_STAMP(K) do { } while (0)
#define FW_STAMPV(K, V) do { } while (0)
#endif

namespace fr {

// Which of the 64 pixels of tile (tile_x0, tile_y0) can pass the blend's alpha >= 1/255 test for this splat: a
// conservative SUPERSET (bit 8*row + column), one x-interval per pixel row from the roots of
//   a' dx^2 + (b' dy) dx + c' dy^2 >= -ln(255 opacity) - slack       (the record's conic (-0.5 a, -b, -0.5 c): the left side is ln G).
// The blend kernels walk only these pairs and apply the exact tests to each, so a bit too many costs one wasted
// evaluation and a missing bit would change the image: the slack covers the fp32 evaluation error of ln G in the
// blend loops, and anything not plainly an ellipse (a' >= 0, NaN) selects the whole row.
__device__ __forceinline__ uint2 footprint_mask(float x0, float y0, float a2, float b2, float c2, float opacity,
                                                float tile_x0, float tile_y0)
{
    const float L = 0.6931471805599453f * __builtin_amdgcn_logf(255.0f * opacity);   // ln (v_log_f32 is log2); alpha >= 1/255 <=> ln G >= -L
    // |terms| of ln G near the footprint edge are O(L + 1); ill-conditioned conics cancel larger terms
    const float far_x = fmaxf(fabsf(x0 - tile_x0), fabsf(x0 - (tile_x0 + 7.f)));
    const float far_y = fmaxf(fabsf(y0 - tile_y0), fabsf(y0 - (tile_y0 + 7.f)));
    const float mag = fabsf(a2) * far_x * far_x + fabsf(c2) * far_y * far_y + fabsf(b2) * far_x * far_y;
    const float thr = -L - (2e-3f + 4e-6f * mag);
    const bool ellipse = a2 < 0.f;
    const float inv2a = __builtin_amdgcn_rcpf(2.f * a2);
    uint32_t m[2] = {0u, 0u};
    // (branch-free, and v_sqrt_f32 as it comes — one ulp, against a slack of 1e-3 pixels: the correctly rounded square
    // root the compiler emits for sqrtf() is eighteen instructions, and eight divergent regions per record cost more
    // than the arithmetic they skip)
#pragma unroll
    for (int r = 0; r < kTile; r++) {
        const float dy = y0 - (tile_y0 + (float)r);
        const float bb = b2 * dy;
        const float cc = c2 * dy * dy - thr;
        const float disc = bb * bb - 4.f * a2 * cc;
        const float sq = __builtin_amdgcn_sqrtf(fmaxf(disc, 0.f));
        // a' < 0: inv2a < 0, so (-bb + sq) * inv2a is the SMALLER root of dx = x0 - px
        const float dx_lo = (-bb + sq) * inv2a, dx_hi = (-bb - sq) * inv2a;
        const float lo = ceilf((x0 - dx_hi) - tile_x0 - 1e-3f), hi = floorf((x0 - dx_lo) - tile_x0 + 1e-3f);
        const int il = (int)fminf(fmaxf(lo, 0.f), 8.f), ih = (int)fminf(fmaxf(hi, -1.f), 7.f);
        const uint32_t span = il <= ih ? ((2u << ih) - 1u) & ~((1u << il) - 1u) : 0u;
        // the whole row unless this plainly is an ellipse with a real (or no) intersection: NaNs anywhere select it
        uint32_t row = 0xFFu;
        row = (ellipse && disc >= 0.f && lo == lo && hi == hi) ? span : row;
        row = (ellipse && disc < 0.f) ? 0u : row;
        m[r >> 2] |= row << (8 * (r & 3));
    }
    return make_uint2(m[0], m[1]);
}

// The pixel-major view of a unit's masks (which records does pixel p touch) is the 64 x 64 bit-matrix transpose of the
// record-major one, done in registers: v_permlane32_swap for the 32 x 32 blocks, rotate + v_bfi for the rest.
__device__ __forceinline__ uint32_t rotr32(uint32_t x, uint32_t s) { return __builtin_amdgcn_alignbit(x, x, s); }

struct TransposeConsts {
    uint32_t rot[5], sel[5];  // per level k = 16, 8, 4, 2, 1
};
__device__ __forceinline__ TransposeConsts transpose_consts(int lane)
{
    TransposeConsts c;
    const uint32_t keep_low[5] = {0x0000FFFFu, 0x00FF00FFu, 0x0F0F0F0Fu, 0x33333333u, 0x55555555u};
#pragma unroll
    for (int i = 0; i < 5; i++) {
        const uint32_t k = 16u >> i;
        const bool upper = ((uint32_t)lane & k) == 0;
        c.rot[i] = upper ? 32u - k : k;             // upper block rows take the partner's bits shifted UP by k
        c.sel[i] = upper ? ~keep_low[i] : keep_low[i];
    }
    return c;
}
// lane j holds row j (64 bits) of a 64 x 64 bit matrix; on return lane p holds column p
__device__ __forceinline__ uint2 transpose_bits64(uint2 row, int lane, const TransposeConsts& c)
{
    auto r = __builtin_amdgcn_permlane32_swap(row.x, row.y, false, false);   // [lo.low | hi.low], [lo.high | hi.high]
    uint32_t lo = (uint32_t)r[0], hi = (uint32_t)r[1];
#define FR_TR_LEVEL(I, K)                                                            \
    {                                                                                \
        const uint32_t ylo = (uint32_t)lane_xor_i32<K>((int)lo, lane), yhi = (uint32_t)lane_xor_i32<K>((int)hi, lane); \
        lo = (c.sel[I] & rotr32(ylo, c.rot[I])) | (~c.sel[I] & lo);                   \
        hi = (c.sel[I] & rotr32(yhi, c.rot[I])) | (~c.sel[I] & hi);                   \
    }
    FR_TR_LEVEL(0, 16)
    FR_TR_LEVEL(1, 8)
    FR_TR_LEVEL(2, 4)
    FR_TR_LEVEL(3, 2)
    FR_TR_LEVEL(4, 1)
#undef FR_TR_LEVEL
    return make_uint2(lo, hi);
}

struct RecRegs {
    float4 q0, q1, q2;
};

__device__ __forceinline__ RecRegs fetch_record(const RecSrc& rs, size_t start, uint32_t i, uint32_t n)
{
    RecRegs r;
    if (i < n) {
        const float4* __restrict__ src = rs.at(start + i);
        r.q0 = src[0];
        r.q1 = src[1];
        r.q2 = src[2];
    } else {  // padding: opacity 0 -> alpha 0 -> never blended
        r.q0 = make_float4(0.f, 0.f, 0.f, 0.f);
        r.q1 = r.q0;
        r.q2 = r.q0;
    }
    return r;
}

struct UnitInfo {
    uint32_t tx, ty, seg, start, n, base, m;  // tile position, segment index, list start, list length, first record, records in unit
    int px, py;
    bool inside;
};

// from the unit's descriptor (BinningView::unit_tile): (tile y << 16 | tile x, segment, list start, list length)
__device__ __forceinline__ UnitInfo unit_info(const uint4 d, int W, int H, int lane)
{
    UnitInfo i;
    i.tx = d.x & 0xFFFFu, i.ty = d.x >> 16;
    i.seg = d.y;
    i.start = d.z;
    i.n = d.w;
    i.base = i.seg * kUnit;
    i.m = min((uint32_t)kUnit, i.n - i.base);
    i.px = (int)i.tx * kTile + (lane & 7);
    i.py = (int)i.ty * kTile + (lane >> 3);
    i.inside = i.px < W && i.py < H;
    return i;
}

struct WalkOut {
    float Cr, Cg, Cb, T;
    uint32_t last;
    bool term;
    uint32_t iters;   // loop iterations taken (wave-uniform): the unit's cost class for the backward
    float Cd;         // PLANES: the depth channel, sum of z alpha T (0 otherwise)
};

// Front-to-back blend of the records in `Bg` (bit j = record j of the staged unit) for this lane's pixel, starting at
// transmittance T0; TERMINATE: apply the reference's T test (forward.cu:346-351).  Two records per iteration: their alpha
// evaluations are independent instruction streams, only the short T / colour recurrence is serial.  PLANES
// (FR_FLAG_DEPTH_ALPHA): the record's view-space depth (third quad, .z) is blended as a fourth colour channel, with the
// colours' arithmetic.  (It is finite for every record that is binned, the null records of non-finite colours included, and
// a pair that fails its tests is weighted by an exact 0.)
template <bool TERMINATE, bool PLANES = false>
__device__ __forceinline__ WalkOut walk_unit_fwd(const float4* __restrict__ rec, u64 Bg, float T0, float fx, float fy, uint32_t base)
{
    WalkOut o;
    o.Cr = o.Cg = o.Cb = o.Cd = 0.f;
    o.T = T0;
    o.last = 0u;
    o.term = false;
    o.iters = 0u;
    while (__any(Bg != 0ull)) {
        o.iters++;
        int j[2];
        bool act[2];
#pragma unroll
        for (int k = 0; k < 2; k++) {
            act[k] = Bg != 0ull;
            j[k] = low_bit_or_any(Bg);
            Bg &= Bg - 1ull;
        }
        float alpha[2], cr[2], cg[2], cb[2], cz[2];
        bool ok[2];
#pragma unroll
        for (int k = 0; k < 2; k++) {
            const float4 q0 = rec[j[k] * kRecQuads + 0];
            const float4 q1 = rec[j[k] * kRecQuads + 1];
            const float q2x = rec[j[k] * kRecQuads + 2].x;
            const float dx = q0.x - fx, dy = q0.y - fy;
            const float power = pair_power(q0.z, q0.w, q1.x, dx, dy);
            alpha[k] = fminf(0.99f, q1.y * __builtin_amdgcn_exp2f(power * kLog2e));
            ok[k] = act[k] && !(power > 0.0f) && !(alpha[k] < 1.0f / 255.0f);
            cr[k] = q1.z, cg[k] = q1.w, cb[k] = q2x;
            cz[k] = PLANES ? rec[j[k] * kRecQuads + 2].z : 0.f;
        }
#pragma unroll
        for (int k = 0; k < 2; k++) {
            bool c = ok[k];
            const float test_T = o.T * (1.f - alpha[k]);
            if (TERMINATE) {
                const bool fin = c && !o.term && (test_T < 0.0001f);
                o.term = o.term || fin;
                c = c && !o.term;
            }
            const float w = c ? alpha[k] * o.T : 0.f;
            o.Cr += cr[k] * w;
            o.Cg += cg[k] * w;
            o.Cb += cb[k] * w;
            if (PLANES) o.Cd += cz[k] * w;
            o.T = c ? test_T : o.T;
            o.last = c ? (base + (uint32_t)j[k] + 1u) : o.last;
        }
        if (TERMINATE) Bg = o.term ? 0ull : Bg;
    }
    return o;
}

// Units in which many of the 64 x 64 pairs pass are cheaper in the all-pairs form (wave-uniform record reads, four
// independent alpha evaluations in flight, no divergent walk): measured break-even around a fifth of the pairs.

// walk_unit_fwd from T = 1 over ALL records of the staged unit
template <bool TERMINATE, bool PLANES = false>
__device__ __forceinline__ WalkOut blend_unit_dense_local(const float4* __restrict__ rec, uint32_t m, bool inside, float fx,
                                                          float fy, uint32_t base)
{
    WalkOut o;
    o.Cr = o.Cg = o.Cb = o.Cd = 0.f;
    o.T = 1.f;
    o.last = 0u;
    o.term = false;
    o.iters = 64u;   // (a dense unit is a heavy unit)
    for (uint32_t j = 0; j < m; j += kGroup) {
        float alpha[kGroup], cr[kGroup], cg[kGroup], cb[kGroup], cz[kGroup];
        bool ok[kGroup];
#pragma unroll
        for (int k = 0; k < kGroup; k++) {   // (records beyond m are zero padding: alpha = 0)
            const float4 q0 = rec[(j + k) * kRecQuads + 0];
            const float4 q1 = rec[(j + k) * kRecQuads + 1];
            const float q2x = rec[(j + k) * kRecQuads + 2].x;
            const float dx = q0.x - fx, dy = q0.y - fy;
            const float power = pair_power(q0.z, q0.w, q1.x, dx, dy);
            alpha[k] = fminf(0.99f, q1.y * __builtin_amdgcn_exp2f(power * kLog2e));
            ok[k] = inside && !(power > 0.0f) && !(alpha[k] < 1.0f / 255.0f);
            cr[k] = q1.z, cg[k] = q1.w, cb[k] = q2x;
            cz[k] = PLANES ? rec[(j + k) * kRecQuads + 2].z : 0.f;
        }
#pragma unroll
        for (int k = 0; k < kGroup; k++) {
            bool c = ok[k];
            const float test_T = o.T * (1.f - alpha[k]);
            if (TERMINATE) {
                const bool fin = c && !o.term && (test_T < 0.0001f);
                o.term = o.term || fin;
                c = c && !o.term;
            }
            const float w = c ? alpha[k] * o.T : 0.f;
            o.Cr += cr[k] * w;
            o.Cg += cg[k] * w;
            o.Cb += cb[k] * w;
            if (PLANES) o.Cd += cz[k] * w;
            o.T = c ? test_T : o.T;
            o.last = c ? (base + j + (uint32_t)k + 1u) : o.last;
        }
        if (TERMINATE && __all(o.term || !inside)) break;
    }
    return o;
}

constexpr uint32_t kDeadBit = 0x80000000u;   // in a unit's `last` word: the pixel entered the unit below 1e-4

// a unit's final row as written by another workgroup of the SAME launch (agent-scope load), or of an earlier one
template <bool COHERENT>
__device__ __forceinline__ float load_row(const float* p)
{
    return COHERENT ? __hip_atomic_load(p, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT) : *p;
}

// The depth and alpha planes of a frame with FR_FLAG_DEPTH_ALPHA: where the forward blend keeps the depth channel's unit
// rows and entry state (PlaneView), and the two output planes.
struct PlaneArgs {
    float* unit_depth;
    float* depth_state;
    float* out_depth;
    float* out_alpha;
};

// One wave, one tile: the image, and the backward entry state of every unit, from the units' final
// contributions.  Pure loads and adds: the rows of 8 units are requested together.  FWD_ONLY (FR_FLAG_FORWARD_ONLY):
// no entry state is stored, the image / final_T / n_contrib are the same.  PLANES (FR_FLAG_DEPTH_ALPHA): the depth rows
// are summed like a colour channel (same order) into out_depth and the entry state's depth, out_alpha = 1 - final_T.
template <bool COHERENT, bool FWD_ONLY, bool PLANES = false>
__device__ __forceinline__ void gather_tile(const ImageView& v, uint32_t tile, uint32_t u0, uint32_t nu, const float* g_out,
                                            float4* __restrict__ unit_state, int W, int H, float bg0, float bg1, float bg2,
                                            float* __restrict__ out_color, int lane, const PlaneArgs& pl = PlaneArgs{})
{
    constexpr int R = 8;
    const int px = (int)(tile % (uint32_t)v.tiles_x) * kTile + (lane & 7);
    const int py = (int)(tile / (uint32_t)v.tiles_x) * kTile + (lane >> 3);
    const bool inside = px < W && py < H;
    const size_t pix = (size_t)py * W + px, HW = (size_t)H * W;
    float Cr = 0.f, Cg = 0.f, Cb = 0.f, Cd = 0.f, Tf = 1.0f;
    uint32_t ncon = 0;
    if (nu <= (uint32_t)R) {   // short tile: one round of loads; the image is the suffix pass's last sum
        float cr[R], cg[R], cb[R], cd[R], To[R];
        uint32_t lw[R];
#pragma unroll
        for (int k = 0; k < R; k++) {
            const uint32_t kk = (uint32_t)k < nu ? (uint32_t)k : 0u;   // (clamped: the loads stay unconditional)
            const float* o = g_out + (size_t)(u0 + kk) * 5 * kUnit + lane;
            cr[k] = load_row<COHERENT>(o), cg[k] = load_row<COHERENT>(o + kUnit), cb[k] = load_row<COHERENT>(o + 2 * kUnit);
            To[k] = load_row<COHERENT>(o + 3 * kUnit);
            lw[k] = __float_as_uint(load_row<COHERENT>(o + 4 * kUnit));
            cd[k] = PLANES ? load_row<COHERENT>(pl.unit_depth + (size_t)(u0 + kk) * kUnit + lane) : 0.f;
        }
#pragma unroll
        for (int k = 0; k < R; k++) {
            if ((uint32_t)k < nu) {
                const bool dead = (lw[k] & kDeadBit) != 0u;
                if (!dead) {
                    Tf = To[k];
                    if (lw[k] & ~kDeadBit) ncon = lw[k] & ~kDeadBit;
                }
            }
        }
        float Sr = 0.f, Sg = 0.f, Sb = 0.f, Sd = 0.f;
#pragma unroll
        for (int k = R - 1; k >= 0; k--) {
            if ((uint32_t)k < nu) {
                const float inv = (To[k] >= 0.0001f) ? __builtin_amdgcn_rcpf(To[k]) : 0.f;   // (dead on entry: T may have underflowed)
                // (the tile's LAST unit has nothing behind it and leaves with final_T: the backward builds that state itself)
                if (!FWD_ONLY && (uint32_t)k + 1u < nu) {
                    unit_state[(size_t)(u0 + (uint32_t)k) * kUnit + lane] = make_float4(Sr * inv, Sg * inv, Sb * inv, To[k]);
                    if (PLANES) pl.depth_state[(size_t)(u0 + (uint32_t)k) * kUnit + lane] = Sd * inv;
                }
                Sr += cr[k], Sg += cg[k], Sb += cb[k];   // (a dead pixel's contribution is stored as 0)
                if (PLANES) Sd += cd[k];
            }
        }
        // the rows are added BACK TO FRONT here as in the long tile below: units that contribute exactly 0 to every pixel behind
        // the real ones (the instances of Gaussians dropped for a non-finite colour) may move a tile from one
        // branch to the other, and the image must not change by a summation order
        Cr = Sr, Cg = Sg, Cb = Sb, Cd = Sd;
    } else {
        // long tile: ONE pass over the rows, back to front, eight units per round of loads — a unit's entry state is the sum
        // of the rows behind it, the image the sum of all of them (in this order), the final transmittance and contributor
        // count come from the last unit that was alive for the pixel.  (Units whose every pixel is dead get no state: the
        // backward never reads it.)
        float Sr = 0.f, Sg = 0.f, Sb = 0.f, Sd = 0.f;
        bool have_T = false, have_n = false;
        for (uint32_t base = (nu - 1u) & ~(uint32_t)(R - 1);; base -= R) {
            float cr[R], cg[R], cb[R], cd[R], To[R];
            uint32_t lw[R];
#pragma unroll
            for (int k = 0; k < R; k++) {
                const uint32_t kk = base + (uint32_t)k < nu ? base + (uint32_t)k : base;   // (clamped: the loads stay unconditional)
                const float* o = g_out + (size_t)(u0 + kk) * 5 * kUnit + lane;
                cr[k] = load_row<COHERENT>(o), cg[k] = load_row<COHERENT>(o + kUnit), cb[k] = load_row<COHERENT>(o + 2 * kUnit);
                To[k] = load_row<COHERENT>(o + 3 * kUnit);
                lw[k] = __float_as_uint(load_row<COHERENT>(o + 4 * kUnit));
                cd[k] = PLANES ? load_row<COHERENT>(pl.unit_depth + (size_t)(u0 + kk) * kUnit + lane) : 0.f;
            }
#pragma unroll
            for (int k = R - 1; k >= 0; k--) {
                if (base + (uint32_t)k < nu) {
                    const bool dead = (lw[k] & kDeadBit) != 0u;
                    const uint32_t last = lw[k] & ~kDeadBit;
                    if (!dead && !have_T) Tf = To[k], have_T = true;
                    if (!dead && !have_n && last) ncon = last, have_n = true;
                    const float inv = (To[k] >= 0.0001f) ? __builtin_amdgcn_rcpf(To[k]) : 0.f;
                    if (!FWD_ONLY && base + (uint32_t)k + 1u < nu && !__all(dead)) {
                        unit_state[(size_t)(u0 + base + (uint32_t)k) * kUnit + lane] = make_float4(Sr * inv, Sg * inv, Sb * inv, To[k]);
                        if (PLANES) pl.depth_state[(size_t)(u0 + base + (uint32_t)k) * kUnit + lane] = Sd * inv;
                    }
                    Sr += cr[k], Sg += cg[k], Sb += cb[k];
                    if (PLANES) Sd += cd[k];
                }
            }
            if (base == 0) break;
        }
        Cr = Sr, Cg = Sg, Cb = Sb, Cd = Sd;
    }
    if (inside) {
        v.final_T[pix] = Tf;
        v.n_contrib[pix] = ncon;
        out_color[pix] = Cr + Tf * bg0;
        out_color[HW + pix] = Cg + Tf * bg1;
        out_color[2 * HW + pix] = Cb + Tf * bg2;
        if (PLANES) pl.out_depth[pix] = Cd, pl.out_alpha[pix] = 1.f - Tf;   // (the depth's background is 0)
    }
}

// ---- the blend with the unit chain resolved INSIDE the unit kernel (decoupled look-back)
// Every unit publishes its per-pixel product as soon as it has it, reads the products of the units in front of it in
// its tile (normally already there: they started at the same time), and so knows its own entering transmittance while
// its records are still in LDS and its walk sets still in registers: the crossing pixels are re-walked on the spot, by
// thousands of waves in parallel.  What is left per tile is a plain gather (gather_tile), done by the tile's LAST unit
// once the others have delivered their rows (or by k_tile_gather as a launch of its own: FR_BLEND_FWD=gather).
//   hand-off: MI355X_MICROARCH.md's data-tagged form — the 4-byte product is its own flag (zeroed by k_tile_sort,
//   valid once non-zero; clamped to >= 1e-30, which still means "dead" to every reader), written and polled with
//   relaxed agent-scope accesses, no fences.
//   progress: a unit only waits for units with SMALLER indices and a workgroup takes exactly its four units and exits
//   (no grid-stride loop), so with workgroups dispatched in index order — what the hardware does — the unfinished
//   workgroup with the smallest index never waits for an undispatched one, whatever else holds compute units.  The
//   kernel does not RELY on that: every wait is a bounded poll (fr_handle_impl::chain_spins), and a unit whose poll
//   runs out computes the missing product or row itself from the other unit's records (unit_product_from_memory,
//   unit_row_from_memory).  Termination and the image are independent of dispatch order, timing and placement.
// A pixel is dead in a unit iff the product in front of it is below 1e-4 (products only shrink).  A pixel predicted to
// cross whose exact walk stops short of the test (the two products differ in the last bits, right at 1e-4) is dead
// behind this unit all the same — and that is what the reference computes too: its next contributor would trip the
// test without being blended, leaving T, the colour and n_contrib as they are.

// ---- what a unit does when a wait runs out: it computes what it was waiting for itself, from memory.
// The chain never depends on another workgroup making progress: every wait is a bounded poll with this behind it, so
// the launch finishes, and finishes with the same image, under ANY dispatch order or placement (cdna_hip_programming.md
// Guideline 16: "results must not depend on dispatch order, timing or workgroup -> XCD placement").  These loops read a
// unit's records straight from memory with wave-uniform addresses (no LDS: the caller's own records live there) in the
// same order and with the same expressions as the fast paths, so a helper and the owner of a unit store the same words.
// `-m gpu` runs whole frames with the poll bound set to zero (FR_CHAIN_SPINS=0): every hand-off takes this path.
struct UnitRow {
    float cr, cg, cb, To;
    uint32_t lw;
};

__device__ __forceinline__ void pair_alpha_from_memory(const float4* __restrict__ r, float fx, float fy, bool inside, float& alpha,
                                                       bool& ok, float& c0, float& c1, float& c2)
{
    const float4 q0 = r[0], q1 = r[1];
    const float dx = q0.x - fx, dy = q0.y - fy;
    const float power = pair_power(q0.z, q0.w, q1.x, dx, dy);
    alpha = fminf(0.99f, q1.y * __builtin_amdgcn_exp2f(power * kLog2e));
    ok = inside && !(power > 0.0f) && !(alpha < 1.0f / 255.0f);
    c0 = q1.z, c1 = q1.w, c2 = r[2].x;
}
// the record's view-space depth (GeomView::rec_tmpl column 10)
__device__ __forceinline__ float depth_from_memory(const float4* __restrict__ r) { return reinterpret_cast<const float*>(r + 2)[2]; }

// per-pixel product of (1 - alpha) over unit p's blendable records: what unit p publishes
__device__ float unit_product_from_memory(const uint4* __restrict__ unit_tile, const RecSrc& recs, uint32_t p, float fx,
                                          float fy, bool inside)
{
    const uint4 d = unit_tile[p];
    const uint32_t base = d.y * kUnit, m = min((uint32_t)kUnit, d.w - base);
    const size_t r0 = (size_t)d.z + base;
    float t = 1.0f;
    for (uint32_t j = 0; j < m; j++) {
        float alpha, c0, c1, c2;
        bool ok;
        pair_alpha_from_memory(recs.at(r0 + j), fx, fy, inside, alpha, ok, c0, c1, c2);
        t = ok ? t * (1.f - alpha) : t;
    }
    return fmaxf(t, 1e-30f);
}

// unit q's final row given the transmittance entering it
__device__ UnitRow unit_row_from_memory(const uint4* __restrict__ unit_tile, const RecSrc& recs, uint32_t q, float Tin,
                                        float fx, float fy, bool inside)
{
    const uint4 d = unit_tile[q];
    const uint32_t base = d.y * kUnit, m = min((uint32_t)kUnit, d.w - base);
    const size_t r0 = (size_t)d.z + base;
    float t = 1.0f, cr = 0.f, cg = 0.f, cb = 0.f;
    uint32_t last = 0u;
    for (uint32_t j = 0; j < m; j++) {   // the local blend (walk_unit_fwd<false> from T = 1)
        float alpha, c0, c1, c2;
        bool ok;
        pair_alpha_from_memory(recs.at(r0 + j), fx, fy, inside, alpha, ok, c0, c1, c2);
        const float w = ok ? alpha * t : 0.f;
        cr += c0 * w, cg += c1 * w, cb += c2 * w;
        t = ok ? t * (1.f - alpha) : t;
        last = ok ? (base + j + 1u) : last;
    }
    const bool dead = !inside || (Tin < 0.0001f);
    const bool crosses = !dead && (Tin * t < 0.0001f);
    UnitRow o;
    o.cr = dead ? 0.f : Tin * cr, o.cg = dead ? 0.f : Tin * cg, o.cb = dead ? 0.f : Tin * cb;
    o.To = dead ? Tin : Tin * t;
    uint32_t lw = dead ? 0u : last;
    if (__any(crosses)) {   // walk_unit_fwd<true> from Tin for the crossing pixels
        float T = Tin, xr = 0.f, xg = 0.f, xb = 0.f;
        uint32_t xl = 0u;
        bool term = false;
        for (uint32_t j = 0; j < m; j++) {
            float alpha, c0, c1, c2;
            bool ok;
            pair_alpha_from_memory(recs.at(r0 + j), fx, fy, inside, alpha, ok, c0, c1, c2);
            bool c = ok && crosses;
            const float test_T = T * (1.f - alpha);
            const bool fin = c && !term && (test_T < 0.0001f);
            term = term || fin;
            c = c && !term;
            const float w = c ? alpha * T : 0.f;
            xr += c0 * w, xg += c1 * w, xb += c2 * w;
            T = c ? test_T : T;
            xl = c ? (base + j + 1u) : xl;
        }
        if (crosses) o.cr = xr, o.cg = xg, o.cb = xb, o.To = T, lw = xl;
    }
    o.lw = lw | (dead ? kDeadBit : 0u);
    return o;
}

// FR_FLAG_DEPTH_ALPHA: the depth word of unit q's final row, the same walks and arithmetic as unit_row_from_memory's colours
__device__ float unit_depth_from_memory(const uint4* __restrict__ unit_tile, const RecSrc& recs, uint32_t q, float Tin, float fx,
                                        float fy, bool inside)
{
    const uint4 d = unit_tile[q];
    const uint32_t base = d.y * kUnit, m = min((uint32_t)kUnit, d.w - base);
    const size_t r0 = (size_t)d.z + base;
    float t = 1.0f, cd = 0.f;
    for (uint32_t j = 0; j < m; j++) {
        float alpha, c0, c1, c2;
        bool ok;
        pair_alpha_from_memory(recs.at(r0 + j), fx, fy, inside, alpha, ok, c0, c1, c2);
        const float w = ok ? alpha * t : 0.f;
        cd += depth_from_memory(recs.at(r0 + j)) * w;
        t = ok ? t * (1.f - alpha) : t;
    }
    const bool dead = !inside || (Tin < 0.0001f);
    const bool crosses = !dead && (Tin * t < 0.0001f);
    float o = dead ? 0.f : Tin * cd;
    if (__any(crosses)) {
        float T = Tin, xd = 0.f;
        bool term = false;
        for (uint32_t j = 0; j < m; j++) {
            float alpha, c0, c1, c2;
            bool ok;
            pair_alpha_from_memory(recs.at(r0 + j), fx, fy, inside, alpha, ok, c0, c1, c2);
            bool c = ok && crosses;
            const float test_T = T * (1.f - alpha);
            const bool fin = c && !term && (test_T < 0.0001f);
            term = term || fin;
            c = c && !term;
            const float w = c ? alpha * T : 0.f;
            xd += depth_from_memory(recs.at(r0 + j)) * w;
            T = c ? test_T : T;
        }
        if (crosses) o = xd;
    }
    return o;
}

// the product unit p published — or, if it has not appeared after `spins` polls, computed here
__device__ __forceinline__ float chain_product(float* g_tseg, const uint4* __restrict__ unit_tile, const RecSrc& recs,
                                               uint32_t p, float first, uint32_t spins, int lane, float fx, float fy, bool inside)
{
    float v = first;
    uint32_t k = 0;
    for (; !__all(v != 0.f) && k < spins; k++) {
        __builtin_amdgcn_s_sleep(2);
        v = __hip_atomic_load(g_tseg + (size_t)p * kUnit + lane, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    }
    if (!__all(v != 0.f)) v = unit_product_from_memory(unit_tile, recs, p, fx, fy, inside);
    return v;
}

struct ChainArgs {
    DeviceCounts* counts;
    const uint4* unit_tile;
    RecSrc recs;
    uint2* masks;
    uint2* walks;
    BwdUnit* bwd_units;
    uint32_t* stripe_cursor;
    uint32_t heavy_pairs;
    uint32_t unit_cap;
    int W, H, tiles_x;
    float* g_tseg;
    float* g_out;
    uint32_t dense_pairs;
    int pair_hist;
    uint32_t* unit_done;
    ImageView v;
    float4* unit_state;
    const float* bg;
    float* out_color;
    uint32_t chain_spins;
};

// FWD_ONLY (FR_FLAG_FORWARD_ONLY): a frame no backward will follow.  The footprint masks are still built and transposed
// (the walks run on them) but neither `masks` nor `walks` is stored, no unit takes a slot in the backward's work list, and
// the gather stores no entry state; the products, rows, unit_done flags and the image are exactly the full forward's.
// PLANES (FR_FLAG_DEPTH_ALPHA): the records keep their view-space depth in the staged third quad (the forward reads the
// footprint masks from registers only), the walks blend it as a fourth colour channel, every unit row gets a depth word in
// PlaneView::unit_depth, and the gather writes the depth and alpha planes; everything the plain forward writes is the same.
template <bool FWD_ONLY, bool PLANES>
__device__ __forceinline__ void unit_blend_chained_body(const ChainArgs& a, const PlaneArgs& pl)
{
    DeviceCounts* __restrict__ counts = a.counts;
    const uint4* __restrict__ unit_tile = a.unit_tile;
    const RecSrc recs = a.recs;
    uint2* __restrict__ masks = a.masks;
    const int W = a.W, H = a.H, pair_hist = a.pair_hist;
    float* g_tseg = a.g_tseg;
    float* g_out = a.g_out;
    const uint32_t dense_pairs = a.dense_pairs, chain_spins = a.chain_spins;
    uint32_t* unit_done = a.unit_done;
    const ImageView v = a.v;
    float4* __restrict__ unit_state = a.unit_state;
    const float* __restrict__ bg = a.bg;
    float* __restrict__ out_color = a.out_color;
    __shared__ float4 s_rec_all[kWavesPerWG][kUnit * kRecQuads];
    const int lane = threadIdx.x & 63;
    const int wave_in_wg = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
    float4* rec = s_rec_all[wave_in_wg];
    const uint32_t nu_all = counts->num_units;
    // (Giving XCD x a contiguous run of the units, as the backward's work list does, takes 4 MB off this kernel's L2
    // fills and 1 us off the isolated launch, but costs 2-3 % with frames in flight and at config 5: the heavy part of the
    // image then sits on one XCD.  Runs of 32 workgroups per XCD inside every 256: -2.6 MB, -0.3 us, still -1.5 % in
    // flight.  Measured, not kept.)
    const uint32_t u = blockIdx.x * kWavesPerWG + wave_in_wg;
    // (the unit's descriptor is requested together with the unit count, not behind it: one dependent round trip less in
    // front of every wave's records; a.unit_cap descriptors exist whatever the frame holds)
    const uint4 d_early = unit_tile[min(u, a.unit_cap - 1u)];
    asm volatile("" ::"v"(d_early.x), "s"(nu_all));
    if (u >= nu_all) return;
    FW_STAMP(0);
    FW_STAMPV(8, __builtin_amdgcn_s_memrealtime());
    const TransposeConsts tc = transpose_consts(lane);
    const UnitInfo ui = unit_info(d_early, W, H, lane);
    RecRegs rr = fetch_record(recs, (size_t)ui.start, ui.base + (uint32_t)lane, ui.n);
    asm volatile("" ::"v"(rr.q0.x), "v"(rr.q1.x), "v"(rr.q2.x));
    FW_STAMP(1);   // records in registers
    FW_STAMPV(10, ui.n);
    FW_STAMPV(11, ui.seg);
    // lane = record here: the footprint mask of this (tile, Gaussian) instance, kept in `masks` for the backward
    uint2 fm = make_uint2(0u, 0u);
    if (ui.base + (uint32_t)lane < ui.n) {
        fm = footprint_mask(rr.q0.x, rr.q0.y, rr.q0.z, rr.q0.w, rr.q1.x, rr.q1.y,
                            (float)((int)ui.tx * kTile), (float)((int)ui.ty * kTile));
        if (!PLANES) rr.q2.z = __uint_as_float(fm.x), rr.q2.w = __uint_as_float(fm.y);
        if (!FWD_ONLY) masks[(size_t)ui.start + ui.base + (uint32_t)lane] = fm;
    }
    rec[lane * kRecQuads + 0] = rr.q0;
    rec[lane * kRecQuads + 1] = rr.q1;
    rec[lane * kRecQuads + 2] = rr.q2;
    const uint2 bt = transpose_bits64(fm, lane, tc);
    if (!FWD_ONLY) a.walks[(size_t)u * kUnit + lane] = bt;   // (BinningView::walks: the backward does not repeat the transpose)
    __builtin_amdgcn_fence(__ATOMIC_ACQ_REL, "wavefront");
    __builtin_amdgcn_wave_barrier();
    const u64 Bp = ui.inside ? (((u64)bt.y << 32) | bt.x) : 0ull;
    const uint32_t npairs = (uint32_t)__builtin_amdgcn_readlane((int)wave_incl_scan_u32((uint32_t)__popc(fm.x) + (uint32_t)__popc(fm.y)), 63);
    if (pair_hist && lane == 0)
        atomicAdd(&counts->pair_hist[npairs <= 500 ? 0 : npairs <= 1000 ? 1 : npairs <= 1500 ? 2 : npairs <= 2500 ? 3 : 4], 1u);
    const float fx = (float)ui.px, fy = (float)ui.py;
    FW_STAMP(2);   // staged, masks, transpose
    FW_STAMPV(9, npairs);
    // ---- local blend from T = 1, no termination test
    const WalkOut o = npairs > dense_pairs ? blend_unit_dense_local<false, PLANES>(rec, ui.m, ui.inside, fx, fy, ui.base)
                                           : walk_unit_fwd<false, PLANES>(rec, Bp, 1.0f, fx, fy, ui.base);
    if (ui.base + kUnit < ui.n)   // (nobody reads the last unit's product)
        __hip_atomic_store(g_tseg + (size_t)u * kUnit + lane, fmaxf(o.T, 1e-30f), __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    // the unit's place in the backward's work list (BwdUnit): long walks from the front of its stripe, the others from the back
    if (!FWD_ONLY && lane == 0) {
        const bool heavy = npairs >= a.heavy_pairs;
        // Which stripe?  Stripe j holds slots j, j + 64, ...: n_j = ceil((nu - j) / 64) of them, and the hardware runs
        // the waves of slot w on XCD (w / 4) % 8, i.e. XCD x owns the eight stripes 4x .. 4x+3 and 32+4x .. 32+4x+3.
        // The units are dealt out so that XCD x gets a CONTIGUOUS run of them (neighbouring tiles: each L2 then
        // gathers its own eighth of the record table instead of all of it): the first N_0 units go to XCD 0, the next
        // N_1 to XCD 1 ... (N_x = the capacity of x's stripes), and inside a run round-robin over the eight stripes,
        // which fills every stripe exactly (the stripes of an XCD that have one slot more are the first ones).
        const uint32_t q = nu_all / kStripes, rem = nu_all % kStripes;
        uint32_t x = 0, first = 0;
        for (; x < 7u; x++) {
            const uint32_t lo4 = 4u * x, hi4 = 32u + 4u * x;
            const uint32_t n_x = 8u * q + (rem > lo4 ? min(rem - lo4, 4u) : 0u) + (rem > hi4 ? min(rem - hi4, 4u) : 0u);
            if (u < first + n_x) break;
            first += n_x;
        }
        const uint32_t t = (u - first) & 7u;
        const uint32_t j = t < 4u ? 4u * x + t : 32u + 4u * x + (t - 4u);
        const uint32_t n_j = (nu_all - j + kStripes - 1u) / kStripes;   // the stripe's slot count
        const uint32_t k = atomicAdd(a.stripe_cursor + (j * 2u + (heavy ? 0u : 1u)) * kStripeWords, 1u);
        BwdUnit* w = a.bwd_units + (j + kStripes * (heavy ? k : n_j - 1u - k));
        w->d = make_uint4(ui.ty << 16 | ui.tx, ui.seg, ui.start, ui.n);
        w->u = u;
        w->pad[0] = npairs, w->pad[1] = o.iters;   // (development: tools/diag/bwd_trace.py, bwd_order.py)
    }

    FW_STAMP(3);   // local walk done, product published
    // ---- transmittance entering the unit: the products of the units in front, in list order
    float Tin = 1.0f;
    for (uint32_t p = u - ui.seg; p < u; p += 4) {
        float pv[4];
#pragma unroll
        for (int k = 0; k < 4; k++)   // (requested together; clamped: the loads stay unconditional)
            pv[k] = __hip_atomic_load(g_tseg + (size_t)min(p + (uint32_t)k, u - 1u) * kUnit + lane, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
#pragma unroll
        for (int k = 0; k < 4; k++)
            if (p + (uint32_t)k < u)
                Tin *= chain_product(g_tseg, unit_tile, recs, p + (uint32_t)k, pv[k], chain_spins, lane, fx, fy, ui.inside);
    }

    FW_STAMP(4);   // entering transmittance known
    // ---- the unit's final contribution
    const bool dead = !ui.inside || (Tin < 0.0001f);
    const bool crosses = !dead && (Tin * o.T < 0.0001f);
    float Cr = dead ? 0.f : Tin * o.Cr, Cg = dead ? 0.f : Tin * o.Cg, Cb = dead ? 0.f : Tin * o.Cb;
    float To = dead ? Tin : Tin * o.T;
    uint32_t last = dead ? 0u : o.last;
    float Cd = PLANES && !dead ? Tin * o.Cd : 0.f;
    if (__any(crosses)) {   // the records are still staged, the walk sets still in registers
        const WalkOut x = walk_unit_fwd<true, PLANES>(rec, crosses ? Bp : 0ull, Tin, fx, fy, ui.base);
        if (crosses) Cr = x.Cr, Cg = x.Cg, Cb = x.Cb, To = x.T, last = x.last;
        if (PLANES && crosses) Cd = x.Cd;
    }
    if (unit_done && ui.seg == 0u && ui.base + kUnit >= ui.n) {
        // the tile's ONLY unit (12 % of BASELINE config 2's tiles; most tiles of a sparser scene): nothing to hand over, nothing to gather — the pixels are
        // final (gather_tile with one row: 0 + C, T, last), and the backward needs no entry state for a last unit
        if (ui.inside) {
            const size_t pix = (size_t)ui.py * W + ui.px, HW = (size_t)H * W;
            v.final_T[pix] = To;
            v.n_contrib[pix] = last;
            out_color[pix] = Cr + To * bg[0];
            out_color[HW + pix] = Cg + To * bg[1];
            out_color[2 * HW + pix] = Cb + To * bg[2];
            if (PLANES) pl.out_depth[pix] = Cd, pl.out_alpha[pix] = 1.f - To;
        }
        return;
    }
    float* out = g_out + (size_t)u * 5 * kUnit + lane;
    const uint32_t lw = last | (dead ? kDeadBit : 0u);
    if (!unit_done) {   // the gather is a launch of its own
        out[0] = Cr;
        out[kUnit] = Cg;
        out[2 * kUnit] = Cb;
        out[3 * kUnit] = To;
        out[4 * kUnit] = __uint_as_float(lw);
        if (PLANES) pl.unit_depth[(size_t)u * kUnit + lane] = Cd;
        return;
    }
    // ---- gather in the chain: the tile's LAST unit adds everything up once the others have delivered.  The rows are
    // written at agent scope (write-through), the wave waits until they are, and only then raises the unit's flag.
    // (Measured against this form: the four values as ONE 16-byte sc1 buffer store per pixel — the same time; the last
    // unit keeping its own row in registers instead of storing and re-reading it — 1 to 3.5 us SLOWER at config 2.)
    __hip_atomic_store(out, Cr, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    __hip_atomic_store(out + kUnit, Cg, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    __hip_atomic_store(out + 2 * kUnit, Cb, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    __hip_atomic_store(out + 3 * kUnit, To, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    __hip_atomic_store(out + 4 * kUnit, __uint_as_float(lw), __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    if (PLANES) __hip_atomic_store(pl.unit_depth + (size_t)u * kUnit + lane, Cd, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
    FW_STAMP(5);   // row written
    FW_STAMPV(12, __builtin_amdgcn_s_memrealtime());
    if (ui.base + kUnit < ui.n) {
        if (lane == 0) __hip_atomic_store(unit_done + u, 1u, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
        return;
    }
    const uint32_t u0 = u - ui.seg;
    for (uint32_t p = u0; p < u; p += 64) {
        const uint32_t q = min(p + (uint32_t)lane, u - 1u);
        uint32_t d = __hip_atomic_load(unit_done + q, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
        for (uint32_t spins = 0; !__all(d != 0u) && spins < chain_spins; spins++) {
            __builtin_amdgcn_s_sleep(2);
            d = __hip_atomic_load(unit_done + q, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
        }
        // rows that have not arrived: this wave writes them itself (see unit_row_from_memory: the same words their
        // owners store, whenever those get to it), front to back so that each one's entering transmittance is known
        u64 missing = __ballot(d == 0u && p + (uint32_t)lane < u);
        while (missing) {
            const uint32_t qq = p + (uint32_t)__builtin_ctzll(missing);
            missing &= missing - 1ull;
            float tin = 1.0f;
            for (uint32_t pp = u0; pp < qq; pp++)
                tin *= chain_product(g_tseg, unit_tile, recs, pp,
                                     __hip_atomic_load(g_tseg + (size_t)pp * kUnit + lane, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT), 0u,
                                     lane, fx, fy, ui.inside);
            const UnitRow rr = unit_row_from_memory(unit_tile, recs, qq, tin, fx, fy, ui.inside);
            float* o2 = g_out + (size_t)qq * 5 * kUnit + lane;
            __hip_atomic_store(o2, rr.cr, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
            __hip_atomic_store(o2 + kUnit, rr.cg, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
            __hip_atomic_store(o2 + 2 * kUnit, rr.cb, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
            __hip_atomic_store(o2 + 3 * kUnit, rr.To, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
            __hip_atomic_store(o2 + 4 * kUnit, __uint_as_float(rr.lw), __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
            if (PLANES)
                __hip_atomic_store(pl.unit_depth + (size_t)qq * kUnit + lane, unit_depth_from_memory(unit_tile, recs, qq, tin, fx, fy, ui.inside),
                                   __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
        }
        asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
    }
    asm volatile("" ::: "memory");
    FW_STAMP(6);   // (a tile's last unit) the other units' rows are there
    gather_tile<true, FWD_ONLY, PLANES>(v, ui.ty * (uint32_t)v.tiles_x + ui.tx, u0, ui.seg + 1u, g_out, unit_state, W, H, bg[0], bg[1], bg[2],
                                        out_color, lane, pl);
    FW_STAMP(7);   // gathered
    FW_STAMPV(12, __builtin_amdgcn_s_memrealtime());
}

__global__ void __launch_bounds__(256) k_unit_blend_chained(ChainArgs a) { unit_blend_chained_body<false, false>(a, PlaneArgs{}); }
__global__ void __launch_bounds__(256) k_unit_blend_chained_batch(BatchOf<ChainArgs> b) { unit_blend_chained_body<false, false>(b.v[blockIdx.y], PlaneArgs{}); }
// forward-only frames (FR_FLAG_FORWARD_ONLY): no backward hand-off
__global__ void __launch_bounds__(256) k_unit_blend_chained_fwd_only(ChainArgs a) { unit_blend_chained_body<true, false>(a, PlaneArgs{}); }
__global__ void __launch_bounds__(256) k_unit_blend_chained_fwd_only_batch(BatchOf<ChainArgs> b) { unit_blend_chained_body<true, false>(b.v[blockIdx.y], PlaneArgs{}); }
// frames with depth and alpha planes (FR_FLAG_DEPTH_ALPHA), with and without the backward hand-off
struct ChainPlanesArgs {
    ChainArgs c;
    PlaneArgs p;
};
__global__ void __launch_bounds__(256) k_unit_blend_chained_planes(ChainPlanesArgs a) { unit_blend_chained_body<false, true>(a.c, a.p); }
__global__ void __launch_bounds__(256) k_unit_blend_chained_planes_batch(BatchOf<ChainPlanesArgs> b)
{
    unit_blend_chained_body<false, true>(b.v[blockIdx.y].c, b.v[blockIdx.y].p);
}
__global__ void __launch_bounds__(256) k_unit_blend_chained_fwd_only_planes(ChainPlanesArgs a) { unit_blend_chained_body<true, true>(a.c, a.p); }
__global__ void __launch_bounds__(256) k_unit_blend_chained_fwd_only_planes_batch(BatchOf<ChainPlanesArgs> b)
{
    unit_blend_chained_body<true, true>(b.v[blockIdx.y].c, b.v[blockIdx.y].p);
}

// the gather as its own launch (FR_BLEND_FWD=gather): one wave per tile
template <bool FWD_ONLY, bool PLANES = false>
__device__ __forceinline__ void tile_gather_body(const DeviceCounts* __restrict__ counts, const ImageView& v,
                                                 const float* __restrict__ g_out, float4* __restrict__ unit_state, int W, int H,
                                                 const float* __restrict__ bg, float* __restrict__ out_color,
                                                 const PlaneArgs& pl = PlaneArgs{})
{
    const uint32_t n_tiles = (uint32_t)v.tiles_x * v.tiles_y;
    const int lane = threadIdx.x & 63;
    const int wave = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
    const uint32_t tile = blockIdx.x * kWavesPerWG + wave;
    if (tile >= n_tiles) return;
    const uint32_t overflow = counts->overflow;
    const uint32_t u0 = v.unit_offset[tile];
    const uint32_t n = v.tile_total[tile];
    const float bg0 = bg[0], bg1 = bg[1], bg2 = bg[2];
    if (overflow) return;
    gather_tile<false, FWD_ONLY, PLANES>(v, tile, u0, (n + kUnit - 1) / kUnit, g_out, unit_state, W, H, bg0, bg1, bg2, out_color, lane, pl);
}
__global__ void __launch_bounds__(256) k_tile_gather(const DeviceCounts* __restrict__ counts, const ImageView v,
                                                    const float* __restrict__ g_out, float4* __restrict__ unit_state, int W,
                                                    int H, const float* __restrict__ bg, float* __restrict__ out_color)
{
    tile_gather_body<false>(counts, v, g_out, unit_state, W, H, bg, out_color);
}
__global__ void __launch_bounds__(256) k_tile_gather_fwd_only(const DeviceCounts* __restrict__ counts, const ImageView v,
                                                             const float* __restrict__ g_out, float4* __restrict__ unit_state,
                                                             int W, int H, const float* __restrict__ bg, float* __restrict__ out_color)
{
    tile_gather_body<true>(counts, v, g_out, unit_state, W, H, bg, out_color);
}
__global__ void __launch_bounds__(256) k_tile_gather_planes(const DeviceCounts* __restrict__ counts, const ImageView v,
                                                           const float* __restrict__ g_out, float4* __restrict__ unit_state, int W,
                                                           int H, const float* __restrict__ bg, float* __restrict__ out_color,
                                                           const PlaneArgs pl)
{
    tile_gather_body<false, true>(counts, v, g_out, unit_state, W, H, bg, out_color, pl);
}
__global__ void __launch_bounds__(256) k_tile_gather_fwd_only_planes(const DeviceCounts* __restrict__ counts, const ImageView v,
                                                                    const float* __restrict__ g_out, float4* __restrict__ unit_state,
                                                                    int W, int H, const float* __restrict__ bg,
                                                                    float* __restrict__ out_color, const PlaneArgs pl)
{
    tile_gather_body<true, true>(counts, v, g_out, unit_state, W, H, bg, out_color, pl);
}

// (launch_tile_sort, which every frame goes through first, has refused a batch whose gather is a launch of its own)
int launch_blend_forward(int n, const FrameView* f, hipStream_t s, bool debug)
{
    fr_handle_impl* h0 = f[0].h;
    const bool fwd_only = (f[0].prm->flags & FR_FLAG_FORWARD_ONLY) != 0;   // (the same for every view of a batch)
    const bool planes = (f[0].prm->flags & FR_FLAG_DEPTH_ALPHA) != 0;      // (likewise)
    ChainArgs ca[kMaxBatch];
    ChainPlanesArgs cp[kMaxBatch];
    uint32_t unit_wgs = 0, gather_blocks = 0;
    for (int k = 0; k < n; k++) {
        fr_handle_impl* h = f[k].h;
        const fr_params& prm = *f[k].prm;
        const ImageView& v = f[k].v;
        const BinningView& b = f[k].b;
        const uint32_t T = (uint32_t)v.tiles_x * v.tiles_y;
        unit_wgs = max(unit_wgs, (uint32_t)((b.unit_cap + kWavesPerWG - 1) / kWavesPerWG));
        gather_blocks = max(gather_blocks, (T + kWavesPerWG - 1) / kWavesPerWG);
        ChainArgs& c = ca[k];
        c.counts = v.counts, c.unit_tile = b.unit_tile, c.masks = b.masks, c.walks = b.walks, c.bwd_units = b.bwd_units, c.stripe_cursor = b.stripe_cursor, c.heavy_pairs = h->heavy_pairs, c.unit_cap = (uint32_t)b.unit_cap;
        c.recs = RecSrc{b.ids, f[k].g.rec_tmpl};
        c.W = prm.W, c.H = prm.H, c.tiles_x = v.tiles_x, c.g_tseg = b.unit_tseg, c.g_out = b.unit_out;
        c.dense_pairs = h->dense_pairs_fwd, c.pair_hist = h->debug_pair_hist ? 1 : 0;
        c.unit_done = h->gather_in_chain ? b.unit_done : nullptr;
        c.v = v, c.unit_state = b.unit_state, c.bg = f[k].in->background, c.out_color = f[k].out_color;
        c.chain_spins = h->chain_spins;
        if (planes) cp[k] = ChainPlanesArgs{c, PlaneArgs{f[k].pv.unit_depth, f[k].pv.depth_state, f[k].out_depth, f[k].out_alpha}};
    }
    {
        StageScope sc(h0, ST_BLEND_FWD, s);
        // (one workgroup per four units, no grid-stride loop: see k_unit_blend_chained on forward progress)
        if (planes) {
            if (fwd_only) launch_views(k_unit_blend_chained_fwd_only_planes, k_unit_blend_chained_fwd_only_planes_batch, n, cp, unit_wgs, 64 * kWavesPerWG, 0, s);
            else launch_views(k_unit_blend_chained_planes, k_unit_blend_chained_planes_batch, n, cp, unit_wgs, 64 * kWavesPerWG, 0, s);
        } else if (fwd_only) launch_views(k_unit_blend_chained_fwd_only, k_unit_blend_chained_fwd_only_batch, n, ca, unit_wgs, 64 * kWavesPerWG, 0, s);
        else launch_views(k_unit_blend_chained, k_unit_blend_chained_batch, n, ca, unit_wgs, 64 * kWavesPerWG, 0, s);
        if (!h0->gather_in_chain && planes)   // (n == 1)
            hipLaunchKernelGGL(fwd_only ? k_tile_gather_fwd_only_planes : k_tile_gather_planes, dim3(gather_blocks), dim3(64 * kWavesPerWG), 0, s,
                               f[0].v.counts, f[0].v, f[0].b.unit_out, f[0].b.unit_state, f[0].prm->W, f[0].prm->H, f[0].in->background,
                               f[0].out_color, cp[0].p);
        else if (!h0->gather_in_chain)
            hipLaunchKernelGGL(fwd_only ? k_tile_gather_fwd_only : k_tile_gather, dim3(gather_blocks), dim3(64 * kWavesPerWG), 0, s, f[0].v.counts, f[0].v,
                               f[0].b.unit_out, f[0].b.unit_state, f[0].prm->W, f[0].prm->H, f[0].in->background, f[0].out_color);
    }
    FR_HIP(hipGetLastError());
    return debug_sync(debug, s, "blend_fwd");
}

}  // namespace fr
