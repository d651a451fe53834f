// Per-Gaussian backward for gfx950: one kernel that turns the blend-backward accumulators
// (dL/dmean2D, dL/dconic, dL/dopacity, dL/dcolour) into every gradient the API returns.
// reference: computeCov2DCUDA (backward.cu:144-274) + preprocessCUDA (backward.cu:346-396) +
// SH backward (backward.cu:20-139) + Sigma3D backward (backward.cu:278-341), fused.
//
// Compiled with -ffp-contract=off and written in the reference's operation order (see
// fr_preprocess.hip).  Every output row is written (zeros for culled Gaussians), so callers
// need not pre-zero anything — or, per array, ADDED to what the array holds (FR_FLAG_ACCUMULATE:
// gradient accumulation over the frames of a batch without a second buffer and an add kernel).
#include "fr_bind_math.hpp"
#include "fr_project_math.hpp"

namespace fr {

__constant__ float bSH_C0 = 0.28209479177387814f;
__constant__ float bSH_C1 = 0.4886025119029199f;
__constant__ float bSH_C2[5] = {1.0925484305920792f, -1.0925484305920792f, 0.31539156525252005f,
                                -1.0925484305920792f, 0.5462742152960396f};
__constant__ float bSH_C3[7] = {-0.5900435899266435f, 2.890611442640554f, -0.4570457994644658f, 0.3731763325901154f,
                                -0.4570457994644658f, 1.445305721320277f,  -0.5900435899266435f};

struct PreBwdArgs {
    int P, D, M, W, H, raw;
    float tan_fovx, tan_fovy, focal_x, focal_y, scale_modifier;
    const float* means3D;
    const float* scales;
    const float* rotations;
    const float* shs;
    const float* cov3D_precomp;
    const float* view;
    const float* proj;
    const float* campos;
    const int* radii;
    GeomView g;
    fr_grads out;
    float* grad_accum;  // optional (fr_aux): += ||dL_dmeans2D[:, :2]|| of visible Gaussians
    float* denom;       // optional (fr_aux): += 1 for visible Gaussians
    float* overflow_out;  // optional (fr_aux): 1.0f if the frame overflowed its binning capacity (all gradients zero), else 0.0f
    const DeviceCounts* counts;   // the frame's counts: an overflowed frame (nothing was blended) adds nothing to the statistics
    uint32_t acc;       // bit k: ADD into the k-th array of fr_grads instead of overwriting it (FR_FLAG_ACCUMULATE)
    int bound;          // fr_aux::binding: the gradients of mean / rotation / scale continue through `bind` into `bg`
    BindArgs bind;
    BindGrads bg;
};

// bit positions of `acc` = position of the pointer in fr_grads
enum { G_MEANS2D = 0, G_COLORS, G_OPACITY, G_MEANS3D, G_COV3D, G_SH, G_SCALES, G_ROTATIONS };

// one gradient element: overwritten, or added to what the array holds (wave-uniform choice per array)
__device__ __forceinline__ void put(float* p, float v, bool add) { *p = add ? *p + v : v; }

__device__ __forceinline__ void store3(float* p, size_t i, float a, float b, float c, bool add)
{
    if (!p) return;
    if (add) a += p[3 * i], b += p[3 * i + 1], c += p[3 * i + 2];
    p[3 * i] = a, p[3 * i + 1] = b, p[3 * i + 2] = c;
}

// Rows of a wave's dL_dsh block in LDS on the 16-byte path: the wave's 64 rows go through a [R][stride] block in 64 / R
// passes of R consecutive Gaussians each (64: one pass, the whole wave's rows at once).  Fewer rows per pass = less LDS per
// wave = more resident waves per CU; every pass still stores one contiguous run of R rows.
#ifndef FR_PREBWD_STAGE_ROWS
#define FR_PREBWD_STAGE_ROWS 32
#endif
constexpr int kPreBwdStageRows = FR_PREBWD_STAGE_ROWS;
// FR_PREBWD_ZERO_RUN: a wave re-zeroes its accumulator rows as ONE contiguous run of whole lines (0: every visible Gaussian
// its own row, for an A/B)
#ifndef FR_PREBWD_ZERO_RUN
#define FR_PREBWD_ZERO_RUN 1
#endif
static_assert(kPreBwdStageRows == 64 || kPreBwdStageRows == 32 || kPreBwdStageRows == 16, "FR_PREBWD_STAGE_ROWS: 64, 32 or 16");

// Row stride (floats) of a wave's block of dL_dsh rows in LDS.  M3 a multiple of 4 (M = 4, 16): the rows are
// written and read in 16-byte pieces, so the stride is a multiple of 4 — and stride / 4 is odd: a lane's ds_write_b128 goes
// to bank (stride * row + 4 k) mod 32, and over the 8 consecutive lanes that share an LDS cycle an odd stride / 4 gives 8
// different 4-bank slots (52 floats at M3 = 48: 20 * row mod 32 = 0, 20, 8, 28, 16, 4, 24, 12).  A pass's writers are R
// consecutive lanes on rows 0 .. R - 1, R a multiple of 8: the same residues in every group of 8, whatever R is.
// unstage_rows reads consecutive 16-byte pieces, one row's 12 behind the other: a 16-lane group of its ds_read_b128
// crosses at most two 4-word row gaps, so at most one slot of the 64-bank row is asked twice (5 LDS cycles instead of 4) —
// a property of 16 consecutive pieces, not of how many rows the block has; at M3 = 12 the stride IS the row length and the
// reads are contiguous.  Other row lengths (M = 1, 9) go word by word with an odd stride, all 64 rows in one block.
__host__ __device__ constexpr bool prebwd_rows_by16(int M3) { return M3 % 4 == 0 && M3 <= 48; }
__host__ __device__ constexpr int prebwd_row_stride(int M3)
{
    return prebwd_rows_by16(M3) ? (((M3 / 4) & 1) ? M3 : M3 + 4) : (M3 | 1);
}
// rows of a wave's LDS block
__host__ __device__ constexpr int prebwd_block_rows(int M3) { return prebwd_rows_by16(M3) ? kPreBwdStageRows : 64; }

// A Gaussian's dL_dsh row on the 16-byte path, kept until its pass: the row is a function of the unit view direction and
// of dRGB alone, so six floats and a flag stand in for its 48.
struct PreBwdRow {
    float x, y, z, dRGB[3];
    bool visible;   // false: the row is zeros (culled, or past the end)
};

// The LDS row in 16-byte pieces (M3 a multiple of 4): write_row's products — the direction factor of coefficient k,
// evaluated with write_row's expression, times dRGB[c] — four of them per ds_write_b128 instead of one per store.
__device__ __forceinline__ void write_row_by16(float* dsh, const PreBwdRow& r, const int deg, const int Mc)
{
    const float x = r.x, y = r.y, z = r.z;
    const int used = (deg + 1) * (deg + 1);
    float f[16] = {0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f};
    f[0] = bSH_C0;
    if (deg > 0) {
        f[1] = -bSH_C1 * y, f[2] = bSH_C1 * z, f[3] = -bSH_C1 * x;
        if (deg > 1) {
            const float xx = x * x, yy = y * y, zz = z * z;
            const float xy = x * y, yz = y * z, xz = x * z;
            f[4] = bSH_C2[0] * xy, f[5] = bSH_C2[1] * yz, f[6] = bSH_C2[2] * (2.f * zz - xx - yy);
            f[7] = bSH_C2[3] * xz, f[8] = bSH_C2[4] * (xx - yy);
            if (deg > 2) {
                f[9] = bSH_C3[0] * y * (3.f * xx - yy), f[10] = bSH_C3[1] * xy * z;
                f[11] = bSH_C3[2] * y * (4.f * zz - xx - yy), f[12] = bSH_C3[3] * z * (2.f * zz - 3.f * xx - 3.f * yy);
                f[13] = bSH_C3[4] * x * (4.f * zz - xx - yy), f[14] = bSH_C3[5] * z * (xx - yy);
                f[15] = bSH_C3[6] * x * (xx - 3.f * yy);
            }
        }
    }
    float4* d4 = reinterpret_cast<float4*>(dsh);
    const int pieces = (Mc * 3) / 4;
#pragma unroll
    for (int j = 0; j < 12; j++) {
        if (j < pieces) {   // (wave-uniform; rows longer than 48 floats do not exist: M <= 16)
            float v[4];
#pragma unroll
            for (int t = 0; t < 4; t++) {
                const int k = (4 * j + t) / 3, c = (4 * j + t) % 3;
                // (coefficients above the active degree: a literal zero, as write_row stores)
                v[t] = k < used ? f[k] * r.dRGB[c] : 0.f;
            }
            d4[j] = make_float4(v[0], v[1], v[2], v[3]);
        }
    }
}
__device__ __forceinline__ void zero_row_by16(float* dsh, const int Mc)
{
    float4* d4 = reinterpret_cast<float4*>(dsh);
    for (int k = 0; k < (Mc * 3) / 4; k++) d4[k] = make_float4(0.f, 0.f, 0.f, 0.f);
}

// Orders a wave's own LDS accesses for the compiler: the hardware executes them in program order, so a lane reads what
// another lane of its wave wrote in front of this point.  No instruction, no waiting for other waves.
__device__ __forceinline__ void wave_lds_fence()
{
    __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");
    __builtin_amdgcn_wave_barrier();
    __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "wavefront");
}

// What k_preprocess_bwd reads for ONE Gaussian, all of it requested by preprocess_bwd_fetch before anything is used or
// stored: the kernel pays one memory round trip for its inputs.  (Read where they are used, the inputs cost a wave seven
// dependent round trips: nothing here is __restrict__, so no load could move up over the stores in front of it, and on
// gfx9 an s_waitcnt vmcnt counts the stores, too.)
struct PreBwdIn {
    int radius;
    float mean[3], q[4], sc[3], c3[6];   // q / sc: with `scales`;  c3: with `cov3D_precomp`
    float opacity;
    uint32_t cl;                         // with `shs`: clamped bits, d colour / d direction
    float dd[9];
    float4 r0, r1, r2;                   // the accumulator row
    uint32_t overflow;                   // DeviceCounts::overflow of the frame (wave-uniform)
    float ga, dn;                        // grad_accum / denom, where the call has them
    float old_m3[3], old_sc[3], old_q[4], old_op;   // accumulating arrays: what they hold
};

// (a pointer that went through an asm operand has lost its address space: named again, or every load through it is a FLAT one)
template <class T> using GlobalPtr = const __attribute__((address_space(1))) T*;
template <class T> __device__ __forceinline__ GlobalPtr<T> as_global(const T* p) { return (GlobalPtr<T>)p; }
typedef float PreBwdF4 __attribute__((ext_vector_type(4)));

// `li`: the Gaussian's index, clamped to P - 1 for the lanes past the end (they load like everyone and store nothing).
// Optional inputs are wave-uniform null tests.  The row of a culled Gaussian is loaded like any other: its dcolor_ddir and
// opacity_act may be scratch the forward never wrote — preprocess_bwd_one uses none of it on that path.
__device__ __forceinline__ void preprocess_bwd_fetch(const PreBwdArgs& a, const int li, PreBwdIn& in)
{
    const size_t i = (size_t)li;
    const auto adds = [&](int k) { return ((a.acc >> k) & 1u) != 0u; };
    // the pointers first, all of them before the first request: read where they are used, each was a scalar load of the
    // kernel-argument block with a wait of its own between two requests
    const int* radii_ = a.radii;
    const DeviceCounts* counts_ = a.counts;
    const float *accum_ = a.g.accum, *means3D_ = a.means3D, *scales_ = a.scales, *rotations_ = a.rotations, *cov3D_ = a.cov3D_precomp;
    const float *opacity_act_ = a.g.opacity_act, *dcolor_ddir_ = a.g.dcolor_ddir, *shs = a.shs;
    const uint8_t* clamped_ = a.g.clamped;
    const float *grad_accum_ = a.grad_accum, *denom_ = a.denom;
    asm volatile("" : "+s"(radii_), "+s"(counts_), "+s"(accum_), "+s"(means3D_), "+s"(scales_), "+s"(rotations_), "+s"(cov3D_),
                 "+s"(opacity_act_), "+s"(dcolor_ddir_), "+s"(shs), "+s"(clamped_), "+s"(grad_accum_), "+s"(denom_));
    const auto radii = as_global(radii_);
    const auto counts = as_global(counts_);
    const auto accum = as_global(accum_), means3D = as_global(means3D_), scales = as_global(scales_), rotations = as_global(rotations_);
    const auto cov3D = as_global(cov3D_), opacity_act = as_global(opacity_act_), dcolor_ddir = as_global(dcolor_ddir_);
    const auto clamped = as_global(clamped_);
    const auto grad_accum = as_global(grad_accum_), denom = as_global(denom_);
    in.radius = radii[li];
    in.overflow = counts->overflow;
    const GlobalPtr<PreBwdF4> row4 = (GlobalPtr<PreBwdF4>)(accum + i * kAccumStride);
    const PreBwdF4 r0 = row4[0], r1 = row4[1], r2 = row4[2];
    in.r0 = make_float4(r0.x, r0.y, r0.z, r0.w), in.r1 = make_float4(r1.x, r1.y, r1.z, r1.w), in.r2 = make_float4(r2.x, r2.y, r2.z, r2.w);
    for (int k = 0; k < 3; k++) in.mean[k] = means3D[3 * i + k];
    for (int k = 0; k < 4; k++) in.q[k] = 0.f;
    for (int k = 0; k < 3; k++) in.sc[k] = 0.f;
    for (int k = 0; k < 6; k++) in.c3[k] = 0.f;
    if (scales) {
        for (int k = 0; k < 4; k++) in.q[k] = rotations[4 * i + k];
        for (int k = 0; k < 3; k++) in.sc[k] = scales[3 * i + k];
    }
    if (cov3D)
        for (int k = 0; k < 6; k++) in.c3[k] = cov3D[6 * i + k];
    in.opacity = opacity_act[li];
    in.cl = 0u;
    for (int k = 0; k < 9; k++) in.dd[k] = 0.f;
    if (shs) {
        in.cl = clamped[li];
        for (int k = 0; k < 9; k++) in.dd[k] = dcolor_ddir[ddir_index(k, i, (size_t)a.P)];   // (planar [9][P]: a wave's load is one run)
    }
    in.ga = in.dn = 0.f;
    if (grad_accum) in.ga = grad_accum[i];
    if (denom) in.dn = denom[i];
    for (int k = 0; k < 3; k++) in.old_m3[k] = 0.f, in.old_sc[k] = 0.f;
    for (int k = 0; k < 4; k++) in.old_q[k] = 0.f;
    in.old_op = 0.f;
    if (a.acc) {
        if (adds(G_MEANS3D) && a.out.dL_dmeans3D)
            for (int k = 0; k < 3; k++) in.old_m3[k] = a.out.dL_dmeans3D[3 * i + k];
        if (adds(G_SCALES) && a.out.dL_dscales)
            for (int k = 0; k < 3; k++) in.old_sc[k] = a.out.dL_dscales[3 * i + k];
        if (adds(G_ROTATIONS) && a.out.dL_drotations)
            for (int k = 0; k < 4; k++) in.old_q[k] = a.out.dL_drotations[4 * i + k];
        if (adds(G_OPACITY) && a.out.dL_dopacity) in.old_op = a.out.dL_dopacity[i];
    }
}

// Everything for ONE Gaussian, from what preprocess_bwd_fetch brought: arithmetic and stores, no input load.  The kernel
// writes the dL_dsh rows of a wave through LDS for coalesced HBM access: `row` (LDS, may be null) receives this Gaussian's
// row word by word; or, with `defer` (the 16-byte path), `deferred` receives what the row is made from and the caller writes it
// in the Gaussian's pass (`deferred.visible` stays false for a culled Gaussian).  PLANES (a backward with a depth gradient, FR_FLAG_DEPTH_ALPHA): the
// accumulated dL/dz of the view-space depth (ACC_Z) joins dL/dmean3D through z = view[2] x + view[6] y + view[10] z + view[14].
template <bool PLANES>
__device__ __forceinline__ void preprocess_bwd_one(const PreBwdArgs& a, const CameraRegs& cam, const PreBwdIn& in,
                                                   const int idx, float* row, const bool defer, PreBwdRow& deferred)
{
    const size_t i = (size_t)idx;
    const int Mc = a.M;
    const int radius = in.radius;
    const auto adds = [&](int k) { return ((a.acc >> k) & 1u) != 0u; };
    if (!(radius > 0)) {   // no gradient: zeros where the arrays are overwritten, nothing where they accumulate
        if (row)
            for (int k = 0; k < Mc * 3; k++) row[k] = 0.f;
        if (!adds(G_MEANS2D)) store3(a.out.dL_dmeans2D, i, 0.f, 0.f, 0.f, false);
        if (!adds(G_COLORS)) store3(a.out.dL_dcolors, i, 0.f, 0.f, 0.f, false);
        if (a.out.dL_dopacity && !adds(G_OPACITY)) a.out.dL_dopacity[i] = 0.f;
        if (!adds(G_MEANS3D)) store3(a.out.dL_dmeans3D, i, 0.f, 0.f, 0.f, false);
        if (a.out.dL_dcov3D && !adds(G_COV3D))
            for (int k = 0; k < 6; k++) a.out.dL_dcov3D[6 * i + k] = 0.f;
        if (a.out.dL_dsh && !row && !defer && !adds(G_SH))
            for (int k = 0; k < Mc * 3; k++) a.out.dL_dsh[i * Mc * 3 + k] = 0.f;
        if (!adds(G_SCALES)) store3(a.out.dL_dscales, i, 0.f, 0.f, 0.f, false);
        if (a.out.dL_drotations && !adds(G_ROTATIONS))
            for (int k = 0; k < 4; k++) a.out.dL_drotations[4 * i + k] = 0.f;
        if (a.bound) bind_bwd_zero(a.bind, idx, a.bg);
        return;
    }
    // (accumulating arrays: what they hold came with the other inputs — a load next to its store would sit behind the
    // stores in front of it)
    const float old_m3[3] = {in.old_m3[0], in.old_m3[1], in.old_m3[2]}, old_sc[3] = {in.old_sc[0], in.old_sc[1], in.old_sc[2]};
    const float old_q[4] = {in.old_q[0], in.old_q[1], in.old_q[2], in.old_q[3]}, old_op = in.old_op;
    // the accumulator row (the caller has left the wave's rows zeroed for the next backward)
    float acc[12];
    {
        const float4 r0 = in.r0, r1 = in.r1, r2 = in.r2;
        if (!FR_PREBWD_ZERO_RUN) {   // (every visible Gaussian the used part of its own row)
            float4* row4 = reinterpret_cast<float4*>(a.g.accum + i * kAccumStride);
            row4[0] = row4[1] = row4[2] = make_float4(0.f, 0.f, 0.f, 0.f);
        }
        acc[0] = r0.x, acc[1] = r0.y, acc[2] = r0.z, acc[3] = r0.w, acc[4] = r1.x, acc[5] = r1.y, acc[6] = r1.z,
        acc[7] = r1.w, acc[8] = r2.x, acc[9] = r2.y, acc[10] = r2.z, acc[11] = r2.w;
    }
    const float3 mean = make_float3(in.mean[0], in.mean[1], in.mean[2]);
    const float* vm = cam.view;
    // Sigma3D: the caller's, or computed again from the scales and rotations — by the function the forward calls
    // (fr_project_math.hpp): the same bits
    const Sigma3D sig = sigma3d_from_inputs(a.scales != nullptr, a.raw != 0, in.sc, in.q, a.scale_modifier, a.cov3D_precomp != nullptr, in.c3);

    // ---------------- conic -> Sigma2D -> Sigma3D and mean (backward.cu:144-274)
    const Ewa e = ewa_project(xform4x3(mean, vm), vm, sig.c3, a.tan_fovx, a.tan_fovy, a.focal_x, a.focal_y);
    // moments of q = dL/dG * G accumulated by the blend backward -> the reference's per-Gaussian sums
    // (backward.cu:538-554): dG/ddelx = -G*(dx*A + dy*B), dG/ddely = -G*(dy*C + dx*B)
    // Neither the conic nor the 2D covariance is read back: ewa_project is what the forward called (forward.cu:74-113,
    // 207-219) — the same bits; only the activated opacity comes from the state.
    const float opacity = in.opacity;
    // (ACC_MX / ACC_MY arrive combined with the conic per pixel: sum of q * dG/d(centre) / G, fr_common.hpp)
    const float g2x = acc[ACC_MX] * (0.5f * a.W);
    const float g2y = acc[ACC_MY] * (0.5f * a.H);
    const float dcx = -0.5f * acc[ACC_CA], dcy = -0.5f * acc[ACC_CB], dcz = -0.5f * acc[ACC_CC];
    const float dop = (opacity != 0.f) ? acc[ACC_OP] / opacity : 0.f;
    float dcol[3] = {acc[ACC_R], acc[ACC_G], acc[ACC_B]};
    store3(a.out.dL_dmeans2D, i, g2x, g2y, 0.f, adds(G_MEANS2D));
    // fused _add_densification_stats (model/fateavatar.py:734-737); this branch is radii > 0
    // (a replayed frame that overflowed its captured binning capacity back-propagates zeros: it must not count as a view)
    if (!in.overflow) {
        if (a.grad_accum) a.grad_accum[i] = in.ga + sqrtf(g2x * g2x + g2y * g2y);
        if (a.denom) a.denom[i] = in.dn + 1.0f;
    }
    store3(a.out.dL_dcolors, i, dcol[0], dcol[1], dcol[2], adds(G_COLORS));
    // raw-parameter mode: d sigmoid = o (1 - o); `opacity` is the activated opacity the forward stored
    if (a.out.dL_dopacity) a.out.dL_dopacity[i] = old_op + (a.raw ? dop * opacity * (1.0f - opacity) : dop);

    const CovGrad cg = conic_bwd(e, dcx, dcy, dcz);
    const float dL_da = cg.dL_da, dL_db = cg.dL_db, dL_dc = cg.dL_dc;
    const float(&T0)[3] = e.T0, (&T1)[3] = e.T1;
    float dcov[6] = {0, 0, 0, 0, 0, 0};
    if (cg.live) {   // (conic_bwd's guard: not from zeros)
        dcov[0] = (T0[0] * T0[0] * dL_da + T0[0] * T1[0] * dL_db + T1[0] * T1[0] * dL_dc);
        dcov[3] = (T0[1] * T0[1] * dL_da + T0[1] * T1[1] * dL_db + T1[1] * T1[1] * dL_dc);
        dcov[5] = (T0[2] * T0[2] * dL_da + T0[2] * T1[2] * dL_db + T1[2] * T1[2] * dL_dc);
        dcov[1] = 2 * T0[0] * T0[1] * dL_da + (T0[0] * T1[1] + T0[1] * T1[0]) * dL_db + 2 * T1[0] * T1[1] * dL_dc;
        dcov[2] = 2 * T0[0] * T0[2] * dL_da + (T0[0] * T1[2] + T0[2] * T1[0]) * dL_db + 2 * T1[0] * T1[2] * dL_dc;
        dcov[4] = 2 * T0[2] * T0[1] * dL_da + (T0[1] * T1[2] + T0[2] * T1[1]) * dL_db + 2 * T1[1] * T1[2] * dL_dc;
    }
    if (a.out.dL_dcov3D)
        for (int k = 0; k < 6; k++) put(a.out.dL_dcov3D + 6 * i + k, dcov[k], adds(G_COV3D));

    // dL/dT -> dL/dJ -> dL/dt (backward.cu:237-270)
    const EwaGrad eg = ewa_bwd(e, vm, sig.c3, cg, a.focal_x, a.focal_y);
    const float dL_dtx = eg.dL_dtx, dL_dty = eg.dL_dty, dL_dtz = eg.dL_dtz;
    float dmx = vm[0] * dL_dtx + vm[1] * dL_dty + vm[2] * dL_dtz;
    float dmy = vm[4] * dL_dtx + vm[5] * dL_dty + vm[6] * dL_dtz;
    float dmz = vm[8] * dL_dtx + vm[9] * dL_dty + vm[10] * dL_dtz;

    // ---------------- projection part of dL/dmean3D (backward.cu:370-387)
    {
        const float* proj = cam.proj;
        float m_w;
        project_mean(mean, proj, m_w);
        const float mul1 = (proj[0] * mean.x + proj[4] * mean.y + proj[8] * mean.z + proj[12]) * m_w * m_w;
        const float mul2 = (proj[1] * mean.x + proj[5] * mean.y + proj[9] * mean.z + proj[13]) * m_w * m_w;
        const float px = (proj[0] * m_w - proj[3] * mul1) * g2x + (proj[1] * m_w - proj[3] * mul2) * g2y;
        const float py = (proj[4] * m_w - proj[7] * mul1) * g2x + (proj[5] * m_w - proj[7] * mul2) * g2y;
        const float pz = (proj[8] * m_w - proj[11] * mul1) * g2x + (proj[9] * m_w - proj[11] * mul2) * g2y;
        dmx += px, dmy += py, dmz += pz;
    }

    // ---------------- SH backward (backward.cu:20-139)
    if (a.shs) {
        // (the derivative of the colour with respect to the direction comes from the forward, GeomView::dcolor_ddir: this
        // kernel does not read the SH coefficients at all; `row`, if staged, only collects the dL_dsh row)
        const ShDirGrad sd = sh_dir_bwd(mean, cam.campos, in.cl, dcol, in.dd);
        const float dox = sd.dox, doy = sd.doy, doz = sd.doz;
        const float len = sqrtf(dox * dox + doy * doy + doz * doz);
        const float x = dox / len, y = doy / len, z = doz / len;
        const float(&dRGB)[3] = sd.dRGB;
        const int deg = a.D;
        const int used = (deg + 1) * (deg + 1);
        // the dL_dsh row: into the wave's LDS block (coalesced to HBM afterwards) or straight into the array.  One body,
        // called once per destination: a pointer that may be either made every access a FLAT one.
        auto write_row = [&](float* dsh, const bool dsh_adds) {
#define DSH(k, c, v_) put(dsh + (k) * 3 + (c), (v_), dsh_adds)
            for (int c = 0; c < 3; c++) {
                DSH(0, c, bSH_C0 * dRGB[c]);
                if (deg > 0) {
                    DSH(1, c, (-bSH_C1 * y) * dRGB[c]);
                    DSH(2, c, (bSH_C1 * z) * dRGB[c]);
                    DSH(3, c, (-bSH_C1 * x) * dRGB[c]);
                    if (deg > 1) {
                        const float xx = x * x, yy = y * y, zz = z * z;
                        const float xy = x * y, yz = y * z, xz = x * z;
                        DSH(4, c, (bSH_C2[0] * xy) * dRGB[c]);
                        DSH(5, c, (bSH_C2[1] * yz) * dRGB[c]);
                        DSH(6, c, (bSH_C2[2] * (2.f * zz - xx - yy)) * dRGB[c]);
                        DSH(7, c, (bSH_C2[3] * xz) * dRGB[c]);
                        DSH(8, c, (bSH_C2[4] * (xx - yy)) * dRGB[c]);
                        if (deg > 2) {
                            DSH(9, c, (bSH_C3[0] * y * (3.f * xx - yy)) * dRGB[c]);
                            DSH(10, c, (bSH_C3[1] * xy * z) * dRGB[c]);
                            DSH(11, c, (bSH_C3[2] * y * (4.f * zz - xx - yy)) * dRGB[c]);
                            DSH(12, c, (bSH_C3[3] * z * (2.f * zz - 3.f * xx - 3.f * yy)) * dRGB[c]);
                            DSH(13, c, (bSH_C3[4] * x * (4.f * zz - xx - yy)) * dRGB[c]);
                            DSH(14, c, (bSH_C3[5] * z * (xx - yy)) * dRGB[c]);
                            DSH(15, c, (bSH_C3[6] * x * (xx - 3.f * yy)) * dRGB[c]);
                        }
                    }
                }
            }
            // coefficients above the active degree receive no gradient (the reference leaves its
            // zero-initialised rows untouched)
            if (!dsh_adds)
                for (int k = used; k < Mc; k++) dsh[k * 3] = 0.f, dsh[k * 3 + 1] = 0.f, dsh[k * 3 + 2] = 0.f;
#undef DSH
        };
        if (defer) {                                                       // (written in its pass, by the caller)
            deferred.x = x, deferred.y = y, deferred.z = z;
            deferred.dRGB[0] = dRGB[0], deferred.dRGB[1] = dRGB[1], deferred.dRGB[2] = dRGB[2];
            deferred.visible = true;
        } else if (row) write_row(row, false);                             // (added to the array by unstage_rows)
        else if (a.out.dL_dsh) write_row(a.out.dL_dsh + i * Mc * 3, adds(G_SH));
        dmx += sd.d[0], dmy += sd.d[1], dmz += sd.d[2];
    } else if (a.out.dL_dsh && !row && !defer && !adds(G_SH)) {
        for (int k = 0; k < Mc * 3; k++) a.out.dL_dsh[i * Mc * 3 + k] = 0.f;
    }
    if (PLANES) {
        const float dz = acc[ACC_Z];
        dmx += dz * vm[2], dmy += dz * vm[6], dmz += dz * vm[10];
    }
    store3(a.out.dL_dmeans3D, i, old_m3[0] + dmx, old_m3[1] + dmy, old_m3[2] + dmz, false);
    const float g_mean[3] = {dmx, dmy, dmz};   // (this frame's, for the binding)
    float g_scl[3] = {0.f, 0.f, 0.f}, g_rot[4] = {0.f, 0.f, 0.f, 0.f};

    // ---------------- Sigma3D -> scale, quaternion (backward.cu:278-341)
    if (a.scales) {
        const float r = sig.q[0], x = sig.q[1], y = sig.q[2], z = sig.q[3];   // (activated above, for Sigma3D)
        const float(&sc)[3] = sig.sc;
        const float rot_inv = sig.rot_inv;
        const float s[3] = {a.scale_modifier * sc[0], a.scale_modifier * sc[1], a.scale_modifier * sc[2]};
        // Rc[c][w]: the reference's column-major R (its column c is row c of the usual rotation matrix)
        const float Rc[3][3] = {{1.f - 2.f * (y * y + z * z), 2.f * (x * y - r * z), 2.f * (x * z + r * y)},
                                {2.f * (x * y + r * z), 1.f - 2.f * (x * x + z * z), 2.f * (y * z - r * x)},
                                {2.f * (x * z - r * y), 2.f * (y * z + r * x), 1.f - 2.f * (x * x + y * y)}};
        // M = S * R : M[c][w] = s_w * Rc[c][w];  dL_dSigma symmetric with halved off-diagonals
        const float dS[3][3] = {{dcov[0], 0.5f * dcov[1], 0.5f * dcov[2]},
                                {0.5f * dcov[1], dcov[3], 0.5f * dcov[4]},
                                {0.5f * dcov[2], 0.5f * dcov[4], dcov[5]}};
        // dL_dM = (2M) * dL_dSigma : dM[c][w] = sum_k (2 M[k][w]) * dS[c][k]
        float dM[3][3];
        for (int c = 0; c < 3; c++)
            for (int w = 0; w < 3; w++)
                dM[c][w] = (s[w] * Rc[0][w] * 2.0f) * dS[c][0] + (s[w] * Rc[1][w] * 2.0f) * dS[c][1] + (s[w] * Rc[2][w] * 2.0f) * dS[c][2];
        // Rt[c][w] = Rc[w][c], dMt[c][w] = dM[w][c];  dL_dscale_c = dot(Rt[c], dMt[c])
        float dMt[3][3];
        for (int c = 0; c < 3; c++)
            for (int w = 0; w < 3; w++) dMt[c][w] = dM[w][c];
        const float dsx = Rc[0][0] * dMt[0][0] + Rc[1][0] * dMt[0][1] + Rc[2][0] * dMt[0][2];
        const float dsy = Rc[0][1] * dMt[1][0] + Rc[1][1] * dMt[1][1] + Rc[2][1] * dMt[1][2];
        const float dsz = Rc[0][2] * dMt[2][0] + Rc[1][2] * dMt[2][1] + Rc[2][2] * dMt[2][2];
        // raw-parameter mode: d exp = the activated scale
        g_scl[0] = a.raw ? dsx * sc[0] : dsx, g_scl[1] = a.raw ? dsy * sc[1] : dsy, g_scl[2] = a.raw ? dsz * sc[2] : dsz;
        store3(a.out.dL_dscales, i, old_sc[0] + g_scl[0], old_sc[1] + g_scl[1], old_sc[2] + g_scl[2], false);
        for (int w = 0; w < 3; w++) dMt[0][w] *= s[0], dMt[1][w] *= s[1], dMt[2][w] *= s[2];
#define Dm(c_, r_) dMt[c_][r_]
        if (a.out.dL_drotations || a.bound) {
            float dq[4];
            dq[0] = 2 * z * (Dm(0, 1) - Dm(1, 0)) + 2 * y * (Dm(2, 0) - Dm(0, 2)) + 2 * x * (Dm(1, 2) - Dm(2, 1));
            dq[1] = 2 * y * (Dm(1, 0) + Dm(0, 1)) + 2 * z * (Dm(2, 0) + Dm(0, 2)) + 2 * r * (Dm(1, 2) - Dm(2, 1)) - 4 * x * (Dm(2, 2) + Dm(1, 1));
            dq[2] = 2 * x * (Dm(1, 0) + Dm(0, 1)) + 2 * r * (Dm(2, 0) - Dm(0, 2)) + 2 * z * (Dm(1, 2) + Dm(2, 1)) - 4 * y * (Dm(2, 2) + Dm(0, 0));
            dq[3] = 2 * r * (Dm(0, 1) - Dm(1, 0)) + 2 * x * (Dm(2, 0) + Dm(0, 2)) + 2 * y * (Dm(1, 2) + Dm(2, 1)) - 4 * z * (Dm(1, 1) + Dm(0, 0));
            if (a.raw) {
                // through q_hat = q / |q|:  dL/dq = (g - q_hat (q_hat . g)) / |q|
                const float dot = r * dq[0] + x * dq[1] + y * dq[2] + z * dq[3];
                dq[0] = (dq[0] - r * dot) * rot_inv;
                dq[1] = (dq[1] - x * dot) * rot_inv;
                dq[2] = (dq[2] - y * dot) * rot_inv;
                dq[3] = (dq[3] - z * dot) * rot_inv;
            }
            if (a.out.dL_drotations)
                for (int k = 0; k < 4; k++) a.out.dL_drotations[4 * i + k] = old_q[k] + dq[k];
            for (int k = 0; k < 4; k++) g_rot[k] = dq[k];
        }
#undef Dm
    } else {
        if (!adds(G_SCALES)) store3(a.out.dL_dscales, i, 0.f, 0.f, 0.f, false);
        if (a.out.dL_drotations && !adds(G_ROTATIONS))
            for (int k = 0; k < 4; k++) a.out.dL_drotations[4 * i + k] = 0.f;
    }
    // ---------------- through the mesh binding (model/fateavatar.py:225-258): fr_bind_backward's expressions
    if (a.bound) bind_bwd(a.bind, idx, g_mean, g_rot, g_scl, a.bg);
}

// A wave's [rows][row_len] block of dL_dsh rows goes from LDS to HBM in coalesced 16-byte stores (the inverse of the
// forward's staging, fr_preprocess.hip).
template <bool ADD>
__device__ __forceinline__ void unstage_rows_t(float* __restrict__ dst, const float* src, int stride, int rows, int row_len, int lane)
{
    const int total = rows * row_len;
    const unsigned magic = (unsigned)((0x100000000ull + (unsigned)row_len - 1u) / (unsigned)row_len);
    // ADD: the array's old values are requested kBatch 16-byte loads at a time before the first one is used
    constexpr int kBatch = ADD ? 6 : 1;
    for (int base = lane * 4; base < total; base += 64 * 4 * kBatch) {
        float4 o[kBatch];
        if (ADD) {
#pragma unroll
            for (int u = 0; u < kBatch; u++) {
                const int c = base + u * 64 * 4;
                o[u] = make_float4(0.f, 0.f, 0.f, 0.f);
                if (c + 3 < total) {
                    o[u] = *reinterpret_cast<const float4*>(dst + c);
                } else {
                    if (c < total) o[u].x = dst[c];
                    if (c + 1 < total) o[u].y = dst[c + 1];
                    if (c + 2 < total) o[u].z = dst[c + 2];
                }
            }
        }
#pragma unroll
        for (int u = 0; u < kBatch; u++) {
            const int c = base + u * 64 * 4;
            if (c >= total) break;
            float v[4];
#pragma unroll
            for (int k = 0; k < 4; k++) {
                const int e = c + k;
                const int r = (int)__umulhi((unsigned)e, magic);  // e / row_len (exact: e < 2^16)
                v[k] = (e < total) ? src[r * stride + (e - r * row_len)] : 0.f;
            }
            if (ADD) v[0] += o[u].x, v[1] += o[u].y, v[2] += o[u].z, v[3] += o[u].w;
            if (c + 3 < total) *reinterpret_cast<float4*>(dst + c) = make_float4(v[0], v[1], v[2], v[3]);
            else
                for (int k = 0; k < 4; k++)
                    if (c + k < total) dst[c + k] = v[k];
        }
    }
}
// The same for rows of whole 16-byte pieces (row_len and stride multiples of 4): a piece never crosses a row, so every
// 16-byte store is ONE ds_read_b128 behind ONE division (instead of four word reads, four divisions and four selects).
template <bool ADD>
__device__ __forceinline__ void unstage_rows_by16_t(float* __restrict__ dst, const float* src, int stride, int rows, int row_len, int lane)
{
    const int total = rows * row_len;   // (a multiple of 4)
    const unsigned magic = (unsigned)((0x100000000ull + (unsigned)row_len - 1u) / (unsigned)row_len);
    constexpr int kBatch = ADD ? 6 : 1;
    for (int base = lane * 4; base < total; base += 64 * 4 * kBatch) {
        float4 o[kBatch];
        if (ADD) {
#pragma unroll
            for (int u = 0; u < kBatch; u++) {
                const int c = base + u * 64 * 4;
                o[u] = make_float4(0.f, 0.f, 0.f, 0.f);
                if (c < total) o[u] = *reinterpret_cast<const float4*>(dst + c);
            }
        }
#pragma unroll
        for (int u = 0; u < kBatch; u++) {
            const int c = base + u * 64 * 4;
            if (c >= total) break;
            const int r = (int)__umulhi((unsigned)c, magic);  // c / row_len (exact: c < 2^16)
            float4 v = *reinterpret_cast<const float4*>(src + r * stride + (c - r * row_len));
            if (ADD) v.x += o[u].x, v.y += o[u].y, v.z += o[u].z, v.w += o[u].w;
            *reinterpret_cast<float4*>(dst + c) = v;
        }
    }
}

#ifndef FR_PREBWD_WAVES
#define FR_PREBWD_WAVES 4
#endif
constexpr int kPreBwdWaves = FR_PREBWD_WAVES;  // waves per workgroup of k_preprocess_bwd

template <bool PLANES>
__device__ __forceinline__ void preprocess_bwd_body(const PreBwdArgs& a)
{
    extern __shared__ __attribute__((aligned(16))) float s_rows[];
    if ((int)(blockIdx.x * blockDim.x) >= a.P) return;   // (a batched launch's grid is the largest view's)
    const int idx = blockIdx.x * blockDim.x + threadIdx.x;
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const int M3 = a.M * 3, stride = prebwd_row_stride(M3);
    const int wave_first = blockIdx.x * (64 * kPreBwdWaves) + wave * 64;
    const int rows = min(64, a.P - wave_first);
    const bool staged = a.shs != nullptr && a.out.dL_dsh != nullptr;
    const bool by16 = prebwd_rows_by16(M3);
    float* w_rows = s_rows + (size_t)wave * prebwd_block_rows(M3) * stride;   // this wave's block: no other wave touches it
    // Every input of the thread, then the camera, are requested before anything is used or stored: one round trip for all
    // of them.  The camera goes LAST: loads come back in order, so the wait in front of its broadcast — the first use of
    // anything — is the kernel's one wait for its inputs.  (The compiler's barrier: without it the loads that only the
    // visible Gaussians use sink into their branch, behind the wait for the radius.)
    PreBwdIn in;
    preprocess_bwd_fetch(a, min(idx, a.P - 1), in);
    const float cam_x = camera_request(a.view, a.proj, a.campos, lane);
    asm volatile("" ::: "memory");
    const CameraRegs cam = camera_broadcast(cam_x);
    // (... and the first arithmetic on a loaded value — ~clamped, denom + 1 — is hoisted to its load otherwise, with a wait
    // of its own in the middle of the requests)
    asm volatile("" : "+v"(in.cl), "+v"(in.ga), "+v"(in.dn), "+v"(in.opacity), "+v"(in.radius));
    // The wave's accumulator rows, left zeroed for the next backward (the rows are zero between backward passes: no zeroing
    // launch, and no zeroing writes in the forward): ONE contiguous run of `rows` 64-byte rows, four coalesced 16-byte stores
    // per lane, whole lines.  (Each visible Gaussian zeroing the 48 used bytes of its own row asked for 3 x 64 part lines per
    // wave.)  The rows of culled Gaussians and the tail of every row are zero already: writing zeros there changes nothing.
    // These are the kernel's first stores, behind its one wait: the zero they store is made to depend on the camera's
    // broadcast, whose wait covers every load in front of it — the rows are in registers by now.  The wave is converged.
    if (FR_PREBWD_ZERO_RUN) {
        float zero = 0.f;
        asm volatile("" : "+v"(zero) : "s"(cam.campos[2]) : "memory");
        float4* z4 = reinterpret_cast<float4*>(a.g.accum + (size_t)max(wave_first, 0) * kAccumStride);
        const int pieces = rows * (kAccumStride / 4);   // (<= 0 for a wave past the end)
#pragma unroll
        for (int t = 0; t < kAccumStride / 4; t++)
            if (lane + 64 * t < pieces) z4[lane + 64 * t] = make_float4(zero, zero, zero, zero);
    }
    // (fr_aux::overflow_out: the step's optimizer kernel reads it — fr_adam_config::skip)
    if (a.overflow_out && blockIdx.x == 0 && threadIdx.x == 0) *a.overflow_out = in.overflow ? 1.0f : 0.0f;
    PreBwdRow mine;
    mine.x = mine.y = mine.z = mine.dRGB[0] = mine.dRGB[1] = mine.dRGB[2] = 0.f, mine.visible = false;
    if (idx < a.P)
        preprocess_bwd_one<PLANES>(a, cam, in, idx, staged && !by16 ? w_rows + lane * stride : nullptr, staged && by16, mine);
    // The whole wave is here, converged (nothing returns inside preprocess_bwd_one's caller), and the waves of a workgroup
    // go their own ways: each unstages only its own block, so there is nothing to wait for another wave for.
    if (!staged || rows <= 0) return;
    float* dst = a.out.dL_dsh + (size_t)wave_first * M3;
    const bool add = ((a.acc >> G_SH) & 1u) != 0u;
    if (!by16) {
        wave_lds_fence();
        if (add) unstage_rows_t<true>(dst, w_rows, stride, rows, M3, lane);
        else unstage_rows_t<false>(dst, w_rows, stride, rows, M3, lane);
        return;
    }
    // pass p: the Gaussians [p R, p R + R) of the wave write their rows (culled: zeros), the wave stores them.  (Unrolled:
    // as a loop the passes cost the single-view kernels 9 more VGPRs, 103 instead of 94, and a wave per SIMD with them.)
    constexpr int R = kPreBwdStageRows;
#pragma unroll
    for (int first = 0; first < 64; first += R) {
        if (first >= rows) break;   // (wave-uniform)
        if (lane >= first && lane < first + R) {
            float* row = w_rows + (lane - first) * stride;
            if (mine.visible) write_row_by16(row, mine, a.D, a.M);
            else zero_row_by16(row, a.M);
        }
        wave_lds_fence();
        const int n = min(R, rows - first);
        if (add) unstage_rows_by16_t<true>(dst + (size_t)first * M3, w_rows, stride, n, M3, lane);
        else unstage_rows_by16_t<false>(dst + (size_t)first * M3, w_rows, stride, n, M3, lane);
        wave_lds_fence();   // (the next pass overwrites what this one read)
    }
}

__global__ void __launch_bounds__(64 * kPreBwdWaves) k_preprocess_bwd(PreBwdArgs a) { preprocess_bwd_body<false>(a); }
__global__ void __launch_bounds__(64 * kPreBwdWaves) k_preprocess_bwd_batch(BatchOf<PreBwdArgs> b) { preprocess_bwd_body<false>(b.v[blockIdx.y]); }
// backward passes handed a depth or alpha gradient (FR_FLAG_DEPTH_ALPHA): + dL/dz
__global__ void __launch_bounds__(64 * kPreBwdWaves) k_preprocess_bwd_planes(PreBwdArgs a) { preprocess_bwd_body<true>(a); }
__global__ void __launch_bounds__(64 * kPreBwdWaves) k_preprocess_bwd_planes_batch(BatchOf<PreBwdArgs> b) { preprocess_bwd_body<true>(b.v[blockIdx.y]); }

int launch_backward(int n, const BackwardCall* calls, hipStream_t s)
{
    GeomView g[kMaxBatch];
    ImageView v[kMaxBatch];
    PreBwdArgs args[kMaxBatch];
    bool capturing = false, debug = false, planes = false;
    for (int k = 0; k < n; k++) capturing = note_capture(calls[k].h, s) || capturing;
    // a depth or alpha gradient in any view (FR_FLAG_DEPTH_ALPHA, checked by fr_backward): the planes instances for all of them
    for (int k = 0; k < n; k++) {
        const fr_aux* aux = calls[k].prm->aux;
        planes = planes || ((calls[k].prm->flags & FR_FLAG_DEPTH_ALPHA) && aux && (aux->dL_ddepth || aux->dL_dalpha));
    }
    size_t lds = 0;
    uint32_t blocks = 0;
    const int wg = 64 * kPreBwdWaves;
    for (int k = 0; k < n; k++) {
        fr_handle_impl* h = calls[k].h;
        const fr_params& prm = *calls[k].prm;
        const fr_inputs& in = *calls[k].in;
        const int P = prm.P;
        g[k] = GeomView::make(calls[k].geometry, (size_t)P);
        // backward passes of one handle share its gradient accumulators (the blend backward adds rows, k_preprocess_bwd
        // reads and re-zeroes them): order this one behind the previous one if that ran on another stream.  (Not inside a
        // capture: a capture is ordered by its own stream, replays by whoever launches them — as for the forward.)
        if (!capturing && h->have_last_bwd && h->last_bwd_stream != s) FR_HIP(hipStreamWaitEvent(s, h->bwd_done, 0));
        {   // gradient accumulators: handle-owned, zero between backward passes (normally sized by the forward already)
            int rc0 = ensure_accum(h, (size_t)P, s);
            if (rc0) return rc0;
            g[k].accum = h->accum;
        }
        v[k] = ImageView::make(const_cast<void*>(calls[k].image), prm.W, prm.H);
        debug = debug || prm.debug != 0;
        PreBwdArgs& a = args[k];
        fill_projection_args(a, prm, in);
        a.D = prm.D, a.M = prm.M, a.shs = in.shs;
        a.radii = calls[k].radii, a.g = g[k], a.out = *calls[k].grads;
        a.grad_accum = prm.aux ? prm.aux->grad_accum : nullptr;
        a.denom = prm.aux ? prm.aux->denom : nullptr;
        a.overflow_out = prm.aux ? prm.aux->overflow_out : nullptr;
        a.counts = v[k].counts;
        a.acc = ((uint32_t)prm.flags >> FR_FLAG_ACCUMULATE_SHIFT) & 0xFFu;
        a.bound = (prm.aux && prm.aux->binding) ? 1 : 0;
        if (a.bound) {
            a.bind = bind_args(*prm.aux->binding);
            a.bg = BindGrads{prm.aux->d_verts, prm.aux->d_offset, prm.aux->d_rotation, prm.aux->d_scaling, prm.aux->d_local_xyz};
        } else {
            a.bind = BindArgs{};
            a.bg = BindGrads{};
        }
        const size_t l = (in.shs && calls[k].grads->dL_dsh) ? (size_t)kPreBwdWaves * prebwd_block_rows(prm.M * 3) * prebwd_row_stride(prm.M * 3) * sizeof(float) : 0;
        lds = l > lds ? l : lds;
        blocks = max(blocks, (uint32_t)((P + wg - 1) / wg));
    }
    // g.accum is all zero here: zeroed when allocated, and again by k_preprocess_bwd after every backward
    int rc = launch_blend_backward(n, calls, g, v, planes, s, debug);
    if (rc) return rc;
    // camera-pose gradients (FR_FLAG_CAMERA_GRAD, the views agree on it): they read the accumulator rows k_preprocess_bwd zeroes
    if (calls[0].prm->flags & FR_FLAG_CAMERA_GRAD) {
        rc = launch_camera_backward(n, calls, g, v, s);
        if (rc) return rc;
        rc = debug_sync(debug, s, "camera backward");
        if (rc) return rc;
    }
    {
        StageScope sc(calls[0].h, ST_PREPROCESS_BWD, s);
        if (planes) launch_views(k_preprocess_bwd_planes, k_preprocess_bwd_planes_batch, n, args, blocks, (uint32_t)wg, lds, s);
        else launch_views(k_preprocess_bwd, k_preprocess_bwd_batch, n, args, blocks, (uint32_t)wg, lds, s);
    }
    FR_HIP(hipGetLastError());
    if (!capturing)
        for (int k = 0; k < n; k++) {
            fr_handle_impl* h = calls[k].h;
            FR_HIP(hipEventRecord(h->bwd_done, s));
            h->last_bwd_stream = s, h->have_last_bwd = true;
        }
    if (debug) FR_HIP(hipStreamSynchronize(s));
    return FR_OK;
}

}  // namespace fr
