// Camera-pose gradients of a frame (FR_FLAG_CAMERA_GRAD): dL/d(viewmatrix), dL/d(projmatrix), dL/d(campos) — the three
// camera inputs of fr_inputs, in the storage the kernels read — summed over the Gaussians in ONE launch.
//
// The reference's rasterizer returns None for all three (diff_gaussian_rasterization/__init__.py:143-153), so its
// `cam_pose` tracking embedding (train/base.py:123,142) never moves.  Everything the sums are made of is what the
// per-Gaussian backward (fr_preprocess_bwd.hip) has in registers anyway; this kernel computes it again from the same
// inputs by calling the same functions (fr_project_math.hpp), between the blend backward (which fills the accumulator
// rows) and k_preprocess_bwd (which reads and re-zeroes them).  It is launched only with the flag: a backward without it makes the launches it made
// before, from unchanged kernels.
//
// With m = (x, y, z, 1) the mean, t = view-space mean, hom = m . proj, m_w = 1 / (hom.w + 1e-7):
//   d view[c + 4 r]  = sum dL/dt_c m_r                         (c < 3, r < 4; dL/dt: k_preprocess_bwd's dL_dtx / dL_dty /
//                                                               dL_dtz with the reference's stop-gradient on guard-band-
//                                                               clamped x / y, + the depth plane's dL/dz for c = 2)
//                    + through W = view[:3,:3] of T = J W:      d view[4 w] += j00 dT0[w], d view[4 w + 1] += j11 dT1[w],
//                                                               d view[4 w + 2] += j02 dT0[w] + j12 dT1[w]
//   d proj[0 + 4 r]  = sum g2x m_w m_r,   d proj[1 + 4 r] = sum g2y m_w m_r,
//   d proj[3 + 4 r]  = - sum (g2x hom.x + g2y hom.y) m_w^2 m_r  ((g2x, g2y) = dL/d ndc: dL_dmeans2D)
//   d campos         = - sum (the SH part of dL/dmean)          (the colour depends on mean - campos alone)
// 27 sums; the entries no kernel reads (view column 3, proj column 2) are written as 0.  The accumulator's Z slot is zero
// in frames without planes (fr_common.hpp), so ONE kernel serves both: adding it is exact there.
//
// 256 threads, at most kCamMaxBlocks workgroups striding over the Gaussians, per-workgroup partials added up in workgroup-index
// order by the workgroup that finishes last (sum_over_workgroups, fr_common.hpp): no float atomics, the same bits on every
// launch and replay; the workspace is zero before the first launch and left zeroed.  Built with the STRICT flags, like the
// per-Gaussian kernels whose projection math it shares.  A thread requests everything it reads of a Gaussian before it looks at
// the radius (camera_bwd_fetch; a culled Gaussian's row is read for nothing), and up to 262 144 Gaussians are one visit per
// thread.  Measured at 100 k visible Gaussians on the MI355X: 16.6 us a launch — with the loads behind the radius test and a
// 256-workgroup grid (two visits) just the same, next to 14.3 us for k_preprocess_bwd: the kernel moves 12.9 MB (0.78 TB/s) and
// is bound by the arithmetic it shares with that kernel (IEEE divisions and square roots under the STRICT flags), not by
// memory (profiles/r22_camera_grad.md).
#include "fr_project_math.hpp"

namespace fr {

constexpr unsigned kCamMaxBlocks = 1024;
constexpr unsigned kCamThreads = kSumThreads;   // (sum_over_workgroups' workgroup)
constexpr int kCamSums = 27;                    // view 3 x 4 (index 3 r + c), proj 3 x 4 (12 + 3 r + {0, 1, 3}), campos 3

struct CamBwdArgs {
    int P, raw, W, H;
    unsigned blocks;     // this view's workgroups (a batched launch's grid is the largest view's)
    float tan_fovx, tan_fovy, focal_x, focal_y, scale_modifier;
    const float* means3D;
    const float* scales;
    const float* rotations;
    const float* cov3D_precomp;
    const float* view;
    const float* proj;
    const float* campos;
    const int* radii;
    const float* accum;         // the handle's accumulator rows, filled by the blend backward
    const float* dcolor_ddir;   // GeomView; null for a frame without SH coefficients (no campos gradient)
    const uint8_t* clamped;
    const DeviceCounts* counts;
    float* d_view;              // [16], [16], [3]; any may be null
    float* d_proj;
    float* d_campos;
    float* partial;             // [kCamSums][kCamMaxBlocks]
    unsigned* counter;
};

// what the kernel reads of ONE Gaussian, all of it requested before any of it is used (optional inputs: wave-uniform null tests)
struct CamBwdIn {
    int radius;
    float4 r0, r1, r2;                   // the accumulator row
    float mean[3], q[4], sc[3], c3[6];   // q / sc: with `scales`;  c3: with `cov3D_precomp`
    uint32_t cl;                         // with SH coefficients: clamped bits, d colour / d direction
    float dd[9];
};
__device__ __forceinline__ void camera_bwd_fetch(const CamBwdArgs& a, const size_t i, CamBwdIn& in)
{
    in.radius = a.radii[i];
    const float4* row4 = reinterpret_cast<const float4*>(a.accum + i * kAccumStride);
    in.r0 = row4[0], in.r1 = row4[1], in.r2 = row4[2];
    for (int k = 0; k < 3; k++) in.mean[k] = a.means3D[3 * i + k];
    for (int k = 0; k < 4; k++) in.q[k] = 0.f;
    for (int k = 0; k < 3; k++) in.sc[k] = 0.f;
    for (int k = 0; k < 6; k++) in.c3[k] = 0.f;
    if (a.cov3D_precomp) {
        for (int k = 0; k < 6; k++) in.c3[k] = a.cov3D_precomp[6 * i + k];
    } else {
        for (int k = 0; k < 4; k++) in.q[k] = a.rotations[4 * i + k];
        for (int k = 0; k < 3; k++) in.sc[k] = a.scales[3 * i + k];
    }
    in.cl = 0u;
    for (int k = 0; k < 9; k++) in.dd[k] = 0.f;
    if (a.dcolor_ddir) {
        in.cl = a.clamped[i];
        for (int k = 0; k < 9; k++) in.dd[k] = a.dcolor_ddir[ddir_index(k, i, (size_t)a.P)];   // (planar [9][P])
    }
}

// one Gaussian's 27 terms, added to `s`: from the functions preprocess_bwd_one (fr_preprocess_bwd.hip) calls, in its order
__device__ __forceinline__ void camera_bwd_one(const CamBwdArgs& a, const CameraRegs& cam, const CamBwdIn& in, float (&s)[kCamSums])
{
    float acc[12];
    {
        const float4 r0 = in.r0, r1 = in.r1, r2 = in.r2;
        acc[0] = r0.x, acc[1] = r0.y, acc[2] = r0.z, acc[3] = r0.w, acc[4] = r1.x, acc[5] = r1.y, acc[6] = r1.z,
        acc[7] = r1.w, acc[8] = r2.x, acc[9] = r2.y, acc[10] = r2.z, acc[11] = r2.w;
    }
    const float3 mean = make_float3(in.mean[0], in.mean[1], in.mean[2]);
    const float* vm = cam.view;
    const bool precomp = a.cov3D_precomp != nullptr;
    const Sigma3D sig = sigma3d_from_inputs(!precomp, a.raw != 0, in.sc, in.q, a.scale_modifier, precomp, in.c3);

    // ---------------- conic -> Sigma2D -> T and t (backward.cu:144-274): fr_project_math.hpp
    const Ewa e = ewa_project(xform4x3(mean, vm), vm, sig.c3, a.tan_fovx, a.tan_fovy, a.focal_x, a.focal_y);
    const float g2x = acc[ACC_MX] * (0.5f * a.W);
    const float g2y = acc[ACC_MY] * (0.5f * a.H);
    const float dcx = -0.5f * acc[ACC_CA], dcy = -0.5f * acc[ACC_CB], dcz = -0.5f * acc[ACC_CC];
    const EwaGrad eg = ewa_bwd(e, vm, sig.c3, conic_bwd(e, dcx, dcy, dcz), a.focal_x, a.focal_y);
    float dL_dtz = eg.dL_dtz;
    dL_dtz += acc[ACC_Z];   // (the depth plane's dL/dz; zero in a frame without planes)

    // ---------------- the view matrix: t = m . view, and W inside T = J W
    const float m_[4] = {mean.x, mean.y, mean.z, 1.0f};
    const float dt[3] = {eg.dL_dtx, eg.dL_dty, dL_dtz};
    for (int r = 0; r < 4; r++)
        for (int c = 0; c < 3; c++) s[3 * r + c] += dt[c] * m_[r];
    for (int w = 0; w < 3; w++) {
        s[3 * w] += e.j00 * eg.dT0[w];
        s[3 * w + 1] += e.j11 * eg.dT1[w];
        s[3 * w + 2] += e.j02 * eg.dT0[w] + e.j12 * eg.dT1[w];
    }

    // ---------------- the projection: ndc = hom.xy m_w (backward.cu:370-387)
    {
        float m_w;
        const float4 m_hom = project_mean(mean, cam.proj, m_w);
        const float gx = g2x * m_w, gy = g2y * m_w;
        const float gw = (g2x * m_hom.x + g2y * m_hom.y) * m_w * m_w;
        for (int r = 0; r < 4; r++) {
            s[12 + 3 * r] += gx * m_[r];
            s[12 + 3 * r + 1] += gy * m_[r];
            s[12 + 3 * r + 2] -= gw * m_[r];
        }
    }

    // ---------------- the camera position: the SH colour's view direction (backward.cu:20-139)
    if (a.dcolor_ddir) {
        const float dcol[3] = {acc[ACC_R], acc[ACC_G], acc[ACC_B]};
        const ShDirGrad sd = sh_dir_bwd(mean, cam.campos, in.cl, dcol, in.dd);
        s[24] -= sd.d[0], s[25] -= sd.d[1], s[26] -= sd.d[2];
    }
}

__device__ __forceinline__ void camera_bwd_body(const CamBwdArgs& a)
{
    if (blockIdx.x >= a.blocks) return;   // (a batched launch's grid is the largest view's; the whole workgroup leaves)
    const CameraRegs cam = load_camera(a.view, a.proj, a.campos, threadIdx.x & 63);
    // (a frame that overflowed its binning capacity blended nothing: it adds nothing and the outputs are zeros)
    const bool live = a.counts->overflow == 0u;
    float s[kCamSums];
#pragma unroll
    for (int k = 0; k < kCamSums; k++) s[k] = 0.f;
    const size_t stride = (size_t)a.blocks * kCamThreads;
    if (live)
        for (size_t i = (size_t)blockIdx.x * kCamThreads + threadIdx.x; i < (size_t)a.P; i += stride) {
            CamBwdIn in;
            camera_bwd_fetch(a, i, in);
            asm volatile("" ::: "memory");   // (the compiler's barrier: the loads stay in front of the branch on the radius)
            if (in.radius > 0) camera_bwd_one(a, cam, in, s);
        }
    if (!sum_over_workgroups(s, a.partial, kCamMaxBlocks, a.counter, blockIdx.x, a.blocks)) return;
    // (thread 0 of the workgroup that finished last: 35 plain stores)
    if (a.d_view)
        for (int r = 0; r < 4; r++) {
            for (int c = 0; c < 3; c++) a.d_view[4 * r + c] = s[3 * r + c];
            a.d_view[4 * r + 3] = 0.f;
        }
    if (a.d_proj)
        for (int r = 0; r < 4; r++) {
            a.d_proj[4 * r] = s[12 + 3 * r], a.d_proj[4 * r + 1] = s[12 + 3 * r + 1];
            a.d_proj[4 * r + 2] = 0.f, a.d_proj[4 * r + 3] = s[12 + 3 * r + 2];
        }
    if (a.d_campos)
        for (int c = 0; c < 3; c++) a.d_campos[c] = s[24 + c];
}

__global__ void __launch_bounds__(kCamThreads) k_camera_bwd(CamBwdArgs a) { camera_bwd_body(a); }
__global__ void __launch_bounds__(kCamThreads) k_camera_bwd_batch(BatchOf<CamBwdArgs> b) { camera_bwd_body(b.v[blockIdx.y]); }

size_t camera_grad_workspace_bytes() { return done_workspace_bytes((size_t)kCamSums * kCamMaxBlocks); }

int launch_camera_backward(int n, const BackwardCall* calls, const GeomView* g, const ImageView* v, hipStream_t s)
{
    CamBwdArgs args[kMaxBatch];
    uint32_t blocks = 0;
    for (int k = 0; k < n; k++) {
        const fr_params& prm = *calls[k].prm;
        const fr_inputs& in = *calls[k].in;
        const fr_aux_camera& aux = *reinterpret_cast<const fr_aux_camera*>(prm.aux);   // (fr_backward has checked the flag's arguments)
        const DoneWorkspace ws = done_workspace(aux.camera_workspace);
        CamBwdArgs& a = args[k];
        fill_projection_args(a, prm, in);
        a.blocks = capped_blocks((unsigned)prm.P, kCamThreads, kCamMaxBlocks);
        a.radii = calls[k].radii, a.accum = g[k].accum;
        a.dcolor_ddir = in.shs ? g[k].dcolor_ddir : nullptr;
        a.clamped = g[k].clamped;
        a.counts = v[k].counts;
        a.d_view = aux.d_viewmatrix, a.d_proj = aux.d_projmatrix, a.d_campos = aux.d_campos;
        a.partial = ws.partial, a.counter = ws.counter;
        blocks = max(blocks, (uint32_t)a.blocks);
    }
    launch_views(k_camera_bwd, k_camera_bwd_batch, n, args, blocks, kCamThreads, 0, s);
    FR_HIP(hipGetLastError());
    return FR_OK;
}

}  // namespace fr
