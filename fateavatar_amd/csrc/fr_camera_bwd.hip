// Camera-pose gradients of a frame (FR_FLAG_CAMERA_GRAD): dL/d(viewmatrix), dL/d(projmatrix), dL/d(campos) — the three
// camera inputs of fr_inputs, in the storage the kernels read — summed over the Gaussians in ONE launch.
//
// The reference's rasterizer returns None for all three (diff_gaussian_rasterization/__init__.py:143-153), so its
// `cam_pose` tracking embedding (train/base.py:123,142) never moves.  Everything the sums are made of is what the
// per-Gaussian backward (fr_preprocess_bwd.hip) has in registers anyway; this kernel computes it again from the same
// inputs with the same expressions, between the blend backward (which fills the accumulator rows) and k_preprocess_bwd
// (which reads and re-zeroes them).  It is launched only with the flag: a backward without it makes the launches it made
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
// per-Gaussian kernels whose expressions it repeats.  A thread requests everything it reads of a Gaussian before it looks at
// the radius (camera_bwd_fetch; a culled Gaussian's row is read for nothing), and up to 262 144 Gaussians are one visit per
// thread.  Measured at 100 k visible Gaussians on the MI355X: 16.6 us a launch — with the loads behind the radius test and a
// 256-workgroup grid (two visits) just the same, next to 14.3 us for k_preprocess_bwd: the kernel moves 12.9 MB (0.78 TB/s) and
// is bound by the arithmetic it shares with that kernel (IEEE divisions and square roots under the STRICT flags), not by
// memory (profiles/r22_camera_grad.md).
#include "fr_common.hpp"

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
        for (int k = 0; k < 9; k++) in.dd[k] = a.dcolor_ddir[i * 9 + k];
    }
}

// one Gaussian's 27 terms, added to `s`: the expressions of preprocess_bwd_one (fr_preprocess_bwd.hip), in its order
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
    float c3[6];
    if (a.cov3D_precomp) {
        for (int k = 0; k < 6; k++) c3[k] = in.c3[k];
    } else {
        float q_r = in.q[0], q_x = in.q[1], q_y = in.q[2], q_z = in.q[3];
        float sc[3] = {in.sc[0], in.sc[1], in.sc[2]};
        if (a.raw) {
            sc[0] = act_exp(sc[0]), sc[1] = act_exp(sc[1]), sc[2] = act_exp(sc[2]);
            const float rot_inv = act_rot_inv_norm(q_r, q_x, q_y, q_z);
            q_r *= rot_inv, q_x *= rot_inv, q_y *= rot_inv, q_z *= rot_inv;
        }
        cov3d_from_scale_rot(sc[0], sc[1], sc[2], q_r, q_x, q_y, q_z, a.scale_modifier, c3);
    }

    // ---------------- conic -> Sigma2D -> T and t (backward.cu:144-274)
    float3 t = xform4x3(mean, vm);
    const float limx = 1.3f * a.tan_fovx, limy = 1.3f * a.tan_fovy;
    const float txtz = t.x / t.z, tytz = t.y / t.z;
    t.x = fminf(limx, fmaxf(-limx, txtz)) * t.z;
    t.y = fminf(limy, fmaxf(-limy, tytz)) * t.z;
    const float x_grad_mul = txtz < -limx || txtz > limx ? 0 : 1;
    const float y_grad_mul = tytz < -limy || tytz > limy ? 0 : 1;
    const float h_x = a.focal_x, h_y = a.focal_y;
    const float j00 = h_x / t.z, j02 = -(h_x * t.x) / (t.z * t.z);
    const float j11 = h_y / t.z, j12 = -(h_y * t.y) / (t.z * t.z);
    float T0[3], T1[3];
    for (int w = 0; w < 3; w++) {
        const float W0 = vm[4 * w], W1 = vm[4 * w + 1], W2 = vm[4 * w + 2];
        T0[w] = W0 * j00 + W1 * 0.0f + W2 * j02;
        T1[w] = W0 * 0.0f + W1 * j11 + W2 * j12;
    }
    const float V[3][3] = {{c3[0], c3[1], c3[2]}, {c3[1], c3[3], c3[4]}, {c3[2], c3[4], c3[5]}};
    float A0[3], A1[3];
    for (int c = 0; c < 3; c++) {
        A0[c] = T0[0] * V[0][c] + T0[1] * V[1][c] + T0[2] * V[2][c];
        A1[c] = T1[0] * V[0][c] + T1[1] * V[1][c] + T1[2] * V[2][c];
    }
    float ca = A0[0] * T0[0] + A0[1] * T0[1] + A0[2] * T0[2];
    const float cb = A1[0] * T0[0] + A1[1] * T0[1] + A1[2] * T0[2];
    float cc = A1[0] * T1[0] + A1[1] * T1[1] + A1[2] * T1[2];
    ca += 0.3f;
    cc += 0.3f;
    const float denom = ca * cc - cb * cb;
    const float g2x = acc[ACC_MX] * (0.5f * a.W);
    const float g2y = acc[ACC_MY] * (0.5f * a.H);
    const float dcx = -0.5f * acc[ACC_CA], dcy = -0.5f * acc[ACC_CB], dcz = -0.5f * acc[ACC_CC];
    float dL_da = 0, dL_db = 0, dL_dc = 0;
    const float denom2inv = 1.0f / ((denom * denom) + 0.0000001f);
    if (denom2inv != 0) {
        dL_da = denom2inv * (-cc * cc * dcx + 2 * cb * cc * dcy + (denom - ca * cc) * dcz);
        dL_dc = denom2inv * (-ca * ca * dcz + 2 * ca * cb * dcy + (denom - ca * cc) * dcx);
        dL_db = denom2inv * 2 * (cb * cc * dcx - (denom + 2 * cb * cb) * dcy + ca * cb * dcz);
    }
    float dT0[3], dT1[3];
    for (int c = 0; c < 3; c++) {
        const float tv0 = T0[0] * V[c][0] + T0[1] * V[c][1] + T0[2] * V[c][2];
        const float tv1 = T1[0] * V[c][0] + T1[1] * V[c][1] + T1[2] * V[c][2];
        dT0[c] = 2 * tv0 * dL_da + tv1 * dL_db;
        dT1[c] = 2 * tv1 * dL_dc + tv0 * dL_db;
    }
    const float dL_dJ00 = vm[0] * dT0[0] + vm[4] * dT0[1] + vm[8] * dT0[2];
    const float dL_dJ02 = vm[2] * dT0[0] + vm[6] * dT0[1] + vm[10] * dT0[2];
    const float dL_dJ11 = vm[1] * dT1[0] + vm[5] * dT1[1] + vm[9] * dT1[2];
    const float dL_dJ12 = vm[2] * dT1[0] + vm[6] * dT1[1] + vm[10] * dT1[2];
    const float tz = 1.f / t.z, tz2 = tz * tz, tz3 = tz2 * tz;
    const float dL_dtx = x_grad_mul * -h_x * tz2 * dL_dJ02;
    const float dL_dty = y_grad_mul * -h_y * tz2 * dL_dJ12;
    float dL_dtz = -h_x * tz2 * dL_dJ00 - h_y * tz2 * dL_dJ11 + (2 * h_x * t.x) * tz3 * dL_dJ02 + (2 * h_y * t.y) * tz3 * dL_dJ12;
    dL_dtz += acc[ACC_Z];   // (the depth plane's dL/dz; zero in a frame without planes)

    // ---------------- the view matrix: t = m . view, and W inside T = J W
    const float m_[4] = {mean.x, mean.y, mean.z, 1.0f};
    const float dt[3] = {dL_dtx, dL_dty, dL_dtz};
    for (int r = 0; r < 4; r++)
        for (int c = 0; c < 3; c++) s[3 * r + c] += dt[c] * m_[r];
    for (int w = 0; w < 3; w++) {
        s[3 * w] += j00 * dT0[w];
        s[3 * w + 1] += j11 * dT1[w];
        s[3 * w + 2] += j02 * dT0[w] + j12 * dT1[w];
    }

    // ---------------- the projection: ndc = hom.xy m_w (backward.cu:370-387)
    {
        const float* proj = cam.proj;
        const float4 m_hom = xform4x4(mean, proj);
        const float m_w = 1.0f / (m_hom.w + 0.0000001f);
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
        const float dox = mean.x - cam.campos[0], doy = mean.y - cam.campos[1], doz = mean.z - cam.campos[2];
        const uint32_t cl = in.cl;
        float dRGB[3];
        for (int c = 0; c < 3; c++) dRGB[c] = acc[ACC_R + c] * (((cl >> c) & 1) ? 0 : 1);
        const float* dd = in.dd;
        const float ddx = dd[0] * dRGB[0] + dd[1] * dRGB[1] + dd[2] * dRGB[2];
        const float ddy = dd[3] * dRGB[0] + dd[4] * dRGB[1] + dd[5] * dRGB[2];
        const float ddz = dd[6] * dRGB[0] + dd[7] * dRGB[1] + dd[8] * dRGB[2];
        const float sum2 = dox * dox + doy * doy + doz * doz;
        const float invsum32 = 1.0f / sqrtf(sum2 * sum2 * sum2);
        s[24] -= ((+sum2 - dox * dox) * ddx - doy * dox * ddy - doz * dox * ddz) * invsum32;
        s[25] -= (-dox * doy * ddx + (sum2 - doy * doy) * ddy - doz * doy * ddz) * invsum32;
        s[26] -= (-dox * doz * ddx - doy * doz * ddy + (sum2 - doz * doz) * ddz) * invsum32;
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
        a.P = prm.P, a.W = prm.W, a.H = prm.H;
        a.raw = (prm.flags & FR_FLAG_RAW_ACTIVATIONS) ? 1 : 0;
        a.blocks = capped_blocks((unsigned)prm.P, kCamThreads, kCamMaxBlocks);
        a.tan_fovx = prm.tan_fovx, a.tan_fovy = prm.tan_fovy;
        a.focal_y = prm.H / (2.0f * prm.tan_fovy);
        a.focal_x = prm.W / (2.0f * prm.tan_fovx);
        a.scale_modifier = prm.scale_modifier;
        a.means3D = in.means3D, a.scales = in.scales, a.rotations = in.rotations, a.cov3D_precomp = in.cov3D_precomp;
        a.view = in.viewmatrix, a.proj = in.projmatrix, a.campos = in.campos;
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
