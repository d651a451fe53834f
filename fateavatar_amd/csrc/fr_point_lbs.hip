// MonoGaussianAvatar's per-point passes (include/fr_rasterizer.h): fr_point_lbs_forward / _backward / _backward_pose,
// fr_nearest_vertex and fr_lbs_terms.
//
// reference: FLAME.forward_pts (flame/FLAME.py:207-237) over flame/lbs.py:103-188 — per point an expression basis S [3,E], a
// pose-corrective basis P [36,3] and skinning weights w [J] the deformer MLP predicted:
//     T_c = sum_j w_j A^c_j,  z = T_c^-1 (p, 1),  x = z[:3] + S (beta - beta_c) + P^T (phi - phi_c),  xyz = (sum_j w_j A_j (x, 1))[:3]
// where the reference expands beta, phi and the [J,4,4] transforms to one copy per point, runs a batched torch.inverse and
// differentiates everything forward-mode (vmap(jacfwd), model/baseline/monogaussianavatar.py:359).  A point's rows are 600 B
// (S at E = 50), 432 B (P) and 24 B (w at J = 6): the pass is memory traffic and nothing else.
//
// A GROUP OF SIXTEEN LANES = one point, four consecutive points per wave.  The group strides through the point's rows sixteen
// floats at a time (one 64-byte segment per group and instruction; the four groups of a wave read four rows that follow one
// another in memory, so a wave's loads walk through ONE contiguous 2.4 KB block instead of 64 cache lines a lane of its own
// would touch), every lane keeps partial sums of the three components of the blendshape offset, and a butterfly over the
// group's lanes (xor 8, 4, 2, 1: the same order on every launch, the same sum in all sixteen lanes) adds them up.  The 3x4
// arithmetic behind it is done by all sixteen lanes alike (no divergence, nothing to broadcast); lane 0 writes xyz / d_points,
// lanes 0 .. J-1 one d_weights entry each, and the rows of d_shapedirs / d_posedirs go out the way S and P came in.
// The frame's (beta - beta_c), (phi - phi_c) and both sets of bone matrices sit in 1.2 KB of LDS per workgroup.
//
// With T_c = [[R, t], [0, s]] (s = sum_j w_j; the bones' last rows are (0,0,0,1)):  T_c^-1 = [[R^-1, -R^-1 t / s], [0, 1 / s]],
//     z3 = R^-1 (p - t / s),  z4 = 1 / s
// backward, with g = dL/dxyz and T = sum_j w_j A_j = [[R_f, t_f], ...]:
//     d_x = R_f^T g                        d_S[k,l] = d_x[k] (beta_l - beta^c_l)        d_P[i,k] = (phi_i - phi^c_i) d_x[k]
//     u3 = R^-T d_x,  u4 = -(t . u3) / s   (u = T_c^-T (d_x, 0))                        d_p = u3
//     d_w_j = g . (R_j x + t_j) - (u3 . (R^c_j z3 + t^c_j z4) + u4 z4)
// d_weights is the only output that needs x, i.e. S and P again: a backward without it reads 36 B per point.
//
// fr_point_lbs_backward_pose (k_point_lbs_pose_bwd): the gradient to the FRAME's pose state is a reduction over the points,
//     d_beta[l] = sum_n sum_k S_n[k,l] d_x_n[k]      d_phi[i] = sum_n sum_k P_n[i,k] d_x_n[k]      d_A[j,r,c] = sum_n w_nj g_n[r] (x_n, 1)[c]
// (E + 36 + 12 J sums; the bones' last rows are constants: 0).  The same sixteen-lane groups, lbs_stage and lbs_point; d_x needs
// w, p and g only, so ONE pass over the point's S and P rows feeds both the blendshape offset (lbs_offset's sums in its order:
// x has the forward's bits) and the running sums a lane keeps for the slots it owns: columns sub, sub + 16, ... of S, elements
// sub, sub + 16, ... of P (folded three to a pose feature at the very end) and, in lane j < J, the twelve products of bone j.
// A dead group adds exact zeros and stays with its wave.  After the sweep: the wave's four groups in index order (shuffles), the
// workgroup's waves in index order (LDS), one row of 272 partials per workgroup, and the workgroup that finishes last adds the
// rows up in workgroup-index order (sum_rows_over_workgroups, fr_common.hpp: fifteen runs of consecutive rows side by side, one
// float4 column per thread, then the runs in order), writes the three outputs and leaves the workspace zeroed: no float atomics,
// the same bits on every launch.  Workgroups of 1 024 threads, at most one per CU (256): the last workgroup's serial read grows with the
// number of rows, not with N.  Compiler (gfx950): 123 VGPRs, no scratch, 18 592 B of LDS, four waves per SIMD = the one
// resident workgroup.  Measured on the MI355X at N = 100 000, E = 50, J = 6 (profiles/r19_mono_pose.md): 0.072 ms a launch,
// i.e. the 1 080 B a point's S, P, w, p and g rows hold are read at 1.50 TB/s = 24 % of the achievable HBM rate, 45 x faster
// than the float32 torch backward to the frame state.  The same code as 512 workgroups of 256 threads (two waves per SIMD, 512
// rows for the last workgroup) took 0.121 ms: what bounds the launch is memory latency at the waves in flight its registers
// allow (and the last workgroup's serial pass), not the HBM rate; how the 0.072 ms split between the two was not measured.
//
// fr_nearest_vertex: one lane per point against the vertices in LDS (struct of arrays, 4 096 vertices = 48 KB at a time, every
// lane of a wave reads the same address: broadcast reads, four vertices per ds_read_b128), strict `<` in ascending order.
// fr_lbs_terms: the same sixteen-lane groups over (pred row, gathered ground-truth row); the three sums go through
// per-workgroup partials added up in index order by the workgroup that finishes last (sum_over_workgroups, fr_common.hpp).
// Built with the STRICT flags: the nearest vertex's expression order is part of its contract.
#include "fr_common.hpp"

namespace fr {

constexpr unsigned kLbsThreads = 256;
constexpr unsigned kLbsGroup = 16;          // lanes per point (a power of two that divides the wave, >= FR_LBS_MAX_J)
constexpr unsigned kLbsMaxBlocks = 2048;
constexpr int kLbsPose = FR_LBS_POSE_FEATURES;
static_assert(kLbsGroup >= FR_LBS_MAX_J, "one lane per bone writes d_weights");

struct LbsArgs {
    const float *points, *shapedirs, *posedirs, *weights;
    const float *beta_c, *phi_c, *A_c, *beta, *phi, *A;
    float* xyz;                                   // forward
    const float* g;                               // backward
    float *d_points, *d_shapedirs, *d_posedirs, *d_weights;
    int N, E, J;
};

struct LbsShared {
    float dbeta[FR_LBS_MAX_E];
    float dphi[kLbsPose];
    float Ac[FR_LBS_MAX_J][12];   // rows 0 .. 2 of every bone matrix
    float A[FR_LBS_MAX_J][12];
};

__device__ __forceinline__ void lbs_stage(const LbsArgs& a, LbsShared& s)
{
    for (unsigned t = threadIdx.x; t < (unsigned)a.E; t += blockDim.x) s.dbeta[t] = a.beta[t] - a.beta_c[t];
    for (unsigned t = threadIdx.x; t < (unsigned)kLbsPose; t += blockDim.x) s.dphi[t] = a.phi[t] - a.phi_c[t];
    for (unsigned t = threadIdx.x; t < (unsigned)a.J * 12u; t += blockDim.x) {
        const unsigned j = t / 12u, e = t % 12u;
        s.Ac[j][e] = a.A_c[j * 16u + e];
        s.A[j][e] = a.A[j * 16u + e];
    }
    __syncthreads();
}

// the blendshape offset S (beta - beta_c) + P^T (phi - phi_c) of point i, in every lane of its group
__device__ __forceinline__ void lbs_offset(const LbsArgs& a, const LbsShared& s, size_t i, unsigned sub, bool live, float o[3])
{
    float acc0 = 0.f, acc1 = 0.f, acc2 = 0.f;
    if (live) {
        const float* __restrict__ S = a.shapedirs + i * 3u * (size_t)a.E;
        const float* __restrict__ P = a.posedirs + i * (size_t)(kLbsPose * 3);
        const unsigned E = (unsigned)a.E;
        for (unsigned l = sub; l < E; l += kLbsGroup) {
            const float b = s.dbeta[l];
            acc0 += S[l] * b, acc1 += S[E + l] * b, acc2 += S[2u * E + l] * b;
        }
        for (unsigned m = sub; m < (unsigned)(kLbsPose * 3); m += kLbsGroup) {
            const float v = P[m] * s.dphi[m / 3u];
            const unsigned k = m % 3u;
            acc0 += k == 0u ? v : 0.f, acc1 += k == 1u ? v : 0.f, acc2 += k == 2u ? v : 0.f;
        }
    }
    o[0] = group_sum<kLbsGroup>(acc0), o[1] = group_sum<kLbsGroup>(acc1), o[2] = group_sum<kLbsGroup>(acc2);
}

struct LbsPoint {
    float Ri[9];       // R^-1 of T_c's 3x3 block
    float t[3];        // T_c's translation column
    float inv_s;       // 1 / sum_j w_j = z[3]
    float z[3];
    float T[12];       // the frame's blended rows
};

// `wl`: lane j of the group holds w_j.  The bones are walked one at a time (ascending j, w_j broadcast from its lane): unrolled,
// the compiler fetches all 2 x 8 x 12 matrix entries from LDS up front and the kernel needs 256 VGPRs.
__device__ __forceinline__ void lbs_point(const LbsShared& s, float wl, int J, const float p[3], LbsPoint& q)
{
    float Tc[12];
#pragma unroll
    for (int e = 0; e < 12; e++) Tc[e] = 0.f, q.T[e] = 0.f;
    float sw = 0.f;
#pragma nounroll
    for (int j = 0; j < J; j++) {
        const float w = __shfl(wl, j, kLbsGroup);
        sw += w;
#pragma unroll
        for (int e = 0; e < 12; e++) Tc[e] += w * s.Ac[j][e], q.T[e] += w * s.A[j][e];
    }
    q.inv_s = 1.0f / sw;
    const float a = Tc[0], b = Tc[1], c = Tc[2], d = Tc[4], e = Tc[5], f = Tc[6], g = Tc[8], h = Tc[9], k = Tc[10];
    const float c00 = e * k - f * h, c01 = f * g - d * k, c02 = d * h - e * g;
    const float inv_det = 1.0f / ((a * c00 + b * c01) + c * c02);
    q.Ri[0] = c00 * inv_det, q.Ri[1] = (c * h - b * k) * inv_det, q.Ri[2] = (b * f - c * e) * inv_det;
    q.Ri[3] = c01 * inv_det, q.Ri[4] = (a * k - c * g) * inv_det, q.Ri[5] = (c * d - a * f) * inv_det;
    q.Ri[6] = c02 * inv_det, q.Ri[7] = (b * g - a * h) * inv_det, q.Ri[8] = (a * e - b * d) * inv_det;
    q.t[0] = Tc[3], q.t[1] = Tc[7], q.t[2] = Tc[11];
    const float r0 = p[0] - q.t[0] * q.inv_s, r1 = p[1] - q.t[1] * q.inv_s, r2 = p[2] - q.t[2] * q.inv_s;
    q.z[0] = (q.Ri[0] * r0 + q.Ri[1] * r1) + q.Ri[2] * r2;
    q.z[1] = (q.Ri[3] * r0 + q.Ri[4] * r1) + q.Ri[5] * r2;
    q.z[2] = (q.Ri[6] * r0 + q.Ri[7] * r1) + q.Ri[8] * r2;
}

__device__ __forceinline__ void lbs_load_point(const LbsArgs& a, size_t i, unsigned sub, bool live, float& wl, float p[3])
{
    wl = (live && sub < (unsigned)a.J) ? a.weights[i * (size_t)a.J + sub] : ((!live && sub == 0) ? 1.f : 0.f);
#pragma unroll
    for (int k = 0; k < 3; k++) p[k] = live ? a.points[i * 3u + k] : 0.f;
}

__global__ void __launch_bounds__(kLbsThreads) k_point_lbs_fwd(LbsArgs a)
{
    __shared__ LbsShared s;
    lbs_stage(a, s);
    const unsigned sub = threadIdx.x & (kLbsGroup - 1);
    const unsigned group = (blockIdx.x * blockDim.x + threadIdx.x) / kLbsGroup, n_groups = gridDim.x * blockDim.x / kLbsGroup;
    // (the trip count is the same for every lane of the launch: the shuffles run with whole waves)
    for (unsigned base = 0; base < (unsigned)a.N; base += n_groups) {
        const size_t i = (size_t)base + group;
        const bool live = i < (size_t)a.N;
        float o[3], wl, p[3];
        lbs_offset(a, s, i, sub, live, o);
        lbs_load_point(a, i, sub, live, wl, p);
        LbsPoint q;
        lbs_point(s, wl, a.J, p, q);
        const float x0 = q.z[0] + o[0], x1 = q.z[1] + o[1], x2 = q.z[2] + o[2];
        if (live && sub == 0) {
            float* out = a.xyz + i * 3u;
            out[0] = ((q.T[0] * x0 + q.T[1] * x1) + q.T[2] * x2) + q.T[3];
            out[1] = ((q.T[4] * x0 + q.T[5] * x1) + q.T[6] * x2) + q.T[7];
            out[2] = ((q.T[8] * x0 + q.T[9] * x1) + q.T[10] * x2) + q.T[11];
        }
    }
}

__global__ void __launch_bounds__(kLbsThreads) k_point_lbs_bwd(LbsArgs a)
{
    __shared__ LbsShared s;
    lbs_stage(a, s);
    const unsigned sub = threadIdx.x & (kLbsGroup - 1);
    const unsigned group = (blockIdx.x * blockDim.x + threadIdx.x) / kLbsGroup, n_groups = gridDim.x * blockDim.x / kLbsGroup;
    const unsigned E = (unsigned)a.E;
    for (unsigned base = 0; base < (unsigned)a.N; base += n_groups) {
        const size_t i = (size_t)base + group;
        const bool live = i < (size_t)a.N;
        float o[3] = {0.f, 0.f, 0.f}, wl, p[3];
        if (a.d_weights) lbs_offset(a, s, i, sub, live, o);     // (uniform over the launch)
        lbs_load_point(a, i, sub, live, wl, p);
        LbsPoint q;
        lbs_point(s, wl, a.J, p, q);
        // every shuffle of the sweep is behind us; what follows is guarded, not skipped, so that the lanes of a dead group stay
        // with their wave whatever the stride of the sweep is
        if (live) {
            const float g0 = a.g[i * 3u], g1 = a.g[i * 3u + 1], g2 = a.g[i * 3u + 2];
            const float dx0 = (q.T[0] * g0 + q.T[4] * g1) + q.T[8] * g2;
            const float dx1 = (q.T[1] * g0 + q.T[5] * g1) + q.T[9] * g2;
            const float dx2 = (q.T[2] * g0 + q.T[6] * g1) + q.T[10] * g2;
            if (a.d_shapedirs) {
                float* __restrict__ dS = a.d_shapedirs + i * 3u * (size_t)E;
                for (unsigned l = sub; l < E; l += kLbsGroup) {
                    const float b = s.dbeta[l];
                    dS[l] = dx0 * b, dS[E + l] = dx1 * b, dS[2u * E + l] = dx2 * b;
                }
            }
            if (a.d_posedirs) {
                float* __restrict__ dP = a.d_posedirs + i * (size_t)(kLbsPose * 3);
                for (unsigned m = sub; m < (unsigned)(kLbsPose * 3); m += kLbsGroup) {
                    const unsigned k = m % 3u;
                    dP[m] = s.dphi[m / 3u] * (k == 0u ? dx0 : (k == 1u ? dx1 : dx2));
                }
            }
            if (a.d_points || a.d_weights) {
                const float u0 = (q.Ri[0] * dx0 + q.Ri[3] * dx1) + q.Ri[6] * dx2;
                const float u1 = (q.Ri[1] * dx0 + q.Ri[4] * dx1) + q.Ri[7] * dx2;
                const float u2 = (q.Ri[2] * dx0 + q.Ri[5] * dx1) + q.Ri[8] * dx2;
                if (a.d_points && sub == 0) {
                    float* out = a.d_points + i * 3u;
                    out[0] = u0, out[1] = u1, out[2] = u2;
                }
                if (a.d_weights && sub < (unsigned)a.J) {
                    const float u3 = -((q.t[0] * u0 + q.t[1] * u1) + q.t[2] * u2) * q.inv_s;
                    const float x0 = q.z[0] + o[0], x1 = q.z[1] + o[1], x2 = q.z[2] + o[2];
                    const float* Aj = s.A[sub];
                    const float* Cj = s.Ac[sub];
                    const float y0 = ((Aj[0] * x0 + Aj[1] * x1) + Aj[2] * x2) + Aj[3];
                    const float y1 = ((Aj[4] * x0 + Aj[5] * x1) + Aj[6] * x2) + Aj[7];
                    const float y2 = ((Aj[8] * x0 + Aj[9] * x1) + Aj[10] * x2) + Aj[11];
                    const float v0 = ((Cj[0] * q.z[0] + Cj[1] * q.z[1]) + Cj[2] * q.z[2]) + Cj[3] * q.inv_s;
                    const float v1 = ((Cj[4] * q.z[0] + Cj[5] * q.z[1]) + Cj[6] * q.z[2]) + Cj[7] * q.inv_s;
                    const float v2 = ((Cj[8] * q.z[0] + Cj[9] * q.z[1]) + Cj[10] * q.z[2]) + Cj[11] * q.inv_s;
                    const float fwd = (g0 * y0 + g1 * y1) + g2 * y2;
                    const float inv = ((u0 * v0 + u1 * v1) + u2 * v2) + u3 * q.inv_s;
                    a.d_weights[i * (size_t)a.J + sub] = fwd - inv;
                }
            }
        }
    }
}

static unsigned lbs_blocks(int N) { return capped_blocks((unsigned)N, kLbsThreads / kLbsGroup, kLbsMaxBlocks); }

static LbsArgs lbs_args(const fr_point_lbs& d)
{
    LbsArgs a = {};
    a.points = d.points, a.shapedirs = d.shapedirs, a.posedirs = d.posedirs, a.weights = d.weights;
    a.beta_c = d.canonical.betas, a.phi_c = d.canonical.pose_feature, a.A_c = d.canonical.transforms;
    a.beta = d.frame.betas, a.phi = d.frame.pose_feature, a.A = d.frame.transforms;
    a.N = d.N, a.E = d.E, a.J = d.J;
    return a;
}

int launch_point_lbs_forward(const fr_point_lbs& d, float* xyz, hipStream_t s)
{
    if (d.N <= 0) return FR_OK;
    LbsArgs a = lbs_args(d);
    a.xyz = xyz;
    hipLaunchKernelGGL(k_point_lbs_fwd, dim3(lbs_blocks(d.N)), dim3(kLbsThreads), 0, s, a);
    FR_HIP(hipGetLastError());
    return FR_OK;
}

int launch_point_lbs_backward(const fr_point_lbs& d, const float* g_xyz, float* d_points, float* d_shapedirs, float* d_posedirs,
                              float* d_weights, hipStream_t s)
{
    if (d.N <= 0 || (!d_points && !d_shapedirs && !d_posedirs && !d_weights)) return FR_OK;
    LbsArgs a = lbs_args(d);
    a.g = g_xyz, a.d_points = d_points, a.d_shapedirs = d_shapedirs, a.d_posedirs = d_posedirs, a.d_weights = d_weights;
    hipLaunchKernelGGL(k_point_lbs_bwd, dim3(lbs_blocks(d.N)), dim3(kLbsThreads), 0, s, a);
    FR_HIP(hipGetLastError());
    return FR_OK;
}

// ---- gradients to the frame's pose state: a reduction over the points
// (workgroups of 1 024 threads, one per CU: the last workgroup reads one row of partials per workgroup, and four waves per SIMD
// from 256 rows cost it a quarter of what they cost from 1 024 workgroups of 256 threads)
constexpr unsigned kPoseThreads = 1024, kPoseWaves = kPoseThreads / 64;
constexpr unsigned kPoseMaxBlocks = 256;
constexpr unsigned kPoseS = (FR_LBS_MAX_E + kLbsGroup - 1) / kLbsGroup;      // 4 columns of S per lane
constexpr unsigned kPoseP = (kLbsPose * 3 + kLbsGroup - 1) / kLbsGroup;      // 7 elements of P per lane
constexpr unsigned kPoseAcc = kPoseS + kPoseP + 12;                          // a lane's running sums
constexpr unsigned kPoseOffP = kPoseS * kLbsGroup;                           // slot of P's element 0 (64)
constexpr unsigned kPoseOffT = kPoseOffP + kPoseP * kLbsGroup;               // slot of the bones' sums (176), [12][FR_LBS_MAX_J]
constexpr unsigned kPoseSlots = kPoseOffT + 12 * FR_LBS_MAX_J;               // 272 floats = 68 float4 per workgroup
// the waves' rows of sums, then — their content read — the workgroup's row and the last workgroup's runs in the same LDS
using PoseRowSums = RowSums<kPoseThreads, kPoseSlots, 4, 8>;
union PoseLds {
    float red[kPoseWaves][kPoseSlots];
    PoseRowSums sum;
};
static_assert(PoseRowSums::kChunks == 15 && PoseRowSums::kChunks < kPoseWaves && offsetof(PoseRowSums, row) == 0,
              "the row lies over wave 0's slots, the runs over the other waves'");

struct LbsPoseOut {
    float *d_betas, *d_phi, *d_A;   // [E], [36], [J,16]; any may be null
    float* partial;                 // [kPoseMaxBlocks][kPoseSlots]
    unsigned* counter;
};

// where running sum `acc` of lane `sub` lives in a row of partials (sub < FR_LBS_MAX_J for the bones' sums)
__device__ __forceinline__ unsigned pose_slot(unsigned acc, unsigned sub)
{
    return acc < kPoseS + kPoseP ? acc * kLbsGroup + sub : kPoseOffT + (acc - (kPoseS + kPoseP)) * FR_LBS_MAX_J + sub;
}

__global__ void __launch_bounds__(kPoseThreads) k_point_lbs_pose_bwd(LbsArgs a, LbsPoseOut out)
{
    __shared__ LbsShared s;
    __shared__ PoseLds lds;
    lbs_stage(a, s);
    const unsigned sub = threadIdx.x & (kLbsGroup - 1);
    const unsigned group = (blockIdx.x * blockDim.x + threadIdx.x) / kLbsGroup, n_groups = gridDim.x * blockDim.x / kLbsGroup;
    const unsigned E = (unsigned)a.E;
    float acc[kPoseAcc];
#pragma unroll
    for (unsigned t = 0; t < kPoseAcc; t++) acc[t] = 0.f;
    for (unsigned base = 0; base < (unsigned)a.N; base += n_groups) {
        const size_t i = (size_t)base + group;
        const bool live = i < (size_t)a.N;
        float wl, p[3];
        lbs_load_point(a, i, sub, live, wl, p);
        LbsPoint q;
        lbs_point(s, wl, a.J, p, q);
        const float g0 = live ? a.g[i * 3u] : 0.f, g1 = live ? a.g[i * 3u + 1] : 0.f, g2 = live ? a.g[i * 3u + 2] : 0.f;
        const float dx0 = (q.T[0] * g0 + q.T[4] * g1) + q.T[8] * g2;
        const float dx1 = (q.T[1] * g0 + q.T[5] * g1) + q.T[9] * g2;
        const float dx2 = (q.T[2] * g0 + q.T[6] * g1) + q.T[10] * g2;
        // ONE pass over the point's S and P rows serves the blendshape offset (lbs_offset's sums, in its order: x has the
        // forward's bits) and the sums of d_betas / d_pose_feature, which need d_x but not x
        float o0 = 0.f, o1 = 0.f, o2 = 0.f;
        if (live) {
            const float* __restrict__ S = a.shapedirs + i * 3u * (size_t)E;
            const float* __restrict__ P = a.posedirs + i * (size_t)(kLbsPose * 3);
#pragma unroll
            for (unsigned t = 0; t < kPoseS; t++) {
                const unsigned l = sub + t * kLbsGroup;
                if (l < E) {
                    const float b = s.dbeta[l], S0 = S[l], S1 = S[E + l], S2 = S[2u * E + l];
                    o0 += S0 * b, o1 += S1 * b, o2 += S2 * b;
                    acc[t] += (S0 * dx0 + S1 * dx1) + S2 * dx2;
                }
            }
#pragma unroll
            for (unsigned t = 0; t < kPoseP; t++) {
                const unsigned m = sub + t * kLbsGroup;
                if (m < (unsigned)(kLbsPose * 3)) {
                    const float Pm = P[m], v = Pm * s.dphi[m / 3u];
                    const unsigned k = m % 3u;
                    o0 += k == 0u ? v : 0.f, o1 += k == 1u ? v : 0.f, o2 += k == 2u ? v : 0.f;
                    acc[kPoseS + t] += Pm * (k == 0u ? dx0 : (k == 1u ? dx1 : dx2));
                }
            }
        }
        o0 = group_sum<kLbsGroup>(o0), o1 = group_sum<kLbsGroup>(o1), o2 = group_sum<kLbsGroup>(o2);
        // (the sweep's last shuffle is behind us; a dead group adds nothing: exact zeros)
        if (live && sub < (unsigned)a.J) {
            const float x0 = q.z[0] + o0, x1 = q.z[1] + o1, x2 = q.z[2] + o2;
            const float wg[3] = {wl * g0, wl * g1, wl * g2};
#pragma unroll
            for (int r = 0; r < 3; r++) {
                float* t = acc + kPoseS + kPoseP + r * 4;
                t[0] += wg[r] * x0, t[1] += wg[r] * x1, t[2] += wg[r] * x2, t[3] += wg[r];
            }
        }
    }
    // the wave's four groups in index order, then the workgroup's waves through LDS in index order
    const unsigned wave = threadIdx.x >> 6, lane = threadIdx.x & 63u;
#pragma unroll
    for (unsigned t = 0; t < kPoseAcc; t++) {
        const float v = groups_sum16(acc[t], sub);
        if (lane < kLbsGroup && (t < kPoseS + kPoseP || sub < (unsigned)FR_LBS_MAX_J)) lds.red[wave][pose_slot(t, sub)] = v;
    }
    __syncthreads();
    // the row: the waves in index order.  (It lies over wave 0's slots, which thread t alone reads, and reads first.)
    if (threadIdx.x < kPoseSlots) {
        float v = lds.red[0][threadIdx.x];
#pragma unroll
        for (unsigned w = 1; w < kPoseWaves; w++) v += lds.red[w][threadIdx.x];
        lds.sum.row[threadIdx.x] = v;
    }
    __syncthreads();
    // the launch's sums: fifteen runs of rows, one float4 column per thread, eight rows in flight
    if (!sum_rows_over_workgroups(lds.sum, out.partial, out.counter)) return;
    const float* fin = lds.sum.row;
    const unsigned t = threadIdx.x;
    if (out.d_betas && t < E) out.d_betas[t] = fin[t];
    if (out.d_phi && t < (unsigned)kLbsPose) out.d_phi[t] = (fin[kPoseOffP + 3u * t] + fin[kPoseOffP + 3u * t + 1u]) + fin[kPoseOffP + 3u * t + 2u];
    if (out.d_A && t < (unsigned)a.J * 16u) {
        const unsigned j = t / 16u, e = t % 16u;
        out.d_A[t] = e < 12u ? fin[kPoseOffT + e * FR_LBS_MAX_J + j] : 0.f;      // (the bones' last rows are constants)
    }
}

size_t point_lbs_pose_workspace_bytes()
{
    return done_workspace_bytes((size_t)kPoseMaxBlocks * kPoseSlots);
}

int launch_point_lbs_backward_pose(const fr_point_lbs& d, const float* g_xyz, float* d_betas, float* d_pose_feature, float* d_transforms,
                                   void* workspace, hipStream_t s)
{
    if (d.N <= 0) return FR_OK;
    LbsArgs a = lbs_args(d);
    a.g = g_xyz;
    LbsPoseOut out;
    out.d_betas = d_betas, out.d_phi = d_pose_feature, out.d_A = d_transforms;
    const DoneWorkspace ws = done_workspace(workspace);
    out.counter = ws.counter, out.partial = ws.partial;
    const unsigned blocks = capped_blocks((unsigned)d.N, kPoseThreads / kLbsGroup, kPoseMaxBlocks);
    hipLaunchKernelGGL(k_point_lbs_pose_bwd, dim3(blocks), dim3(kPoseThreads), 0, s, a, out);
    FR_HIP(hipGetLastError());
    return FR_OK;
}

// ---- nearest vertex
constexpr int kNvThreads = 256;
constexpr int kNvChunk = 4096;              // vertices in LDS at a time (3 x 16 KB)
static_assert(FR_NEAREST_MAX_V % kNvChunk == 0, "whole chunks");

__device__ __forceinline__ void nv_take(float px, float py, float pz, float vx, float vy, float vz, int v, float& best, int& bi)
{
    const float dx = px - vx, dy = py - vy, dz = pz - vz;
    const float d = (dx * dx + dy * dy) + dz * dz;
    if (d < best) best = d, bi = v;         // strict: a tie keeps the lower index
}

__global__ void __launch_bounds__(kNvThreads) k_nearest_vertex(int N, const float* __restrict__ points, int V,
                                                               const float* __restrict__ verts, int* __restrict__ index,
                                                               float* __restrict__ dist2)
{
    __shared__ __attribute__((aligned(16))) float sv[3][kNvChunk];
    const size_t i = (size_t)blockIdx.x * kNvThreads + threadIdx.x;
    const bool live = i < (size_t)N;
    const float px = live ? points[i * 3u] : 0.f, py = live ? points[i * 3u + 1] : 0.f, pz = live ? points[i * 3u + 2] : 0.f;
    float best = __builtin_inff();
    int bi = 0;
    for (int base = 0; base < V; base += kNvChunk) {
        const int n = V - base < kNvChunk ? V - base : kNvChunk;
        __syncthreads();                    // (the previous chunk has been read)
        for (int f = threadIdx.x; f < 3 * n; f += kNvThreads) sv[f % 3][f / 3] = verts[(size_t)base * 3u + f];
        __syncthreads();
        const int n4 = n & ~3;
        for (int v = 0; v < n4; v += 4) {
            const float4 X = *reinterpret_cast<const float4*>(&sv[0][v]);
            const float4 Y = *reinterpret_cast<const float4*>(&sv[1][v]);
            const float4 Z = *reinterpret_cast<const float4*>(&sv[2][v]);
            nv_take(px, py, pz, X.x, Y.x, Z.x, base + v, best, bi);
            nv_take(px, py, pz, X.y, Y.y, Z.y, base + v + 1, best, bi);
            nv_take(px, py, pz, X.z, Y.z, Z.z, base + v + 2, best, bi);
            nv_take(px, py, pz, X.w, Y.w, Z.w, base + v + 3, best, bi);
        }
        for (int v = n4; v < n; v++) nv_take(px, py, pz, sv[0][v], sv[1][v], sv[2][v], base + v, best, bi);
    }
    if (live) {
        index[i] = bi;
        if (dist2) dist2[i] = best;
    }
}

int launch_nearest_vertex(int N, const float* points, int V, const float* verts, int* index, float* dist2, hipStream_t s)
{
    if (N <= 0) return FR_OK;
    const unsigned blocks = ((unsigned)N + kNvThreads - 1u) / kNvThreads;
    hipLaunchKernelGGL(k_nearest_vertex, dim3(blocks), dim3(kNvThreads), 0, s, N, points, V, verts, index, dist2);
    FR_HIP(hipGetLastError());
    return FR_OK;
}

// ---- the three blendshape terms
constexpr unsigned kTermsMaxBlocks = 1024;

struct LbsTermsArgs {
    const int* index;
    const float *w, *P, *S, *gw, *gP, *gS;
    float *d_w, *d_P, *d_S;     // null: that term's loss only
    float* partial;             // [3][kTermsMaxBlocks]
    unsigned* counter;
    float* loss;
    int N, V, E, J;
    float c_w, c_P, c_S;        // weight * 2 / count
    float inv_w, inv_P, inv_S;  // 1 / count
};

// one term's share of a lane: elements sub, sub + 16, ... of a row of `len` floats
__device__ __forceinline__ float terms_row(const float* __restrict__ pred, const float* __restrict__ gt, float* grad, unsigned len,
                                           unsigned sub, float c)
{
    float acc = 0.f;
    for (unsigned m = sub; m < len; m += kLbsGroup) {
        const float d = pred[m] - gt[m];
        acc += d * d;
        if (grad) {
            const float add = c * d;
            if (add != 0.f) grad[m] += add;     // (an element that gets nothing keeps its bits, a -0 included)
        }
    }
    return acc;
}

__global__ void __launch_bounds__(kLbsThreads) k_lbs_terms(LbsTermsArgs a)
{
    static_assert(kLbsThreads == kSumThreads, "sum_over_workgroups' workgroup");
    const unsigned sub = threadIdx.x & (kLbsGroup - 1);
    const unsigned group = (blockIdx.x * blockDim.x + threadIdx.x) / kLbsGroup, n_groups = gridDim.x * blockDim.x / kLbsGroup;
    const unsigned J = (unsigned)a.J, lenP = (unsigned)(kLbsPose * 3), lenS = 3u * (unsigned)a.E;
    float acc[3] = {0.f, 0.f, 0.f};
    for (size_t i = group; i < (size_t)a.N; i += n_groups) {
        int v = a.index[i];
        v = v < 0 ? 0 : (v >= a.V ? a.V - 1 : v);
        acc[0] += terms_row(a.w + i * J, a.gw + (size_t)v * J, a.d_w ? a.d_w + i * J : nullptr, J, sub, a.c_w);
        acc[1] += terms_row(a.P + i * lenP, a.gP + (size_t)v * lenP, a.d_P ? a.d_P + i * lenP : nullptr, lenP, sub, a.c_P);
        acc[2] += terms_row(a.S + i * lenS, a.gS + (size_t)v * lenS, a.d_S ? a.d_S + i * lenS : nullptr, lenS, sub, a.c_S);
    }
    // (every lane of the workgroup arrives here: the loop above holds no shuffle)
    if (!sum_over_workgroups(acc, a.partial, kTermsMaxBlocks, a.counter, blockIdx.x, gridDim.x)) return;
    a.loss[0] = acc[0] * a.inv_w;
    a.loss[1] = acc[1] * a.inv_P;
    a.loss[2] = acc[2] * a.inv_S;
}

size_t lbs_terms_workspace_bytes() { return done_workspace_bytes(3 * kTermsMaxBlocks); }

int launch_lbs_terms(const fr_lbs_terms_config& cfg, int N, int V, int E, int J, const int* index, const float* weights,
                     const float* posedirs, const float* shapedirs, const float* gt_weights, const float* gt_posedirs,
                     const float* gt_shapedirs, float* d_weights, float* d_posedirs, float* d_shapedirs, float* loss, void* workspace,
                     hipStream_t s)
{
    if (N <= 0) return FR_OK;
    LbsTermsArgs a;
    a.index = index, a.w = weights, a.P = posedirs, a.S = shapedirs, a.gw = gt_weights, a.gP = gt_posedirs, a.gS = gt_shapedirs;
    // a weight of 0: that array is not touched at all
    a.d_w = cfg.weights_weight != 0.f ? d_weights : nullptr;
    a.d_P = cfg.posedirs_weight != 0.f ? d_posedirs : nullptr;
    a.d_S = cfg.shapedirs_weight != 0.f ? d_shapedirs : nullptr;
    const DoneWorkspace ws = done_workspace(workspace);
    a.counter = ws.counter, a.partial = ws.partial;
    a.loss = loss, a.N = N, a.V = V, a.E = E, a.J = J;
    const double n_w = (double)N * J, n_P = (double)N * (kLbsPose * 3), n_S = (double)N * 3.0 * E;
    a.c_w = (float)((double)cfg.weights_weight * 2.0 / n_w), a.inv_w = (float)(1.0 / n_w);
    a.c_P = (float)((double)cfg.posedirs_weight * 2.0 / n_P), a.inv_P = (float)(1.0 / n_P);
    a.c_S = (float)((double)cfg.shapedirs_weight * 2.0 / n_S), a.inv_S = (float)(1.0 / n_S);
    hipLaunchKernelGGL(k_lbs_terms, dim3(capped_blocks((unsigned)N, kLbsThreads / kLbsGroup, kTermsMaxBlocks)), dim3(kLbsThreads), 0, s, a);
    FR_HIP(hipGetLastError());
    return FR_OK;
}

}  // namespace fr
