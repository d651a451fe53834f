// FLAME's linear blend skinning with FateAvatar's personalised deltas (include/fr_rasterizer.h): fr_flame_forward / _backward.
//
// reference: FLAME.forward_with_delta_blendshape (flame/FLAME.py:156-204) over lbs() (flame/lbs.py:24-101) with a batch of one,
// used by model/fateavatar.py:212-223 — a few dozen small torch launches forward, twice (with and without the deltas), and
// their autograd backward.  Here, with e = expression [NE], r = pose [15], L = NS + NE:
//     v_shaped = (v_template + delta_vertex) + (S + dS)[:, :, NS:] e          (the NS shape columns meet exact zeros: not read)
//     Jnt      = J_regressor v_shaped                                          (5 x 3 sums over ALL vertices)
//     R_j      = rodrigues(r[3j : 3j + 3]),  phi = (R_1 .. R_4 - I).flatten()   (taken before I is added: fl_rodrigues)
//     v_posed  = v_shaped + phi (P + dP)
//     A        = the chain of (R_j, Jnt_j - Jnt_parent) with G_j[:3,:3] Jnt_j taken off the translation
//     verts    = (sum_j w_vj A_j) (v_posed, 1)
// and `verts_orig`, the same with every delta zero (its v_shaped differs, so it has joint sums and a chain of its own).
//
// FOUR LAUNCHES, two per direction; every sum over the vertices goes through per-workgroup partials that the workgroup which
// finishes last adds up in workgroup-index order (sum_rows_over_workgroups, fr_common.hpp: kFlThreads / slots runs of consecutive
// rows side by side, then the runs in order): no float atomics, the same bits on every launch and every graph replay.
//   k_flame_shape      a group of sixteen lanes per vertex walks the vertex's three [NE] rows of S and dS (contiguous along l) and
//                      a butterfly adds them up (fr_point_lbs.hip's layout); lane j < 5 of the group keeps joint j's three sums.
//                      The last workgroup runs Rodrigues and the chain (one thread per mesh) and leaves phi, A, and what the
//                      backward needs of the chain, in the workspace's state block.
//   k_flame_skin       a workgroup takes 64 vertices = 192 consecutive floats of the 3V axis: lane m reads posedirs [36, 3V]
//                      coalesced, v_posed goes through LDS to the 64 threads that skin one vertex each.
//   k_flame_bwd_pose   the same tiling: d_v_posed = T^T g per vertex (kept in the workspace), the rank-1 rows of d_delta_posedirs,
//                      and the 60 + 36 sums of d_A and d_phi; the last workgroup's thread 0 runs the backward of the chain and of
//                      Rodrigues: d_Jnt (to the workspace) and d_pose.
//   k_flame_bwd_shape  sixteen lanes per vertex again: d_v_shaped = d_v_posed + J_regressor^T d_Jnt, d_delta_vertex, the rank-1
//                      rows of d_delta_exp, and the NE sums of d_expression (lane `sub` owns columns sub, sub + 16, ...).
// Grids are capped at kFlMaxBlocks workgroups; the kernels stride over the rest.
//
// The workspace: [the counters of last_workgroup_of | kFlMaxBlocks rows of kFlRow partials] — zeroed once by the caller, left
// zeroed by every launch (fr_flame_workspace_zeroed_bytes) — then the frame's STATE, which a forward overwrites and the
// backward reads: kStateHead floats (phi, A, A_orig, R, the chain's rotations, Jnt, d_Jnt) and four [3V] arrays (v_shaped,
// v_shaped of the plain mesh, v_posed, d_v_posed).
// Built with the STRICT flags (no contraction).  Inputs are assumed finite.
#include "fr_common.hpp"

namespace fr {

constexpr unsigned kFlThreads = 256;
constexpr unsigned kFlGroup = 16;              // lanes per vertex in the two shape kernels
constexpr unsigned kFlMaxBlocks = 256;         // of every launch
constexpr unsigned kFlRow = 128;               // floats of a workgroup's row of partials, at most
constexpr unsigned kFlSkinVerts = 64;          // vertices per workgroup and pass of the two skinning kernels
constexpr unsigned kFlSkinElems = 3 * kFlSkinVerts;
constexpr int kFlJ = FR_FLAME_JOINTS;
constexpr int kFlPhi = FR_FLAME_POSE_FEATURES;
constexpr unsigned kFlAccE = FR_FLAME_MAX_E / kFlGroup;   // columns of S a lane owns in k_flame_bwd_shape
static_assert(kFlJ == 5 && kFlPhi == 9 * (kFlJ - 1), "the slot layouts below");
static_assert(FR_FLAME_MAX_E == kFlRow && kFlThreads == kSumThreads && kFlThreads % kFlRow == 0 && kFlThreads % 32 == 0,
              "one slot per expression column; whole runs of rows in the last workgroup");
static_assert(kFlSkinElems <= kFlThreads && kFlGroup >= kFlJ, "one lane per element / per joint");

// the state block (floats)
constexpr unsigned kStPhi = 0, kStA = 40, kStAo = 100, kStR = 160, kStGR = 208, kStJ = 256, kStDJ = 272, kStateHead = 512;
static inline size_t flame_plane(int V) { return align_up((size_t)3 * (size_t)V, 4); }

struct FlameArgs {
    int V, NS, NE;
    const int* parents;
    const float *vt, *S, *P, *Jreg, *W, *dE, *dP, *dV, *expr, *pose;
    float* state;           // kStateHead floats, then the four planes
    size_t plane;
    float* partial;
    unsigned* counter;
    float *verts, *verts_orig, *pose_feature, *transforms;                 // forward
    const float* g;                                                        // backward
    float *d_dE, *d_dP, *d_dV, *d_expr, *d_pose;
};

__device__ __forceinline__ float* fl_vshaped(const FlameArgs& a) { return a.state + kStateHead; }
__device__ __forceinline__ float* fl_vshaped_orig(const FlameArgs& a) { return a.state + kStateHead + a.plane; }
__device__ __forceinline__ float* fl_vposed(const FlameArgs& a) { return a.state + kStateHead + 2 * a.plane; }
__device__ __forceinline__ float* fl_dvposed(const FlameArgs& a) { return a.state + kStateHead + 3 * a.plane; }

// a launch's sums of kSlots <= kFlRow values, one row per workgroup: kFlThreads / kSlots whole runs of rows, 32 rows in flight
template <unsigned kSlots>
using FlRowSums = RowSums<kFlThreads, kSlots, 1, 32>;

// ---- Rodrigues and the chain, by ONE thread (their arrays live in LDS: the parents are run-time indices)
struct FlRod {
    float a[3], angle, d[3], s, c1, cosv;
    float K[9], KK[9];
};

// batch_rodrigues (flame/lbs.py:238-269): angle = |r + 1e-8|, dir = r / angle, R = I + D with D = sin K + (1 - cos) K K.
// Unlike the reference's float32, 1 - cos is taken as 2 sin^2(angle / 2) and D = R - I is handed out as it is summed, before I
// is added: below 2.4e-4 rad float32's cos rounds to 1 and 1 - cos is 0, and (I + D) - I rounds D to the spacing of 1 — up to
// 1.2e-4 relative in the pose feature and in d_pose at the rotations a tracked neck and eyes have.  So the kernel departs from
// the reference's float32 rounding TOWARDS its float64 value; the derivative below is unchanged (d(1 - cos) / d angle = sin).
__device__ __forceinline__ void fl_rodrigues(const float* r, FlRod& q, float* R, float* D)
{
#pragma unroll
    for (int k = 0; k < 3; k++) q.a[k] = r[k] + 1e-8f;
    q.angle = sqrtf((q.a[0] * q.a[0] + q.a[1] * q.a[1]) + q.a[2] * q.a[2]);
#pragma unroll
    for (int k = 0; k < 3; k++) q.d[k] = r[k] / q.angle;
    const float sh = sinf(0.5f * q.angle);
    q.s = sinf(q.angle), q.cosv = cosf(q.angle), q.c1 = 2.0f * sh * sh;
    const float x = q.d[0], y = q.d[1], z = q.d[2];
    const float K[9] = {0.f, -z, y, z, 0.f, -x, -y, x, 0.f};
#pragma unroll
    for (int e = 0; e < 9; e++) q.K[e] = K[e];
#pragma unroll
    for (int i = 0; i < 3; i++)
#pragma unroll
        for (int j = 0; j < 3; j++) q.KK[i * 3 + j] = (K[i * 3] * K[j] + K[i * 3 + 1] * K[3 + j]) + K[i * 3 + 2] * K[6 + j];
#pragma unroll
    for (int e = 0; e < 9; e++) {
        D[e] = q.s * q.K[e] + q.c1 * q.KK[e];
        R[e] = (e % 4 == 0 ? 1.f : 0.f) + D[e];
    }
}

// dLoss/dr from dLoss/dR
__device__ __forceinline__ void fl_rodrigues_bwd(const float* r, const float* dR, float* dr)
{
    FlRod q;
    float R[9], D[9];
    fl_rodrigues(r, q, R, D);
    float ds = 0.f, dc1 = 0.f;
#pragma unroll
    for (int e = 0; e < 9; e++) ds += dR[e] * q.K[e], dc1 += dR[e] * q.KK[e];
    // KK = K K:  dL/dK = s dR + c1 (dR K^T + K^T dR)
    float dK[9];
#pragma unroll
    for (int i = 0; i < 3; i++)
#pragma unroll
        for (int j = 0; j < 3; j++) {
            float m = 0.f;
#pragma unroll
            for (int k = 0; k < 3; k++) m += dR[i * 3 + k] * q.K[j * 3 + k] + q.K[k * 3 + i] * dR[k * 3 + j];
            dK[i * 3 + j] = q.s * dR[i * 3 + j] + q.c1 * m;
        }
    const float dd[3] = {dK[7] - dK[5], dK[2] - dK[6], dK[3] - dK[1]};
    const float ddr = (dd[0] * r[0] + dd[1] * r[1]) + dd[2] * r[2];
    const float dangle = (ds * q.cosv + dc1 * q.s) - ddr / (q.angle * q.angle);
#pragma unroll
    for (int k = 0; k < 3; k++) dr[k] = dd[k] / q.angle + dangle * (q.a[k] / q.angle);
}

struct FlChain {
    float R[kFlJ][9], D[kFlJ][9], GR[kFlJ][9], Gt[kFlJ][3], J[kFlJ][3];      // D = R - I, summed without I
    float dGR[kFlJ][9], dGt[kFlJ][3], dJ[kFlJ][3], dR[9], d_pose[3 * kFlJ];
    int parent[kFlJ];
};

__device__ __forceinline__ void fl_parents(const int* parents, FlChain& c)
{
    c.parent[0] = -1;
    for (int i = 1; i < kFlJ; i++) {
        const int p = parents[i];
        c.parent[i] = p < 0 ? 0 : (p >= i ? i - 1 : p);     // (the host side of the binding refuses parents[i] >= i)
    }
}

// batch_rigid_transform (flame/lbs.py:285-342) for the joints `Jnt` [5][3]: A [5][12] (rows 0 .. 2 of every 4x4)
__device__ __forceinline__ void fl_chain_forward(const FlameArgs& a, const float* Jnt, FlChain& c, float* A)
{
    fl_parents(a.parents, c);
    FlRod q;
    for (int j = 0; j < kFlJ; j++) {
        fl_rodrigues(a.pose + 3 * j, q, c.R[j], c.D[j]);
        for (int k = 0; k < 3; k++) c.J[j][k] = Jnt[j * 3 + k];
    }
    for (int e = 0; e < 9; e++) c.GR[0][e] = c.R[0][e];
    for (int k = 0; k < 3; k++) c.Gt[0][k] = c.J[0][k];
    for (int i = 1; i < kFlJ; i++) {
        const int p = c.parent[i];
        float rel[3];
        for (int k = 0; k < 3; k++) rel[k] = c.J[i][k] - c.J[p][k];
        for (int r = 0; r < 3; r++) {
            for (int col = 0; col < 3; col++)
                c.GR[i][r * 3 + col] = (c.GR[p][r * 3] * c.R[i][col] + c.GR[p][r * 3 + 1] * c.R[i][3 + col]) + c.GR[p][r * 3 + 2] * c.R[i][6 + col];
            c.Gt[i][r] = ((c.GR[p][r * 3] * rel[0] + c.GR[p][r * 3 + 1] * rel[1]) + c.GR[p][r * 3 + 2] * rel[2]) + c.Gt[p][r];
        }
    }
    for (int j = 0; j < kFlJ; j++)
        for (int r = 0; r < 3; r++) {
            for (int col = 0; col < 3; col++) A[j * 12 + r * 4 + col] = c.GR[j][r * 3 + col];
            A[j * 12 + r * 4 + 3] = c.Gt[j][r] - ((c.GR[j][r * 3] * c.J[j][0] + c.GR[j][r * 3 + 1] * c.J[j][1]) + c.GR[j][r * 3 + 2] * c.J[j][2]);
        }
}

// from dA [5][12] and d_phi [36] (`tot`: 60 + 36 floats) and the forward's R, GR, Jnt in the state block: d_Jnt and d_pose
__device__ __forceinline__ void fl_chain_backward(const FlameArgs& a, const float* tot, FlChain& c)
{
    fl_parents(a.parents, c);
    for (int j = 0; j < kFlJ; j++) {
        for (int e = 0; e < 9; e++) c.R[j][e] = a.state[kStR + j * 9 + e], c.GR[j][e] = a.state[kStGR + j * 9 + e];
        for (int k = 0; k < 3; k++) c.J[j][k] = a.state[kStJ + j * 3 + k];
    }
    for (int i = 0; i < kFlJ; i++) {
        const float* dA = tot + i * 12;
        for (int r = 0; r < 3; r++) {
            for (int col = 0; col < 3; col++) c.dGR[i][r * 3 + col] = dA[r * 4 + col] - dA[r * 4 + 3] * c.J[i][col];
            c.dGt[i][r] = dA[r * 4 + 3];
        }
        for (int col = 0; col < 3; col++)
            c.dJ[i][col] = -((c.GR[i][col] * dA[3] + c.GR[i][3 + col] * dA[7]) + c.GR[i][6 + col] * dA[11]);
    }
    float* const dR = c.dR;
    float* const d_pose = c.d_pose;
    for (int i = kFlJ - 1; i >= 0; i--) {
        if (i == 0) {
            for (int e = 0; e < 9; e++) dR[e] = c.dGR[0][e];
            for (int k = 0; k < 3; k++) c.dJ[0][k] += c.dGt[0][k];
        } else {
            const int p = c.parent[i];
            float rel[3], drel[3];
            for (int k = 0; k < 3; k++) rel[k] = c.J[i][k] - c.J[p][k];
            for (int r = 0; r < 3; r++)
                for (int col = 0; col < 3; col++)
                    dR[r * 3 + col] = ((c.GR[p][r] * c.dGR[i][col] + c.GR[p][3 + r] * c.dGR[i][3 + col]) + c.GR[p][6 + r] * c.dGR[i][6 + col]) +
                                      tot[60 + (i - 1) * 9 + r * 3 + col];
            for (int col = 0; col < 3; col++)
                drel[col] = (c.GR[p][col] * c.dGt[i][0] + c.GR[p][3 + col] * c.dGt[i][1]) + c.GR[p][6 + col] * c.dGt[i][2];
            for (int r = 0; r < 3; r++) {
                for (int col = 0; col < 3; col++)
                    c.dGR[p][r * 3 + col] += ((c.dGR[i][r * 3] * c.R[i][col * 3] + c.dGR[i][r * 3 + 1] * c.R[i][col * 3 + 1]) +
                                              c.dGR[i][r * 3 + 2] * c.R[i][col * 3 + 2]) + c.dGt[i][r] * rel[col];
                c.dGt[p][r] += c.dGt[i][r];
            }
            for (int k = 0; k < 3; k++) c.dJ[i][k] += drel[k], c.dJ[p][k] -= drel[k];
        }
        fl_rodrigues_bwd(a.pose + 3 * i, dR, d_pose + 3 * i);
    }
    for (int j = 0; j < kFlJ; j++)
        for (int k = 0; k < 3; k++) a.state[kStDJ + j * 3 + k] = c.dJ[j][k];
    if (a.d_pose)
        for (int k = 0; k < 3 * kFlJ; k++) a.d_pose[k] = d_pose[k];
}

// ---- forward, launch one: v_shaped and the joint sums; the last workgroup runs the chain
__global__ void __launch_bounds__(kFlThreads) k_flame_shape(FlameArgs a)
{
    __shared__ float s_e[FR_FLAME_MAX_E];
    __shared__ float s_red[kFlThreads / 64][32];
    __shared__ FlRowSums<32> s_sum;
    __shared__ FlChain s_chain[2];
    __shared__ float s_A[2][kFlJ * 12];
    const bool orig = a.verts_orig != nullptr;
    for (unsigned t = threadIdx.x; t < (unsigned)a.NE; t += blockDim.x) s_e[t] = a.expr[t];
    __syncthreads();
    const unsigned sub = threadIdx.x & (kFlGroup - 1);
    const unsigned group = (blockIdx.x * blockDim.x + threadIdx.x) / kFlGroup, n_groups = gridDim.x * blockDim.x / kFlGroup;
    const unsigned NE = (unsigned)a.NE;
    const size_t L = (size_t)a.NS + NE;
    float* const vs_out = fl_vshaped(a);
    float* const vo_out = fl_vshaped_orig(a);
    float aj[3] = {0.f, 0.f, 0.f}, ao[3] = {0.f, 0.f, 0.f};
    // (the trip count is the same for every lane of the launch: the shuffles run with whole waves)
    for (unsigned base = 0; base < (unsigned)a.V; base += n_groups) {
        const size_t v = (size_t)base + group;
        const bool live = v < (size_t)a.V;
        float d[3] = {0.f, 0.f, 0.f}, o[3] = {0.f, 0.f, 0.f};
        if (live) {
            for (unsigned l = sub; l < NE; l += kFlGroup) {
                const float e = s_e[l];
#pragma unroll
                for (int k = 0; k < 3; k++) {
                    const float Sv = a.S[(v * 3u + k) * L + a.NS + l];
                    const float dv = a.dE ? a.dE[(v * 3u + k) * NE + l] : 0.f;
                    d[k] += (Sv + dv) * e;
                    o[k] += Sv * e;
                }
            }
        }
#pragma unroll
        for (int k = 0; k < 3; k++) d[k] = group_sum<kFlGroup>(d[k]);
        if (orig) {
#pragma unroll
            for (int k = 0; k < 3; k++) o[k] = group_sum<kFlGroup>(o[k]);
        }
        // (the sweep's last shuffle is behind us; a dead group adds nothing)
        if (live) {
            float vs[3], vo[3];
#pragma unroll
            for (int k = 0; k < 3; k++) {
                const float t = a.vt[v * 3u + k];
                vs[k] = (t + (a.dV ? a.dV[v * 3u + k] : 0.f)) + d[k];
                vo[k] = t + o[k];
            }
            if (sub < 3u) {
                vs_out[v * 3u + sub] = sub == 0u ? vs[0] : (sub == 1u ? vs[1] : vs[2]);
                if (orig) vo_out[v * 3u + sub] = sub == 0u ? vo[0] : (sub == 1u ? vo[1] : vo[2]);
            }
            if (sub < (unsigned)kFlJ) {
                const float w = a.Jreg[(size_t)sub * (size_t)a.V + v];
#pragma unroll
                for (int k = 0; k < 3; k++) aj[k] += w * vs[k], ao[k] += w * vo[k];
            }
        }
    }
    // slots: joint j, component k of the delta mesh at j * 3 + k, of the plain mesh at 15 + j * 3 + k
    const unsigned wave = threadIdx.x >> 6, lane = threadIdx.x & 63u;
#pragma unroll
    for (int k = 0; k < 3; k++) {
        const float x = groups_sum16(aj[k], sub), y = groups_sum16(ao[k], sub);
        if (lane < (unsigned)kFlJ) s_red[wave][lane * 3u + k] = x, s_red[wave][15u + lane * 3u + k] = orig ? y : 0.f;
    }
    if (lane >= 30u && lane < 32u) s_red[wave][lane] = 0.f;
    __syncthreads();
    if (threadIdx.x < 32u) s_sum.row[threadIdx.x] = ((s_red[0][threadIdx.x] + s_red[1][threadIdx.x]) + s_red[2][threadIdx.x]) + s_red[3][threadIdx.x];
    __syncthreads();
    if (!sum_rows_over_workgroups(s_sum, a.partial, a.counter)) return;
    const unsigned which = threadIdx.x >> 6;       // wave 0's first lane: the delta mesh; wave 1's: the plain one
    if (lane != 0u || which > (orig ? 1u : 0u)) return;
    FlChain& c = s_chain[which];
    fl_chain_forward(a, s_sum.row + 15u * which, c, s_A[which]);
    float* const A_out = a.state + (which ? kStAo : kStA);
    for (int e = 0; e < kFlJ * 12; e++) A_out[e] = s_A[which][e];
    if (which) return;
    for (int j = 0; j < kFlJ; j++) {
        for (int e = 0; e < 9; e++) a.state[kStR + j * 9 + e] = c.R[j][e], a.state[kStGR + j * 9 + e] = c.GR[j][e];
        for (int k = 0; k < 3; k++) a.state[kStJ + j * 3 + k] = c.J[j][k];
    }
    for (int i = 0; i < kFlPhi; i++) {
        const float phi = c.D[1 + i / 9][i % 9];
        a.state[kStPhi + i] = phi;
        if (a.pose_feature) a.pose_feature[i] = phi;
    }
    if (a.transforms)
        for (int j = 0; j < kFlJ; j++)
            for (int e = 0; e < 16; e++) a.transforms[j * 16 + e] = e < 12 ? s_A[0][j * 12 + e] : (e == 15 ? 1.f : 0.f);
}

// T = sum_j w_j A_j (rows 0 .. 2), the joints in ascending order
__device__ __forceinline__ void fl_blend(const float* __restrict__ w, const float* A, float T[12])
{
#pragma unroll
    for (int e = 0; e < 12; e++) T[e] = w[0] * A[e];
#pragma unroll
    for (int j = 1; j < kFlJ; j++)
#pragma unroll
        for (int e = 0; e < 12; e++) T[e] += w[j] * A[j * 12 + e];
}

// ---- forward, launch two: the pose offsets and the skinning
__global__ void __launch_bounds__(kFlThreads) k_flame_skin(FlameArgs a)
{
    __shared__ float s_phi[kFlPhi];
    __shared__ float s_A[2][kFlJ * 12];
    __shared__ float s_vp[2][kFlSkinElems];
    const bool orig = a.verts_orig != nullptr;
    const unsigned t = threadIdx.x;
    if (t < (unsigned)kFlPhi) s_phi[t] = a.state[kStPhi + t];
    if (t < (unsigned)kFlJ * 12u) s_A[0][t] = a.state[kStA + t], s_A[1][t] = orig ? a.state[kStAo + t] : 0.f;
    __syncthreads();
    const size_t n3 = (size_t)3 * (size_t)a.V;
    const float* const vs = fl_vshaped(a);
    const float* const vo = fl_vshaped_orig(a);
    float* const vp_out = fl_vposed(a);
    for (size_t first = (size_t)blockIdx.x * kFlSkinVerts; first < (size_t)a.V; first += (size_t)gridDim.x * kFlSkinVerts) {
        const size_t m = first * 3u + t;
        if (t < kFlSkinElems && m < n3) {
            float off = 0.f, offo = 0.f;
#pragma unroll 6
            for (int i = 0; i < kFlPhi; i++) {
                const float p = a.P[(size_t)i * n3 + m];
                off += s_phi[i] * (p + (a.dP ? a.dP[(size_t)i * n3 + m] : 0.f));
                offo += s_phi[i] * p;
            }
            const float vp = vs[m] + off;
            s_vp[0][t] = vp;
            vp_out[m] = vp;
            if (orig) s_vp[1][t] = vo[m] + offo;
        }
        __syncthreads();
        const size_t v = first + t;
        if (t < kFlSkinVerts && v < (size_t)a.V) {
            const float* __restrict__ w = a.W + v * (size_t)kFlJ;
            float T[12];
            fl_blend(w, s_A[0], T);
            const float x = s_vp[0][3u * t], y = s_vp[0][3u * t + 1u], z = s_vp[0][3u * t + 2u];
#pragma unroll
            for (int r = 0; r < 3; r++) a.verts[v * 3u + r] = ((T[r * 4] * x + T[r * 4 + 1] * y) + T[r * 4 + 2] * z) + T[r * 4 + 3];
            if (orig) {
                fl_blend(w, s_A[1], T);
                const float xo = s_vp[1][3u * t], yo = s_vp[1][3u * t + 1u], zo = s_vp[1][3u * t + 2u];
#pragma unroll
                for (int r = 0; r < 3; r++)
                    a.verts_orig[v * 3u + r] = ((T[r * 4] * xo + T[r * 4 + 1] * yo) + T[r * 4 + 2] * zo) + T[r * 4 + 3];
            }
        }
        __syncthreads();     // (the next pass overwrites s_vp)
    }
}

// ---- backward, launch one: d_v_posed, d_delta_posedirs, the sums of d_A and d_phi; the last workgroup: d_Jnt and d_pose
__global__ void __launch_bounds__(kFlThreads) k_flame_bwd_pose(FlameArgs a)
{
    __shared__ float s_phi[kFlPhi];
    __shared__ float s_A[kFlJ * 12];
    __shared__ float s_dvp[kFlSkinElems];
    __shared__ float s_red[kFlThreads / 64][kFlPhi];
    __shared__ FlRowSums<kFlRow> s_sum;
    __shared__ FlChain s_chain;
    const unsigned t = threadIdx.x;
    if (t < (unsigned)kFlPhi) s_phi[t] = a.state[kStPhi + t];
    if (t < (unsigned)kFlJ * 12u) s_A[t] = a.state[kStA + t];
    __syncthreads();
    const size_t n3 = (size_t)3 * (size_t)a.V;
    const float* const vp_in = fl_vposed(a);
    float* const dvp_out = fl_dvposed(a);
    float accA[kFlJ * 12], accP[kFlPhi];
#pragma unroll
    for (int e = 0; e < kFlJ * 12; e++) accA[e] = 0.f;
#pragma unroll
    for (int i = 0; i < kFlPhi; i++) accP[i] = 0.f;
    for (size_t first = (size_t)blockIdx.x * kFlSkinVerts; first < (size_t)a.V; first += (size_t)gridDim.x * kFlSkinVerts) {
        const size_t v = first + t;
        if (t < kFlSkinVerts) {
            float dvp[3] = {0.f, 0.f, 0.f};
            if (v < (size_t)a.V) {
                const float* __restrict__ w = a.W + v * (size_t)kFlJ;
                float T[12];
                fl_blend(w, s_A, T);
                const float g[3] = {a.g[v * 3u], a.g[v * 3u + 1u], a.g[v * 3u + 2u]};
                const float vp[3] = {vp_in[v * 3u], vp_in[v * 3u + 1u], vp_in[v * 3u + 2u]};
#pragma unroll
                for (int col = 0; col < 3; col++) {
                    dvp[col] = (T[col] * g[0] + T[4 + col] * g[1]) + T[8 + col] * g[2];
                    dvp_out[v * 3u + col] = dvp[col];
                }
#pragma unroll
                for (int j = 0; j < kFlJ; j++)
#pragma unroll
                    for (int r = 0; r < 3; r++) {
                        const float wg = w[j] * g[r];
                        float* acc = accA + j * 12 + r * 4;
                        acc[0] += wg * vp[0], acc[1] += wg * vp[1], acc[2] += wg * vp[2], acc[3] += wg;
                    }
            }
#pragma unroll
            for (int col = 0; col < 3; col++) s_dvp[3u * t + col] = dvp[col];
        }
        __syncthreads();
        const size_t m = first * 3u + t;
        if (t < kFlSkinElems && m < n3) {
            const float d = s_dvp[t];
#pragma unroll       // (whole: accP stays in registers)
            for (int i = 0; i < kFlPhi; i++) {
                const float p = a.P[(size_t)i * n3 + m] + (a.dP ? a.dP[(size_t)i * n3 + m] : 0.f);
                accP[i] += p * d;
                if (a.d_dP) a.d_dP[(size_t)i * n3 + m] = s_phi[i] * d;
            }
        }
        __syncthreads();     // (the next pass overwrites s_dvp)
    }
    // slots: d_A at j * 12 + r * 4 + c (wave 0 alone holds them), d_phi at 60 + i (the waves in index order)
    const unsigned wave = t >> 6, lane = t & 63u;
#pragma unroll
    for (int e = 0; e < kFlJ * 12; e++) {
        const float x = wave_sum(accA[e]);
        if (t == 0u) s_sum.row[e] = x;
    }
#pragma unroll
    for (int i = 0; i < kFlPhi; i++) {
        const float x = wave_sum(accP[i]);
        if (lane == 0u) s_red[wave][i] = x;
    }
    if (t >= 96u && t < kFlRow) s_sum.row[t] = 0.f;
    __syncthreads();
    if (t < (unsigned)kFlPhi) s_sum.row[60u + t] = ((s_red[0][t] + s_red[1][t]) + s_red[2][t]) + s_red[3][t];
    __syncthreads();
    if (!sum_rows_over_workgroups(s_sum, a.partial, a.counter)) return;
    if (t == 0u) fl_chain_backward(a, s_sum.row, s_chain);
}

// ---- backward, launch two: d_v_shaped, d_delta_vertex, d_delta_exp and the sums of d_expression
__global__ void __launch_bounds__(kFlThreads) k_flame_bwd_shape(FlameArgs a)
{
    __shared__ float s_e[FR_FLAME_MAX_E];
    __shared__ float s_dJ[kFlJ * 3];
    __shared__ float s_red[kFlThreads / 64][kFlRow];
    __shared__ FlRowSums<kFlRow> s_sum;
    for (unsigned t = threadIdx.x; t < (unsigned)FR_FLAME_MAX_E; t += blockDim.x) s_e[t] = t < (unsigned)a.NE ? a.expr[t] : 0.f;
    if (threadIdx.x < (unsigned)kFlJ * 3u) s_dJ[threadIdx.x] = a.state[kStDJ + threadIdx.x];
    __syncthreads();
    const unsigned sub = threadIdx.x & (kFlGroup - 1);
    const unsigned group = (blockIdx.x * blockDim.x + threadIdx.x) / kFlGroup, n_groups = gridDim.x * blockDim.x / kFlGroup;
    const unsigned NE = (unsigned)a.NE;
    const size_t L = (size_t)a.NS + NE;
    const float* const dvp_in = fl_dvposed(a);
    float acc[kFlAccE];
#pragma unroll
    for (unsigned q = 0; q < kFlAccE; q++) acc[q] = 0.f;
    for (size_t v = group; v < (size_t)a.V; v += n_groups) {
        float dvs[3];
#pragma unroll
        for (int k = 0; k < 3; k++) {
            float jr = a.Jreg[v] * s_dJ[k];
#pragma unroll
            for (int j = 1; j < kFlJ; j++) jr += a.Jreg[(size_t)j * (size_t)a.V + v] * s_dJ[j * 3 + k];
            dvs[k] = dvp_in[v * 3u + k] + jr;
        }
        if (a.d_dV && sub < 3u) a.d_dV[v * 3u + sub] = sub == 0u ? dvs[0] : (sub == 1u ? dvs[1] : dvs[2]);
#pragma unroll
        for (unsigned q = 0; q < kFlAccE; q++) {
            const unsigned l = sub + q * kFlGroup;
            if (l < NE) {
                const float e = s_e[l];
                float Sk[3];
#pragma unroll
                for (int k = 0; k < 3; k++) {
                    Sk[k] = a.S[(v * 3u + k) * L + a.NS + l] + (a.dE ? a.dE[(v * 3u + k) * NE + l] : 0.f);
                    if (a.d_dE) a.d_dE[(v * 3u + k) * NE + l] = dvs[k] * e;
                }
                acc[q] += (Sk[0] * dvs[0] + Sk[1] * dvs[1]) + Sk[2] * dvs[2];
            }
        }
    }
    // (every lane of the workgroup arrives here: the loop above holds no shuffle)
    const unsigned wave = threadIdx.x >> 6, lane = threadIdx.x & 63u;
#pragma unroll
    for (unsigned q = 0; q < kFlAccE; q++) {
        const float x = groups_sum16(acc[q], sub);
        if (lane < kFlGroup) s_red[wave][q * kFlGroup + sub] = x;
    }
    __syncthreads();
    if (threadIdx.x < kFlRow)
        s_sum.row[threadIdx.x] = ((s_red[0][threadIdx.x] + s_red[1][threadIdx.x]) + s_red[2][threadIdx.x]) + s_red[3][threadIdx.x];
    __syncthreads();
    if (!sum_rows_over_workgroups(s_sum, a.partial, a.counter)) return;
    if (a.d_expr && threadIdx.x < NE) a.d_expr[threadIdx.x] = s_sum.row[threadIdx.x];
}

// ---- host side
size_t flame_workspace_zeroed_bytes() { return done_workspace_bytes((size_t)kFlMaxBlocks * kFlRow); }

size_t flame_workspace_bytes(int V, int NE)
{
    (void)NE;      // (the rows of partials are FR_FLAME_MAX_E wide whatever NE is)
    return flame_workspace_zeroed_bytes() + (kStateHead + 4 * flame_plane(V < 0 ? 0 : V)) * sizeof(float);
}

static FlameArgs flame_args(const fr_flame& f, void* workspace)
{
    FlameArgs a = {};
    a.V = f.V, a.NS = f.NS, a.NE = f.NE;
    a.parents = f.parents;
    a.vt = f.v_template, a.S = f.shapedirs, a.P = f.posedirs, a.Jreg = f.J_regressor, a.W = f.lbs_weights;
    a.dE = f.delta_exp, a.dP = f.delta_posedirs, a.dV = f.delta_vertex, a.expr = f.expression, a.pose = f.pose;
    const DoneWorkspace ws = done_workspace(workspace);
    a.counter = ws.counter, a.partial = ws.partial;
    a.state = reinterpret_cast<float*>(static_cast<char*>(workspace) + flame_workspace_zeroed_bytes());
    a.plane = flame_plane(f.V);
    return a;
}

int launch_flame_forward(const fr_flame& f, float* verts, float* verts_orig, float* pose_feature, float* transforms, void* workspace,
                         hipStream_t s)
{
    if (f.V <= 0) return FR_OK;
    FlameArgs a = flame_args(f, workspace);
    a.verts = verts, a.verts_orig = verts_orig, a.pose_feature = pose_feature, a.transforms = transforms;
    hipLaunchKernelGGL(k_flame_shape, dim3(capped_blocks((unsigned)f.V, kFlThreads / kFlGroup, kFlMaxBlocks)), dim3(kFlThreads), 0, s, a);
    FR_HIP(hipGetLastError());
    hipLaunchKernelGGL(k_flame_skin, dim3(capped_blocks((unsigned)f.V, kFlSkinVerts, kFlMaxBlocks)), dim3(kFlThreads), 0, s, a);
    FR_HIP(hipGetLastError());
    return FR_OK;
}

int launch_flame_backward(const fr_flame& f, const float* g_verts, float* d_delta_exp, float* d_delta_posedirs, float* d_delta_vertex,
                          float* d_expression, float* d_pose, void* workspace, hipStream_t s)
{
    if (f.V <= 0) return FR_OK;
    FlameArgs a = flame_args(f, workspace);
    a.g = g_verts, a.d_dE = d_delta_exp, a.d_dP = d_delta_posedirs, a.d_dV = d_delta_vertex, a.d_expr = d_expression, a.d_pose = d_pose;
    hipLaunchKernelGGL(k_flame_bwd_pose, dim3(capped_blocks((unsigned)f.V, kFlSkinVerts, kFlMaxBlocks)), dim3(kFlThreads), 0, s, a);
    FR_HIP(hipGetLastError());
    hipLaunchKernelGGL(k_flame_bwd_shape, dim3(capped_blocks((unsigned)f.V, kFlThreads / kFlGroup, kFlMaxBlocks)), dim3(kFlThreads), 0, s, a);
    FR_HIP(hipGetLastError());
    return FR_OK;
}

}  // namespace fr
