// The vertex gradient of SplattingAvatar's Phong-surface binding on gfx950: what the reference gets from autograd through
// model/baseline/splattingavatar.py:203-246 (the barycentric point, verts_normals_packed, PerVertQuaternion and
// calc_face_area_change).  The arithmetic is in fr_bind_math.hpp beside the forward it differentiates; two entry points:
//
//   * k_bind_phong_frame_bwd (fr_bind_backward_phong_frame): one thread per Gaussian; the gradients of its bound values go to
//     d_verts and to the gradients of the mesh pass's three arrays at its face's corners, with float atomics into arrays the
//     caller zeroed — as the other three modes scatter dL/dverts.
//   * fr_phong_frame_backward: the backward of the mesh pass (k_phong_frame), a GATHER over the same CSR incidence list.  No
//     float atomics: the same bits on every launch and every graph replay.
//
// The mesh pass's backward is TWO launches with a [V,7] workspace, not one two-ring launch.  A face's gradient needs the
// gradients of the unnormalised sums ns_u / qs_u of all three of its corners, and each of those needs the sums themselves: the
// forward's gather over the corner's whole row.  In one launch a vertex with r faces would redo that gather for 3 r corners,
// ~r each (~100 face quaternions at r = 6, ~250 flops each, behind ~r^2 dependent index loads); with the seven values stored
// once per vertex the second launch does r face backwards per vertex.  Both launches are latency-bound at a head mesh's size
// (V = 5 023, F = 10 006: ~0.5 MB of cached gathers), so the price of the second launch is one launch gap and 28 V bytes through
// L2, which is less than the two-ring's ~r-fold longer dependent chain per thread.  The second launch recomputes a face's backward
// once per corner (3x over a per-face launch that stores nine floats): a third launch and 36 F bytes would cost more than the
// flops.  A face has no thread of its own in either launch, so the grids are sized by V alone — by 8 V lanes: a row holds 1 .. 32
// faces on the head template (mean 6), and with one lane per vertex (k_phong_frame's layout: 20 workgroups, every wave waiting for
// its longest row) the two launches took 90 + 142 us; eight lanes per row, their partial sums added in a fixed butterfly, take
// 13 + 17 us (profiles/r23_phong_vertex_grad.md) and still give the same bits on every launch.
// Built without FMA contraction like every unit that includes fr_bind_math.hpp.
#include "fr_bind_math.hpp"

namespace fr {

__global__ void __launch_bounds__(256) k_bind_phong_frame_bwd(BindArgs a, const float* g_xyz, const float* g_rot, const float* g_scale,
                                                              PhongFrameGrads o)
{
    const int n = blockIdx.x * blockDim.x + threadIdx.x;
    if (n >= a.N) return;
    float gp[3] = {0.f, 0.f, 0.f}, gq[4] = {0.f, 0.f, 0.f, 0.f}, gs[3] = {0.f, 0.f, 0.f};
    if (g_xyz)
        for (int k = 0; k < 3; k++) gp[k] = g_xyz[3 * n + k];
    if (g_rot)
        for (int k = 0; k < 4; k++) gq[k] = g_rot[4 * n + k];
    if (g_scale)
        for (int k = 0; k < 3; k++) gs[k] = g_scale[3 * n + k];
    // a Gaussian the frame dropped (culled, or non-finite: INTEGRATION.md) arrives with zero rows and adds nothing — its own
    // values may be NaN or inf, and 0 x NaN would reach every vertex of the face's two-ring through the atomics below
    if (bind_rows_all_zero(gp, gq, gs)) return;
    bind_phong_frame_bwd(a, n, gp, gq, gs, o);
}

// kRowLanes consecutive lanes share a vertex: lane l of the group takes the row's entries l, l + kRowLanes, ...; the partial
// sums meet in an xor butterfly (group_sum: 4, 2, 1), the same order on every launch, and lane 0 of the group finishes.  Every lane of a
// wave reaches the shuffles (a group past V walks an empty row).
constexpr int kRowLanes = 8;
constexpr int kVertsPerBlock = 256 / kRowLanes;

__global__ void __launch_bounds__(256) k_phong_sums_bwd(PhongFrameBwdArgs a)
{
    const int v = blockIdx.x * kVertsPerBlock + threadIdx.x / kRowLanes, lane = threadIdx.x % kRowLanes;
    Vec3 ns = {0.f, 0.f, 0.f};
    float qs[4] = {0.f, 0.f, 0.f, 0.f};
    if (v < a.V) phong_vertex_sums_partial(a, v, lane, kRowLanes, ns, qs);
    ns.x = group_sum<kRowLanes>(ns.x), ns.y = group_sum<kRowLanes>(ns.y), ns.z = group_sum<kRowLanes>(ns.z);
#pragma unroll
    for (int k = 0; k < 4; k++) qs[k] = group_sum<kRowLanes>(qs[k]);
    if (v < a.V && lane == 0) phong_vertex_sums_finish(a, v, ns, qs);
}

__global__ void __launch_bounds__(256) k_phong_gather_bwd(PhongFrameBwdArgs a)
{
    const int v = blockIdx.x * kVertsPerBlock + threadIdx.x / kRowLanes, lane = threadIdx.x % kRowLanes;
    Vec3 acc = {0.f, 0.f, 0.f};
    if (v < a.V) acc = phong_vertex_gather_partial(a, v, lane, kRowLanes);
    acc.x = group_sum<kRowLanes>(acc.x), acc.y = group_sum<kRowLanes>(acc.y), acc.z = group_sum<kRowLanes>(acc.z);
    if (v < a.V && lane == 0) phong_vertex_gather_finish(a, v, acc);
}

int launch_bind_backward_phong_frame(const fr_binding& b, const float* g_xyz, const float* g_rot, const float* g_scale, float* d_verts,
                                     float* d_vert_normals, float* d_vert_quats, float* d_face_ratio, hipStream_t s)
{
    if (b.N <= 0) return FR_OK;
    if (!d_verts && !d_vert_normals && !d_vert_quats && !d_face_ratio) return FR_OK;
    if (!g_xyz && !g_rot && !g_scale) return FR_OK;   // all zero: nothing to add
    hipLaunchKernelGGL(k_bind_phong_frame_bwd, dim3((b.N + 255) / 256), dim3(256), 0, s, bind_args(b), g_xyz, g_rot, g_scale,
                       PhongFrameGrads{d_verts, d_vert_normals, d_vert_quats, d_face_ratio});
    FR_HIP(hipGetLastError());
    return FR_OK;
}

size_t phong_frame_backward_workspace_bytes(int V) { return V > 0 ? (size_t)V * 7 * sizeof(float) : 0; }

int launch_phong_frame_backward(int V, int F, const float* verts, const float* cano_verts, const int* faces, const int* vf_offsets,
                                const int* vf_faces, const float* area_cano, const float* d_vert_normals, const float* d_vert_quats,
                                const float* d_face_ratio, float* d_verts, void* workspace, hipStream_t s)
{
    if (V <= 0 || F <= 0) return FR_OK;   // without faces no vertex has a gradient
    const PhongFrameBwdArgs a = {V, F, verts, cano_verts, faces, vf_offsets, vf_faces, area_cano, d_vert_normals, d_vert_quats,
                                 d_face_ratio, static_cast<float*>(workspace), d_verts};
    const dim3 grid((V + kVertsPerBlock - 1) / kVertsPerBlock), block(256);
    hipLaunchKernelGGL(k_phong_sums_bwd, grid, block, 0, s, a);
    hipLaunchKernelGGL(k_phong_gather_bwd, grid, block, 0, s, a);
    FR_HIP(hipGetLastError());
    return FR_OK;
}

}  // namespace fr
