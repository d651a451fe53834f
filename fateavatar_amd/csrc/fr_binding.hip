// FateAvatar's mesh binding on gfx950: the step right before the rasterizer.
//
// reference: model/fateavatar.py:225-258 — per frame, every Gaussian n bound to face f = face_index[n] with
// barycentrics bary[n] gets
//     xyz      = sum_k bary_k v_k + (e1 x e2) * shell_len * tanh(offset_n)          (:236-241, :258; the normal is NOT normalised)
//     rotation = standardize(q_face (x) rotation_n),  q_face = matrix_to_quaternion([a0 a1 a2])   (:231-232, :257)
//     scaling  = scaling_n + log(face_scale / face_scale_canonical)                 (:228-229, :256)
// with the face frame / scale of volume_rendering/mesh_compute.py:36-59 and pytorch3d 0.7.7's quaternion conversion
// and product.  The reference evaluates this as ~40 PyTorch kernels over [F] and [N] temporaries (plus their autograd
// twins); here ONE kernel per direction, one thread per Gaussian, recomputing the ~150 flops of its face's frame
// instead of gathering per-face temporaries.  The same two kernels serve GaussianAvatars' face-local binding
// (fr_binding::mode == FR_BIND_FACE_LOCAL, model/baseline/gaussianavatars.py:144-171) and SplattingAvatar's Phong-surface
// binding (FR_BIND_PHONG, model/baseline/splattingavatar.py:224-246; its per-frame mesh pass is k_phong_frame) and FlashAvatar's
// MLP-deformed binding (FR_BIND_DEFORM, model/baseline/flashavatar.py:242-276; no face frame): the mode is a
// kernel argument.  The backward scatters dL/dverts with float atomics (a vertex is shared
// by the Gaussians of ~6 faces x ~10 Gaussians each).  Built without FMA contraction, in the oracle's operation order.
#include "fr_bind_math.hpp"

namespace fr {

__global__ void __launch_bounds__(256) k_bind_fwd(BindArgs a, float* xyz, float* rot_out, float* scale_out)
{
    const int n = blockIdx.x * blockDim.x + threadIdx.x;
    if (n >= a.N) return;
    float p[3], q[4], s[3];
    bind_fwd(a, n, p, q, s);
    for (int k = 0; k < 3; k++) xyz[3 * n + k] = p[k];
    for (int k = 0; k < 4; k++) rot_out[4 * n + k] = q[k];
    for (int k = 0; k < 3; k++) scale_out[3 * n + k] = s[k];
}

__global__ void __launch_bounds__(256) k_bind_bwd(BindArgs a, const float* g_xyz, const float* g_rot, const float* g_scale,
                                                  BindGrads o)
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
    // a Gaussian the frame dropped (culled, or non-finite: INTEGRATION.md) arrives with zero rows: zero rows out and nothing
    // for the vertices, as preprocess_bwd_one does inside the frame — 0 x its own NaN or inf must not reach d_verts
    if (bind_rows_all_zero(gp, gq, gs)) {
        bind_bwd_zero(a, n, o);
        return;
    }
    bind_bwd(a, n, gp, gq, gs, o);
}

// per-face scale of a mesh (the canonical one, computed once): mesh_compute.py:51-56
__global__ void __launch_bounds__(256) k_face_scale(int F, const float* verts, const int* faces, float* out)
{
    const int fi = blockIdx.x * blockDim.x + threadIdx.x;
    if (fi >= F) return;
    const FaceFrame f = face_frame(load3(verts, faces[3 * fi]), load3(verts, faces[3 * fi + 1]), load3(verts, faces[3 * fi + 2]));
    out[fi] = f.scale;
}

// SplattingAvatar's per-frame mesh pass (model/baseline/splattingavatar.py:203-215, PerVertQuaternion :819-902) in ONE launch:
// thread i writes face i's area ratio (i < F) and gathers vertex i's normal and quaternion over its faces (i < V)
__global__ void __launch_bounds__(256) k_phong_frame(PhongFrameArgs a)
{
    const int i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i < a.F) {
        const int i0 = a.faces[3 * i], i1 = a.faces[3 * i + 1], i2 = a.faces[3 * i + 2];
        a.face_ratio[i] = phong_face_ratio(load3(a.verts, i0), load3(a.verts, i1), load3(a.verts, i2), a.area_cano[i]);
    }
    if (i < a.V) phong_vertex(a, i);
}

BindArgs bind_args(const fr_binding& b)
{
    BindArgs a;
    a.N = b.N, a.verts = b.verts, a.faces = b.faces, a.face_index = b.face_index, a.bary = b.bary;
    a.canon = b.face_scale_canonical, a.shell_len = b.shell_len, a.resize_scale = b.resize_scale;
    a.offset = b.offset, a.rotation = b.rotation, a.scaling = b.scaling;
    a.mode = b.mode, a.local_xyz = b.local_xyz;
    a.vert_normals = a.vert_quats = a.face_ratio = nullptr;
    if (b.mode == FR_BIND_PHONG) {   // (the descriptor is the `base` of a fr_binding_phong: include/fr_rasterizer.h)
        const fr_binding_phong& p = reinterpret_cast<const fr_binding_phong&>(b);
        a.vert_normals = p.vert_normals, a.vert_quats = p.vert_quats, a.face_ratio = p.face_ratio;
    }
    return a;
}

int launch_bind_forward(const fr_binding& b, float* xyz, float* rot, float* scale, hipStream_t s)
{
    if (b.N <= 0) return FR_OK;
    hipLaunchKernelGGL(k_bind_fwd, dim3((b.N + 255) / 256), dim3(256), 0, s, bind_args(b), xyz, rot, scale);
    FR_HIP(hipGetLastError());
    return FR_OK;
}

int launch_bind_backward(const fr_binding& b, const float* g_xyz, const float* g_rot, const float* g_scale, float* d_verts,
                         float* d_offset, float* d_rotation, float* d_scaling, float* d_local_xyz, hipStream_t s)
{
    if (b.N <= 0) return FR_OK;
    hipLaunchKernelGGL(k_bind_bwd, dim3((b.N + 255) / 256), dim3(256), 0, s, bind_args(b), g_xyz, g_rot, g_scale,
                       BindGrads{d_verts, d_offset, d_rotation, d_scaling, d_local_xyz});
    FR_HIP(hipGetLastError());
    return FR_OK;
}

int launch_phong_frame(int V, int F, const float* verts, const float* cano_verts, const int* faces, const int* vf_offsets,
                       const int* vf_faces, const float* area_cano, float* vert_normals, float* vert_quats, float* face_ratio,
                       hipStream_t s)
{
    const int n = V > F ? V : F;
    if (n <= 0) return FR_OK;
    const PhongFrameArgs a = {V, F, verts, cano_verts, faces, vf_offsets, vf_faces, area_cano, vert_normals, vert_quats, face_ratio};
    hipLaunchKernelGGL(k_phong_frame, dim3((n + 255) / 256), dim3(256), 0, s, a);
    FR_HIP(hipGetLastError());
    return FR_OK;
}

int launch_face_scale(int F, const float* verts, const int* faces, float* out, hipStream_t s)
{
    if (F <= 0) return FR_OK;
    hipLaunchKernelGGL(k_face_scale, dim3((F + 255) / 256), dim3(256), 0, s, F, verts, faces, out);
    FR_HIP(hipGetLastError());
    return FR_OK;
}

}  // namespace fr
