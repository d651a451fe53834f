// FateAvatar's mesh binding, per Gaussian: the arithmetic shared by the stand-alone binding kernels
// (fr_binding.hip) and by the per-Gaussian kernels of the rasterizer when a frame is rendered straight from its binding
// (fr_aux::binding: fr_preprocess.hip evaluates bind_one_fwd in front of its own work, fr_preprocess_bwd.hip continues
// through bind_one_bwd).  One source of the expressions = the same bits on both routes.
//
// reference: model/fateavatar.py:225-258 with volume_rendering/mesh_compute.py:27-59 and pytorch3d 0.7.7's
// matrix_to_quaternion / quaternion_multiply / standardize_quaternion.  Every translation unit that includes this is
// built with -ffp-contract=off: the expressions are in the oracle's operation order.
//
// Four bindings share the quaternion code (BindArgs::mode, the same for every Gaussian of a launch):
//   FR_BIND_SHELL       FateAvatar's own: barycentric point + shell offset along the face normal (bind_one_fwd / _bwd)
//   FR_BIND_FACE_LOCAL  GaussianAvatars': a free position in the face's local frame (bind_local_fwd / _bwd;
//                       model/baseline/gaussianavatars.py:144-171)
//   FR_BIND_PHONG       SplattingAvatar's: a point of the posed mesh's Phong surface (bind_phong_fwd / _bwd;
//                       model/baseline/splattingavatar.py:224-246) from the per-vertex normals / quaternions and per-face
//                       area ratios that phong_vertex / phong_face_ratio (below; fr_phong_frame) compute once per frame
//   FR_BIND_DEFORM      FlashAvatar's: barycentric point + the ten outputs of the caller's deformation MLP for this frame
//                       (bind_deform_fwd / _bwd; model/baseline/flashavatar.py:242-276, :380-390): no face frame at all
// bind_fwd / bind_bwd pick by the mode; the kernels call those (and bind_bwd_zero for a Gaussian without a gradient, which
// learns the width of the mode's own gradient row from bind_own_cols).
#pragma once
#include "fr_common.hpp"

namespace fr {

struct BindArgs {
    int N;
    const float* verts;       // [V,3]
    const int* faces;         // [F,3]
    const int* face_index;    // [N]
    const float* bary;        // [N,3]
    const float* canon;       // [F] face scale of the canonical mesh
    float shell_len;
    int resize_scale;
    const float* offset;      // [N]
    const float* rotation;    // [N,4]
    const float* scaling;     // [N,3]
    int mode;                 // FR_BIND_SHELL / _FACE_LOCAL / _PHONG / _DEFORM (wave-uniform: a kernel argument)
    const float* local_xyz;   // [N,3] FR_BIND_FACE_LOCAL: position in the face's frame (bary .. offset are not read);
                              //       FR_BIND_PHONG: uvd (only column 2, the offset along the normal, is read);
                              // [N,10] FR_BIND_DEFORM: the RAW outputs of the deformation MLP (canon .. offset are not read)
    const float* vert_normals;  // [V,3] FR_BIND_PHONG (fr_binding_phong's tail): fr_phong_frame's outputs for the posed mesh
    const float* vert_quats;    // [V,4]
    const float* face_ratio;    // [F]
};

struct Vec3 {
    float x, y, z;
};
__device__ __forceinline__ Vec3 sub(Vec3 a, Vec3 b) { return {a.x - b.x, a.y - b.y, a.z - b.z}; }
__device__ __forceinline__ Vec3 add(Vec3 a, Vec3 b) { return {a.x + b.x, a.y + b.y, a.z + b.z}; }
__device__ __forceinline__ Vec3 mul(Vec3 a, float s) { return {a.x * s, a.y * s, a.z * s}; }
__device__ __forceinline__ float dot3(Vec3 a, Vec3 b) { return a.x * b.x + a.y * b.y + a.z * b.z; }
__device__ __forceinline__ Vec3 cross3(Vec3 a, Vec3 b) { return {a.y * b.z - a.z * b.y, a.z * b.x - a.x * b.z, a.x * b.y - a.y * b.x}; }
__device__ __forceinline__ Vec3 load3(const float* p, size_t i) { return {p[3 * i], p[3 * i + 1], p[3 * i + 2]}; }

constexpr float kLenEps = 1e-20f;  // mesh_compute.py:17

// x / sqrt(max(x.x, eps)); `clamped` tells the backward that the length did not depend on x
__device__ __forceinline__ Vec3 safe_normalize(Vec3 x, float& len, bool& clamped)
{
    const float d = dot3(x, x);
    clamped = !(d > kLenEps);
    len = sqrtf(fmaxf(d, kLenEps));
    return {x.x / len, x.y / len, x.z / len};
}
// gradient of y = x / len w.r.t. x
__device__ __forceinline__ Vec3 safe_normalize_bwd(Vec3 g, Vec3 y, float len, bool clamped)
{
    if (clamped) return {g.x / len, g.y / len, g.z / len};
    const float t = dot3(y, g);
    return {(g.x - y.x * t) / len, (g.y - y.y * t) / len, (g.z - y.z * t) / len};
}

struct FaceFrame {
    Vec3 e1, e2, a0, a1, a2, c1, c2;
    float l1, lc1, lc2, d, scale;
    bool k1, kc1, kc2;  // clamps
};

__device__ __forceinline__ FaceFrame face_frame(Vec3 v0, Vec3 v1, Vec3 v2)
{
    FaceFrame f;
    f.e1 = sub(v1, v0), f.e2 = sub(v2, v0);
    f.a0 = safe_normalize(f.e1, f.l1, f.k1);
    f.c1 = cross3(f.a0, f.e2);
    f.a1 = safe_normalize(f.c1, f.lc1, f.kc1);
    f.c2 = cross3(f.a1, f.a0);
    const Vec3 y = safe_normalize(f.c2, f.lc2, f.kc2);
    f.a2 = {-y.x, -y.y, -y.z};
    f.d = dot3(f.a2, f.e2);
    f.scale = (f.l1 + fabsf(f.d)) / 2.0f;
    return f;
}

// pytorch3d matrix_to_quaternion of R = [a0 a1 a2] (columns); returns the selected candidate index and sign
struct QuatSel {
    float q[4];
    float num[4], den, qa;
    int sel;
    float sgn;
};
__device__ __forceinline__ QuatSel frame_to_quaternion(Vec3 a0, Vec3 a1, Vec3 a2)
{
    const float m00 = a0.x, m10 = a0.y, m20 = a0.z;
    const float m01 = a1.x, m11 = a1.y, m21 = a1.z;
    const float m02 = a2.x, m12 = a2.y, m22 = a2.z;
    const float x[4] = {1.0f + m00 + m11 + m22, 1.0f + m00 - m11 - m22, 1.0f - m00 + m11 - m22, 1.0f - m00 - m11 + m22};
    float qa[4];
    int sel = 0;
    for (int k = 0; k < 4; k++) {
        qa[k] = x[k] > 0.f ? sqrtf(x[k]) : 0.f;
        if (qa[k] > qa[sel]) sel = k;
    }
    QuatSel s;
    s.sel = sel, s.qa = qa[sel];
    const float diag = qa[sel] * qa[sel];
    switch (sel) {
        case 0: s.num[0] = diag, s.num[1] = m21 - m12, s.num[2] = m02 - m20, s.num[3] = m10 - m01; break;
        case 1: s.num[0] = m21 - m12, s.num[1] = diag, s.num[2] = m10 + m01, s.num[3] = m02 + m20; break;
        case 2: s.num[0] = m02 - m20, s.num[1] = m10 + m01, s.num[2] = diag, s.num[3] = m12 + m21; break;
        default: s.num[0] = m10 - m01, s.num[1] = m20 + m02, s.num[2] = m21 + m12, s.num[3] = diag; break;
    }
    s.den = 2.0f * fmaxf(qa[sel], 0.1f);
    for (int k = 0; k < 4; k++) s.q[k] = s.num[k] / s.den;
    s.sgn = s.q[0] < 0.f ? -1.f : 1.f;
    for (int k = 0; k < 4; k++) s.q[k] *= s.sgn;
    return s;
}
__device__ __forceinline__ QuatSel frame_to_quaternion(const FaceFrame& f) { return frame_to_quaternion(f.a0, f.a1, f.a2); }

// the Hamilton product a (x) b as it comes, sign kept: the sixteen products every binding's rotation is made of
// (FlashAvatar's quatProduct_batch, model/baseline/flashavatar.py:380-390, is exactly this)
__device__ __forceinline__ void quat_product(const float a[4], const float b[4], float o[4])
{
    const float aw = a[0], ax = a[1], ay = a[2], az = a[3];
    const float bw = b[0], bx = b[1], by = b[2], bz = b[3];
    o[0] = aw * bw - ax * bx - ay * by - az * bz, o[1] = aw * bx + ax * bw + ay * bz - az * by;
    o[2] = aw * by - ax * bz + ay * bw + az * bx, o[3] = aw * bz + ax * by - ay * bx + az * bw;
}
// its gradient: dL/d(o) in, dL/da and dL/db out
__device__ __forceinline__ void quat_product_bwd(const float a[4], const float b[4], const float g[4], float da[4], float db[4])
{
    const float aw = a[0], ax = a[1], ay = a[2], az = a[3];
    const float bw = b[0], bx = b[1], by = b[2], bz = b[3];
    const float gw = g[0], gx = g[1], gy = g[2], gz = g[3];
    db[0] = gw * aw + gx * ax + gy * ay + gz * az;
    db[1] = -gw * ax + gx * aw + gy * az - gz * ay;
    db[2] = -gw * ay - gx * az + gy * aw + gz * ax;
    db[3] = -gw * az + gx * ay - gy * ax + gz * aw;
    da[0] = gw * bw + gx * bx + gy * by + gz * bz;
    da[1] = -gw * bx + gx * bw - gy * bz + gz * by;
    da[2] = -gw * by + gx * bz + gy * bw - gz * bx;
    da[3] = -gw * bz - gx * by + gy * bx + gz * bw;
}
// pytorch3d quaternion_multiply: the product with the real part made non-negative
__device__ __forceinline__ void quat_multiply(const float a[4], const float b[4], float out[4])
{
    float o[4];
    quat_product(a, b, o);
    const float sg = o[0] < 0.f ? -1.f : 1.f;
    for (int k = 0; k < 4; k++) out[k] = sg * o[k];
}
// its gradient: dL/d(out) in, dL/da and dL/db out
__device__ __forceinline__ void quat_multiply_bwd(const float a[4], const float b[4], const float g_out[4], float da[4], float db[4])
{
    float o[4];
    quat_product(a, b, o);   // (for the sign of its real part)
    const float sg = o[0] < 0.f ? -1.f : 1.f;
    const float g[4] = {sg * g_out[0], sg * g_out[1], sg * g_out[2], sg * g_out[3]};
    quat_product_bwd(a, b, g, da, db);
}

// gradient of the face quaternion (frame_to_quaternion's q) on to the frame's axes: through standardize, the selected
// candidate row and the matrix entries it reads.  `dq` is consumed.
__device__ __forceinline__ void frame_to_quaternion_bwd(const QuatSel& qs, float dq[4], Vec3& da0, Vec3& da1, Vec3& da2)
{
    // through standardize + the selected candidate row: q_k = sgn * num_k / den
    float dnum[4], dden = 0.f;
    for (int k = 0; k < 4; k++) {
        dq[k] *= qs.sgn;
        dnum[k] = dq[k] / qs.den;
        dden -= dq[k] * qs.num[k] / (qs.den * qs.den);
    }
    float dqa = (qs.qa > 0.1f) ? 2.0f * dden : 0.f;   // den = 2 max(qa, 0.1)
    dqa += 2.0f * qs.qa * dnum[qs.sel];               // diagonal numerator qa^2
    const float dx = qs.qa > 0.f ? dqa / (2.0f * qs.qa) : 0.f;   // qa = sqrt(x), zero subgradient at x <= 0
    // x_sel = 1 +- m00 +- m11 +- m22
    const float s00 = (qs.sel == 0 || qs.sel == 1) ? 1.f : -1.f;
    const float s11 = (qs.sel == 0 || qs.sel == 2) ? 1.f : -1.f;
    const float s22 = (qs.sel == 0 || qs.sel == 3) ? 1.f : -1.f;
    float dm[3][3] = {{s00 * dx, 0, 0}, {0, s11 * dx, 0}, {0, 0, s22 * dx}};  // dm[r][c]
    switch (qs.sel) {
        case 0:  // num = (diag, m21 - m12, m02 - m20, m10 - m01)
            dm[2][1] += dnum[1], dm[1][2] -= dnum[1], dm[0][2] += dnum[2], dm[2][0] -= dnum[2], dm[1][0] += dnum[3], dm[0][1] -= dnum[3];
            break;
        case 1:  // (m21 - m12, diag, m10 + m01, m02 + m20)
            dm[2][1] += dnum[0], dm[1][2] -= dnum[0], dm[1][0] += dnum[2], dm[0][1] += dnum[2], dm[0][2] += dnum[3], dm[2][0] += dnum[3];
            break;
        case 2:  // (m02 - m20, m10 + m01, diag, m12 + m21)
            dm[0][2] += dnum[0], dm[2][0] -= dnum[0], dm[1][0] += dnum[1], dm[0][1] += dnum[1], dm[1][2] += dnum[3], dm[2][1] += dnum[3];
            break;
        default:  // (m10 - m01, m20 + m02, m21 + m12, diag)
            dm[1][0] += dnum[0], dm[0][1] -= dnum[0], dm[2][0] += dnum[1], dm[0][2] += dnum[1], dm[2][1] += dnum[2], dm[1][2] += dnum[2];
            break;
    }
    // m[r][c] = a_c[r]
    da0 = add(da0, Vec3{dm[0][0], dm[1][0], dm[2][0]});
    da1 = add(da1, Vec3{dm[0][1], dm[1][1], dm[2][1]});
    da2 = add(da2, Vec3{dm[0][2], dm[1][2], dm[2][2]});
}

// gradients of the frame's axes (and of length(e1), `dl1`) on to the two edges: mesh_compute.py:45-47, last to first
__device__ __forceinline__ void face_frame_bwd(const FaceFrame& f, Vec3 da0, Vec3 da1, Vec3 da2, float dl1, Vec3& de1, Vec3& de2)
{
    {   // a2 = -normalize(c2), c2 = a1 x a0
        const Vec3 y = {-f.a2.x, -f.a2.y, -f.a2.z};
        const Vec3 dc2 = safe_normalize_bwd(Vec3{-da2.x, -da2.y, -da2.z}, y, f.lc2, f.kc2);
        da1 = add(da1, cross3(f.a0, dc2));
        da0 = add(da0, cross3(dc2, f.a1));
    }
    {   // a1 = normalize(c1), c1 = a0 x e2
        const Vec3 dc1 = safe_normalize_bwd(da1, f.a1, f.lc1, f.kc1);
        da0 = add(da0, cross3(f.e2, dc1));
        de2 = add(de2, cross3(dc1, f.a0));
    }
    {   // a0 = normalize(e1); s0 = length(e1)
        de1 = add(de1, safe_normalize_bwd(da0, f.a0, f.l1, f.k1));
        if (!f.k1) de1 = add(de1, mul(f.a0, dl1));
    }
}

// edge gradients on to the face's three vertices (e1 = v1 - v0, e2 = v2 - v0), then the float atomics of dL/dverts
__device__ __forceinline__ void scatter_vertex_grads(float* d_verts, int i0, int i1, int i2, Vec3 dv0, Vec3 dv1, Vec3 dv2, Vec3 de1,
                                                     Vec3 de2)
{
    dv1 = add(dv1, de1);
    dv2 = add(dv2, de2);
    dv0 = sub(dv0, add(de1, de2));
    if (d_verts) {
        atomic_add_f32(d_verts + 3 * i0, dv0.x), atomic_add_f32(d_verts + 3 * i0 + 1, dv0.y), atomic_add_f32(d_verts + 3 * i0 + 2, dv0.z);
        atomic_add_f32(d_verts + 3 * i1, dv1.x), atomic_add_f32(d_verts + 3 * i1 + 1, dv1.y), atomic_add_f32(d_verts + 3 * i1 + 2, dv1.z);
        atomic_add_f32(d_verts + 3 * i2, dv2.x), atomic_add_f32(d_verts + 3 * i2 + 1, dv2.y), atomic_add_f32(d_verts + 3 * i2 + 2, dv2.z);
    }
}

// forward of one Gaussian: what the reference assigns to gaussian._xyz / _rotation / _scaling before render()
__device__ __forceinline__ void bind_one_fwd(const BindArgs& a, int n, float xyz[3], float rot[4], float scl[3])
{
    const int fi = a.face_index[n];
    const int i0 = a.faces[3 * fi], i1 = a.faces[3 * fi + 1], i2 = a.faces[3 * fi + 2];
    const Vec3 v0 = load3(a.verts, i0), v1 = load3(a.verts, i1), v2 = load3(a.verts, i2);
    const FaceFrame f = face_frame(v0, v1, v2);
    // position: barycentric point + shell offset along the (unnormalised) face normal
    const float b0 = a.bary[3 * n], b1 = a.bary[3 * n + 1], b2 = a.bary[3 * n + 2];
    const Vec3 pos = {b0 * v0.x + b1 * v1.x + b2 * v2.x, b0 * v0.y + b1 * v1.y + b2 * v2.y, b0 * v0.z + b1 * v1.z + b2 * v2.z};
    const Vec3 nrm = cross3(f.e1, f.e2);
    const float t = tanhf(a.offset[n]);
    xyz[0] = pos.x + nrm.x * a.shell_len * t;
    xyz[1] = pos.y + nrm.y * a.shell_len * t;
    xyz[2] = pos.z + nrm.z * a.shell_len * t;
    // rotation: face quaternion (x) own quaternion, real part made non-negative
    const QuatSel qs = frame_to_quaternion(f);
    const float r[4] = {a.rotation[4 * n], a.rotation[4 * n + 1], a.rotation[4 * n + 2], a.rotation[4 * n + 3]};
    quat_multiply(qs.q, r, rot);
    // scale: log of the face's stretch relative to the canonical mesh
    const float ls = a.resize_scale ? logf(f.scale / a.canon[fi]) : 0.f;
    for (int k = 0; k < 3; k++) scl[k] = a.scaling[3 * n + k] + ls;
}

// where the backward of one Gaussian puts its results; any member may be null
struct BindGrads {
    float* d_verts;     // [V,3] ADDED with float atomics
    float* d_offset;    // [N]   written
    float* d_rotation;  // [N,4] written
    float* d_scaling;   // [N,3] written
    float* d_local_xyz; // [N,3] written (FR_BIND_FACE_LOCAL, FR_BIND_PHONG; d_offset is the shell mode's); [N,10] FR_BIND_DEFORM
};

constexpr int kDeformCols = 10;   // FR_BIND_DEFORM: position 3, rotation 4 (log of the real part first), log-scale factor 3
// floats per row of the mode's own parameter in BindArgs::local_xyz, and of its gradient in BindGrads::d_local_xyz
__device__ __forceinline__ int bind_own_cols(int mode) { return mode == FR_BIND_DEFORM ? kDeformCols : 3; }

// a Gaussian without any gradient (culled by the frame): zero rows, nothing for the vertices
__device__ __forceinline__ void bind_bwd_zero(const BindArgs& a, int n, const BindGrads& o)
{
    if (o.d_offset) o.d_offset[n] = 0.f;
    if (o.d_local_xyz) {
        const int cols = bind_own_cols(a.mode);
        for (int k = 0; k < cols; k++) o.d_local_xyz[(size_t)cols * n + k] = 0.f;
    }
    if (o.d_rotation)
        for (int k = 0; k < 4; k++) o.d_rotation[4 * n + k] = 0.f;
    if (o.d_scaling)
        for (int k = 0; k < 3; k++) o.d_scaling[3 * n + k] = 0.f;
}

// the upstream rows of a Gaussian the frame gave no gradient: all ten exactly zero (a NaN row is not)
__device__ __forceinline__ bool bind_rows_all_zero(const float g_xyz[3], const float g_rot[4], const float g_scl[3])
{
    bool z = true;
    for (int k = 0; k < 3; k++) z = z && g_xyz[k] == 0.f && g_scl[k] == 0.f;
    for (int k = 0; k < 4; k++) z = z && g_rot[k] == 0.f;
    return z;
}

// backward of one Gaussian: gradients of its three bound values in, gradients of offset / rotation / scaling written,
// dL/dverts of its face's three vertices added
__device__ __forceinline__ void bind_one_bwd(const BindArgs& a, int n, const float g_xyz[3], const float g_rot[4],
                                             const float g_scl[3], const BindGrads& o)
{
    const int fi = a.face_index[n];
    const int i0 = a.faces[3 * fi], i1 = a.faces[3 * fi + 1], i2 = a.faces[3 * fi + 2];
    const Vec3 v0 = load3(a.verts, i0), v1 = load3(a.verts, i1), v2 = load3(a.verts, i2);
    const FaceFrame f = face_frame(v0, v1, v2);
    Vec3 de1 = {0, 0, 0}, de2 = {0, 0, 0}, da0 = {0, 0, 0}, da1 = {0, 0, 0}, da2 = {0, 0, 0};
    float dl1 = 0.f;

    // ---- scaling
    float gs = 0.f;
    for (int k = 0; k < 3; k++) {
        const float g = g_scl[k];
        if (o.d_scaling) o.d_scaling[3 * n + k] = g;
        gs += g;
    }
    if (a.resize_scale) {
        const float dscale = gs / f.scale;           // d log(scale / canon) / d scale
        dl1 += 0.5f * dscale;
        const float dd = 0.5f * dscale * (f.d < 0.f ? -1.f : (f.d > 0.f ? 1.f : 0.f));
        da2 = add(da2, mul(f.e2, dd));
        de2 = add(de2, mul(f.a2, dd));
    }

    // ---- position
    const Vec3 gx = {g_xyz[0], g_xyz[1], g_xyz[2]};
    const Vec3 nrm = cross3(f.e1, f.e2);
    const float t = tanhf(a.offset[n]);
    if (o.d_offset) o.d_offset[n] = a.shell_len * dot3(gx, nrm) * (1.0f - t * t);
    const Vec3 dnrm = mul(gx, a.shell_len * t);
    de1 = add(de1, cross3(f.e2, dnrm));              // d(e1 x e2)/de1 . g = e2 x g
    de2 = add(de2, cross3(dnrm, f.e1));
    const float b0 = a.bary[3 * n], b1 = a.bary[3 * n + 1], b2 = a.bary[3 * n + 2];
    Vec3 dv0 = mul(gx, b0), dv1 = mul(gx, b1), dv2 = mul(gx, b2);

    // ---- rotation: out = standardize(qf (x) r)
    const QuatSel qs = frame_to_quaternion(f);
    const float r[4] = {a.rotation[4 * n], a.rotation[4 * n + 1], a.rotation[4 * n + 2], a.rotation[4 * n + 3]};
    float dq[4], dr[4];
    quat_multiply_bwd(qs.q, r, g_rot, dq, dr);
    if (o.d_rotation)
        for (int k = 0; k < 4; k++) o.d_rotation[4 * n + k] = dr[k];
    frame_to_quaternion_bwd(qs, dq, da0, da1, da2);
    face_frame_bwd(f, da0, da1, da2, dl1, de1, de2);
    scatter_vertex_grads(o.d_verts, i0, i1, i2, dv0, dv1, dv2, de1, de2);
}

// ---------------------------------------------------------------------------------------------------------------------
// FR_BIND_FACE_LOCAL — GaussianAvatars' binding (model/baseline/gaussianavatars.py:144-171): with R = [a0 a1 a2], s the
// face scale and c the mean of the face's three vertices,
//     xyz = (R local_xyz) * s + c;  rotation = standardize(normalize(q_face) (x) rotation);  scaling = scaling + log(s)
// normalize = F.normalize: q / max(|q|, 1e-12).
constexpr float kNormEps = 1e-12f;

struct UnitQuat {
    float q[4];
    float len;      // max(|q|, eps)
    bool clamped;   // the length did not depend on q
};
__device__ __forceinline__ UnitQuat normalize_quat(const float q[4])
{
    UnitQuat u;
    const float n = sqrtf(q[0] * q[0] + q[1] * q[1] + q[2] * q[2] + q[3] * q[3]);
    u.clamped = !(n > kNormEps);
    u.len = fmaxf(n, kNormEps);
    for (int k = 0; k < 4; k++) u.q[k] = q[k] / u.len;
    return u;
}

__device__ __forceinline__ void bind_local_fwd(const BindArgs& a, int n, float xyz[3], float rot[4], float scl[3])
{
    const int fi = a.face_index[n];
    const int i0 = a.faces[3 * fi], i1 = a.faces[3 * fi + 1], i2 = a.faces[3 * fi + 2];
    const Vec3 v0 = load3(a.verts, i0), v1 = load3(a.verts, i1), v2 = load3(a.verts, i2);
    const FaceFrame f = face_frame(v0, v1, v2);
    // position: the local point turned into the face's frame, stretched by the face scale, moved to the face centre
    const Vec3 l = load3(a.local_xyz, n);
    const Vec3 u = {f.a0.x * l.x + f.a1.x * l.y + f.a2.x * l.z, f.a0.y * l.x + f.a1.y * l.y + f.a2.y * l.z,
                    f.a0.z * l.x + f.a1.z * l.y + f.a2.z * l.z};
    xyz[0] = u.x * f.scale + (v0.x + v1.x + v2.x) / 3.0f;
    xyz[1] = u.y * f.scale + (v0.y + v1.y + v2.y) / 3.0f;
    xyz[2] = u.z * f.scale + (v0.z + v1.z + v2.z) / 3.0f;
    // rotation: normalised face quaternion (x) own quaternion, real part made non-negative
    const QuatSel qs = frame_to_quaternion(f);
    const UnitQuat uq = normalize_quat(qs.q);
    const float r[4] = {a.rotation[4 * n], a.rotation[4 * n + 1], a.rotation[4 * n + 2], a.rotation[4 * n + 3]};
    quat_multiply(uq.q, r, rot);
    // scale: log of the face scale itself
    const float ls = logf(f.scale);
    for (int k = 0; k < 3; k++) scl[k] = a.scaling[3 * n + k] + ls;
}

// gradients of local_xyz / rotation / scaling written, dL/dverts added: through the centre, R (position and normalised
// quaternion), s and log s
__device__ __forceinline__ void bind_local_bwd(const BindArgs& a, int n, const float g_xyz[3], const float g_rot[4],
                                               const float g_scl[3], const BindGrads& o)
{
    const int fi = a.face_index[n];
    const int i0 = a.faces[3 * fi], i1 = a.faces[3 * fi + 1], i2 = a.faces[3 * fi + 2];
    const Vec3 v0 = load3(a.verts, i0), v1 = load3(a.verts, i1), v2 = load3(a.verts, i2);
    const FaceFrame f = face_frame(v0, v1, v2);
    Vec3 de1 = {0, 0, 0}, de2 = {0, 0, 0};

    // ---- scaling: + log(s)
    float gs = 0.f;
    for (int k = 0; k < 3; k++) {
        const float g = g_scl[k];
        if (o.d_scaling) o.d_scaling[3 * n + k] = g;
        gs += g;
    }
    float dscale = gs / f.scale;

    // ---- position: xyz = u * s + c, u = R l
    const Vec3 gx = {g_xyz[0], g_xyz[1], g_xyz[2]};
    const Vec3 l = load3(a.local_xyz, n);
    const Vec3 u = {f.a0.x * l.x + f.a1.x * l.y + f.a2.x * l.z, f.a0.y * l.x + f.a1.y * l.y + f.a2.y * l.z,
                    f.a0.z * l.x + f.a1.z * l.y + f.a2.z * l.z};
    dscale += dot3(gx, u);
    const Vec3 du = mul(gx, f.scale);
    if (o.d_local_xyz) o.d_local_xyz[3 * n] = dot3(f.a0, du), o.d_local_xyz[3 * n + 1] = dot3(f.a1, du), o.d_local_xyz[3 * n + 2] = dot3(f.a2, du);
    Vec3 da0 = mul(du, l.x), da1 = mul(du, l.y), da2 = mul(du, l.z);
    const Vec3 dc = {gx.x / 3.0f, gx.y / 3.0f, gx.z / 3.0f};   // c = (v0 + v1 + v2) / 3

    // ---- the face scale s = (length(e1) + |a2 . e2|) / 2
    const float dl1 = 0.5f * dscale;
    const float dd = 0.5f * dscale * (f.d < 0.f ? -1.f : (f.d > 0.f ? 1.f : 0.f));
    da2 = add(da2, mul(f.e2, dd));
    de2 = add(de2, mul(f.a2, dd));

    // ---- rotation: out = standardize(normalize(qf) (x) r)
    const QuatSel qs = frame_to_quaternion(f);
    const UnitQuat uq = normalize_quat(qs.q);
    const float r[4] = {a.rotation[4 * n], a.rotation[4 * n + 1], a.rotation[4 * n + 2], a.rotation[4 * n + 3]};
    float dq[4], dr[4];
    quat_multiply_bwd(uq.q, r, g_rot, dq, dr);
    if (o.d_rotation)
        for (int k = 0; k < 4; k++) o.d_rotation[4 * n + k] = dr[k];
    if (!uq.clamped) {   // through q / |q|; a clamped length did not depend on q (as safe_normalize_bwd)
        const float t = uq.q[0] * dq[0] + uq.q[1] * dq[1] + uq.q[2] * dq[2] + uq.q[3] * dq[3];
        for (int k = 0; k < 4; k++) dq[k] = dq[k] - uq.q[k] * t;
    }
    for (int k = 0; k < 4; k++) dq[k] = dq[k] / uq.len;
    frame_to_quaternion_bwd(qs, dq, da0, da1, da2);
    face_frame_bwd(f, da0, da1, da2, dl1, de1, de2);
    scatter_vertex_grads(o.d_verts, i0, i1, i2, dc, dc, dc, de1, de2);
}

// ---------------------------------------------------------------------------------------------------------------------
// FR_BIND_PHONG — SplattingAvatar's binding (model/baseline/splattingavatar.py:203-246).  Two parts:
//
// (1) the per-frame mesh pass (fr_phong_frame): per face the area ratio of :899-902, per vertex the normal of pytorch3d's
//     verts_normals_packed (:206) and the area-weighted mean of its faces' quaternions (PerVertQuaternion, :846-881).  The
//     reference sums both with index_add (float atomics); here every vertex GATHERS its faces in the order of a CSR
//     incidence list and recomputes each face's contribution (~250 flops) — no scratch, no atomics, the same bits every run.
// (2) the per-Gaussian binding from those arrays (bind_phong_fwd / _bwd).  Nothing of it reaches the posed vertices
//     (DESIGN.md).
constexpr float kPhongDamping = 1e-4f;   // calc_face_area_change (:899)
constexpr float kVertEps = 1e-6f;        // F.normalize(eps=1e-6) of the per-vertex sums (:879, verts_normals_packed)

// F.normalize: x / max(|x|, eps)
__device__ __forceinline__ Vec3 f_normalize(Vec3 x, float eps)
{
    const float n = fmaxf(sqrtf(dot3(x, x)), eps);
    return {x.x / n, x.y / n, x.z / n};
}

// cross(v2 - v1, v0 - v1): calc_face_areas' (:781-791) and verts_normals_packed's face vector; |.| / 2 is the area
__device__ __forceinline__ Vec3 phong_face_cross(Vec3 v0, Vec3 v1, Vec3 v2) { return cross3(sub(v2, v1), sub(v0, v1)); }

__device__ __forceinline__ float phong_face_ratio(Vec3 p0, Vec3 p1, Vec3 p2, float area_cano)
{
    const Vec3 c = phong_face_cross(p0, p1, p2);
    return (sqrtf(dot3(c, c)) / 2.0f + kPhongDamping) / (area_cano + kPhongDamping);
}

// tbn (:756-765): the columns X, Y, Z of a triangle's frame
__device__ __forceinline__ void phong_tbn(Vec3 a, Vec3 b, Vec3 c, Vec3& X, Vec3& Y, Vec3& Z)
{
    const Vec3 d = sub(b, a);
    const Vec3 n = f_normalize(cross3(d, sub(c, a)), kNormEps);
    X = f_normalize(cross3(d, n), kNormEps);
    Y = f_normalize(cross3(d, X), kNormEps);
    Z = f_normalize(d, kNormEps);
}

// matrix_to_quaternion(R_posed R_cano^T) of one face (:795-802, :891-894; the rotation block of deform_Rt cano_Rt^-1: tbn
// is orthonormal, so the inverse is the transpose)
__device__ __forceinline__ void phong_face_quat(Vec3 p0, Vec3 p1, Vec3 p2, Vec3 c0, Vec3 c1, Vec3 c2, float q[4])
{
    Vec3 Xp, Yp, Zp, Xc, Yc, Zc;
    phong_tbn(p0, p1, p2, Xp, Yp, Zp);
    phong_tbn(c0, c1, c2, Xc, Yc, Zc);
    // column j of M = R_p R_c^T:  X_p X_c[j] + Y_p Y_c[j] + Z_p Z_c[j]
    const Vec3 m0 = add(add(mul(Xp, Xc.x), mul(Yp, Yc.x)), mul(Zp, Zc.x));
    const Vec3 m1 = add(add(mul(Xp, Xc.y), mul(Yp, Yc.y)), mul(Zp, Zc.y));
    const Vec3 m2 = add(add(mul(Xp, Xc.z), mul(Yp, Yc.z)), mul(Zp, Zc.z));
    const QuatSel qs = frame_to_quaternion(m0, m1, m2);
    for (int k = 0; k < 4; k++) q[k] = qs.q[k];
}

struct PhongFrameArgs {
    int V, F;
    const float* verts;       // [V,3] posed
    const float* cano_verts;  // [V,3]
    const int* faces;         // [F,3]
    const int* vf_offsets;    // [V+1] CSR rows: the faces of every vertex ...
    const int* vf_faces;      // [3F]  ... ascending within a row
    const float* area_cano;   // [F]
    float* vert_normals;      // [V,3] out
    float* vert_quats;        // [V,4] out
    float* face_ratio;        // [F]   out
};

__device__ __forceinline__ void phong_vertex(const PhongFrameArgs& a, int v)
{
    Vec3 ns = {0.f, 0.f, 0.f};
    float qs[4] = {0.f, 0.f, 0.f, 0.f};
    const int end = a.vf_offsets[v + 1];
    for (int e = a.vf_offsets[v]; e < end; e++) {
        const int fi = a.vf_faces[e];
        const int i0 = a.faces[3 * fi], i1 = a.faces[3 * fi + 1], i2 = a.faces[3 * fi + 2];
        const Vec3 p0 = load3(a.verts, i0), p1 = load3(a.verts, i1), p2 = load3(a.verts, i2);
        ns = add(ns, phong_face_cross(p0, p1, p2));
        float q[4];
        phong_face_quat(p0, p1, p2, load3(a.cano_verts, i0), load3(a.cano_verts, i1), load3(a.cano_verts, i2), q);
        const float w = a.area_cano[fi];
        for (int k = 0; k < 4; k++) qs[k] = qs[k] + w * q[k];
    }
    const Vec3 n = f_normalize(ns, kVertEps);
    a.vert_normals[3 * v] = n.x, a.vert_normals[3 * v + 1] = n.y, a.vert_normals[3 * v + 2] = n.z;
    const float len = fmaxf(sqrtf(qs[0] * qs[0] + qs[1] * qs[1] + qs[2] * qs[2] + qs[3] * qs[3]), kVertEps);
    for (int k = 0; k < 4; k++) a.vert_quats[4 * v + k] = qs[k] / len;
}

// xyz = sum_k b_k v_k + normalize(sum_k b_k n_k) * uvd.z;  rotation = standardize((sum_k b_k q_k) (x) rotation) — the sum is
// NOT normalised (:235, :245);  scaling = scaling * face_ratio — the raw log-scale is MULTIPLIED (:244, kept as it is)
__device__ __forceinline__ Vec3 phong_unit_normal(const BindArgs& a, int i0, int i1, int i2, float b0, float b1, float b2)
{
    const Vec3 n0 = load3(a.vert_normals, i0), n1 = load3(a.vert_normals, i1), n2 = load3(a.vert_normals, i2);
    const Vec3 nb = {b0 * n0.x + b1 * n1.x + b2 * n2.x, b0 * n0.y + b1 * n1.y + b2 * n2.y, b0 * n0.z + b1 * n1.z + b2 * n2.z};
    return f_normalize(nb, kNormEps);
}
__device__ __forceinline__ void phong_base_quat(const BindArgs& a, int i0, int i1, int i2, float b0, float b1, float b2, float q[4])
{
    for (int k = 0; k < 4; k++) q[k] = b0 * a.vert_quats[4 * i0 + k] + b1 * a.vert_quats[4 * i1 + k] + b2 * a.vert_quats[4 * i2 + k];
}

__device__ __forceinline__ void bind_phong_fwd(const BindArgs& a, int n, float xyz[3], float rot[4], float scl[3])
{
    const int fi = a.face_index[n];
    const int i0 = a.faces[3 * fi], i1 = a.faces[3 * fi + 1], i2 = a.faces[3 * fi + 2];
    const Vec3 v0 = load3(a.verts, i0), v1 = load3(a.verts, i1), v2 = load3(a.verts, i2);
    const float b0 = a.bary[3 * n], b1 = a.bary[3 * n + 1], b2 = a.bary[3 * n + 2];
    const Vec3 nh = phong_unit_normal(a, i0, i1, i2, b0, b1, b2);
    const float d = a.local_xyz[3 * n + 2];
    xyz[0] = (b0 * v0.x + b1 * v1.x + b2 * v2.x) + nh.x * d;
    xyz[1] = (b0 * v0.y + b1 * v1.y + b2 * v2.y) + nh.y * d;
    xyz[2] = (b0 * v0.z + b1 * v1.z + b2 * v2.z) + nh.z * d;
    float qb[4];
    phong_base_quat(a, i0, i1, i2, b0, b1, b2, qb);
    const float r[4] = {a.rotation[4 * n], a.rotation[4 * n + 1], a.rotation[4 * n + 2], a.rotation[4 * n + 3]};
    quat_multiply(qb, r, rot);
    const float ratio = a.face_ratio[fi];
    for (int k = 0; k < 3; k++) scl[k] = a.scaling[3 * n + k] * ratio;
}

// gradients of uvd (through its third column only) / rotation / scaling written; the posed mesh gets none
__device__ __forceinline__ void bind_phong_bwd(const BindArgs& a, int n, const float g_xyz[3], const float g_rot[4],
                                               const float g_scl[3], const BindGrads& o)
{
    const int fi = a.face_index[n];
    const int i0 = a.faces[3 * fi], i1 = a.faces[3 * fi + 1], i2 = a.faces[3 * fi + 2];
    const float b0 = a.bary[3 * n], b1 = a.bary[3 * n + 1], b2 = a.bary[3 * n + 2];
    if (o.d_scaling) {
        const float ratio = a.face_ratio[fi];
        for (int k = 0; k < 3; k++) o.d_scaling[3 * n + k] = g_scl[k] * ratio;
    }
    if (o.d_local_xyz) {
        const Vec3 nh = phong_unit_normal(a, i0, i1, i2, b0, b1, b2);
        o.d_local_xyz[3 * n] = 0.f, o.d_local_xyz[3 * n + 1] = 0.f;
        o.d_local_xyz[3 * n + 2] = dot3(Vec3{g_xyz[0], g_xyz[1], g_xyz[2]}, nh);
    }
    if (o.d_rotation) {
        float qb[4], dq[4], dr[4];
        phong_base_quat(a, i0, i1, i2, b0, b1, b2, qb);
        const float r[4] = {a.rotation[4 * n], a.rotation[4 * n + 1], a.rotation[4 * n + 2], a.rotation[4 * n + 3]};
        quat_multiply_bwd(qb, r, g_rot, dq, dr);
        for (int k = 0; k < 4; k++) o.d_rotation[4 * n + k] = dr[k];
    }
}

// ---- the vertex gradient of the Phong mode (fr_phong_grad.hip).  bind_phong_bwd above is untouched: these are separate
// launches behind it.
//
// (a) per Gaussian: the gradients of the bound values on to the posed vertices (the barycentric point) and on to the three
//     arrays of the mesh pass, ADDED with float atomics at the face's three corners (as scatter_vertex_grads); any output may
//     be null.
struct PhongFrameGrads {
    float* d_verts;         // [V,3]
    float* d_vert_normals;  // [V,3]
    float* d_vert_quats;    // [V,4]
    float* d_face_ratio;    // [F]
};

__device__ __forceinline__ void bind_phong_frame_bwd(const BindArgs& a, int n, const float g_xyz[3], const float g_rot[4],
                                                     const float g_scl[3], const PhongFrameGrads& o)
{
    const int fi = a.face_index[n];
    const int ix[3] = {a.faces[3 * fi], a.faces[3 * fi + 1], a.faces[3 * fi + 2]};
    const float b[3] = {a.bary[3 * n], a.bary[3 * n + 1], a.bary[3 * n + 2]};
    const Vec3 gx = {g_xyz[0], g_xyz[1], g_xyz[2]};
    if (o.d_verts)
        for (int k = 0; k < 3; k++) {
            atomic_add_f32(o.d_verts + 3 * ix[k], b[k] * gx.x), atomic_add_f32(o.d_verts + 3 * ix[k] + 1, b[k] * gx.y);
            atomic_add_f32(o.d_verts + 3 * ix[k] + 2, b[k] * gx.z);
        }
    if (o.d_vert_normals) {   // xyz = .. + nb / max(|nb|, eps) * d
        const Vec3 n0 = load3(a.vert_normals, ix[0]), n1 = load3(a.vert_normals, ix[1]), n2 = load3(a.vert_normals, ix[2]);
        const Vec3 nb = {b[0] * n0.x + b[1] * n1.x + b[2] * n2.x, b[0] * n0.y + b[1] * n1.y + b[2] * n2.y,
                         b[0] * n0.z + b[1] * n1.z + b[2] * n2.z};
        const float raw = sqrtf(dot3(nb, nb)), len = fmaxf(raw, kNormEps);
        const Vec3 nh = {nb.x / len, nb.y / len, nb.z / len};
        const float d = a.local_xyz[3 * n + 2];
        const float t = raw > kNormEps ? dot3(nh, gx) : 0.f;   // a clamped length did not depend on nb
        const Vec3 dnb = {d * (gx.x - nh.x * t) / len, d * (gx.y - nh.y * t) / len, d * (gx.z - nh.z * t) / len};
        for (int k = 0; k < 3; k++) {
            atomic_add_f32(o.d_vert_normals + 3 * ix[k], b[k] * dnb.x), atomic_add_f32(o.d_vert_normals + 3 * ix[k] + 1, b[k] * dnb.y);
            atomic_add_f32(o.d_vert_normals + 3 * ix[k] + 2, b[k] * dnb.z);
        }
    }
    if (o.d_vert_quats) {   // rotation = standardize(qb (x) r), qb = sum_k b_k vq[i_k]
        float qb[4], dq[4], dr[4];
        phong_base_quat(a, ix[0], ix[1], ix[2], b[0], b[1], b[2], qb);
        const float r[4] = {a.rotation[4 * n], a.rotation[4 * n + 1], a.rotation[4 * n + 2], a.rotation[4 * n + 3]};
        quat_multiply_bwd(qb, r, g_rot, dq, dr);
        for (int k = 0; k < 3; k++)
            for (int c = 0; c < 4; c++) atomic_add_f32(o.d_vert_quats + 4 * ix[k] + c, b[k] * dq[c]);
    }
    if (o.d_face_ratio)   // scaling = scaling * face_ratio[f]
        atomic_add_f32(o.d_face_ratio + fi, g_scl[0] * a.scaling[3 * n] + g_scl[1] * a.scaling[3 * n + 1] + g_scl[2] * a.scaling[3 * n + 2]);
}

// (b) the backward of the mesh pass.  gradient of y = x / max(|x|, eps) w.r.t. x: `len` is the clamped length
__device__ __forceinline__ Vec3 f_normalize_bwd(Vec3 g, Vec3 y, float len, float eps)
{
    const float t = len > eps ? dot3(y, g) : 0.f;
    return {(g.x - y.x * t) / len, (g.y - y.y * t) / len, (g.z - y.z * t) / len};
}

// phong_tbn with what its backward needs: the same expressions in the same order
struct PhongTbn {
    Vec3 d, e, n, X, Y, Z;
    float l0, l1, l2, ld;   // the clamped lengths of cross(d, e), cross(d, n), cross(d, X), d
};
__device__ __forceinline__ Vec3 f_normalize_len(Vec3 x, float eps, float& len)
{
    len = fmaxf(sqrtf(dot3(x, x)), eps);
    return {x.x / len, x.y / len, x.z / len};
}
__device__ __forceinline__ PhongTbn phong_tbn_full(Vec3 a, Vec3 b, Vec3 c)
{
    PhongTbn t;
    t.d = sub(b, a), t.e = sub(c, a);
    t.n = f_normalize_len(cross3(t.d, t.e), kNormEps, t.l0);
    t.X = f_normalize_len(cross3(t.d, t.n), kNormEps, t.l1);
    t.Y = f_normalize_len(cross3(t.d, t.X), kNormEps, t.l2);
    t.Z = f_normalize_len(t.d, kNormEps, t.ld);
    return t;
}
// gradients of X, Y, Z on to the triangle's corners (z = x cross y: dx = y cross g, dy = g cross x), last to first
__device__ __forceinline__ void phong_tbn_bwd(const PhongTbn& t, Vec3 dX, Vec3 dY, Vec3 dZ, Vec3& da, Vec3& db, Vec3& dc)
{
    Vec3 dd = f_normalize_bwd(dZ, t.Z, t.ld, kNormEps);
    const Vec3 dc2 = f_normalize_bwd(dY, t.Y, t.l2, kNormEps);     // Y = normalize(d x X)
    dd = add(dd, cross3(t.X, dc2));
    dX = add(dX, cross3(dc2, t.d));
    const Vec3 dc1 = f_normalize_bwd(dX, t.X, t.l1, kNormEps);     // X = normalize(d x n)
    dd = add(dd, cross3(t.n, dc1));
    const Vec3 dn = cross3(dc1, t.d);
    const Vec3 dc0 = f_normalize_bwd(dn, t.n, t.l0, kNormEps);     // n = normalize(d x e)
    dd = add(dd, cross3(t.e, dc0));
    const Vec3 de = cross3(dc0, t.d);
    db = add(db, dd), dc = add(dc, de), da = sub(da, add(dd, de));
}

struct PhongFrameBwdArgs {
    int V, F;
    const float* verts;           // [V,3] posed
    const float* cano_verts;      // [V,3]
    const int* faces;             // [F,3]
    const int* vf_offsets;        // [V+1]
    const int* vf_faces;          // [3F]
    const float* area_cano;       // [F]
    const float* d_vert_normals;  // [V,3] upstream, may be null (zero)
    const float* d_vert_quats;    // [V,4] upstream, may be null
    const float* d_face_ratio;    // [F]   upstream, may be null
    float* sums;                  // [V,7] workspace: the gradients of the unnormalised sums ns_u (3) and qs_u (4)
    float* d_verts;               // [V,3] added to
};

// first launch, vertex v: ns_v and qs_v again from the expressions phong_vertex forms them with, then the upstream gradients
// through the two F.normalize(eps=1e-6).  The row is walked by `stride` lanes (lane `first` takes the entries first,
// first + stride, ...; the kernel adds the lanes' partial sums in a fixed butterfly order): a head mesh's rows hold 1 .. 32
// faces, and one lane per vertex makes its whole wave wait for the longest row.
__device__ __forceinline__ void phong_vertex_sums_partial(const PhongFrameBwdArgs& a, int v, int first, int stride, Vec3& ns, float qs[4])
{
    const int end = a.vf_offsets[v + 1];
    for (int e = a.vf_offsets[v] + first; e < end; e += stride) {
        const int fi = a.vf_faces[e];
        const int i0 = a.faces[3 * fi], i1 = a.faces[3 * fi + 1], i2 = a.faces[3 * fi + 2];
        const Vec3 p0 = load3(a.verts, i0), p1 = load3(a.verts, i1), p2 = load3(a.verts, i2);
        ns = add(ns, phong_face_cross(p0, p1, p2));
        float q[4];
        phong_face_quat(p0, p1, p2, load3(a.cano_verts, i0), load3(a.cano_verts, i1), load3(a.cano_verts, i2), q);
        const float w = a.area_cano[fi];
        for (int k = 0; k < 4; k++) qs[k] = qs[k] + w * q[k];
    }
}
__device__ __forceinline__ void phong_vertex_sums_finish(const PhongFrameBwdArgs& a, int v, Vec3 ns, const float qs[4])
{
    float* out = a.sums + 7 * (size_t)v;
    {
        float len;
        const Vec3 y = f_normalize_len(ns, kVertEps, len);
        const Vec3 g = a.d_vert_normals ? load3(a.d_vert_normals, v) : Vec3{0.f, 0.f, 0.f};
        const Vec3 d = f_normalize_bwd(g, y, len, kVertEps);
        out[0] = d.x, out[1] = d.y, out[2] = d.z;
    }
    {
        const float len = fmaxf(sqrtf(qs[0] * qs[0] + qs[1] * qs[1] + qs[2] * qs[2] + qs[3] * qs[3]), kVertEps);
        float g[4] = {0.f, 0.f, 0.f, 0.f}, t = 0.f;
        if (a.d_vert_quats)
            for (int k = 0; k < 4; k++) g[k] = a.d_vert_quats[4 * v + k];
        if (len > kVertEps)
            for (int k = 0; k < 4; k++) t += (qs[k] / len) * g[k];
        for (int k = 0; k < 4; k++) out[3 + k] = (g[k] - (qs[k] / len) * t) / len;
    }
}

// what face fi hands to its three corners: through the face cross product (vertex normals, area ratio) and through the face
// quaternion (matrix_to_quaternion of M = R_p R_c^T, tbn of the posed triangle; the canonical mesh is constant)
__device__ __forceinline__ void phong_face_bwd(const PhongFrameBwdArgs& a, int fi, Vec3& dv0, Vec3& dv1, Vec3& dv2)
{
    const int i0 = a.faces[3 * fi], i1 = a.faces[3 * fi + 1], i2 = a.faces[3 * fi + 2];
    const Vec3 p0 = load3(a.verts, i0), p1 = load3(a.verts, i1), p2 = load3(a.verts, i2);
    const float* s0 = a.sums + 7 * (size_t)i0;
    const float* s1 = a.sums + 7 * (size_t)i1;
    const float* s2 = a.sums + 7 * (size_t)i2;
    const float area = a.area_cano[fi];
    dv0 = dv1 = dv2 = Vec3{0.f, 0.f, 0.f};
    {   // c = (p2 - p1) x (p0 - p1): every corner's ns takes c; ratio = (|c| / 2 + damping) / (A + damping)
        const Vec3 u = sub(p2, p1), w = sub(p0, p1);
        const Vec3 c = cross3(u, w);
        Vec3 gc = {(s0[0] + s1[0]) + s2[0], (s0[1] + s1[1]) + s2[1], (s0[2] + s1[2]) + s2[2]};
        const float len = sqrtf(dot3(c, c));
        if (a.d_face_ratio && len > 0.f) gc = add(gc, mul(c, a.d_face_ratio[fi] / (2.0f * len * (area + kPhongDamping))));
        const Vec3 du = cross3(w, gc), dw = cross3(gc, u);
        dv2 = add(dv2, du), dv0 = add(dv0, dw), dv1 = sub(dv1, add(du, dw));
    }
    {   // every corner's qs takes A q_f
        float gq[4];
        for (int k = 0; k < 4; k++) gq[k] = area * ((s0[3 + k] + s1[3 + k]) + s2[3 + k]);
        const PhongTbn tp = phong_tbn_full(p0, p1, p2);
        Vec3 Xc, Yc, Zc;
        phong_tbn(load3(a.cano_verts, i0), load3(a.cano_verts, i1), load3(a.cano_verts, i2), Xc, Yc, Zc);
        const Vec3 m0 = add(add(mul(tp.X, Xc.x), mul(tp.Y, Yc.x)), mul(tp.Z, Zc.x));
        const Vec3 m1 = add(add(mul(tp.X, Xc.y), mul(tp.Y, Yc.y)), mul(tp.Z, Zc.y));
        const Vec3 m2 = add(add(mul(tp.X, Xc.z), mul(tp.Y, Yc.z)), mul(tp.Z, Zc.z));
        const QuatSel qs = frame_to_quaternion(m0, m1, m2);
        Vec3 dm0 = {0.f, 0.f, 0.f}, dm1 = {0.f, 0.f, 0.f}, dm2 = {0.f, 0.f, 0.f};
        frame_to_quaternion_bwd(qs, gq, dm0, dm1, dm2);
        // column j of M = X_p X_c[j] + Y_p Y_c[j] + Z_p Z_c[j]
        const Vec3 dX = add(add(mul(dm0, Xc.x), mul(dm1, Xc.y)), mul(dm2, Xc.z));
        const Vec3 dY = add(add(mul(dm0, Yc.x), mul(dm1, Yc.y)), mul(dm2, Yc.z));
        const Vec3 dZ = add(add(mul(dm0, Zc.x), mul(dm1, Zc.y)), mul(dm2, Zc.z));
        phong_tbn_bwd(tp, dX, dY, dZ, dv0, dv1, dv2);
    }
}

// second launch, vertex v: the sum over its incidence row of what every face hands to THIS corner, the row walked by `stride`
// lanes as above.  A face with a repeated corner is in the row once per corner (phong_canonical): the k-th of its entries
// takes the k-th matching corner.
__device__ __forceinline__ Vec3 phong_vertex_gather_partial(const PhongFrameBwdArgs& a, int v, int first, int stride)
{
    Vec3 acc = {0.f, 0.f, 0.f};
    const int begin = a.vf_offsets[v], end = a.vf_offsets[v + 1];
    for (int e = begin + first; e < end; e += stride) {
        const int fi = a.vf_faces[e];
        int occ = 0;
        if (e - 1 >= begin && a.vf_faces[e - 1] == fi) occ++;
        if (e - 2 >= begin && a.vf_faces[e - 2] == fi) occ++;
        Vec3 dv0, dv1, dv2;
        phong_face_bwd(a, fi, dv0, dv1, dv2);
        int seen = 0;
        Vec3 mine = {0.f, 0.f, 0.f};
        if (a.faces[3 * fi] == v && seen++ == occ) mine = dv0;
        if (a.faces[3 * fi + 1] == v && seen++ == occ) mine = dv1;
        if (a.faces[3 * fi + 2] == v && seen++ == occ) mine = dv2;
        acc = add(acc, mine);
    }
    return acc;
}
// the owning lane's plain read-add-store; a vertex without a face is not touched
__device__ __forceinline__ void phong_vertex_gather_finish(const PhongFrameBwdArgs& a, int v, Vec3 acc)
{
    if (a.vf_offsets[v + 1] > a.vf_offsets[v]) {
        a.d_verts[3 * v] = a.d_verts[3 * v] + acc.x, a.d_verts[3 * v + 1] = a.d_verts[3 * v + 1] + acc.y;
        a.d_verts[3 * v + 2] = a.d_verts[3 * v + 2] + acc.z;
    }
}

// ---------------------------------------------------------------------------------------------------------------------
// FR_BIND_DEFORM — FlashAvatar's binding (model/baseline/flashavatar.py:242-276): with t = tanh(deform) of the ten RAW outputs
// of the deformation MLP for this Gaussian in this frame,
//     xyz = sum_k b_k v_k + t[0:3];  rotation = rotation (x) (exp(t[3]), t[4], t[5], t[6]);  scaling = scaling * exp(t[7:10])
// The product is quatProduct_batch (:380-390): the PARAMETER is the first factor and the sign is kept.  The raw log-scale is
// MULTIPLIED (:272, kept as it is, as in the Phong mode).  Nothing is normalised here: the rasterizer does that.
__device__ __forceinline__ void bind_deform_fwd(const BindArgs& a, int n, float xyz[3], float rot[4], float scl[3])
{
    const int fi = a.face_index[n];
    const int i0 = a.faces[3 * fi], i1 = a.faces[3 * fi + 1], i2 = a.faces[3 * fi + 2];
    const Vec3 v0 = load3(a.verts, i0), v1 = load3(a.verts, i1), v2 = load3(a.verts, i2);
    const float b0 = a.bary[3 * n], b1 = a.bary[3 * n + 1], b2 = a.bary[3 * n + 2];
    float t[kDeformCols];
    for (int k = 0; k < kDeformCols; k++) t[k] = tanhf(a.local_xyz[(size_t)kDeformCols * n + k]);
    xyz[0] = (b0 * v0.x + b1 * v1.x + b2 * v2.x) + t[0];
    xyz[1] = (b0 * v0.y + b1 * v1.y + b2 * v2.y) + t[1];
    xyz[2] = (b0 * v0.z + b1 * v1.z + b2 * v2.z) + t[2];
    const float r[4] = {a.rotation[4 * n], a.rotation[4 * n + 1], a.rotation[4 * n + 2], a.rotation[4 * n + 3]};
    const float delta[4] = {expf(t[3]), t[4], t[5], t[6]};
    quat_product(r, delta, rot);
    for (int k = 0; k < 3; k++) scl[k] = a.scaling[3 * n + k] * expf(t[7 + k]);
}

// gradients of deform (all ten columns) / rotation / scaling written, dL/dverts added: b_k g_xyz to the face's three corners
__device__ __forceinline__ void bind_deform_bwd(const BindArgs& a, int n, const float g_xyz[3], const float g_rot[4],
                                                const float g_scl[3], const BindGrads& o)
{
    float t[kDeformCols], gt[kDeformCols];
    for (int k = 0; k < kDeformCols; k++) t[k] = tanhf(a.local_xyz[(size_t)kDeformCols * n + k]);
    for (int k = 0; k < 3; k++) gt[k] = g_xyz[k];
    const float r[4] = {a.rotation[4 * n], a.rotation[4 * n + 1], a.rotation[4 * n + 2], a.rotation[4 * n + 3]};
    const float e3 = expf(t[3]);
    const float delta[4] = {e3, t[4], t[5], t[6]};
    float dr[4], dd[4];
    quat_product_bwd(r, delta, g_rot, dr, dd);
    if (o.d_rotation)
        for (int k = 0; k < 4; k++) o.d_rotation[4 * n + k] = dr[k];
    gt[3] = dd[0] * e3, gt[4] = dd[1], gt[5] = dd[2], gt[6] = dd[3];
    for (int k = 0; k < 3; k++) {
        const float e = expf(t[7 + k]);
        gt[7 + k] = g_scl[k] * a.scaling[3 * n + k] * e;
        if (o.d_scaling) o.d_scaling[3 * n + k] = g_scl[k] * e;
    }
    if (o.d_local_xyz)
        for (int k = 0; k < kDeformCols; k++) o.d_local_xyz[(size_t)kDeformCols * n + k] = gt[k] * (1.0f - t[k] * t[k]);
    if (o.d_verts) {
        const int fi = a.face_index[n];
        const int i0 = a.faces[3 * fi], i1 = a.faces[3 * fi + 1], i2 = a.faces[3 * fi + 2];
        const float b0 = a.bary[3 * n], b1 = a.bary[3 * n + 1], b2 = a.bary[3 * n + 2];
        const Vec3 gx = {g_xyz[0], g_xyz[1], g_xyz[2]}, z = {0.f, 0.f, 0.f};
        scatter_vertex_grads(o.d_verts, i0, i1, i2, mul(gx, b0), mul(gx, b1), mul(gx, b2), z, z);
    }
}

// ---------------------------------------------------------------------------------------------------------------------
// what the kernels call: the binding of BindArgs::mode (one value per launch, so the branch is wave-uniform)
__device__ __forceinline__ void bind_fwd(const BindArgs& a, int n, float xyz[3], float rot[4], float scl[3])
{
    if (a.mode == FR_BIND_FACE_LOCAL) bind_local_fwd(a, n, xyz, rot, scl);
    else if (a.mode == FR_BIND_PHONG) bind_phong_fwd(a, n, xyz, rot, scl);
    else if (a.mode == FR_BIND_DEFORM) bind_deform_fwd(a, n, xyz, rot, scl);
    else bind_one_fwd(a, n, xyz, rot, scl);
}
__device__ __forceinline__ void bind_bwd(const BindArgs& a, int n, const float g_xyz[3], const float g_rot[4], const float g_scl[3],
                                         const BindGrads& o)
{
    if (a.mode == FR_BIND_FACE_LOCAL) bind_local_bwd(a, n, g_xyz, g_rot, g_scl, o);
    else if (a.mode == FR_BIND_PHONG) bind_phong_bwd(a, n, g_xyz, g_rot, g_scl, o);
    else if (a.mode == FR_BIND_DEFORM) bind_deform_bwd(a, n, g_xyz, g_rot, g_scl, o);
    else bind_one_bwd(a, n, g_xyz, g_rot, g_scl, o);
}

}  // namespace fr
