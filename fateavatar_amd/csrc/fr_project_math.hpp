// The per-Gaussian projection math, written ONCE: Sigma3D from a Gaussian's inputs, the EWA projection to the 2D covariance
// and the way back from dL/dconic to dL/dt — what k_preprocess_fwd (fr_preprocess.hip), k_preprocess_bwd
// (fr_preprocess_bwd.hip) and k_camera_bwd (fr_camera_bwd.hip) have in common.  The backward kernels do not read the conic,
// Sigma3D or T back from the forward: they compute them again from the same inputs, and get the forward's bits because they
// call the forward's functions — same operands, order and parentheses, the `W1 * 0.0f` products, divisions as divisions, no
// FMA contraction (all three units are STRICT_UNITS of the Makefile).  One text to edit, nothing to keep in step.
// Everything here is __device__ __forceinline__ arithmetic on values: no loads, no stores, no barriers.  A kernel fetches its
// inputs its own way, calls these, and stores its outputs in its own order.
#pragma once
#include "fr_common.hpp"

namespace fr {

// Sigma3D = R S^2 R^T as its 6 upper-triangular floats (forward.cu:118-152) from the ACTIVATED scale and unit quaternion.
__device__ __forceinline__ void cov3d_from_scale_rot(float sc0, float sc1, float sc2, float r, float x, float y, float z,
                                                     float scale_modifier, float (&c3)[6])
{
    const float s0 = scale_modifier * sc0, s1 = scale_modifier * sc1, s2 = scale_modifier * sc2;
    // rows of the rotation matrix, each entry scaled by the scale of its COLUMN index
    const float m00 = s0 * (1.f - 2.f * (y * y + z * z)), m01 = s1 * (2.f * (x * y - r * z)), m02 = s2 * (2.f * (x * z + r * y));
    const float m10 = s0 * (2.f * (x * y + r * z)), m11 = s1 * (1.f - 2.f * (x * x + z * z)), m12 = s2 * (2.f * (y * z - r * x));
    const float m20 = s0 * (2.f * (x * z - r * y)), m21 = s1 * (2.f * (y * z + r * x)), m22 = s2 * (1.f - 2.f * (x * x + y * y));
    c3[0] = m00 * m00 + m01 * m01 + m02 * m02;
    c3[1] = m10 * m00 + m11 * m01 + m12 * m02;
    c3[2] = m20 * m00 + m21 * m01 + m22 * m02;
    c3[3] = m10 * m10 + m11 * m11 + m12 * m12;
    c3[4] = m20 * m10 + m21 * m11 + m22 * m12;
    c3[5] = m20 * m20 + m21 * m21 + m22 * m22;
}

// A Gaussian's Sigma3D and what it was made from: the activated scale, the unit quaternion (r, x, y, z) and, with raw
// inputs, 1 / |q| — the backward continues through all three.
struct Sigma3D {
    float c3[6], sc[3], q[4], rot_inv;
};
// `use_scale_rot`: the scales and rotations were given (else sc = q = 0); `raw` (FR_FLAG_RAW_ACTIVATIONS): they are the
// model's parameters and are activated here; `precomp`: the caller's six floats ARE Sigma3D.  (Wave-uniform, all three.)
__device__ __forceinline__ Sigma3D sigma3d_from_inputs(const bool use_scale_rot, const bool raw, const float (&in_sc)[3],
                                                       const float (&in_q)[4], const float scale_modifier, const bool precomp,
                                                       const float (&in_c3)[6])
{
    Sigma3D s;
    s.q[0] = s.q[1] = s.q[2] = s.q[3] = s.sc[0] = s.sc[1] = s.sc[2] = 0.f, s.rot_inv = 1.0f;
    if (use_scale_rot) {
        s.q[0] = in_q[0], s.q[1] = in_q[1], s.q[2] = in_q[2], s.q[3] = in_q[3];
        s.sc[0] = in_sc[0], s.sc[1] = in_sc[1], s.sc[2] = in_sc[2];
        if (raw) {
            s.sc[0] = act_exp(s.sc[0]), s.sc[1] = act_exp(s.sc[1]), s.sc[2] = act_exp(s.sc[2]);
            s.rot_inv = act_rot_inv_norm(s.q[0], s.q[1], s.q[2], s.q[3]);
            s.q[0] *= s.rot_inv, s.q[1] *= s.rot_inv, s.q[2] *= s.rot_inv, s.q[3] *= s.rot_inv;
        }
    }
    if (precomp) {
        for (int k = 0; k < 6; k++) s.c3[k] = in_c3[k];
    } else {
        cov3d_from_scale_rot(s.sc[0], s.sc[1], s.sc[2], s.q[0], s.q[1], s.q[2], s.q[3], scale_modifier, s.c3);
    }
    return s;
}

// clip-space mean and m_w = 1 / (hom.w + 1e-7): ndc = hom.xy m_w (forward.cu:196-198, backward.cu:370-373)
__device__ __forceinline__ float4 project_mean(const float3 mean, const float* proj, float& m_w)
{
    const float4 hom = xform4x4(mean, proj);
    m_w = 1.0f / (hom.w + 0.0000001f);
    return hom;
}

// EWA projection of Sigma3D to the 2D covariance (forward.cu:74-113, backward.cu:144-205)
struct Ewa {
    float3 t;                        // view-space mean, x / y clamped to the guard band
    float x_grad_mul, y_grad_mul;    // 0 where the clamp was active (the reference's stop-gradient), else 1
    float j00, j02, j11, j12;        // the Jacobian's non-zero entries
    float T0[3], T1[3];              // T = J W: T0[w] = T[0][w], T1[w] = T[1][w] of the reference's column-major T
    float cov_a, cov_b, cov_c;       // T Sigma3D T^T + 0.3 I
};
// `t`: xform4x3(mean, vm);  `vm`: the view matrix;  (h_x, h_y): the focal lengths in pixels
__device__ __forceinline__ Ewa ewa_project(float3 t, const float* vm, const float (&c3)[6], const float tan_fovx,
                                           const float tan_fovy, const float h_x, const float h_y)
{
    Ewa e;
    const float limx = 1.3f * tan_fovx, limy = 1.3f * tan_fovy;
    const float txtz = t.x / t.z, tytz = t.y / t.z;
    t.x = fminf(limx, fmaxf(-limx, txtz)) * t.z;
    t.y = fminf(limy, fmaxf(-limy, tytz)) * t.z;
    e.t = t;
    e.x_grad_mul = txtz < -limx || txtz > limx ? 0 : 1;
    e.y_grad_mul = tytz < -limy || tytz > limy ? 0 : 1;
    e.j00 = h_x / t.z, e.j02 = -(h_x * t.x) / (t.z * t.z);
    e.j11 = h_y / t.z, e.j12 = -(h_y * t.y) / (t.z * t.z);
    for (int w = 0; w < 3; w++) {   // (the zero products are kept so the sums round identically)
        const float W0 = vm[4 * w], W1 = vm[4 * w + 1], W2 = vm[4 * w + 2];
        e.T0[w] = W0 * e.j00 + W1 * 0.0f + W2 * e.j02;
        e.T1[w] = W0 * 0.0f + W1 * e.j11 + W2 * e.j12;
    }
    const float V[3][3] = {{c3[0], c3[1], c3[2]}, {c3[1], c3[3], c3[4]}, {c3[2], c3[4], c3[5]}};
    float A0[3], A1[3];  // (T * Sigma) rows
    for (int c = 0; c < 3; c++) {
        A0[c] = e.T0[0] * V[0][c] + e.T0[1] * V[1][c] + e.T0[2] * V[2][c];
        A1[c] = e.T1[0] * V[0][c] + e.T1[1] * V[1][c] + e.T1[2] * V[2][c];
    }
    e.cov_a = A0[0] * e.T0[0] + A0[1] * e.T0[1] + A0[2] * e.T0[2];
    e.cov_b = A1[0] * e.T0[0] + A1[1] * e.T0[1] + A1[2] * e.T0[2];
    e.cov_c = A1[0] * e.T1[0] + A1[1] * e.T1[1] + A1[2] * e.T1[2];
    e.cov_a += 0.3f;
    e.cov_c += 0.3f;
    return e;
}

// conic = (Sigma2D)^-1 backwards: dL/d(cov_a, cov_b, cov_c) from (dcx, dcy, dcz) = dL/d(conic a, b, c), b counted once
// (backward.cu:207-227).  `live` is false where 1 / (denom^2 + 1e-7) came out 0: the three are zeros then, and nothing that
// multiplies them may be evaluated (T holds infinities there).
struct CovGrad {
    float dL_da, dL_db, dL_dc;
    bool live;
};
__device__ __forceinline__ CovGrad conic_bwd(const Ewa& e, const float dcx, const float dcy, const float dcz)
{
    const float ca = e.cov_a, cb = e.cov_b, cc = e.cov_c;
    const float denom = ca * cc - cb * cb;
    const float denom2inv = 1.0f / ((denom * denom) + 0.0000001f);
    CovGrad g{0, 0, 0, denom2inv != 0};
    if (g.live) {
        g.dL_da = denom2inv * (-cc * cc * dcx + 2 * cb * cc * dcy + (denom - ca * cc) * dcz);
        g.dL_dc = denom2inv * (-ca * ca * dcz + 2 * ca * cb * dcy + (denom - ca * cc) * dcx);
        g.dL_db = denom2inv * 2 * (cb * cc * dcx - (denom + 2 * cb * cb) * dcy + ca * cb * dcz);
    }
    return g;
}

// dL/dT (upper 2x3, backward.cu:237-248; Vrk is symmetric) -> dL/dJ (backward.cu:252-255, W[c][r] = vm[c + 4 r]) -> dL/dt.
// NB the clamped t.x / t.y are treated as constants (stop-gradient quirk of the reference).
struct EwaGrad {
    float dT0[3], dT1[3], dL_dtx, dL_dty, dL_dtz;
};
__device__ __forceinline__ EwaGrad ewa_bwd(const Ewa& e, const float* vm, const float (&c3)[6], const CovGrad& g, const float h_x,
                                           const float h_y)
{
    EwaGrad o;
    const float V[3][3] = {{c3[0], c3[1], c3[2]}, {c3[1], c3[3], c3[4]}, {c3[2], c3[4], c3[5]}};
    for (int c = 0; c < 3; c++) {
        const float tv0 = e.T0[0] * V[c][0] + e.T0[1] * V[c][1] + e.T0[2] * V[c][2];
        const float tv1 = e.T1[0] * V[c][0] + e.T1[1] * V[c][1] + e.T1[2] * V[c][2];
        o.dT0[c] = 2 * tv0 * g.dL_da + tv1 * g.dL_db;
        o.dT1[c] = 2 * tv1 * g.dL_dc + tv0 * g.dL_db;
    }
    const float dL_dJ00 = vm[0] * o.dT0[0] + vm[4] * o.dT0[1] + vm[8] * o.dT0[2];
    const float dL_dJ02 = vm[2] * o.dT0[0] + vm[6] * o.dT0[1] + vm[10] * o.dT0[2];
    const float dL_dJ11 = vm[1] * o.dT1[0] + vm[5] * o.dT1[1] + vm[9] * o.dT1[2];
    const float dL_dJ12 = vm[2] * o.dT1[0] + vm[6] * o.dT1[1] + vm[10] * o.dT1[2];
    const float3 t = e.t;
    const float tz = 1.f / t.z, tz2 = tz * tz, tz3 = tz2 * tz;
    o.dL_dtx = e.x_grad_mul * -h_x * tz2 * dL_dJ02;
    o.dL_dty = e.y_grad_mul * -h_y * tz2 * dL_dJ12;
    o.dL_dtz = -h_x * tz2 * dL_dJ00 - h_y * tz2 * dL_dJ11 + (2 * h_x * t.x) * tz3 * dL_dJ02 + (2 * h_y * t.y) * tz3 * dL_dJ12;
    return o;
}

// The SH colour backwards to the view direction mean - campos (backward.cu:20-139): the clamped-channel mask on dL/dcolour,
// d colour / d direction (GeomView::dcolor_ddir, from the forward) and dnormvdv (auxiliary.h:107-117).  `d`: the three terms
// of dL/d(mean - campos) — added to dL/dmean, subtracted from dL/dcampos.
struct ShDirGrad {
    float dox, doy, doz, dRGB[3], d[3];   // mean - campos;  dL/dcolour, zero in the channels the forward clamped;  the terms
};
__device__ __forceinline__ ShDirGrad sh_dir_bwd(const float3 mean, const float* campos, const uint32_t cl, const float (&dcol)[3],
                                                const float (&dd)[9])
{
    ShDirGrad o;
    const float dox = mean.x - campos[0], doy = mean.y - campos[1], doz = mean.z - campos[2];
    o.dox = dox, o.doy = doy, o.doz = doz;
    float(&dRGB)[3] = o.dRGB;
    for (int c = 0; c < 3; c++) dRGB[c] = dcol[c] * (((cl >> c) & 1) ? 0 : 1);
    const float ddx = dd[0] * dRGB[0] + dd[1] * dRGB[1] + dd[2] * dRGB[2];
    const float ddy = dd[3] * dRGB[0] + dd[4] * dRGB[1] + dd[5] * dRGB[2];
    const float ddz = dd[6] * dRGB[0] + dd[7] * dRGB[1] + dd[8] * dRGB[2];
    const float sum2 = dox * dox + doy * doy + doz * doz;
    const float invsum32 = 1.0f / sqrtf(sum2 * sum2 * sum2);
    o.d[0] = ((+sum2 - dox * dox) * ddx - doy * dox * ddy - doz * dox * ddz) * invsum32;
    o.d[1] = (-dox * doy * ddx + (sum2 - doy * doy) * ddy - doz * doy * ddz) * invsum32;
    o.d[2] = (-dox * doz * ddx - doy * doz * ddy + (sum2 - doz * doz) * ddz) * invsum32;
    return o;
}

}  // namespace fr
