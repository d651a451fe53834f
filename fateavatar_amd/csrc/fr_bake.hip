// Neural baking on gfx950: the decoder's packed 11-channel output decoded into the five per-Gaussian attribute arrays in ONE
// launch per direction, and the rotation term of the baking objective in one more.
//
// reference: `UVDecoder.forward` (model/uv_decoder.py:387-542) -> `_gather_attribute` (:85-107) on the channel slices of
// :225-245 (colour 0:3, opacity 3:4, scaling 4:7, rotation 7:10, offset 10:11), each slice behind its activation (:133-174)
// and one F.grid_sample(.., "bilinear", "border", align_corners=True) (:179-202); `UVDecoderLoss`'s rot_loss
// (train/loss.py:612-617) on raw_rot = quaternion_to_axis_angle(decode_rotation) (uv_decoder.py:516).  There: a dozen
// element-wise launches for the rotation activation alone, five grid_sample launches, and as many again in autograd, which
// scatter every point's gradient into the maps with float atomics.  Here:
//   k_bake_decode      lane = POINT: the four texels and weights once (fr_tex_math.hpp: the look-up's own expressions, so
//                      the same texels and weight bits), then all five attributes, the ROTATION ACTIVATION applied to each
//                      corner texel in registers (tanh x 2 pi -> axis-angle -> quaternion -> the reference's shuffle) before
//                      the interpolation: the activated map is never materialised;
//   k_bake_decode_bwd  lane = TEXEL: ONE walk over the plan's list of (point, corner) entries of that texel, all twelve
//                      gradient channels (3 + 1 + 3 + 4 + 1) summed in list order, then the per-texel Jacobians (the 1 -> 1
//                      ones are tex_act_grad; rotation is the 4 -> 3 transpose through the quaternion map and the tanh),
//                      STORED for every texel of d_tex_out: no zero fill, no float atomics, the same bits on every run;
//   k_rot_term         lane = ROW of the decoded rotation [N,4]: the unweighted loss through sum_over_workgroups and
//                      weight x its gradient ADDED to the row by the lane that owns it.
// Built without FMA contraction, like fr_texture.hip: the colour / opacity / scaling / offset rows are those of
// fr_texture_lookup bit for bit.
#include "fr_tex_math.hpp"
#include <cstdio>

namespace fr {

constexpr int kBakeChannels = 11;
constexpr int kColor = 0, kOpacity = 3, kScaling = 4, kRotation = 7, kOffset = 10;   // first channel of every slice
constexpr float kColorScale = (float)(0.5 / 0.28209479177387814);                    // 0.5 / C0 (uv_decoder.py:138)
constexpr float kTwoPi = 6.283185307179586f;                                         // float32(2 pi)
constexpr float kSmallAngle = 1e-6f;

// `_rotation_activation` (uv_decoder.py:158-174) of one texel's three channels:
//   a = tanh(t) 2 pi;  theta = |a|;  q = (cos(theta / 2), a s),  s = sin(theta / 2) / theta, for theta < 1e-6 the Taylor
//   series 0.5 - theta^2 / 48 (pytorch3d 0.7.7 axis_angle_to_quaternion);  out = (q[3], q[0], q[1], q[2]): the reference's
//   shuffle as it runs on a real-first quaternion.
struct RotTexel {
    float th[3];     // tanh(t)
    float a[3];      // the axis-angle vector
    float theta, s, c;
};

__device__ __forceinline__ RotTexel rot_texel(float t0, float t1, float t2)
{
    RotTexel r;
    r.th[0] = tanhf(t0), r.th[1] = tanhf(t1), r.th[2] = tanhf(t2);
#pragma unroll
    for (int i = 0; i < 3; i++) r.a[i] = r.th[i] * kTwoPi;
    r.theta = sqrtf(r.a[0] * r.a[0] + r.a[1] * r.a[1] + r.a[2] * r.a[2]);
    const float half = r.theta * 0.5f;
    r.c = cosf(half);
    r.s = r.theta < kSmallAngle ? 0.5f - (r.theta * r.theta) / 48.f : sinf(half) / r.theta;   // (never divides by a zero angle)
    return r;
}

__device__ __forceinline__ void rot_texel_out(const RotTexel& r, float (&q)[4])
{
    q[0] = r.a[2] * r.s, q[1] = r.c, q[2] = r.a[0] * r.s, q[3] = r.a[1] * r.s;
}

// The 4 -> 3 transpose: g = dL/d(out) of the texel (summed over its entries) -> dL/dt.  With v = a s:
//   d cos(theta / 2) / da_i = -(s / 2) a_i
//   d v_j / da_i            = s [i == j] + a_j a_i s'(theta) / theta,   s' / theta = (cos(theta / 2) / 2 - s) / theta^2,
// and in the Taylor branch s' / theta = -1 / 24: nothing divides by theta there, so at a texel whose three channels are 0 the
// Jacobian is d q / d a = I / 2 and every non-zero entry of d out / d t is pi.
__device__ __forceinline__ void rot_texel_grad(const RotTexel& r, const float (&g)[4], float (&dt)[3])
{
    const float gw = g[1], gv[3] = {g[2], g[3], g[0]};
    const float dot = gv[0] * r.a[0] + gv[1] * r.a[1] + gv[2] * r.a[2];
    const float k = r.theta < kSmallAngle ? -1.f / 24.f : (r.c * 0.5f - r.s) / (r.theta * r.theta);
    const float along = dot * k - gw * (r.s * 0.5f);      // what multiplies a_i
#pragma unroll
    for (int i = 0; i < 3; i++) {
        const float da = gv[i] * r.s + along * r.a[i];
        dt[i] = da * ((1.f - r.th[i] * r.th[i]) * kTwoPi);
    }
}

struct BakeArgs {
    int N, H, W;
    const float2* uv;
    const float* tex;          // [11,H,W]
    float mean, cap;           // the scaling activation's a0, a1
    // forward: the five outputs [N,C]; backward: their gradients (null: zero)
    float* out[5];
    const float* d_out[5];
    const int* row_start;
    const int* entries;
    float* d_tex;              // [11,H,W]
};

__global__ void __launch_bounds__(256) k_bake_decode(BakeArgs a)
{
    const int n = blockIdx.x * blockDim.x + threadIdx.x;
    if (n >= a.N) return;
    const float2 p = a.uv[n];
    const TexCoord t = tex_coord(p.x, p.y, a.H, a.W);
    int idx[4];
    float w[4];
#pragma unroll
    for (int k = 0; k < 4; k++) idx[k] = tex_corner_index(t, k, a.W), w[k] = tex_corner_weight(t, k);
    const size_t plane = (size_t)a.H * a.W;
    const float* __restrict__ tex = a.tex;
    // colour, opacity, scaling, offset: fr_texture_lookup's expressions in its order
#pragma unroll
    for (int c = 0; c < 3; c++) {
        float col = 0.f, scl = 0.f;
#pragma unroll
        for (int k = 0; k < 4; k++)
            if (idx[k] >= 0) {
                col += tex_act(FR_TEX_ACT_TANH_SCALE, kColorScale, 0.f, tex[(kColor + c) * plane + idx[k]]) * w[k];
                scl += tex_act(FR_TEX_ACT_SOFTPLUS_CAP, a.mean, a.cap, tex[(kScaling + c) * plane + idx[k]]) * w[k];
            }
        a.out[0][(size_t)n * 3 + c] = col;
        a.out[2][(size_t)n * 3 + c] = scl;
    }
    float opa = 0.f, off = 0.f, q[4] = {0.f, 0.f, 0.f, 0.f};
#pragma unroll
    for (int k = 0; k < 4; k++)
        if (idx[k] >= 0) {
            opa += tex_act(FR_TEX_ACT_IDENTITY, 0.f, 0.f, tex[kOpacity * plane + idx[k]]) * w[k];
            off += tex_act(FR_TEX_ACT_TANH_SCALE, 1.f, 0.f, tex[kOffset * plane + idx[k]]) * w[k];
            float qk[4];
            rot_texel_out(rot_texel(tex[kRotation * plane + idx[k]], tex[(kRotation + 1) * plane + idx[k]],
                                    tex[(kRotation + 2) * plane + idx[k]]), qk);
#pragma unroll
            for (int j = 0; j < 4; j++) q[j] += qk[j] * w[k];
        }
    a.out[1][n] = opa;
    a.out[4][n] = off;
    reinterpret_cast<float4*>(a.out[3])[n] = make_float4(q[0], q[1], q[2], q[3]);
}

__global__ void __launch_bounds__(256) k_bake_decode_bwd(BakeArgs a)
{
    const int texel = blockIdx.x * blockDim.x + threadIdx.x;
    const size_t plane = (size_t)a.H * a.W;
    if ((size_t)texel >= plane) return;
    const int begin = a.row_start[texel], end = a.row_start[texel + 1];
    const float* __restrict__ d_col = a.d_out[0];
    const float* __restrict__ d_opa = a.d_out[1];
    const float* __restrict__ d_scl = a.d_out[2];
    const float* __restrict__ d_rot = a.d_out[3];
    const float* __restrict__ d_off = a.d_out[4];
    float gc[3] = {0.f, 0.f, 0.f}, gs[3] = {0.f, 0.f, 0.f}, gr[4] = {0.f, 0.f, 0.f, 0.f}, go = 0.f, gf = 0.f;
    for (int j = begin; j < end; j++) {
        const int e = a.entries[j], point = e >> 2;            // entry = 4 * point + corner
        if ((unsigned)point >= (unsigned)a.N) continue;        // (a plan of another UV set: read nothing out of bounds)
        const float2 p = a.uv[point];
        const float w = tex_corner_weight(tex_coord(p.x, p.y, a.H, a.W), e & 3);
        if (d_col) {
#pragma unroll
            for (int c = 0; c < 3; c++) gc[c] += w * d_col[(size_t)point * 3 + c];
        }
        if (d_opa) go += w * d_opa[point];
        if (d_scl) {
#pragma unroll
            for (int c = 0; c < 3; c++) gs[c] += w * d_scl[(size_t)point * 3 + c];
        }
        if (d_rot) {
            const float4 g = reinterpret_cast<const float4*>(d_rot)[point];
            gr[0] += w * g.x, gr[1] += w * g.y, gr[2] += w * g.z, gr[3] += w * g.w;
        }
        if (d_off) gf += w * d_off[point];
    }
    const float* __restrict__ tex = a.tex + texel;
    float* __restrict__ d_tex = a.d_tex + texel;
#pragma unroll
    for (int c = 0; c < 3; c++) {
        d_tex[(kColor + c) * plane] = gc[c] * tex_act_grad(FR_TEX_ACT_TANH_SCALE, kColorScale, 0.f, tex[(kColor + c) * plane]);
        d_tex[(kScaling + c) * plane] = gs[c] * tex_act_grad(FR_TEX_ACT_SOFTPLUS_CAP, a.mean, a.cap, tex[(kScaling + c) * plane]);
    }
    d_tex[kOpacity * plane] = go;
    d_tex[kOffset * plane] = gf * tex_act_grad(FR_TEX_ACT_TANH_SCALE, 1.f, 0.f, tex[kOffset * plane]);
    float dt[3];
    rot_texel_grad(rot_texel(tex[kRotation * plane], tex[(kRotation + 1) * plane], tex[(kRotation + 2) * plane]), gr, dt);
#pragma unroll
    for (int c = 0; c < 3; c++) d_tex[(kRotation + c) * plane] = dt[c];
}

// ---------------------------------------------------------------- the rotation term, one launch
// reference: train/loss.py:612-617 on raw_rot = quaternion_to_axis_angle(decode_rotation) (pytorch3d 0.7.7), element 0 of
// the row taken for the real part (after the reference's shuffle it is not: restated as it runs):
//     n = |q[1:]|;  half = atan2(n, q[0]);  ang = 2 half;  s = sin(half) / ang, or 0.5 - ang^2 / 48 for |ang| < 1e-6
//     raw = q[1:] / s;   rot_loss = mean(raw[:,0]^2) + mean(raw[:,2]^2)
// Gradient of a row, with G = (2 raw0, 0, 2 raw2) / N:
//     dL/ds = -(G . raw) / s;   ds/dang = (cos(half) / 2 - s) / ang, or -ang / 24 in the Taylor branch
//     dang/dn = 2 q0 / (n^2 + q0^2),  dang/dq0 = -2 n / (n^2 + q0^2),  dn/dq[1:] = q[1:] / n — and 0 where n = 0 (autograd's
//     rule for the norm), so the rows (1,0,0,0), (-1,0,0,0) and an all-zero row add nothing anywhere.
constexpr unsigned kRotMaxBlocks = 256;

struct RotTermArgs {
    const float4* rotation;
    float4* d_rotation;   // null: no gradient traffic (also what a zero weight gives)
    float* partial;       // [2][kRotMaxBlocks]
    unsigned* counter;
    float* loss;
    int N;
    float g;              // weight / N
};

__global__ void __launch_bounds__(kSumThreads) k_rot_term(RotTermArgs a)
{
    const unsigned stride = gridDim.x * blockDim.x;
    float acc[2] = {0.f, 0.f};   // sum of raw0^2, sum of raw2^2
    for (unsigned i = blockIdx.x * blockDim.x + threadIdx.x; i < (unsigned)a.N; i += stride) {
        const float4 q = a.rotation[i];
        const float n2 = q.y * q.y + q.z * q.z + q.w * q.w;
        const float n = sqrtf(n2);
        const float half = atan2f(n, q.x), ang = 2.f * half;
        const bool small = fabsf(ang) < kSmallAngle;
        const float ch = cosf(half);
        const float s = small ? 0.5f - (ang * ang) / 48.f : sinf(half) / ang;
        const float raw0 = q.y / s, raw2 = q.w / s;
        acc[0] += raw0 * raw0, acc[1] += raw2 * raw2;
        if (!a.d_rotation) continue;
        const float G0 = 2.f * raw0 * a.g, G2 = 2.f * raw2 * a.g;
        const float dLds = -(G0 * raw0 + G2 * raw2) / s;
        const float dsdang = small ? -ang / 24.f : (ch * 0.5f - s) / ang;
        const float d = n2 + q.x * q.x;
        const float dLdang = dLds * dsdang * (d > 0.f ? 2.f / d : 0.f);
        const float along = n > 0.f ? dLdang * q.x / n : 0.f;       // through the norm: what multiplies q[1:]
        float4 o = a.d_rotation[i];
        o.x += -(dLdang * n);
        o.y += G0 / s + along * q.y;
        o.z += along * q.z;
        o.w += G2 / s + along * q.w;
        a.d_rotation[i] = o;
    }
    if (!sum_over_workgroups(acc, a.partial, kRotMaxBlocks, a.counter, blockIdx.x, gridDim.x)) return;
    a.loss[0] = acc[0] / (float)a.N + acc[1] / (float)a.N;
}

// (the [N,4] rows travel as float4; null passes: it is refused, or means "no gradient", elsewhere)
static bool aligned16(const void* p) { return (reinterpret_cast<uintptr_t>(p) & 15u) == 0; }

static int check_bake(const char* who, int32_t N, const float* uv, int32_t H, int32_t W, const float* tex_out)
{
    char msg[160];
    if (N < 0 || N > (1 << 29) || H <= 0 || W <= 0 || (int64_t)H * W > (1 << 29) / kBakeChannels) {
        snprintf(msg, sizeof(msg), "%s: N must be 0 .. 2^29 and H x W 1 .. 2^29 / 11 texels", who);
        return fail_msg(FR_ERR_INVALID_ARGUMENT, msg);
    }
    if (N > 0 && !uv) {
        snprintf(msg, sizeof(msg), "%s: null uv", who);
        return fail_msg(FR_ERR_INVALID_ARGUMENT, msg);
    }
    if (!tex_out) {
        snprintf(msg, sizeof(msg), "%s: null tex_out", who);
        return fail_msg(FR_ERR_INVALID_ARGUMENT, msg);
    }
    return FR_OK;
}

}  // namespace fr

using namespace fr;

extern "C" {

int fr_bake_decode(int32_t N, const float* uv, int32_t H, int32_t W, const float* tex_out, float mean_scaling, float max_scaling,
                   float* color, float* opacity, float* scaling, float* rotation, float* offset, void* stream)
{
    int rc = check_bake("fr_bake_decode", N, uv, H, W, tex_out);
    if (rc) return rc;
    if (N == 0) return FR_OK;
    if (!color || !opacity || !scaling || !rotation || !offset) return fail_msg(FR_ERR_INVALID_ARGUMENT, "fr_bake_decode: null output array");
    if (!aligned16(rotation)) return fail_msg(FR_ERR_INVALID_ARGUMENT, "fr_bake_decode: the rotation rows must be 16-byte aligned");
    BakeArgs a = {};
    a.N = N, a.H = H, a.W = W, a.uv = reinterpret_cast<const float2*>(uv), a.tex = tex_out, a.mean = mean_scaling, a.cap = max_scaling;
    a.out[0] = color, a.out[1] = opacity, a.out[2] = scaling, a.out[3] = rotation, a.out[4] = offset;
    hipLaunchKernelGGL(k_bake_decode, dim3((N + 255) / 256), dim3(256), 0, static_cast<hipStream_t>(stream), a);
    FR_HIP(hipGetLastError());
    return FR_OK;
}

int fr_bake_decode_backward(int32_t N, const float* uv, int32_t H, int32_t W, const int32_t* row_start, const int32_t* entries,
                            const float* tex_out, float mean_scaling, float max_scaling, const float* d_color, const float* d_opacity,
                            const float* d_scaling, const float* d_rotation, const float* d_offset, float* d_tex_out, void* stream)
{
    int rc = check_bake("fr_bake_decode_backward", N, uv, H, W, tex_out);
    if (rc) return rc;
    if (!d_tex_out) return fail_msg(FR_ERR_INVALID_ARGUMENT, "fr_bake_decode_backward: null d_tex_out");
    if (!row_start || (N > 0 && !entries)) return fail_msg(FR_ERR_INVALID_ARGUMENT, "fr_bake_decode_backward: null plan (row_start / entries)");
    if (!aligned16(d_rotation)) return fail_msg(FR_ERR_INVALID_ARGUMENT, "fr_bake_decode_backward: the rotation rows must be 16-byte aligned");
    BakeArgs a = {};
    a.N = N, a.H = H, a.W = W, a.uv = reinterpret_cast<const float2*>(uv), a.tex = tex_out, a.mean = mean_scaling, a.cap = max_scaling;
    a.d_out[0] = d_color, a.d_out[1] = d_opacity, a.d_out[2] = d_scaling, a.d_out[3] = d_rotation, a.d_out[4] = d_offset;
    a.row_start = row_start, a.entries = entries, a.d_tex = d_tex_out;
    const int texels = H * W;
    hipLaunchKernelGGL(k_bake_decode_bwd, dim3((texels + 255) / 256), dim3(256), 0, static_cast<hipStream_t>(stream), a);
    FR_HIP(hipGetLastError());
    return FR_OK;
}

size_t fr_rot_term_workspace_bytes(void) { return done_workspace_bytes(2 * kRotMaxBlocks); }

int fr_rot_term(float weight, int32_t N, const float* rotation, float* d_rotation, float* loss, void* workspace, void* stream)
{
    if (N < 0) return fail_msg(FR_ERR_INVALID_ARGUMENT, "fr_rot_term: negative N");
    if (N > 0 && !rotation) return fail_msg(FR_ERR_INVALID_ARGUMENT, "fr_rot_term: null rotation array");
    if (!workspace || !loss) return fail_msg(FR_ERR_INVALID_ARGUMENT, "fr_rot_term: null workspace or loss");
    if (N == 0) return FR_OK;
    if (!aligned16(rotation) || !aligned16(d_rotation)) return fail_msg(FR_ERR_INVALID_ARGUMENT, "fr_rot_term: the rotation rows must be 16-byte aligned");
    const unsigned blocks = capped_blocks((unsigned)N, kSumThreads, kRotMaxBlocks);
    const DoneWorkspace ws = done_workspace(workspace);
    RotTermArgs a;
    a.rotation = reinterpret_cast<const float4*>(rotation);
    a.d_rotation = weight != 0.f ? reinterpret_cast<float4*>(d_rotation) : nullptr;   // a zero weight: the array is not touched
    a.counter = ws.counter, a.partial = ws.partial;
    a.loss = loss, a.N = N;
    a.g = (float)((double)weight / (double)N);
    hipLaunchKernelGGL(k_rot_term, dim3(blocks), dim3(kSumThreads), 0, static_cast<hipStream_t>(stream), a);
    FR_HIP(hipGetLastError());
    return FR_OK;
}

}  // extern "C"
