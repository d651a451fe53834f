// Gaussian attributes looked up in UV attribute maps on gfx950: what a BAKED FateAvatar does every frame in front of the
// binding + render() sequence.
//
// reference: model/uv_decoder.py:179-202 (`UVSampling._texture_look_up`: F.grid_sample(texture, 2 uv - 1, "bilinear",
// "border", align_corners=True), once per attribute map) behind the per-texture activations of :133-156, called by
// `_gather_attribute` (:85-107) and `_gather_attribute_from_texture_dict` (:109-131).  There: per frame five grid_sample
// launches, their activations and permutes, and for training their five autograd twins, which scatter every point's
// gradient into the textures with float atomics.  Here:
//   k_tex_lookup      lane = POINT: the four texels and weights once, then every layer and channel of up to
//                     FR_TEX_MAX_LAYERS textures, written row-major [N, C] (the layout the rasterizer takes);
//   k_tex_corners     lane = point: the four texel indices of every point (the plan is built from them, once per UV set);
//   k_tex_lookup_bwd  lane = TEXEL: a gather over the plan's list of (point, corner) entries of that texel — weights
//                     recomputed from uv with the forward's own function, summed in list order, times act'(texel), STORED.
//                     Every texel of every layer is written: no zero fill, no float atomics, the same bits on every run.
// Built without FMA contraction (the order of grid_sample's roundings is part of the contract: fr_tex_math.hpp).
#include "fr_tex_math.hpp"
#include <cstdio>

namespace fr {

// the layers of one launch, by value in the kernel arguments (indexed by unrolled constants only)
struct TexLayers {
    int n;
    const float* tex[FR_TEX_MAX_LAYERS];   // [C,H,W] raw texture
    const float* in[FR_TEX_MAX_LAYERS];    // backward: d_out [N,C]
    float* out[FR_TEX_MAX_LAYERS];         // forward: out [N,C]; backward: d_texture [C,H,W]
    int C[FR_TEX_MAX_LAYERS];
    int act[FR_TEX_MAX_LAYERS];
    float a0[FR_TEX_MAX_LAYERS], a1[FR_TEX_MAX_LAYERS];
};

__global__ void __launch_bounds__(256) k_tex_lookup(int N, const float2* uv, int H, int W, TexLayers L)
{
    const int n = blockIdx.x * blockDim.x + threadIdx.x;
    if (n >= N) return;
    const float2 p = uv[n];
    const TexCoord t = tex_coord(p.x, p.y, H, W);
    int idx[4];
    float w[4];
#pragma unroll
    for (int k = 0; k < 4; k++) idx[k] = tex_corner_index(t, k, W), w[k] = tex_corner_weight(t, k);
    const size_t plane = (size_t)H * W;
#pragma unroll
    for (int l = 0; l < FR_TEX_MAX_LAYERS; l++) {
        if (l >= L.n) break;
        const int C = L.C[l];
#pragma unroll
        for (int c = 0; c < 4; c++) {
            if (c >= C) break;
            const float* tex = L.tex[l] + c * plane;
            float acc = 0.f;
#pragma unroll
            for (int k = 0; k < 4; k++)
                if (idx[k] >= 0) acc += tex_act(L.act[l], L.a0[l], L.a1[l], tex[idx[k]]) * w[k];
            L.out[l][(size_t)n * C + c] = acc;
        }
    }
}

__global__ void __launch_bounds__(256) k_tex_corners(int N, const float2* uv, int H, int W, int4* corners)
{
    const int n = blockIdx.x * blockDim.x + threadIdx.x;
    if (n >= N) return;
    const float2 p = uv[n];
    const TexCoord t = tex_coord(p.x, p.y, H, W);
    corners[n] = make_int4(tex_corner_index(t, 0, W), tex_corner_index(t, 1, W), tex_corner_index(t, 2, W), tex_corner_index(t, 3, W));
}

__global__ void __launch_bounds__(256) k_tex_lookup_bwd(int N, const float2* uv, int H, int W, const int* row_start, const int* entries,
                                                        TexLayers L)
{
    const int texel = blockIdx.x * blockDim.x + threadIdx.x;
    const size_t plane = (size_t)H * W;
    if ((size_t)texel >= plane) return;
    const int begin = row_start[texel], end = row_start[texel + 1];
#pragma unroll
    for (int l = 0; l < FR_TEX_MAX_LAYERS; l++) {
        if (l >= L.n) break;
        const int C = L.C[l];
        float a0 = 0.f, a1 = 0.f, a2 = 0.f, a3 = 0.f;
        for (int j = begin; j < end; j++) {
            const int e = entries[j], point = e >> 2;          // entry = 4 * point + corner
            if ((unsigned)point >= (unsigned)N) continue;      // (a plan of another UV set: read nothing out of bounds)
            const float2 p = uv[point];
            const float w = tex_corner_weight(tex_coord(p.x, p.y, H, W), e & 3);
            const float* g = L.in[l] + (size_t)point * C;
            a0 += w * g[0];
            if (C > 1) a1 += w * g[1];
            if (C > 2) a2 += w * g[2];
            if (C > 3) a3 += w * g[3];
        }
        const float acc[4] = {a0, a1, a2, a3};
#pragma unroll
        for (int c = 0; c < 4; c++) {
            if (c >= C) break;
            float d = acc[c];
            if (L.act[l] != FR_TEX_ACT_IDENTITY) d *= tex_act_grad(L.act[l], L.a0[l], L.a1[l], L.tex[l][c * plane + texel]);
            L.out[l][c * plane + texel] = d;
        }
    }
}

static int check_common(const char* who, int32_t N, const float* uv, int32_t H, int32_t W)
{
    char msg[160];
    if (N < 0 || N > (1 << 29) || H <= 0 || W <= 0 || (int64_t)H * W > (1 << 29)) {
        snprintf(msg, sizeof(msg), "%s: N must be 0 .. 2^29 and H x W 1 .. 2^29 texels", who);
        return fail_msg(FR_ERR_INVALID_ARGUMENT, msg);
    }
    if (N > 0 && !uv) {
        snprintf(msg, sizeof(msg), "%s: null uv", who);
        return fail_msg(FR_ERR_INVALID_ARGUMENT, msg);
    }
    return FR_OK;
}

static int pack_layers(const char* who, int32_t n_layers, const fr_tex_layer* layers, bool backward, TexLayers& L)
{
    char msg[160];
    if (n_layers < 1 || n_layers > FR_TEX_MAX_LAYERS || !layers) {
        snprintf(msg, sizeof(msg), "%s: 1 .. FR_TEX_MAX_LAYERS (%d) layers", who, FR_TEX_MAX_LAYERS);
        return fail_msg(FR_ERR_INVALID_ARGUMENT, msg);
    }
    L = TexLayers{};
    L.n = n_layers;
    for (int l = 0; l < n_layers; l++) {
        const fr_tex_layer& s = layers[l];
        if (s.channels < 1 || s.channels > 4) {
            snprintf(msg, sizeof(msg), "%s: layer %d has %d channels (1 .. 4)", who, l, s.channels);
            return fail_msg(FR_ERR_INVALID_ARGUMENT, msg);
        }
        if (s.activation != FR_TEX_ACT_IDENTITY && s.activation != FR_TEX_ACT_TANH_SCALE && s.activation != FR_TEX_ACT_SOFTPLUS_CAP) {
            snprintf(msg, sizeof(msg), "%s: layer %d: unknown activation %d", who, l, s.activation);
            return fail_msg(FR_ERR_INVALID_ARGUMENT, msg);
        }
        const bool missing = backward ? (!s.d_out || !s.d_texture || (s.activation != FR_TEX_ACT_IDENTITY && !s.texture))
                                      : (!s.texture || !s.out);
        if (missing) {
            snprintf(msg, sizeof(msg), "%s: layer %d: null array", who, l);
            return fail_msg(FR_ERR_INVALID_ARGUMENT, msg);
        }
        L.tex[l] = s.texture, L.in[l] = s.d_out, L.out[l] = backward ? s.d_texture : s.out;
        L.C[l] = s.channels, L.act[l] = s.activation, L.a0[l] = s.a0, L.a1[l] = s.a1;
    }
    return FR_OK;
}

}  // namespace fr

using namespace fr;

extern "C" {

int fr_texture_corners(int32_t N, const float* uv, int32_t H, int32_t W, int32_t* corners, void* stream)
{
    int rc = check_common("fr_texture_corners", N, uv, H, W);
    if (rc) return rc;
    if (N == 0) return FR_OK;
    if (!corners) return fail_msg(FR_ERR_INVALID_ARGUMENT, "fr_texture_corners: null corners");
    hipLaunchKernelGGL(k_tex_corners, dim3((N + 255) / 256), dim3(256), 0, static_cast<hipStream_t>(stream), N,
                       reinterpret_cast<const float2*>(uv), H, W, reinterpret_cast<int4*>(corners));
    FR_HIP(hipGetLastError());
    return FR_OK;
}

int fr_texture_lookup(int32_t N, const float* uv, int32_t H, int32_t W, int32_t n_layers, const fr_tex_layer* layers, void* stream)
{
    int rc = check_common("fr_texture_lookup", N, uv, H, W);
    if (rc) return rc;
    TexLayers L;
    rc = pack_layers("fr_texture_lookup", n_layers, layers, false, L);
    if (rc) return rc;
    if (N == 0) return FR_OK;
    hipLaunchKernelGGL(k_tex_lookup, dim3((N + 255) / 256), dim3(256), 0, static_cast<hipStream_t>(stream), N,
                       reinterpret_cast<const float2*>(uv), H, W, L);
    FR_HIP(hipGetLastError());
    return FR_OK;
}

int fr_texture_lookup_backward(int32_t N, const float* uv, int32_t H, int32_t W, const int32_t* row_start, const int32_t* entries,
                               int32_t n_layers, const fr_tex_layer* layers, void* stream)
{
    int rc = check_common("fr_texture_lookup_backward", N, uv, H, W);
    if (rc) return rc;
    TexLayers L;
    rc = pack_layers("fr_texture_lookup_backward", n_layers, layers, true, L);
    if (rc) return rc;
    if (!row_start || (N > 0 && !entries)) return fail_msg(FR_ERR_INVALID_ARGUMENT, "fr_texture_lookup_backward: null plan (row_start / entries)");
    const int texels = H * W;
    hipLaunchKernelGGL(k_tex_lookup_bwd, dim3((texels + 255) / 256), dim3(256), 0, static_cast<hipStream_t>(stream), N,
                       reinterpret_cast<const float2*>(uv), H, W, row_start, entries, L);
    FR_HIP(hipGetLastError());
    return FR_OK;
}

}  // extern "C"
