// Bilinear look-up of Gaussian attributes in UV attribute maps, per point: the arithmetic shared by the forward kernel, the
// plan's corner kernel and the gather backward (fr_texture.hip).  One source of the expressions = the same texels and the
// same weight bits in all three.
//
// reference: model/uv_decoder.py:179-202 — F.grid_sample(texture, 2 uv - 1, mode="bilinear", padding_mode="border",
// align_corners=True) — behind the per-texture activations of :133-156.  The coordinate arithmetic is grid_sample's own, in
// its order and in fp32 (unnormalise with align_corners, clip to the border, floor, the four weights as differences); every
// translation unit that includes this is built with -ffp-contract=off.
#pragma once
#include "fr_common.hpp"

namespace fr {

// corner ids, in grid_sample's summation order: 0 = (y0, x0), 1 = (y0, x1), 2 = (y1, x0), 3 = (y1, x1)
struct TexCoord {
    int x0, y0;          // always inside the texture
    float ix, iy;        // clipped sample position in texels
    bool x1_in, y1_in;   // x0 + 1 < W, y0 + 1 < H: a corner past the last column / row has weight 0 and is not read
};

// one axis: g = 2u - 1; i = ((g + 1) / 2) * (size - 1); clip to [0, size - 1]  (a NaN coordinate clips to 0, as in torch)
__device__ __forceinline__ float tex_axis(float u, int size)
{
    const float g = 2.f * u - 1.f;
    const float i = ((g + 1.f) / 2.f) * (float)(size - 1);
    return fminf((float)(size - 1), fmaxf(i, 0.f));
}

__device__ __forceinline__ TexCoord tex_coord(float u, float v, int H, int W)
{
    TexCoord t;
    t.ix = tex_axis(u, W);   // u is x (width), v is y (height), no flip
    t.iy = tex_axis(v, H);
    t.x0 = (int)floorf(t.ix);
    t.y0 = (int)floorf(t.iy);
    t.x1_in = t.x0 + 1 < W;
    t.y1_in = t.y0 + 1 < H;
    return t;
}

// texel index (y * W + x) of a corner, -1 for a corner past the last row / column
__device__ __forceinline__ int tex_corner_index(const TexCoord& t, int corner, int W)
{
    const bool right = corner & 1, down = corner & 2;
    if ((right && !t.x1_in) || (down && !t.y1_in)) return -1;
    return (t.y0 + (down ? 1 : 0)) * W + t.x0 + (right ? 1 : 0);
}

// grid_sample's weights: nw = (x1 - ix)(y1 - iy), ne = (ix - x0)(y1 - iy), sw = (x1 - ix)(iy - y0), se = (ix - x0)(iy - y0)
__device__ __forceinline__ float tex_corner_weight(const TexCoord& t, int corner)
{
    const float x0 = (float)t.x0, y0 = (float)t.y0, x1 = x0 + 1.f, y1 = y0 + 1.f;
    const float wx = (corner & 1) ? (t.ix - x0) : (x1 - t.ix);
    const float wy = (corner & 2) ? (t.iy - y0) : (y1 - t.iy);
    return wx * wy;
}

// ---- per-texture activations (uv_decoder.py:133-156), applied to the TEXEL before interpolation
// softplus with torch's defaults: beta 1, linear above 20
__device__ __forceinline__ float tex_act(int act, float a0, float a1, float t)
{
    if (act == FR_TEX_ACT_TANH_SCALE) return tanhf(t) * a0;
    if (act == FR_TEX_ACT_SOFTPLUS_CAP) {
        const float x = -(t + a0) + a1;
        const float sp = x > 20.f ? x : log1pf(expf(x));
        return a1 - sp;
    }
    return t;
}

// d act / d t
__device__ __forceinline__ float tex_act_grad(int act, float a0, float a1, float t)
{
    if (act == FR_TEX_ACT_TANH_SCALE) {
        const float th = tanhf(t);
        return (1.f - th * th) * a0;
    }
    if (act == FR_TEX_ACT_SOFTPLUS_CAP) {
        const float x = -(t + a0) + a1;   // d/dt (a1 - softplus(x)) = softplus'(x) = e^x / (e^x + 1); 1 in the linear part
        if (x > 20.f) return 1.f;
        const float z = expf(x);
        return z / (z + 1.f);
    }
    return 1.f;
}

}  // namespace fr
