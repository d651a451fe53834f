// The index math of the perceptual term (fr_vgg.hip), shared with the host so that a stand-alone program can enumerate it
// (tests/test_vgg_host.py): where a convolution tap of a pixel lies, and which source pixels a resized pixel blends.
// Plain C++: no HIP types, no includes beyond <math.h>.
#pragma once
#include <math.h>

#if defined(__HIPCC__)
#define FR_VGG_HD __host__ __device__ __forceinline__
#else
#define FR_VGG_HD static inline
#endif

namespace fr {

// Row `m` of an NHWC activation of n images of h x w pixels is pixel (y, x) of image m / (h w).  The row of its 3 x 3
// neighbour `tap` = 3 ky + kx, i.e. of (y + ky - 1, x + kx - 1) in the same image, or -1 when that lies outside the image
// (the convolution's zero padding).  The bounds are tested on the COORDINATES: an out-of-image coordinate is never turned
// into a row, so the result is -1 or a row of the same image.
FR_VGG_HD int vgg_neighbour(int m, int y, int x, int h, int w, int tap)
{
    const int dy = tap / 3 - 1, dx = tap % 3 - 1;
    const int ny = y + dy, nx = x + dx;
    if (ny < 0 || ny >= h || nx < 0 || nx >= w) return -1;
    return m + dy * w + dx;
}

// F.interpolate(mode='bilinear', align_corners=False, antialias=False) along one axis: output index `o` blends the source
// indices i0 and i1 with weights (1 - lam) and lam.  scale = (float)in_size / (float)out_size.  The source coordinate
// (o + 0.5) scale - 0.5 is clamped at 0 and the upper index at the edge (i1 == i0 there, and both weights go to it).
// scale == 1 gives i0 = o, lam = 0 exactly: the identity.
FR_VGG_HD void vgg_source(int o, float scale, int in_size, int& i0, int& i1, float& lam)
{
    float s = fmaf(scale, (float)o + 0.5f, -0.5f);
    if (s < 0.f) s = 0.f;
    i0 = (int)s;
    if (i0 > in_size - 1) i0 = in_size - 1;
    i1 = i0 + (i0 < in_size - 1 ? 1 : 0);
    lam = s - (float)i0;
}

// The output indices that can blend source index `i`: a closed range [lo, hi] inside [0, out_size - 1] (possibly empty:
// lo > hi) that CONTAINS every o with i0 == i or i1 == i.  It is generous by two on either side; the gather tests every
// candidate with vgg_source itself.
FR_VGG_HD void vgg_source_range(int i, float scale, int out_size, int& lo, int& hi)
{
    lo = (int)floorf(((float)i - 0.5f) / scale - 0.5f) - 2;
    hi = (int)ceilf(((float)i + 1.5f) / scale - 0.5f) + 2;
    if (lo < 0) lo = 0;
    if (hi > out_size - 1) hi = out_size - 1;
}

// the weight with which output index o takes source index i (0 when it does not)
FR_VGG_HD float vgg_source_weight(int o, int i, float scale, int in_size)
{
    int i0, i1;
    float lam;
    vgg_source(o, scale, in_size, i0, i1, lam);
    return (i0 == i ? 1.f - lam : 0.f) + (i1 == i ? lam : 0.f);
}

}  // namespace fr
