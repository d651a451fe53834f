// FateAvatar's VGG perceptual term on gfx950's exact-f32 MFMA: a frozen stack of 3 x 3 convolutions on the rendered image and
// its target, the mean |difference| of chosen layer outputs, and the gradient to the rendered image (fr_vgg_loss_grad,
// include/fr_rasterizer.h).
//
// reference: VGGPerceptualLoss.forward (tools/loss_utils/vgg_feature.py:24-47): (x - mean) / std, F.interpolate to 224^2,
// vgg16.features[:23] block by block, l1_loss of the four block outputs — about sixty vendor-library launches through
// autograd.  Nothing here mirrors a reference operation order.
//
// A 3 x 3 convolution over NHWC activations is fr_mlp.hip's GEMM with a GATHERED A tile: M = the pixels (of both images in
// the forward, of the rendered one in the backward), N = c_out, K = 9 c_in in tap-major, channel-minor order.  c_in is a
// multiple of the K step (32), so one K step lies inside ONE tap: the tap's (dy, dx) is uniform over the workgroup, a thread's
// 32 k are 32 consecutive channels of one neighbour pixel (a 128-byte line), and the neighbour's row comes from
// vgg_neighbour (fr_vgg_math.hpp) — which tests the COORDINATES and returns -1 for the halo, so that an out-of-image
// coordinate never becomes an address; rows past M carry y = -1 and are never looked up.  The rows' (y, x) are divided out
// ONCE per thread, ahead of the K loop.  B is the pre-packed weight [K][N], n contiguous.  Tiles, LDS layout (k-major, odd
// row stride) and the one step of software pipelining are k_mlp_gemm's.
//     forward      a_l = relu(gather(in) Wf_l + b_l)                                      epilogue: bias + ReLU
//     gradient     dIn_l = gather(dZ_l) Wb_l     Wb: taps flipped, c_in / c_out exchanged
//                  epilogue, no pool in front of l:  dZ_{l-1} = (dIn_l + tap gradient of l-1) * [a_{l-1} > 0]
//                  epilogue, pool in front of l:     dIn_l stored as it is; k_vgg_unpool routes it to the argmaxes of
//                                                    a_{l-1}'s windows and applies the tap gradient and the mask there
//     the LAST layer's dZ = sign(a - a_gt) / numel * [a > 0] is never stored: the gathered fetch of its gradient GEMM
//     computes it from the two saved activations (SEED).
// Occupancy: block 4 of VGG-16 at 224^2 is 1568 rows forward and 784 in the gradient — 200, 104 and 52 workgroups of 64 x 64 for
// 256 compute units.  A GEMM whose grid is that small is split over the nine taps into 3 or 9 planes (grid z), each storing its
// partial product, and k_vgg_split_reduce adds the planes in plane order and applies the epilogue: a fixed order, no atomics.
// 64 x 64 tiles everywhere: measured faster than 128 x 64 at every layer (EXPERIMENTS.md "r29"); the larger tile stays
// selectable (FR_VGG_TILE_128) and changes no bit, the split depends on the GEMM's shape alone.
// Layer 0 (K = 27, 0.6 % of the work) and its data gradient are plain VALU kernels.  The three max-pools are a small kernel
// of their own.  The terms' sums go through sum_over_workgroups: per-workgroup partials added by the last workgroup in index
// order.  The resize's backward is a gather per SOURCE pixel over the output pixels that blend it.  No float atomics.
// FAST flags (FMA contraction): the products are MFMA either way.
// The LPIPS term (fr_lpips_loss_grad) runs the same forward and the same gradient GEMMs with another term kind
// (VGG_TERM_LPIPS): its tap kernels and what they cost are described where they stand, below the L1 term's.
#include "fr_common.hpp"
#include "fr_vgg_math.hpp"

namespace fr {

constexpr int kVggBK = 32;          // K step through LDS
constexpr int kVggPad = 33;         // LDS row = tile + 33 floats (odd: the transposing store stays off a common bank)
constexpr int kVggThreads = 256;
constexpr unsigned kVggLossBlocks = FR_VGG_LOSS_BLOCKS;
constexpr int kVggFullGrid = 256;   // workgroups that fill the device's compute units: a smaller grid is split over the taps
static_assert(FR_VGG_REDUCE_BYTES == done_workspace_bytes(FR_VGG_LOSS_BLOCKS), "the header's size of the reduction scratch");

enum { VGG_EPI_BIAS_RELU = 0, VGG_EPI_PLAIN = 1, VGG_EPI_MASK = 2 };
// What a tap contributes to the gradient in the backward's epilogues, a compile-time kind.  L1: sign(a - a_gt) * tap_scale,
// computed in place from the two saved activations.  LPIPS: the tap's seed READ from a buffer the seed kernel has filled
// (`act_gt` then points at it; see the LPIPS section below).  The L1 instantiations contain no trace of the other kind.
enum { VGG_TERM_L1 = 0, VGG_TERM_LPIPS = 1 };

typedef float f32x16 __attribute__((ext_vector_type(16)));

__device__ __forceinline__ float sign_of(float d) { return d > 0.f ? 1.f : (d < 0.f ? -1.f : 0.f); }   // torch.sign: 0 at 0
// the last layer's dZ from its two saved activations
__device__ __forceinline__ float seed_value(float a, float a_gt, float scale) { return a > 0.f ? sign_of(a - a_gt) * scale : 0.f; }

struct VggGemmArgs {
    const float* A;        // gathered operand: NHWC rows of `ca` channels (an activation, a pooled input, or dZ)
    const float* A_gt;     // SEED: the target's rows of the same activation
    const float* B;        // packed weights [9 ca][N]
    float* C;              // [M, N]
    const float* bias;     // BIAS_RELU: [N]
    const float* act;      // MASK: the rendered image's saved output of the layer in front, [M, N]
    const float* act_gt;   // MASK with a tap on that layer: the target's (L1), or the tap's seed [M, N] (LPIPS)
    float seed_scale;      // SEED: 1 / numel of the last layer's term
    float tap_scale;       // MASK: 1 / numel of that layer's term, 0 without a tap
    int M, N, ca;
    int h, w;              // the extent of the rows' images (M = images x h x w)
    int taps;              // grid plane z sums the taps [z taps, (z + 1) taps) and stores at C + z plane (9 and one plane: all of K)
    unsigned plane;
};

// B tile: kVggBK x 64 values, lanes along n (contiguous)
__device__ __forceinline__ void vgg_fetch_b(float (&r)[8], const float* __restrict__ B, int N, int n0, int k0, int K, unsigned t)
{
#pragma unroll
    for (int i = 0; i < 8; i++) {
        const int n = n0 + (int)(t & 63u), k = k0 + (int)(t >> 6) + i * 4;
        float v = 0.f;
        if (n < N && k < K) v = B[(size_t)k * N + n];
        r[i] = v;
    }
}

// A tile: BM rows x kVggBK channels of ONE tap.  32 lanes = 32 consecutive channels of one row's neighbour.
template <int BM, bool SEED>
__device__ __forceinline__ void vgg_fetch_a(float (&r)[BM / 8], const VggGemmArgs& g, const int (&yx)[BM / 8], int m0, int k0, unsigned t)
{
    const float* __restrict__ A = g.A;
    const float* __restrict__ A_gt = g.A_gt;
    const int tap = k0 / g.ca, c = k0 - tap * g.ca + (int)(t & 31u);
#pragma unroll
    for (int i = 0; i < BM / 8; i++) {
        float v = 0.f;
        if (yx[i] >= 0) {      // (a row past M: -1)
            const int m = m0 + (int)(t >> 5) + i * 8;
            const int nb = vgg_neighbour(m, yx[i] >> 16, yx[i] & 0xffff, g.h, g.w, tap);
            if (nb >= 0) {
                const size_t o = (size_t)nb * g.ca + c;
                v = A[o];
                if (SEED) v = seed_value(v, A_gt[o], g.seed_scale);
            }
        }
        r[i] = v;
    }
}

template <int TM, bool SEED, int EPI, int KIND = VGG_TERM_L1>
__global__ void __launch_bounds__(kVggThreads) k_vgg_gemm(VggGemmArgs g)
{
    constexpr int BM = 64 * TM, BN = 64;
    __shared__ float As[kVggBK][BM + kVggPad];
    __shared__ float Bs[kVggBK][BN + kVggPad];
    const unsigned t = threadIdx.x, lane = t & 63u, wave = t >> 6;
    const int lr = (int)(lane & 31u), lh = (int)(lane >> 5);
    const int wm = (int)(wave >> 1) * 32 * TM, wn = (int)(wave & 1u) * 32;
    const int m0 = (int)blockIdx.x * BM, n0 = (int)blockIdx.y * BN;
    const int K = ((int)blockIdx.z + 1) * g.taps * g.ca, k_begin = (int)blockIdx.z * g.taps * g.ca;

    // this thread's rows: (y << 16) | x, or -1 past M
    int yx[BM / 8];
    {
        const int hw = g.h * g.w;
#pragma unroll
        for (int i = 0; i < BM / 8; i++) {
            const int m = m0 + (int)(t >> 5) + i * 8;
            yx[i] = -1;
            if (m < g.M) {
                const int p = m % hw;
                yx[i] = ((p / g.w) << 16) | (p % g.w);
            }
        }
    }

    // TWO accumulators per tile: the products of a K step go alternately to one and the other (k pairs 0, 2, 4 .. and 1, 3, 5 ..),
    // each a k-ordered chain of half the length, added once at the end — a chain of 9 x 512 products carries about 1.4 times
    // the rounding error of two of half that (measured against float64, EXPERIMENTS.md), and the second accumulator gives the
    // MFMA pipe an independent instruction to issue behind each dependent one.
    f32x16 acc[TM], acc_odd[TM];
#pragma unroll
    for (int i = 0; i < TM; i++)
#pragma unroll
        for (int r = 0; r < 16; r++) acc[i][r] = 0.f, acc_odd[i][r] = 0.f;

    float ra[BM / 8], rb[8];
    vgg_fetch_a<BM, SEED>(ra, g, yx, m0, k_begin, t);
    vgg_fetch_b(rb, g.B, g.N, n0, k_begin, K, t);
    for (int k0 = k_begin; k0 < K; k0 += kVggBK) {
        __syncthreads();    // (the previous step's operand reads are done)
#pragma unroll
        for (int i = 0; i < BM / 8; i++) As[t & 31u][(t >> 5) + i * 8] = ra[i];
#pragma unroll
        for (int i = 0; i < 8; i++) Bs[(t >> 6) + i * 4][t & 63u] = rb[i];
        __syncthreads();
        if (k0 + kVggBK < K) {
            vgg_fetch_a<BM, SEED>(ra, g, yx, m0, k0 + kVggBK, t);
            vgg_fetch_b(rb, g.B, g.N, n0, k0 + kVggBK, K, t);
        }
#pragma unroll
        for (int kk = 0; kk < kVggBK; kk += 2) {
            float a[TM];
#pragma unroll
            for (int i = 0; i < TM; i++) a[i] = As[kk + lh][wm + i * 32 + lr];
            const float b = Bs[kk + lh][wn + lr];
#pragma unroll
            for (int i = 0; i < TM; i++) {
                if ((kk & 2) == 0) acc[i] = __builtin_amdgcn_mfma_f32_32x32x2f32(a[i], b, acc[i], 0, 0, 0);
                else acc_odd[i] = __builtin_amdgcn_mfma_f32_32x32x2f32(a[i], b, acc_odd[i], 0, 0, 0);
            }
        }
    }
#pragma unroll
    for (int i = 0; i < TM; i++) acc[i] += acc_odd[i];

    // C/D map of the 32 x 32 tile: column = lane & 31, row = (r & 3) + 8 (r >> 2) + 4 (lane >> 5)
    const int col = n0 + wn + lr;
    if (col >= g.N) return;
    float* __restrict__ C = g.C + (size_t)blockIdx.z * g.plane;
    float bias = 0.f;
    if (EPI == VGG_EPI_BIAS_RELU) bias = g.bias[col];
#pragma unroll
    for (int i = 0; i < TM; i++) {
#pragma unroll
        for (int r = 0; r < 16; r++) {
            const int row = m0 + wm + i * 32 + (r & 3) + 8 * (r >> 2) + 4 * lh;
            if (row >= g.M) continue;
            const size_t o = (size_t)row * g.N + col;
            float v = acc[i][r];
            if (EPI == VGG_EPI_BIAS_RELU) v = fmaxf(v + bias, 0.f);
            if (EPI == VGG_EPI_MASK) {
                const float a = g.act[o];
                if (g.tap_scale != 0.f) v += KIND == VGG_TERM_LPIPS ? g.act_gt[o] : sign_of(a - g.act_gt[o]) * g.tap_scale;
                v = a > 0.f ? v : 0.f;
            }
            C[o] = v;
        }
    }
}

// A GEMM split over the taps: the planes' partial products added in plane order, then the epilogue the unsplit kernel would have
// applied.  One thread per four consecutive columns of a row (N is a multiple of 4).
template <int EPI, int KIND = VGG_TERM_L1>
__global__ void __launch_bounds__(kVggThreads) k_vgg_split_reduce(VggGemmArgs g, const float* __restrict__ partial, int planes)
{
    const unsigned i = blockIdx.x * kVggThreads + threadIdx.x, n4 = (unsigned)g.M * (unsigned)g.N / 4u;
    if (i >= n4) return;
    float4 s = reinterpret_cast<const float4*>(partial)[i];
    for (int z = 1; z < planes; z++) {
        const float4 p = reinterpret_cast<const float4*>(partial + (size_t)z * g.plane)[i];
        s.x += p.x, s.y += p.y, s.z += p.z, s.w += p.w;
    }
    float v[4] = {s.x, s.y, s.z, s.w};
    const size_t o = (size_t)i * 4;
    if (EPI == VGG_EPI_BIAS_RELU) {
        const float4 b = reinterpret_cast<const float4*>(g.bias)[(o % (unsigned)g.N) / 4];
        v[0] = fmaxf(v[0] + b.x, 0.f), v[1] = fmaxf(v[1] + b.y, 0.f), v[2] = fmaxf(v[2] + b.z, 0.f), v[3] = fmaxf(v[3] + b.w, 0.f);
    }
    if (EPI == VGG_EPI_MASK) {
        const float4 a4 = reinterpret_cast<const float4*>(g.act)[i];
        const float a[4] = {a4.x, a4.y, a4.z, a4.w};
        if (g.tap_scale != 0.f) {
            const float4 t4 = reinterpret_cast<const float4*>(g.act_gt)[i];
            const float t[4] = {t4.x, t4.y, t4.z, t4.w};
#pragma unroll
            for (int c = 0; c < 4; c++) v[c] += KIND == VGG_TERM_LPIPS ? t[c] : sign_of(a[c] - t[c]) * g.tap_scale;
        }
#pragma unroll
        for (int c = 0; c < 4; c++) v[c] = a[c] > 0.f ? v[c] : 0.f;
    }
    reinterpret_cast<float4*>(g.C)[i] = make_float4(v[0], v[1], v[2], v[3]);
}

// ---- the input: (x - mean) / std of both images, resized, NHWC.  One thread per output pixel.
struct VggInputArgs {
    const float* image;
    const float* target;
    float* x;                  // [2, sh, sw, 3]
    float* d_image;            // backward: [3,H,W]
    const float* d_x;          // backward: [sh, sw, 3] of image 0
    float mean[3], std[3];
    float scale_h, scale_w;    // (float)H / sh, (float)W / sw
    float weight;
    int H, W, sh, sw, accumulate;
};

__global__ void __launch_bounds__(kVggThreads) k_vgg_input(VggInputArgs a)
{
    const int n = a.sh * a.sw;
    const int i = (int)(blockIdx.x * kVggThreads + threadIdx.x);
    if (i >= 2 * n) return;
    const int img = i / n, p = i - img * n, oy = p / a.sw, ox = p - oy * a.sw;
    const float* __restrict__ src = img == 0 ? a.image : a.target;
    int y0, y1, x0, x1;
    float ly, lx;
    vgg_source(oy, a.scale_h, a.H, y0, y1, ly);
    vgg_source(ox, a.scale_w, a.W, x0, x1, lx);
    const size_t plane = (size_t)a.H * a.W;
#pragma unroll
    for (int c = 0; c < 3; c++) {
        const float* __restrict__ s = src + c * plane;
        const float v00 = (s[(size_t)y0 * a.W + x0] - a.mean[c]) / a.std[c], v01 = (s[(size_t)y0 * a.W + x1] - a.mean[c]) / a.std[c];
        const float v10 = (s[(size_t)y1 * a.W + x0] - a.mean[c]) / a.std[c], v11 = (s[(size_t)y1 * a.W + x1] - a.mean[c]) / a.std[c];
        // (torch's form; lam = 0 gives v00 exactly)
        a.x[(size_t)i * 3 + c] = (1.f - ly) * ((1.f - lx) * v00 + lx * v01) + ly * ((1.f - lx) * v10 + lx * v11);
    }
}

// the resize's backward: one thread per SOURCE pixel gathers from the output pixels that blend it, rows then columns ascending
__global__ void __launch_bounds__(kVggThreads) k_vgg_input_bwd(VggInputArgs a)
{
    const int i = (int)(blockIdx.x * kVggThreads + threadIdx.x);
    if (i >= a.H * a.W) return;
    const int Y = i / a.W, X = i - Y * a.W;
    int ylo, yhi, xlo, xhi;
    vgg_source_range(Y, a.scale_h, a.sh, ylo, yhi);
    vgg_source_range(X, a.scale_w, a.sw, xlo, xhi);
    const float* __restrict__ d_x = a.d_x;
    float s[3] = {0.f, 0.f, 0.f};
    for (int oy = ylo; oy <= yhi; oy++) {
        const float wy = vgg_source_weight(oy, Y, a.scale_h, a.H);
        if (wy == 0.f) continue;
        for (int ox = xlo; ox <= xhi; ox++) {
            const float wx = vgg_source_weight(ox, X, a.scale_w, a.W);
            if (wx == 0.f) continue;
            const float* __restrict__ d = d_x + ((size_t)oy * a.sw + ox) * 3;
#pragma unroll
            for (int c = 0; c < 3; c++) s[c] += wy * wx * d[c];
        }
    }
    const size_t plane = (size_t)a.H * a.W;
#pragma unroll
    for (int c = 0; c < 3; c++) {
        // (rounded on its own, then added: what accumulate adds is bit for bit what a storing call stores)
        const float v = __fmul_rn(a.weight, s[c] / a.std[c]);
        float* __restrict__ o = a.d_image + c * plane + i;
        *o = a.accumulate ? __fadd_rn(*o, v) : v;
    }
}

// ---- layer 0 (c_in = 3) and its data gradient: plain VALU
// one thread per (row, four output channels): 27 fmaf in k order each, the weights as float4
__global__ void __launch_bounds__(kVggThreads) k_vgg_conv0(const float* __restrict__ x, const float* __restrict__ Wf, const float* __restrict__ bias,
                                                        float* __restrict__ out, int M, int N, int h, int w)
{
    const unsigned n4 = (unsigned)N / 4u;
    const unsigned i = blockIdx.x * kVggThreads + threadIdx.x;
    if (i >= (unsigned)M * n4) return;
    const int m = (int)(i / n4), c4 = (int)(i % n4);
    const int p = m % (h * w), y = p / w, xx = p % w;
    float4 s = reinterpret_cast<const float4*>(bias)[c4];
#pragma unroll
    for (int tap = 0; tap < 9; tap++) {
        const int nb = vgg_neighbour(m, y, xx, h, w, tap);
        if (nb < 0) continue;
#pragma unroll
        for (int ci = 0; ci < 3; ci++) {
            const float v = x[(size_t)nb * 3 + ci];
            const float4 k = reinterpret_cast<const float4*>(Wf)[(size_t)(tap * 3 + ci) * n4 + c4];
            s.x = fmaf(v, k.x, s.x), s.y = fmaf(v, k.y, s.y), s.z = fmaf(v, k.z, s.z), s.w = fmaf(v, k.w, s.w);
        }
    }
    reinterpret_cast<float4*>(out)[i] = make_float4(fmaxf(s.x, 0.f), fmaxf(s.y, 0.f), fmaxf(s.z, 0.f), fmaxf(s.w, 0.f));
}

// one thread per row, its three input channels: 9 N products each in four interleaved chains (channel co goes to chain co % 4),
// combined as a fixed tree.  The weights' addresses are uniform over the wave.
template <bool SEED>
__global__ void __launch_bounds__(kVggThreads) k_vgg_conv0_bwd(const float* __restrict__ dz, const float* __restrict__ a_gt, float seed_scale,
                                                            const float* __restrict__ Wb, float* __restrict__ dx, int M, int N, int h, int w)
{
    const int m = (int)(blockIdx.x * kVggThreads + threadIdx.x);
    if (m >= M) return;
    const int y = m / w, xx = m % w;        // (image 0 only: m < h w)
    float s[3][4] = {};
    for (int tap = 0; tap < 9; tap++) {
        const int nb = vgg_neighbour(m, y, xx, h, w, tap);
        if (nb < 0) continue;
        const float4* __restrict__ row = reinterpret_cast<const float4*>(dz + (size_t)nb * N);
        const float4* __restrict__ row_gt = reinterpret_cast<const float4*>(a_gt + (size_t)nb * N);
        const float* __restrict__ wrow = Wb + (size_t)tap * N * 3;
        for (int co = 0; co < N; co += 4) {
            const float4 r = row[co / 4];
            float v[4] = {r.x, r.y, r.z, r.w};
            if (SEED) {
                const float4 t = row_gt[co / 4];
                v[0] = seed_value(v[0], t.x, seed_scale), v[1] = seed_value(v[1], t.y, seed_scale);
                v[2] = seed_value(v[2], t.z, seed_scale), v[3] = seed_value(v[3], t.w, seed_scale);
            }
#pragma unroll
            for (int q = 0; q < 4; q++)
#pragma unroll
                for (int ci = 0; ci < 3; ci++) s[ci][q] = fmaf(v[q], wrow[(size_t)(co + q) * 3 + ci], s[ci][q]);
        }
    }
#pragma unroll
    for (int ci = 0; ci < 3; ci++) dx[(size_t)m * 3 + ci] = (s[ci][0] + s[ci][1]) + (s[ci][2] + s[ci][3]);
}

// ---- 2 x 2 / 2 max-pool of an NHWC activation of `images` images of h x w (h, w even): one thread per (pooled pixel, channel)
__global__ void __launch_bounds__(kVggThreads) k_vgg_pool(const float* __restrict__ in, float* __restrict__ out, int images, int h, int w, int c)
{
    const int ph = h / 2, pw = w / 2;
    const unsigned i = blockIdx.x * kVggThreads + threadIdx.x;
    if (i >= (unsigned)(images * ph * pw) * (unsigned)c) return;
    const int ch = (int)(i % (unsigned)c), pm = (int)(i / (unsigned)c);
    const int img = pm / (ph * pw), q = pm - img * ph * pw, py = q / pw, px = q - py * pw;
    const size_t o = ((size_t)(img * h + 2 * py) * w + 2 * px) * c + ch, dn = (size_t)w * c;
    out[i] = fmaxf(fmaxf(in[o], in[o + c]), fmaxf(in[o + dn], in[o + dn + c]));
}

// the pool's backward with the layer in front's tap gradient and ReLU mask: dZ[window] of image 0 from the pooled gradient.
// The gradient goes to the FIRST maximum of the window in row-major order (torch's rule).
template <int KIND = VGG_TERM_L1>
__global__ void __launch_bounds__(kVggThreads) k_vgg_unpool(const float* __restrict__ d_pooled, const float* __restrict__ act,
                                                         const float* __restrict__ act_gt, float tap_scale, float* __restrict__ dz, int h,
                                                         int w, int c)
{
    const int ph = h / 2, pw = w / 2;
    const unsigned i = blockIdx.x * kVggThreads + threadIdx.x;
    if (i >= (unsigned)(ph * pw) * (unsigned)c) return;
    const int ch = (int)(i % (unsigned)c), pm = (int)(i / (unsigned)c);
    const int py = pm / pw, px = pm - py * pw;
    const size_t o = ((size_t)(2 * py) * w + 2 * px) * c + ch, dn = (size_t)w * c;
    const size_t at[4] = {o, o + c, o + dn, o + dn + c};
    float a[4];
#pragma unroll
    for (int k = 0; k < 4; k++) a[k] = act[at[k]];
    int best = 0;
#pragma unroll
    for (int k = 1; k < 4; k++)
        if (a[k] > a[best]) best = k;
    const float g = d_pooled[i];
#pragma unroll
    for (int k = 0; k < 4; k++) {
        float v = k == best ? g : 0.f;
        if (tap_scale != 0.f) v += KIND == VGG_TERM_LPIPS ? act_gt[at[k]] : sign_of(a[k] - act_gt[at[k]]) * tap_scale;
        dz[at[k]] = a[k] > 0.f ? v : 0.f;
    }
}

// ---- one term: mean |a - a_gt| over n elements, through the last-workgroup sum.  The LAST term's launch also adds the terms
// up, in order (the earlier terms' launches have completed: the stream orders them).
__global__ void __launch_bounds__(kSumThreads) k_vgg_tap_loss(const float* __restrict__ a, const float* __restrict__ a_gt, unsigned n,
                                                            float* partial, unsigned* counter, float* loss_out, int term, int total_terms)
{
    float acc[1] = {0.f};
    const unsigned n4 = n / 4, stride = gridDim.x * kSumThreads;     // (n = c_out h w: a multiple of 64)
    for (unsigned i = blockIdx.x * kSumThreads + threadIdx.x; i < n4; i += stride) {
        const float4 u = reinterpret_cast<const float4*>(a)[i], v = reinterpret_cast<const float4*>(a_gt)[i];
        acc[0] += (fabsf(u.x - v.x) + fabsf(u.y - v.y)) + (fabsf(u.z - v.z) + fabsf(u.w - v.w));
    }
    if (!sum_over_workgroups(acc, partial, kVggLossBlocks, counter, blockIdx.x, gridDim.x)) return;
    loss_out[1 + term] = acc[0] / (float)n;      // ((float)n is exact below 2^24; the quotient rounds once, a product with 1 / n twice)
    if (term + 1 == total_terms) {
        float s = 0.f;
        for (int k = 0; k < total_terms; k++) s += loss_out[1 + k];
        loss_out[0] = s;
    }
}

// ---- the LPIPS term (fr_lpips_loss_grad): per tap, with a / b the rendered / target feature [h,w,C] and w_c the learnt weights,
//     n_a(p) = sqrt(sum_c a_c(p)^2),  r_a = 1 / (n_a + 1e-10),  a^ = a r_a        (the same for b)
//     term   = (1 / (h w)) sum_p sum_c w_c (a^_c - b^_c)^2
//     dterm/da_c = r_a g_c - a^_c T / n_a,   g_c = 2 w_c (a^_c - b^_c) / (h w),   T = sum_c g_c a^_c
// A pixel with n == 0 has r = 0 (its hat vector is 0, it contributes sum_c w_c b^_c^2) and T / n_a = 0 (its gradient is exactly
// 0): stock autograd gives NaN there (sqrt's backward at 0); every unit behind such a pixel is a ReLU at 0 that passes nothing.
// One wave takes one pixel at a time: lane i holds channels i, 64 + i, .. (C / 64 <= 8 values per image, in registers), the sums
// over the channels are a per-lane chain in channel order and then the xor butterfly (the same bits in every lane).  The
// pixels' contributions stay per lane and go through sum_over_workgroups: a fixed grid, fixed orders, no float atomics.
// It leaves px[p] = (r_a, r_b, T / n_a) for the backward.
constexpr int kLpipsMaxPerLane = 8;     // C <= 512
constexpr float kLpipsEps = 1e-10f;

// a r_a - b r_b with both unit values rounded on their own: this unit compiles with -ffp-contract=fast, under which the
// back end fuses a product into the difference whatever the source says (a contract(off) pragma and __fmul_rn were both
// tried: the ISA kept v_fma), and the fused form leaves the other product's rounding error behind — identical images must
// give exactly 0.  The empty asm makes both products opaque to the combiner; it emits no instruction.
__device__ __forceinline__ float lpips_unit_diff(float a, float r_a, float b, float r_b, float& ah)
{
    ah = a * r_a;
    float bh = b * r_b;
    asm volatile("" : "+v"(ah), "+v"(bh));
    return ah - bh;
}

__global__ void __launch_bounds__(kSumThreads) k_lpips_tap(const float* __restrict__ a, const float* __restrict__ b, const float* __restrict__ lin,
                                                         float* __restrict__ px, unsigned P, int C, float* partial, unsigned* counter,
                                                         float* loss_out, int term, int total_terms)
{
    const unsigned lane = threadIdx.x & 63u, wave = threadIdx.x >> 6;
    const int nv = C / 64;
    float wl[kLpipsMaxPerLane];
#pragma unroll
    for (int j = 0; j < kLpipsMaxPerLane; j++) wl[j] = j < nv ? lin[j * 64 + (int)lane] : 0.f;
    const float two_inv = 2.f / (float)P;
    float acc[1] = {0.f};
    for (unsigned p = blockIdx.x * 4u + wave; p < P; p += gridDim.x * 4u) {     // (uniform over the wave)
        const float* __restrict__ ra = a + (size_t)p * C + lane;
        const float* __restrict__ rb = b + (size_t)p * C + lane;
        float va[kLpipsMaxPerLane], vb[kLpipsMaxPerLane];
        float sa = 0.f, sb = 0.f;
#pragma unroll
        for (int j = 0; j < kLpipsMaxPerLane; j++) {
            va[j] = j < nv ? ra[j * 64] : 0.f, vb[j] = j < nv ? rb[j * 64] : 0.f;
            sa = fmaf(va[j], va[j], sa), sb = fmaf(vb[j], vb[j], sb);
        }
        const float na = sqrtf(group_sum<64>(sa)), nb = sqrtf(group_sum<64>(sb));
        const float r_a = na > 0.f ? 1.f / (na + kLpipsEps) : 0.f, r_b = nb > 0.f ? 1.f / (nb + kLpipsEps) : 0.f;
        float s = 0.f, t = 0.f;
#pragma unroll
        for (int j = 0; j < kLpipsMaxPerLane; j++) {
            float ah;
            const float d = lpips_unit_diff(va[j], r_a, vb[j], r_b, ah), wd = wl[j] * d;
            s = fmaf(wd, d, s), t = fmaf(wd, ah, t);
        }
        acc[0] += s;
        t = group_sum<64>(t) * two_inv;
        if (lane == 0) {
            float* o = px + (size_t)p * 3;
            o[0] = r_a, o[1] = r_b, o[2] = na > 0.f ? t / na : 0.f;
        }
    }
    if (!sum_over_workgroups(acc, partial, kVggLossBlocks, counter, blockIdx.x, gridDim.x)) return;
    loss_out[1 + term] = acc[0] / (float)P;
    if (term + 1 == total_terms) {
        float s = 0.f;
        for (int k = 0; k < total_terms; k++) s += loss_out[1 + k];
        loss_out[0] = s;
    }
}

// A tap's gradient seed, already behind the layer's ReLU mask: seed(p, c) = [a > 0] (r_a (2 w_c / (h w)) (a r_a - b r_b) - a r_a T/n_a).
// One thread per four channels of a pixel.  The LAST tap's seed is that layer's dZ and is written to a gradient buffer; an
// earlier tap's goes to the seed buffer, which the epilogue that leaves the layer behind it adds (VGG_TERM_LPIPS).
__global__ void __launch_bounds__(kVggThreads) k_lpips_seed(const float* __restrict__ a, const float* __restrict__ b, const float* __restrict__ lin,
                                                          const float* __restrict__ px, float* __restrict__ out, unsigned P, int C)
{
    const unsigned c4n = (unsigned)C / 4u, i = blockIdx.x * kVggThreads + threadIdx.x;
    if (i >= P * c4n) return;
    const unsigned p = i / c4n, c4 = i - p * c4n;
    const float r_a = px[(size_t)p * 3], r_b = px[(size_t)p * 3 + 1], tn = px[(size_t)p * 3 + 2];
    const float two_inv = 2.f / (float)P;
    const float4 u = reinterpret_cast<const float4*>(a)[i], v = reinterpret_cast<const float4*>(b)[i], w4 = reinterpret_cast<const float4*>(lin)[c4];
    const float ua[4] = {u.x, u.y, u.z, u.w}, ub[4] = {v.x, v.y, v.z, v.w}, w[4] = {w4.x, w4.y, w4.z, w4.w};
    float o[4];
#pragma unroll
    for (int c = 0; c < 4; c++) {
        float ah;
        const float d = lpips_unit_diff(ua[c], r_a, ub[c], r_b, ah);
        o[c] = ua[c] > 0.f ? r_a * (two_inv * w[c]) * d - ah * tn : 0.f;
    }
    reinterpret_cast<float4*>(out)[i] = make_float4(o[0], o[1], o[2], o[3]);
}

// ---- host side
struct VggPlan {
    int n_layers, terms;
    int h[FR_VGG_MAX_LAYERS], w[FR_VGG_MAX_LAYERS];     // layer l's output extent
    size_t wf[FR_VGG_MAX_LAYERS], wb[FR_VGG_MAX_LAYERS];  // float offsets of its packed weights
    size_t off_x, off_act[FR_VGG_MAX_LAYERS], off_pool, off_grad[2], off_raw, off_split, bytes;
    // LPIPS only, appended BEHIND the layout above (which keeps its offsets): every tap's per-pixel scalars, one seed buffer
    size_t lin[FR_VGG_MAX_LAYERS];      // float offset of a tapped layer's weights inside `lin`
    size_t off_px[FR_VGG_MAX_LAYERS], off_seed, lpips_bytes;
};

// Into how many groups of taps a GEMM of M rows and N columns is split: a grid of 64 x 64 tiles that would leave compute units
// idle is multiplied by 3 or by 9 planes (block 4 of VGG-16 at 224^2: 200 workgroups forward, 104 and 52 in the gradient, for
// 256 CUs).  A function of the GEMM's shape alone: the tile choice does not enter, so it changes no bit.
static int vgg_splits(long long M, long long N)
{
    const long long tiles = ((M + 63) / 64) * ((N + 63) / 64);
    return tiles >= kVggFullGrid ? 1 : (3 * tiles >= kVggFullGrid ? 3 : 9);
}

const char* vgg_invalid(const fr_vgg* v)
{
    if (!v) return "null descriptor";
    if (v->n_layers < 1 || v->n_layers > FR_VGG_MAX_LAYERS) return "1 <= n_layers <= FR_VGG_MAX_LAYERS";
    if (v->H < 1 || v->W < 1 || (long long)v->H * v->W * 3 > 0x7fffffffLL) return "H, W >= 1 and 3 H W < 2^31";
    if (v->size_h < 1 || v->size_w < 1 || v->size_h > 32767 || v->size_w > 32767) return "1 <= size_h, size_w <= 32767";
    if ((v->tile & ~(3 | FR_VGG_NO_SPLIT)) || (v->tile & 3) == 3) return "tile is FR_VGG_TILE_AUTO, _64 or _128, plus FR_VGG_NO_SPLIT";
    int pools = 0;
    long long widest = 0;
    for (int l = 0; l < v->n_layers; l++) {
        const fr_vgg_layer& y = v->layers[l];
        if (y.c_in != (l == 0 ? 3 : v->layers[l - 1].c_out)) return "layer 0 has c_in = 3, every later c_in is the c_out in front of it";
        if (l > 0 && y.c_in % 32 != 0) return "c_in of every layer but the first is a multiple of 32";
        if (y.c_out < 64 || y.c_out % 64 != 0) return "every c_out is a multiple of 64";
        if (l == 0 && y.pool_before) return "layer 0 takes no pool";
        pools += y.pool_before ? 1 : 0;
        if (pools > 15 || v->size_h % (1 << pools) != 0 || v->size_w % (1 << pools) != 0) return "size_h and size_w are divisible by 2^(number of pools)";
        const long long rows = 2LL * (v->size_h >> pools) * (v->size_w >> pools);
        widest = widest > rows * y.c_out ? widest : rows * y.c_out;
        if (y.pool_before) widest = widest > 4 * rows * y.c_in ? widest : 4 * rows * y.c_in;
    }
    if (!v->layers[v->n_layers - 1].tap_after) return "the last layer must have tap_after";
    if (widest > 0x7fffffffLL) return "an activation of 2^31 or more elements";
    for (int c = 0; c < 3; c++)
        if (!(v->std[c] != 0.f)) return "std is nonzero";
    return nullptr;
}

static VggPlan vgg_plan(const fr_vgg& v)
{
    VggPlan p{};
    p.n_layers = v.n_layers;
    int h = v.size_h, w = v.size_w;
    size_t wf = 0, wb = 0, pool_max = 0, grad_max = 0, split_max = 0, o = align_up(FR_VGG_REDUCE_BYTES, 256);
    p.off_x = o, o += align_up((size_t)2 * h * w * 3 * sizeof(float), 256);
    for (int l = 0; l < v.n_layers; l++) {
        const fr_vgg_layer& y = v.layers[l];
        if (y.pool_before) {
            h /= 2, w /= 2;
            pool_max = pool_max > (size_t)h * w * y.c_in ? pool_max : (size_t)h * w * y.c_in;
        }
        p.h[l] = h, p.w[l] = w;
        p.wf[l] = wf, wf += (size_t)9 * y.c_in * y.c_out + y.c_out;
        p.wb[l] = wb, wb += (size_t)9 * y.c_in * y.c_out;
        p.terms += y.tap_after ? 1 : 0;
        p.off_act[l] = o, o += align_up((size_t)2 * h * w * y.c_out * sizeof(float), 256);
        grad_max = grad_max > (size_t)h * w * y.c_out ? grad_max : (size_t)h * w * y.c_out;
        if (l > 0) {    // the forward GEMM (both images) and the gradient GEMM (one), where they are split
            const int sf = vgg_splits(2LL * h * w, y.c_out), sb = vgg_splits((long long)h * w, y.c_in);
            const size_t need_f = sf > 1 ? (size_t)sf * 2 * h * w * y.c_out : 0, need_b = sb > 1 ? (size_t)sb * h * w * y.c_in : 0;
            split_max = split_max > need_f ? split_max : need_f;
            split_max = split_max > need_b ? split_max : need_b;
        }
    }
    p.off_pool = o, o += align_up(2 * pool_max * sizeof(float), 256);
    for (int k = 0; k < 2; k++) p.off_grad[k] = o, o += align_up(grad_max * sizeof(float), 256);
    p.off_raw = o, o += align_up(pool_max * sizeof(float), 256);
    p.off_split = o, o += align_up(split_max * sizeof(float), 256);
    p.bytes = o;
    size_t lin = 0, seed_max = 0;
    for (int l = 0; l < v.n_layers; l++) {
        if (!v.layers[l].tap_after) continue;
        const size_t px = (size_t)p.h[l] * p.w[l];
        p.lin[l] = lin, lin += v.layers[l].c_out;
        p.off_px[l] = o, o += align_up(px * 3 * sizeof(float), 256);
        if (l + 1 < v.n_layers) seed_max = seed_max > px * v.layers[l].c_out ? seed_max : px * v.layers[l].c_out;
    }
    p.off_seed = o, o += align_up(seed_max * sizeof(float), 256);
    p.lpips_bytes = o;
    return p;
}

size_t vgg_workspace_bytes(const fr_vgg& v) { return vgg_plan(v).bytes; }
size_t lpips_workspace_bytes(const fr_vgg& v) { return vgg_plan(v).lpips_bytes; }

const char* lpips_invalid(const fr_vgg* v)
{
    if (const char* why = vgg_invalid(v)) return why;
    for (int l = 0; l < v->n_layers; l++)
        if (v->layers[l].tap_after && v->layers[l].c_out > 64 * kLpipsMaxPerLane) return "a tapped layer of the LPIPS term has c_out <= 512";
    return nullptr;
}

static unsigned vgg_blocks(size_t n) { return (unsigned)((n + kVggThreads - 1) / kVggThreads); }

template <bool SEED, int EPI, int KIND = VGG_TERM_L1>
static void vgg_gemm(VggGemmArgs g, int tile, float* split_space, hipStream_t s)
{
    const unsigned ny = (unsigned)((g.N + 63) / 64);
    const unsigned nx128 = (unsigned)((g.M + 127) / 128), nx64 = (unsigned)((g.M + 63) / 64);
    const bool big = (tile & 3) == FR_VGG_TILE_128;      // (FR_VGG_TILE_AUTO: 64 x 64 everywhere, the faster at every layer measured)
    const unsigned planes = (tile & FR_VGG_NO_SPLIT) ? 1u : (unsigned)vgg_splits(g.M, g.N);
    g.taps = 9 / (int)planes, g.plane = 0;
    if (planes == 1) {
        if (big) hipLaunchKernelGGL((k_vgg_gemm<2, SEED, EPI, KIND>), dim3(nx128, ny), dim3(kVggThreads), 0, s, g);
        else hipLaunchKernelGGL((k_vgg_gemm<1, SEED, EPI, KIND>), dim3(nx64, ny), dim3(kVggThreads), 0, s, g);
        return;
    }
    VggGemmArgs part = g;
    part.C = split_space, part.plane = (unsigned)g.M * (unsigned)g.N;
    if (big) hipLaunchKernelGGL((k_vgg_gemm<2, SEED, VGG_EPI_PLAIN>), dim3(nx128, ny, planes), dim3(kVggThreads), 0, s, part);
    else hipLaunchKernelGGL((k_vgg_gemm<1, SEED, VGG_EPI_PLAIN>), dim3(nx64, ny, planes), dim3(kVggThreads), 0, s, part);
    g.plane = part.plane;
    hipLaunchKernelGGL((k_vgg_split_reduce<EPI, KIND>), dim3(vgg_blocks((size_t)g.M * g.N / 4)), dim3(kVggThreads), 0, s, g, split_space, (int)planes);
}

template <int KIND>
static int vgg_run(const fr_vgg& v, const float* lin, float weight, int accumulate, float* loss_out, float* d_image, void* workspace, hipStream_t s)
{
    const VggPlan p = vgg_plan(v);
    char* base = static_cast<char*>(workspace);
    const DoneWorkspace done = done_workspace(workspace);
    auto at = [&](size_t off) { return reinterpret_cast<float*>(base + off); };
    float* x = at(p.off_x);
    const int L = v.n_layers;

    VggInputArgs in{};
    in.image = v.image, in.target = v.target, in.x = x;
    for (int c = 0; c < 3; c++) in.mean[c] = v.mean[c], in.std[c] = v.std[c];
    in.scale_h = (float)v.H / (float)v.size_h, in.scale_w = (float)v.W / (float)v.size_w;
    in.H = v.H, in.W = v.W, in.sh = v.size_h, in.sw = v.size_w;
    hipLaunchKernelGGL(k_vgg_input, dim3(vgg_blocks((size_t)2 * v.size_h * v.size_w)), dim3(kVggThreads), 0, s, in);

    // ---- forward, both images
    for (int l = 0; l < L; l++) {
        const fr_vgg_layer& y = v.layers[l];
        const int h = p.h[l], w = p.w[l], M = 2 * h * w;
        const float* Wf = v.weights_fwd + p.wf[l];
        const float* bias = Wf + (size_t)9 * y.c_in * y.c_out;
        if (l == 0) {
            hipLaunchKernelGGL(k_vgg_conv0, dim3(vgg_blocks((size_t)M * y.c_out / 4)), dim3(kVggThreads), 0, s, x, Wf, bias, at(p.off_act[0]), M,
                               y.c_out, h, w);
            continue;
        }
        const float* src = at(p.off_act[l - 1]);
        if (y.pool_before) {
            hipLaunchKernelGGL(k_vgg_pool, dim3(vgg_blocks((size_t)M * y.c_in)), dim3(kVggThreads), 0, s, src, at(p.off_pool), 2, 2 * h, 2 * w,
                               y.c_in);
            src = at(p.off_pool);
        }
        VggGemmArgs g{};
        g.A = src, g.B = Wf, g.C = at(p.off_act[l]), g.bias = bias;
        g.M = M, g.N = y.c_out, g.ca = y.c_in, g.h = h, g.w = w;
        vgg_gemm<false, VGG_EPI_BIAS_RELU>(g, v.tile, at(p.off_split), s);
    }

    // ---- the terms
    float inv_n[FR_VGG_MAX_LAYERS];
    for (int l = 0, term = 0; l < L; l++) {
        const size_t n = (size_t)p.h[l] * p.w[l] * v.layers[l].c_out;
        inv_n[l] = (float)(1.0 / (double)n);
        if (!v.layers[l].tap_after) continue;
        const float* a = at(p.off_act[l]);
        if (KIND == VGG_TERM_LPIPS) {
            const unsigned P = (unsigned)(p.h[l] * p.w[l]);
            hipLaunchKernelGGL(k_lpips_tap, dim3(capped_blocks(P, 4, kVggLossBlocks)), dim3(kSumThreads), 0, s, a, a + n, lin + p.lin[l], at(p.off_px[l]),
                               P, v.layers[l].c_out, done.partial, done.counter, loss_out, term, p.terms);
        } else {
            hipLaunchKernelGGL(k_vgg_tap_loss, dim3(capped_blocks(n / 4, kSumThreads, kVggLossBlocks)), dim3(kSumThreads), 0, s, a, a + n, (unsigned)n,
                               done.partial, done.counter, loss_out, term, p.terms);
        }
        term++;
    }
    if (!d_image) {
        FR_HIP(hipGetLastError());
        return FR_OK;
    }

    // ---- the data gradient of the rendered branch, last layer first.  `cur`: dZ of the layer being left (none yet for the last)
    int side = 0;
    const float* cur = nullptr;
    // LPIPS: a tap's seed from its two activations, the pixels' scalars and its weights
    auto lpips_seed = [&](int l, float* out) {
        const unsigned P = (unsigned)(p.h[l] * p.w[l]);
        const int C = v.layers[l].c_out;
        const float* a = at(p.off_act[l]);
        hipLaunchKernelGGL(k_lpips_seed, dim3(vgg_blocks((size_t)P * C / 4)), dim3(kVggThreads), 0, s, a, a + (size_t)P * C, lin + p.lin[l],
                           at(p.off_px[l]), out, P, C);
    };
    if (KIND == VGG_TERM_LPIPS) {       // the last layer's dZ is materialised: the plain (non-SEED) fetch from the start
        lpips_seed(L - 1, at(p.off_grad[0]));
        cur = at(p.off_grad[0]), side = 1;
    }
    for (int l = L - 1; l >= 1; l--) {
        const fr_vgg_layer& y = v.layers[l];
        const fr_vgg_layer& front = v.layers[l - 1];
        const int h = p.h[l], w = p.w[l], M = h * w;
        const float* act = at(p.off_act[l - 1]);
        const float* act_gt = act + (size_t)p.h[l - 1] * p.w[l - 1] * front.c_out;
        const float tap_scale = front.tap_after ? inv_n[l - 1] : 0.f;
        float* next = at(p.off_grad[side]);
        VggGemmArgs g{};
        g.B = v.weights_bwd + p.wb[l];
        g.M = M, g.N = y.c_in, g.ca = y.c_out, g.h = h, g.w = w;
        g.C = y.pool_before ? at(p.off_raw) : next;
        g.act = act, g.act_gt = act_gt, g.tap_scale = tap_scale;
        if (KIND == VGG_TERM_LPIPS) {
            if (front.tap_after) lpips_seed(l - 1, at(p.off_seed)), g.act_gt = at(p.off_seed);
            g.A = cur;
            if (y.pool_before) {
                vgg_gemm<false, VGG_EPI_PLAIN>(g, v.tile, at(p.off_split), s);
                hipLaunchKernelGGL((k_vgg_unpool<VGG_TERM_LPIPS>), dim3(vgg_blocks((size_t)M * y.c_in)), dim3(kVggThreads), 0, s, at(p.off_raw), act,
                                   g.act_gt, tap_scale, next, 2 * h, 2 * w, y.c_in);
            } else {
                vgg_gemm<false, VGG_EPI_MASK, VGG_TERM_LPIPS>(g, v.tile, at(p.off_split), s);
            }
            cur = next, side ^= 1;
            continue;
        }
        if (cur) {
            g.A = cur;
            if (y.pool_before) vgg_gemm<false, VGG_EPI_PLAIN>(g, v.tile, at(p.off_split), s);
            else vgg_gemm<false, VGG_EPI_MASK>(g, v.tile, at(p.off_split), s);
        } else {
            g.A = at(p.off_act[l]), g.A_gt = g.A + (size_t)M * y.c_out, g.seed_scale = inv_n[l];
            if (y.pool_before) vgg_gemm<true, VGG_EPI_PLAIN>(g, v.tile, at(p.off_split), s);
            else vgg_gemm<true, VGG_EPI_MASK>(g, v.tile, at(p.off_split), s);
        }
        if (y.pool_before)
            hipLaunchKernelGGL((k_vgg_unpool<VGG_TERM_L1>), dim3(vgg_blocks((size_t)M * y.c_in)), dim3(kVggThreads), 0, s, at(p.off_raw), act, act_gt, tap_scale,
                               next, 2 * h, 2 * w, y.c_in);
        cur = next, side ^= 1;
    }
    {
        const int h = p.h[0], w = p.w[0], M = h * w, N = v.layers[0].c_out;
        const float* Wb = v.weights_bwd + p.wb[0];
        float* dx = at(p.off_grad[side]);
        const float* a0 = at(p.off_act[0]);
        if (cur) hipLaunchKernelGGL((k_vgg_conv0_bwd<false>), dim3(vgg_blocks((size_t)M)), dim3(kVggThreads), 0, s, cur, cur, 0.f, Wb, dx, M, N, h, w);
        else hipLaunchKernelGGL((k_vgg_conv0_bwd<true>), dim3(vgg_blocks((size_t)M)), dim3(kVggThreads), 0, s, a0, a0 + (size_t)M * N, inv_n[0], Wb, dx, M, N, h, w);
        in.d_x = dx, in.d_image = d_image, in.weight = weight, in.accumulate = accumulate;
        hipLaunchKernelGGL(k_vgg_input_bwd, dim3(vgg_blocks((size_t)v.H * v.W)), dim3(kVggThreads), 0, s, in);
    }
    FR_HIP(hipGetLastError());
    return FR_OK;
}

int launch_vgg_loss_grad(const fr_vgg& v, float weight, int accumulate, float* loss_out, float* d_image, void* workspace, hipStream_t s)
{
    return vgg_run<VGG_TERM_L1>(v, nullptr, weight, accumulate, loss_out, d_image, workspace, s);
}

int launch_lpips_loss_grad(const fr_vgg& v, const float* lin, float weight, int accumulate, float* loss_out, float* d_image, void* workspace,
                           hipStream_t s)
{
    return vgg_run<VGG_TERM_LPIPS>(v, lin, weight, accumulate, loss_out, d_image, workspace, s);
}

}  // namespace fr
