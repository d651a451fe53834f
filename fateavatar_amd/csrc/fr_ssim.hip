// Fused L1 + D-SSIM image loss and its gradient with respect to the rendered image, two launches.
//
// reference: GaussianAvatarsLoss (train/loss.py:351-365, weights of config/gaussianavatars.yaml:16-20) and the original 3DGS
// objective: loss = rgb_weight x L1(render, gt) + dssim_weight x d_ssim(render, gt), with d_ssim of
// tools/loss_utils/dssim.py:28-56 — five grouped F.conv2d with an 11 x 11 Gaussian window (sigma 1.5, zero padding 5) and a
// dozen elementwise kernels, all of them again in autograd's backward.  Per channel, x = render, y = target:
//     mu1 = conv(x), mu2 = conv(y), E11 = conv(x x), E22 = conv(y y), E12 = conv(x y)
//     s11 = E11 - mu1^2, s22 = E22 - mu2^2, s12 = E12 - mu1 mu2
//     A = 2 mu1 mu2 + C1, B = 2 s12 + C2, Cc = mu1^2 + mu2^2 + C1, D = s11 + s22 + C2,   S = A B / (Cc D)
//     d_ssim = 1 - mean(S)
// and, with dS11 = dS/ds11 = -A B / (Cc D^2), dS12 = dS/ds12 = 2 A / (Cc D),
//     dM = dS/dmu1 = 2 mu2 B / (Cc D) - 2 mu1 A B / (Cc^2 D) - 2 mu1 dS11 - mu2 dS12
//     d d_ssim / dx = -(1/N) [ conv(dM) + 2 x conv(dS11) + y conv(dS12) ]        (the window is symmetric)
//
// Pass 1 (k_image_loss_maps) evaluates S and the three derivative maps per pixel and stores the maps; pass 2
// (k_image_loss_grad) convolves the maps and writes the gradient, the L1 term folded in.  Two launches, because pass 2 needs
// pass 1's maps of the neighbouring tiles.  Both convolve separably: a workgroup of 256 threads owns a 32 x 32 tile of one
// channel of one image, stages the 42 x 42 halo in LDS, runs the horizontal 11-tap pass into LDS (42 rows x 32 columns per
// quantity) and the vertical pass in registers (a thread owns 4 consecutive rows of one column: 14 LDS reads per quantity
// for 44 multiply-adds).  LDS row strides: 43 words for the staged halo (odd: the rows of a wave's two half-rows fall on
// different banks) and 40 for the horizontal results (a wave reads columns 0 .. 31 of rows r and r + 4: 4 x 40 = 160 = 32
// mod 64, the two halves of the wave use the two halves of the 64 banks).  48 KB (pass 1) and 42 KB (pass 2) of LDS per
// workgroup: three workgroups per CU.  No float atomics: every output has one owner, and the loss sums go through
// per-workgroup partials that the workgroup finishing last adds up in index order (sum_over_workgroups, fr_common.hpp) — results are
// bit-reproducible.  Built with FMA contraction (Makefile).
#include "fr_common.hpp"

#include <cmath>

namespace fr {

constexpr int kSsimTile = 32, kRad = 5, kTaps = 2 * kRad + 1, kHalo = kSsimTile + 2 * kRad;
constexpr int kInStride = 43, kRowStride = 40;
constexpr int kRowsPerThread = 4, kThreads = kSsimTile * kSsimTile / kRowsPerThread;   // 256
constexpr float kC1 = 0.01f * 0.01f, kC2 = 0.03f * 0.03f;
static_assert(kThreads == kSumThreads && (kRowsPerThread * kRowStride) % 64 == 32 && kRowStride >= kSsimTile && kInStride >= kHalo, "tile geometry");

struct SsimView {   // one image of a launch
    const float* img;
    const float* gt;
    float* grad;          // null: losses only (no maps stored, pass 2 does nothing for the image)
    float* loss;          // {total, l1, d_ssim}
    unsigned* counter;
    float* partial;       // [2][n_wg]: sums of 1 - S and of |x - y|
    float* maps;          // [3][C][H][W]: dM, dS11, dS12
};

struct SsimArgs {
    BatchOf<SsimView> b;
    int C, H, W;
    unsigned tiles_x, tiles_y;
    float w[kTaps];
    float inv_n;          // 1 / (C H W)
    float g_l1, g_ssim;   // rgb_weight / N, -dssim_weight / N
    float rgb_weight, dssim_weight;
};

// the (tile + 10)^2 halo of one plane; pixels outside the image are zero
__device__ __forceinline__ void stage_halo(float* s, const float* __restrict__ plane, int H, int W, int y0, int x0)
{
    for (int i = threadIdx.x; i < kHalo * kHalo; i += kThreads) {
        const int r = i / kHalo, c = i - r * kHalo;
        const int y = y0 - kRad + r, x = x0 - kRad + c;
        s[r * kInStride + c] = (y >= 0 && y < H && x >= 0 && x < W) ? plane[(size_t)y * W + x] : 0.f;
    }
}

__global__ void __launch_bounds__(256) k_image_loss_maps(SsimArgs a)
{
    __shared__ float s_x[kHalo * kInStride], s_y[kHalo * kInStride];
    __shared__ float s_h[5][kHalo * kRowStride];
    const SsimView& v = a.b.v[blockIdx.z / (unsigned)a.C];
    const int ch = blockIdx.z % (unsigned)a.C;
    const int H = a.H, W = a.W, x0 = blockIdx.x * kSsimTile, y0 = blockIdx.y * kSsimTile;
    const size_t plane = (size_t)H * W;
    stage_halo(s_x, v.img + ch * plane, H, W, y0, x0);
    stage_halo(s_y, v.gt + ch * plane, H, W, y0, x0);
    __syncthreads();
    // horizontal pass: 42 rows x 32 columns, five quantities
    for (int i = threadIdx.x; i < kHalo * kSsimTile; i += kThreads) {
        const int r = i / kSsimTile, c = i % kSsimTile;
        float h0 = 0.f, h1 = 0.f, h2 = 0.f, h3 = 0.f, h4 = 0.f;
#pragma unroll
        for (int k = 0; k < kTaps; k++) {
            const float xv = s_x[r * kInStride + c + k], yv = s_y[r * kInStride + c + k], wk = a.w[k];
            h0 += wk * xv;
            h1 += wk * yv;
            h2 += wk * (xv * xv);
            h3 += wk * (yv * yv);
            h4 += wk * (xv * yv);
        }
        const int o = r * kRowStride + c;
        s_h[0][o] = h0, s_h[1][o] = h1, s_h[2][o] = h2, s_h[3][o] = h3, s_h[4][o] = h4;
    }
    __syncthreads();
    // vertical pass: the thread's column, four consecutive rows
    const int tx = threadIdx.x % kSsimTile, r0 = (threadIdx.x / kSsimTile) * kRowsPerThread;
    float acc[5][kRowsPerThread];
#pragma unroll
    for (int q = 0; q < 5; q++)
#pragma unroll
        for (int o = 0; o < kRowsPerThread; o++) acc[q][o] = 0.f;
#pragma unroll
    for (int j = 0; j < kTaps + kRowsPerThread - 1; j++) {
        float hv[5];
#pragma unroll
        for (int q = 0; q < 5; q++) hv[q] = s_h[q][(r0 + j) * kRowStride + tx];
#pragma unroll
        for (int o = 0; o < kRowsPerThread; o++) {
            if (j - o >= 0 && j - o < kTaps) {
#pragma unroll
                for (int q = 0; q < 5; q++) acc[q][o] += a.w[j - o] * hv[q];
            }
        }
    }
    float sums[2] = {0.f, 0.f};   // 1 - S, |x - y|
    const int x = x0 + tx;
    float* const maps = v.maps + ch * plane;
    const size_t map_stride = (size_t)a.C * plane;
#pragma unroll
    for (int o = 0; o < kRowsPerThread; o++) {
        const int y = y0 + r0 + o;
        if (x < W && y < H) {
            const float mu1 = acc[0][o], mu2 = acc[1][o];
            const float s11 = acc[2][o] - mu1 * mu1, s22 = acc[3][o] - mu2 * mu2, s12 = acc[4][o] - mu1 * mu2;
            const float A = 2.f * mu1 * mu2 + kC1, B = 2.f * s12 + kC2;
            const float Cc = mu1 * mu1 + mu2 * mu2 + kC1, D = s11 + s22 + kC2;
            const float inv = 1.f / (Cc * D);
            const float S = A * B * inv;
            const float dS12 = 2.f * A * inv, dS11 = -S / D;
            const float dM = 2.f * mu2 * B * inv - 2.f * mu1 * (S / Cc) - 2.f * mu1 * dS11 - mu2 * dS12;
            sums[0] += 1.f - S;
            const int li = (r0 + o + kRad) * kInStride + tx + kRad;
            sums[1] += fabsf(s_x[li] - s_y[li]);
            if (v.grad) {
                const size_t p = (size_t)y * W + x;
                maps[p] = dM, maps[map_stride + p] = dS11, maps[2 * map_stride + p] = dS12;
            }
        }
    }
    const unsigned n_wg = (unsigned)a.C * a.tiles_x * a.tiles_y;
    const unsigned id = ((unsigned)ch * a.tiles_y + blockIdx.y) * a.tiles_x + blockIdx.x;
    if (!sum_over_workgroups(sums, v.partial, n_wg, v.counter, id, n_wg)) return;
    const float d = sums[0] * a.inv_n, l1 = sums[1] * a.inv_n;
    // (spelt out: which of the two products the compiler folds into the addition is its choice, and it shows in the last bit)
    v.loss[0] = __builtin_fmaf(a.dssim_weight, d, a.rgb_weight * l1), v.loss[1] = l1, v.loss[2] = d;
}

__global__ void __launch_bounds__(256) k_image_loss_grad(SsimArgs a)
{
    __shared__ float s_m[3][kHalo * kInStride];
    __shared__ float s_h[3][kHalo * kRowStride];
    const SsimView& v = a.b.v[blockIdx.z / (unsigned)a.C];
    if (!v.grad) return;
    const int ch = blockIdx.z % (unsigned)a.C;
    const int H = a.H, W = a.W, x0 = blockIdx.x * kSsimTile, y0 = blockIdx.y * kSsimTile;
    const size_t plane = (size_t)H * W, map_stride = (size_t)a.C * plane;
#pragma unroll
    for (int q = 0; q < 3; q++) stage_halo(s_m[q], v.maps + q * map_stride + ch * plane, H, W, y0, x0);
    __syncthreads();
    for (int i = threadIdx.x; i < kHalo * kSsimTile; i += kThreads) {
        const int r = i / kSsimTile, c = i % kSsimTile;
        float h0 = 0.f, h1 = 0.f, h2 = 0.f;
#pragma unroll
        for (int k = 0; k < kTaps; k++) {
            const float wk = a.w[k];
            h0 += wk * s_m[0][r * kInStride + c + k];
            h1 += wk * s_m[1][r * kInStride + c + k];
            h2 += wk * s_m[2][r * kInStride + c + k];
        }
        const int o = r * kRowStride + c;
        s_h[0][o] = h0, s_h[1][o] = h1, s_h[2][o] = h2;
    }
    __syncthreads();
    const int tx = threadIdx.x % kSsimTile, r0 = (threadIdx.x / kSsimTile) * kRowsPerThread;
    float acc[3][kRowsPerThread];
#pragma unroll
    for (int q = 0; q < 3; q++)
#pragma unroll
        for (int o = 0; o < kRowsPerThread; o++) acc[q][o] = 0.f;
#pragma unroll
    for (int j = 0; j < kTaps + kRowsPerThread - 1; j++) {
        float hv[3];
#pragma unroll
        for (int q = 0; q < 3; q++) hv[q] = s_h[q][(r0 + j) * kRowStride + tx];
#pragma unroll
        for (int o = 0; o < kRowsPerThread; o++) {
            if (j - o >= 0 && j - o < kTaps) {
#pragma unroll
                for (int q = 0; q < 3; q++) acc[q][o] += a.w[j - o] * hv[q];
            }
        }
    }
    const int x = x0 + tx;
    const float* __restrict__ img = v.img + ch * plane;
    const float* __restrict__ gt = v.gt + ch * plane;
    float* __restrict__ grad = v.grad + ch * plane;
#pragma unroll
    for (int o = 0; o < kRowsPerThread; o++) {
        const int y = y0 + r0 + o;
        if (x < W && y < H) {
            const size_t p = (size_t)y * W + x;
            const float xv = img[p], yv = gt[p], d = xv - yv;
            const float sgn = d > 0.f ? 1.f : (d < 0.f ? -1.f : 0.f);   // torch.sign: 0 at 0
            grad[p] = a.g_ssim * (acc[0][o] + 2.f * xv * acc[1][o] + yv * acc[2][o]) + sgn * a.g_l1;
        }
    }
}

// gaussian(11, 1.5) of tools/loss_utils/dssim.py:18-20 in the reference's arithmetic: float32 roundings of the doubles
// exp(-(i - 5)^2 / (2 sigma^2)), their float32 sum, float32 division.  The order of that sum decides the last bit: summed
// pairwise (a balanced tree over the taps padded to 16) it is 3.7592328, which is also the correctly rounded sum and what
// torch.sum returns for these eleven floats on its vectorised CPU paths (4-, 8- and 16-lane accumulators reduced as a tree
// all give it); summed left to right it is 3.7592325 and the taps differ in the last bit.  torch's order is a property of its
// build and of the CPU, not a contract: the pairwise order is what this function DEFINES, and tests/test_image_loss_host.py
// pins it against an explicit pairwise sum first and against torch's own arithmetic second.
void ssim_window(float out[11])
{
    float g[kTaps], t[16];
    for (int i = 0; i < kTaps; i++) g[i] = (float)std::exp(-(double)((i - kRad) * (i - kRad)) / (2.0 * 1.5 * 1.5));
    for (int i = 0; i < 16; i++) t[i] = i < kTaps ? g[i] : 0.f;
    for (int n = 16; n > 1; n /= 2)
        for (int i = 0; i < n / 2; i++) t[i] = t[2 * i] + t[2 * i + 1];
    for (int i = 0; i < kTaps; i++) out[i] = g[i] / t[0];
}

static inline size_t n_tiles(int n) { return ((size_t)n + kSsimTile - 1) / kSsimTile; }
// counters | partials (at least what k_l1_loss_grad_terms uses: the D-SSIM-free path runs that kernel) | maps
static inline size_t maps_offset(int C, int H, int W)
{
    const size_t bytes = done_workspace_bytes(2 * (size_t)C * n_tiles(H) * n_tiles(W));
    return align_up(bytes < l1_workspace_bytes() ? l1_workspace_bytes() : bytes, 256);
}

size_t image_loss_workspace_bytes(int C, int H, int W)
{
    if (C < 1 || H < 1 || W < 1) return 0;
    return maps_offset(C, H, W) + 3 * sizeof(float) * (size_t)C * H * W;
}

int launch_image_loss_grad(const fr_image_loss_config& cfg, int n_images, int C, int H, int W, const float* const* img,
                           const float* const* gt, float* const* grad, float* const* loss, void* const* workspace, hipStream_t s)
{
    const unsigned long long n = (unsigned long long)C * H * W;
    if (cfg.dssim_weight == 0.f) return launch_l1_loss_grad_terms(n_images, n, cfg.rgb_weight, img, gt, grad, loss, workspace, s);
    SsimArgs a;
    bool any_grad = false;
    const size_t off = maps_offset(C, H, W);
    for (int k = 0; k < kMaxBatch; k++) {
        const int j = k < n_images ? k : 0;   // (unused entries are never indexed: blockIdx.z < n_images x C)
        const DoneWorkspace ws = done_workspace(workspace[j]);
        a.b.v[k] = SsimView{img[j], gt[j], grad ? grad[j] : nullptr, loss[j], ws.counter, ws.partial,
                            reinterpret_cast<float*>(static_cast<char*>(workspace[j]) + off)};
        any_grad = any_grad || a.b.v[k].grad != nullptr;
    }
    a.C = C, a.H = H, a.W = W;
    a.tiles_x = (unsigned)n_tiles(W), a.tiles_y = (unsigned)n_tiles(H);
    ssim_window(a.w);
    a.inv_n = (float)(1.0 / (double)n);
    a.g_l1 = (float)((double)cfg.rgb_weight / (double)n), a.g_ssim = (float)(-(double)cfg.dssim_weight / (double)n);
    a.rgb_weight = cfg.rgb_weight, a.dssim_weight = cfg.dssim_weight;
    const dim3 grid(a.tiles_x, a.tiles_y, (unsigned)(n_images * C));
    hipLaunchKernelGGL(k_image_loss_maps, grid, dim3(kThreads), 0, s, a);
    FR_HIP(hipGetLastError());
    if (any_grad) {
        hipLaunchKernelGGL(k_image_loss_grad, grid, dim3(kThreads), 0, s, a);
        FR_HIP(hipGetLastError());
    }
    return FR_OK;
}

}  // namespace fr
