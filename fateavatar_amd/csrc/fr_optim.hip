// Fused Adam over the flat Gaussian parameter buffer.
//
// reference: the per-frame step ends with torch.optim.Adam.step() over five or six parameter groups
// (train/optim.py:11-37, train/iteration.py:58-60) — with the default (foreach) implementation a dozen
// elementwise kernels per step, each streaming the whole state.  Here: ONE pass, 16 B per lane per array,
// 28 B of HBM traffic per parameter (read p, g, m, v; write p, m, v) — the HBM roofline of the update.
// Arithmetic follows torch.optim.Adam (betas, eps outside the sqrt, bias correction as step_size / denom);
// this file is built without FMA contraction so that the update matches torch's to rounding.
#include "fr_common.hpp"

namespace fr {

struct AdamArgs {
    int n_seg;
    unsigned long long seg_end[FR_ADAM_MAX_SEGMENTS];
    float seg_lr[FR_ADAM_MAX_SEGMENTS];
    unsigned seg_period[FR_ADAM_MAX_SEGMENTS], seg_split[FR_ADAM_MAX_SEGMENTS];
    float seg_lr2[FR_ADAM_MAX_SEGMENTS];
    float beta1, beta2, omb1, omb2, eps, grad_scale;  // omb = 1 - beta, rounded from double
    double beta1_d, beta2_d, omb1_d, omb2_d;          // the same, unrounded: the bias corrections are carried in double
    int n_skip;                                        // fr_adam_config::skip: any non-zero word -> the step does nothing
    const float* skip[FR_ADAM_MAX_GRADS];
};

// state = {step, 1 - beta1^step, 1 - beta2^step, -, the two corrections as doubles in words 4..7, ..., done-counters from
// word 32}: advanced on the device so that the host passes nothing that changes from step to step (graph replay).  The
// bias corrections c_t = 1 - beta^t are carried by the recurrence c_{t+1} = (1 - beta) + beta c_t.  All its terms are
// positive, so no single step cancels, but every step rounds, and the map contracts errors only by beta per step: in
// float32 with beta = 0.999f about a thousand roundings stay alive, the sequence is off by 40 x 2^-24 at step 1000, and
// it stops moving at 0.99997020 instead of reaching 1 (every later update 1.5e-5 too large).  So the recurrence runs in
// DOUBLE, with beta and 1 - beta as the doubles the configuration holds (1 - 0.999f alone is off by 1.3e-5): accumulated
// error at most 2^-53 / (1 - beta) = 1.1e-13 at any step count, far inside the float32 rounding of the value the update uses.  Words 1 and 2 keep
// the corrections rounded to float for readers of the state.  Every workgroup of k_adam derives this step's corrections
// from the OLD state; the workgroup that finishes last (last_workgroup_of) stores the new one — no launch of its own.
__device__ __forceinline__ float adam_one(float& p, float g, float& m, float& v, float lr_over_bc1, float inv_sqrt_bc2,
                                          const AdamArgs& a)
{
    g *= a.grad_scale;
    m = a.beta1 * m + a.omb1 * g;
    v = a.beta2 * v + a.omb2 * (g * g);
    const float denom = sqrtf(v) * inv_sqrt_bc2 + a.eps;
    p -= lr_over_bc1 * (m / denom);
    return p;
}

// the gradient of the step = the SUM of up to FR_ADAM_MAX_GRADS buffers (the views of a batch rendered in flight
// together, each into its own buffer; grad_scale turns the sum into the mean): no pass of its own to add them up
struct AdamGrads {
    int n;
    const float* g[FR_ADAM_MAX_GRADS];
};

__device__ __forceinline__ float4 adam_grad4(const AdamGrads& gs, unsigned long long i)
{
    float4 r = reinterpret_cast<const float4*>(gs.g[0])[i];
#pragma unroll
    for (int k = 1; k < FR_ADAM_MAX_GRADS; k++) {
        if (k < gs.n) {
            const float4 t = reinterpret_cast<const float4*>(gs.g[k])[i];
            r.x += t.x, r.y += t.y, r.z += t.z, r.w += t.w;
        }
    }
    return r;
}

__global__ void __launch_bounds__(256) k_adam(AdamArgs a, float4* __restrict__ param, AdamGrads grads,
                                              float4* __restrict__ exp_avg, float4* __restrict__ exp_avg_sq,
                                              unsigned long long n, float* state)
{
    // a frame that feeds this step overflowed its binning capacity inside a replayed graph and back-propagated zeros
    // (fr_aux::overflow_out): the whole step is skipped — every workgroup takes the same decision from the same words
    for (int k = 0; k < a.n_skip; k++)
        if (a.skip[k][0] != 0.0f) return;
    const float step_new = state[0] + 1.0f;
    const double* const carried = reinterpret_cast<const double*>(state + 4);   // (8-byte aligned: fr_adam_step checks)
    const double bc1_d = a.omb1_d + a.beta1_d * carried[0], bc2_d = a.omb2_d + a.beta2_d * carried[1];
    const float bc1 = (float)bc1_d, bc2 = (float)bc2_d;
    const float inv_sqrt_bc2 = 1.0f / sqrtf(bc2);
    const unsigned long long n4 = n / 4, stride = (unsigned long long)gridDim.x * blockDim.x;
    for (unsigned long long i = (unsigned long long)blockIdx.x * blockDim.x + threadIdx.x; i < (n + 3) / 4; i += stride) {
        const unsigned long long e0 = 4 * i;
        float lr[4];
#pragma unroll
        for (int k = 0; k < 4; k++) {  // a quad may straddle a segment boundary
            int sg = 0;
            for (int q = 0; q + 1 < a.n_seg; q++) sg += (e0 + k >= a.seg_end[q]) ? 1 : 0;
            float l = a.seg_lr[sg];
            if (a.seg_period[sg]) {
                const unsigned long long rel = e0 + k - (sg ? a.seg_end[sg - 1] : 0ull);
                if ((unsigned)(rel % a.seg_period[sg]) >= a.seg_split[sg]) l = a.seg_lr2[sg];
            }
            lr[k] = l / bc1;
        }
        if (i < n4) {
            float4 p = param[i], m = exp_avg[i], v = exp_avg_sq[i];
            const float4 g = adam_grad4(grads, i);
            adam_one(p.x, g.x, m.x, v.x, lr[0], inv_sqrt_bc2, a);
            adam_one(p.y, g.y, m.y, v.y, lr[1], inv_sqrt_bc2, a);
            adam_one(p.z, g.z, m.z, v.z, lr[2], inv_sqrt_bc2, a);
            adam_one(p.w, g.w, m.w, v.w, lr[3], inv_sqrt_bc2, a);
            param[i] = p, exp_avg[i] = m, exp_avg_sq[i] = v;
        } else {  // tail of a buffer whose length is not a multiple of 4
            float* ps = reinterpret_cast<float*>(param);
            float* ms = reinterpret_cast<float*>(exp_avg);
            float* vs = reinterpret_cast<float*>(exp_avg_sq);
            for (int k = 0; k < 4 && e0 + k < n; k++) {
                float g1 = grads.g[0][e0 + k];
                for (int q = 1; q < grads.n; q++) g1 += grads.g[q][e0 + k];
                adam_one(ps[e0 + k], g1, ms[e0 + k], vs[e0 + k], lr[k], inv_sqrt_bc2, a);
            }
        }
    }
    // every thread of this workgroup has read the old state (above) before the barrier; the last workgroup to get here
    // knows that all have
    __syncthreads();
    if (threadIdx.x == 0) {
        if (last_workgroup_of(reinterpret_cast<unsigned*>(state + 32), blockIdx.x, gridDim.x)) {
            double* const carry = reinterpret_cast<double*>(state + 4);
            state[0] = step_new, state[1] = bc1, state[2] = bc2, carry[0] = bc1_d, carry[1] = bc2_d;
        }
    }
}

int launch_adam(const fr_adam_config& cfg, float* param, const float* const* grad_bufs, int n_grads, float* exp_avg,
                float* exp_avg_sq, unsigned long long n, float* state, hipStream_t s)
{
    if (n == 0) return FR_OK;
    AdamGrads grads;
    grads.n = n_grads;
    for (int k = 0; k < FR_ADAM_MAX_GRADS; k++) grads.g[k] = k < n_grads ? grad_bufs[k] : grad_bufs[0];
    AdamArgs a;
    a.n_seg = cfg.n_segments;
    for (int i = 0; i < FR_ADAM_MAX_SEGMENTS; i++) {
        a.seg_end[i] = i < cfg.n_segments ? cfg.segment_end[i] : 0ull;
        a.seg_lr[i] = i < cfg.n_segments ? cfg.segment_lr[i] : 0.f;
        a.seg_period[i] = i < cfg.n_segments ? cfg.segment_period[i] : 0u;
        a.seg_split[i] = i < cfg.n_segments ? cfg.segment_split[i] : 0u;
        a.seg_lr2[i] = i < cfg.n_segments ? cfg.segment_lr2[i] : 0.f;
    }
    a.beta1 = (float)cfg.beta1, a.beta2 = (float)cfg.beta2, a.eps = (float)cfg.eps, a.grad_scale = cfg.grad_scale;
    a.omb1 = (float)(1.0 - cfg.beta1), a.omb2 = (float)(1.0 - cfg.beta2);
    a.beta1_d = cfg.beta1, a.beta2_d = cfg.beta2, a.omb1_d = 1.0 - cfg.beta1, a.omb2_d = 1.0 - cfg.beta2;
    a.n_skip = cfg.n_skip < 0 ? 0 : (cfg.n_skip > FR_ADAM_MAX_GRADS ? FR_ADAM_MAX_GRADS : cfg.n_skip);
    for (int k = 0; k < FR_ADAM_MAX_GRADS; k++) a.skip[k] = k < a.n_skip ? cfg.skip[k] : nullptr;
    const unsigned long long quads = (n + 3) / 4;
    unsigned long long blocks = (quads + 255) / 256;
    if (blocks > 2048) blocks = 2048;
    hipLaunchKernelGGL(k_adam, dim3((unsigned)blocks), dim3(256), 0, s, a, reinterpret_cast<float4*>(param), grads,
                       reinterpret_cast<float4*>(exp_avg),
                       reinterpret_cast<float4*>(exp_avg_sq), n, state);
    FR_HIP(hipGetLastError());
    return FR_OK;
}

// ---------------------------------------------------------------- L1 image loss and its gradient, one launch
// reference: nn.L1Loss(reduction='mean') on the rendered image (model/loss.py:92) followed by loss.backward() — in
// PyTorch eight launch-bound elementwise / reduction kernels (sub, abs, mean, fill, sign, mul, ...: 41 us of a 205 us
// optimisation step at 512 x 512).  Here: grad = sign(img - gt) / n and per-workgroup partial sums of |img - gt| in one
// pass; the workgroup that finishes last adds the partials up in index order (deterministic) and stores the loss
// (sum_over_workgroups, fr_common.hpp: every fused loss kernel of the library ends with it).
constexpr unsigned kL1MaxBlocks = 1024;

struct L1View {   // one image of a (possibly batched) launch
    const float* img;
    const float* gt;
    float* grad;
    float* partial;
    unsigned* counter;
    float* loss;
};

// kTerms (fr_image_loss_grad with a D-SSIM weight of 0): the gradient's magnitude is `g` = rgb_weight / n instead of 1 / n,
// `loss` takes {rgb_weight x l1, l1, 0} and the partials are put back to zero; the sums are those of the plain kernel, bit for bit.
template <bool kTerms>
__device__ __forceinline__ void l1_loss_grad_body(const L1View& v, unsigned long long n, float inv_n, float g_mag, float rgb_weight)
{
    const float* __restrict__ img = v.img;
    const float* __restrict__ gt = v.gt;
    float* __restrict__ grad = v.grad;
    float* __restrict__ loss = v.loss;
    const unsigned long long n4 = n / 4, stride = (unsigned long long)gridDim.x * blockDim.x;
    float acc[1] = {0.f};
    for (unsigned long long i = (unsigned long long)blockIdx.x * blockDim.x + threadIdx.x; i < n4; i += stride) {
        const float4 a = reinterpret_cast<const float4*>(img)[i], b = reinterpret_cast<const float4*>(gt)[i];
        const float d[4] = {a.x - b.x, a.y - b.y, a.z - b.z, a.w - b.w};
        float g[4];
#pragma unroll
        for (int k = 0; k < 4; k++) {
            acc[0] += fabsf(d[k]);
            g[k] = d[k] > 0.f ? g_mag : (d[k] < 0.f ? -g_mag : 0.f);   // torch.sign: 0 at 0
        }
        if (grad) reinterpret_cast<float4*>(grad)[i] = make_float4(g[0], g[1], g[2], g[3]);
    }
    if (blockIdx.x == 0 && threadIdx.x < (unsigned)(n - 4 * n4)) {   // tail of a length that is not a multiple of 4
        const unsigned long long e = 4 * n4 + threadIdx.x;
        const float d = img[e] - gt[e];
        acc[0] += fabsf(d);
        if (grad) grad[e] = d > 0.f ? g_mag : (d < 0.f ? -g_mag : 0.f);
    }
    if (!sum_over_workgroups<1, kTerms>(acc, v.partial, 0u, v.counter, blockIdx.x, gridDim.x)) return;
    const float l1 = acc[0] * inv_n;
    if (kTerms) loss[0] = rgb_weight * l1, loss[1] = l1, loss[2] = 0.f;
    else *loss = l1;
}

__global__ void __launch_bounds__(kSumThreads) k_l1_loss_grad(L1View v, unsigned long long n, float inv_n) { l1_loss_grad_body<false>(v, n, inv_n, inv_n, 1.f); }
// the images of the frames of a batch (same size), one workspace each: grid (x, images)
__global__ void __launch_bounds__(kSumThreads) k_l1_loss_grad_batch(BatchOf<L1View> b, unsigned long long n, float inv_n)
{
    l1_loss_grad_body<false>(b.v[blockIdx.y], n, inv_n, inv_n, 1.f);
}
// the L1 term alone behind fr_image_loss_grad (three loss words per image, weighted gradient)
__global__ void __launch_bounds__(kSumThreads) k_l1_loss_grad_terms(BatchOf<L1View> b, unsigned long long n, float inv_n, float g_mag, float rgb_weight)
{
    l1_loss_grad_body<true>(b.v[blockIdx.y], n, inv_n, g_mag, rgb_weight);
}

size_t l1_workspace_bytes() { return done_workspace_bytes(kL1MaxBlocks); }

// a float4 per thread and sweep: what the L1 and Huber kernels take per workgroup
static unsigned l1_blocks(unsigned long long n) { return capped_blocks(n / 4, kSumThreads, kL1MaxBlocks); }

static L1View l1_view(const float* img, const float* gt, float* grad, float* loss, void* workspace)
{
    const DoneWorkspace ws = done_workspace(workspace);
    return L1View{img, gt, grad, ws.partial, ws.counter, loss};
}

static BatchOf<L1View> l1_views(int n_images, const float* const* img, const float* const* gt, float* const* grad, float* const* loss,
                                void* const* workspace)
{
    BatchOf<L1View> b;
    for (int k = 0; k < kMaxBatch; k++) {
        const int j = k < n_images ? k : 0;   // (unused entries: never indexed, blockIdx.y < n_images)
        b.v[k] = l1_view(img[j], gt[j], grad ? grad[j] : nullptr, loss[j], workspace[j]);
    }
    return b;
}

int launch_l1_loss_grad(unsigned long long n, const float* img, const float* gt, float* grad, float* loss, void* workspace,
                        hipStream_t s)
{
    if (n == 0) return FR_OK;
    hipLaunchKernelGGL(k_l1_loss_grad, dim3(l1_blocks(n)), dim3(kSumThreads), 0, s, l1_view(img, gt, grad, loss, workspace), n,
                       (float)(1.0 / (double)n));
    FR_HIP(hipGetLastError());
    return FR_OK;
}

int launch_l1_loss_grad_batch(int n_images, unsigned long long n, const float* const* img, const float* const* gt, float* const* grad,
                              float* const* loss, void* const* workspace, hipStream_t s)
{
    if (n == 0 || n_images <= 0) return FR_OK;
    hipLaunchKernelGGL(k_l1_loss_grad_batch, dim3(l1_blocks(n), (unsigned)n_images), dim3(kSumThreads), 0, s,
                       l1_views(n_images, img, gt, grad, loss, workspace), n, (float)(1.0 / (double)n));
    FR_HIP(hipGetLastError());
    return FR_OK;
}

int launch_l1_loss_grad_terms(int n_images, unsigned long long n, float rgb_weight, const float* const* img, const float* const* gt,
                              float* const* grad, float* const* loss, void* const* workspace, hipStream_t s)
{
    if (n == 0 || n_images <= 0) return FR_OK;
    hipLaunchKernelGGL(k_l1_loss_grad_terms, dim3(l1_blocks(n), (unsigned)n_images), dim3(kSumThreads), 0, s,
                       l1_views(n_images, img, gt, grad, loss, workspace), n, (float)(1.0 / (double)n),
                       (float)((double)rgb_weight / (double)n), rgb_weight);
    FR_HIP(hipGetLastError());
    return FR_OK;
}

// ---------------------------------------------------------------- Huber image term and its gradient, one launch
// reference: FlashAvatarLoss.get_huber_loss (train/loss.py:217-221) on the image and, with a mouth mask, once more on the
// masked image and target at weight 40 (:231-239), followed by loss.backward(): about thirty launch-bound elementwise /
// reduction kernels with autograd's twins.  Here k_l1_loss_grad's scheme with TWO sums: float4 pieces plus a tail,
// per-workgroup partials, the workgroup that finishes last adds them up in index order and puts the workspace back to zero.
//   h(x) = 0.5 x^2 if |x| < alpha else alpha (|x| - 0.5 alpha);  h'(x) = x if |x| < alpha else alpha sign(x)
struct HuberArgs {
    const float* img;
    const float* gt;
    const float* mask;   // [HW] or null
    float* grad;         // or null
    float* partial;      // [2][kL1MaxBlocks]
    unsigned* counter;
    float* loss;         // {huber + mask_weight x mouth, huber, mouth}
    unsigned long long n;
    unsigned hw;
    float alpha, mask_weight, inv_n;
};

// h and h' of one difference x: the value is added to `acc`, the derivative returned
__device__ __forceinline__ float huber_term(float x, float alpha, float& acc)
{
    const float ax = fabsf(x);
    if (ax < alpha) {
        acc += 0.5f * x * x;
        return x;
    }
    acc += alpha * (ax - 0.5f * alpha);
    return x < 0.f ? -alpha : alpha;
}

// element e of the image: both terms' sums, and the gradient word
__device__ __forceinline__ float huber_one(const HuberArgs& a, unsigned long long e, float d, float& acc_h, float& acc_m)
{
    float g = huber_term(d, a.alpha, acc_h);
    if (a.mask) {
        const float m = a.mask[e % a.hw];   // [1,H,W] broadcast over the channels
        g += a.mask_weight * m * huber_term(m * d, a.alpha, acc_m);
    }
    return g * a.inv_n;
}

__global__ void __launch_bounds__(256) k_huber_loss_grad(HuberArgs a)
{
    const float* __restrict__ img = a.img;
    const float* __restrict__ gt = a.gt;
    float* __restrict__ grad = a.grad;
    const unsigned long long n = a.n, n4 = n / 4, stride = (unsigned long long)gridDim.x * blockDim.x;
    float acc[2] = {0.f, 0.f};   // huber, mouth
    for (unsigned long long i = (unsigned long long)blockIdx.x * blockDim.x + threadIdx.x; i < n4; i += stride) {
        const float4 x = reinterpret_cast<const float4*>(img)[i], y = reinterpret_cast<const float4*>(gt)[i];
        const float d[4] = {x.x - y.x, x.y - y.y, x.z - y.z, x.w - y.w};
        float g[4];
#pragma unroll
        for (int k = 0; k < 4; k++) g[k] = huber_one(a, 4 * i + k, d[k], acc[0], acc[1]);
        if (grad) reinterpret_cast<float4*>(grad)[i] = make_float4(g[0], g[1], g[2], g[3]);
    }
    if (blockIdx.x == 0 && threadIdx.x < (unsigned)(n - 4 * n4)) {   // tail of a length that is not a multiple of 4
        const unsigned long long e = 4 * n4 + threadIdx.x;
        const float g = huber_one(a, e, img[e] - gt[e], acc[0], acc[1]);
        if (grad) grad[e] = g;
    }
    if (!sum_over_workgroups(acc, a.partial, kL1MaxBlocks, a.counter, blockIdx.x, gridDim.x)) return;
    const float huber = acc[0] * a.inv_n, mouth = acc[1] * a.inv_n;
    a.loss[0] = huber + a.mask_weight * mouth, a.loss[1] = huber, a.loss[2] = mouth;
}

size_t huber_workspace_bytes() { return done_workspace_bytes(2 * kL1MaxBlocks); }

int launch_huber_loss_grad(const fr_huber_config& cfg, int C, int H, int W, const float* img, const float* gt, const float* mask,
                           float* grad, float* loss, void* workspace, hipStream_t s)
{
    const unsigned long long hw = (unsigned long long)H * (unsigned long long)W, n = hw * (unsigned long long)C;
    if (n == 0) return FR_OK;
    const DoneWorkspace ws = done_workspace(workspace);
    HuberArgs a;
    a.img = img, a.gt = gt, a.mask = mask, a.grad = grad, a.loss = loss;
    a.counter = ws.counter, a.partial = ws.partial;
    a.n = n, a.hw = (unsigned)hw;
    a.alpha = cfg.alpha, a.mask_weight = mask ? cfg.mask_weight : 0.f, a.inv_n = (float)(1.0 / (double)n);
    hipLaunchKernelGGL(k_huber_loss_grad, dim3(l1_blocks(n)), dim3(kSumThreads), 0, s, a);
    FR_HIP(hipGetLastError());
    return FR_OK;
}

// ---------------------------------------------------------------- SplattingAvatar's L1 + MSE image term and its gradient, one launch
// reference: SplattingAvatarLoss.accumulate_gradients (train/loss.py:288-323; get_rgb_loss / get_mse_loss :279-283) with
// rgb_loss 1.0 and mse_loss 10.0 of config/splattingavatar.yaml:13-20, followed by loss.backward(): two mean reductions with
// their elementwise kernels and autograd's twins.  Here the Huber kernel's scheme: float4 pieces plus a tail, TWO sums.  The
// L1 sum has its own accumulator and takes its addends in k_l1_loss_grad's order, on k_l1_loss_grad's grid, through the same
// tree: loss[1] is fr_l1_loss_grad's loss, bit for bit.
struct PixelArgs {
    const float* img;
    const float* gt;
    float* grad;         // or null
    float* partial;      // [2][kL1MaxBlocks]
    unsigned* counter;
    float* loss;         // {rgb_weight x l1 + mse_weight x mse, l1, mse}
    unsigned long long n;
    float rgb_weight, mse_weight, inv_n;
    float g_l1, g_mse;   // rgb_weight / n, 2 mse_weight / n
};

// one difference d: both sums, and the gradient word  rgb_weight sign(d) / n + mse_weight 2 d / n  (torch.sign: 0 at 0)
__device__ __forceinline__ float pixel_one(const PixelArgs& a, float d, float& acc_l1, float& acc_mse)
{
    acc_l1 += fabsf(d);
    acc_mse += d * d;
    return (d > 0.f ? a.g_l1 : (d < 0.f ? -a.g_l1 : 0.f)) + a.g_mse * d;
}

__global__ void __launch_bounds__(kSumThreads) k_pixel_loss_grad(PixelArgs a)
{
    const float* __restrict__ img = a.img;
    const float* __restrict__ gt = a.gt;
    float* __restrict__ grad = a.grad;
    const unsigned long long n = a.n, n4 = n / 4, stride = (unsigned long long)gridDim.x * blockDim.x;
    float acc[2] = {0.f, 0.f};   // l1, mse
    for (unsigned long long i = (unsigned long long)blockIdx.x * blockDim.x + threadIdx.x; i < n4; i += stride) {
        const float4 x = reinterpret_cast<const float4*>(img)[i], y = reinterpret_cast<const float4*>(gt)[i];
        const float d[4] = {x.x - y.x, x.y - y.y, x.z - y.z, x.w - y.w};
        float g[4];
#pragma unroll
        for (int k = 0; k < 4; k++) g[k] = pixel_one(a, d[k], acc[0], acc[1]);
        if (grad) reinterpret_cast<float4*>(grad)[i] = make_float4(g[0], g[1], g[2], g[3]);
    }
    if (blockIdx.x == 0 && threadIdx.x < (unsigned)(n - 4 * n4)) {   // tail of a length that is not a multiple of 4
        const unsigned long long e = 4 * n4 + threadIdx.x;
        const float g = pixel_one(a, img[e] - gt[e], acc[0], acc[1]);
        if (grad) grad[e] = g;
    }
    if (!sum_over_workgroups(acc, a.partial, kL1MaxBlocks, a.counter, blockIdx.x, gridDim.x)) return;
    const float l1 = acc[0] * a.inv_n, mse = acc[1] * a.inv_n;
    a.loss[0] = a.rgb_weight * l1 + a.mse_weight * mse, a.loss[1] = l1, a.loss[2] = mse;
}

size_t pixel_loss_workspace_bytes() { return done_workspace_bytes(2 * kL1MaxBlocks); }

int launch_pixel_loss_grad(const fr_pixel_loss_config& cfg, int C, int H, int W, const float* img, const float* gt, float* grad,
                           float* loss, void* workspace, hipStream_t s)
{
    const unsigned long long n = (unsigned long long)H * (unsigned long long)W * (unsigned long long)C;
    if (n == 0) return FR_OK;
    const DoneWorkspace ws = done_workspace(workspace);
    PixelArgs a;
    a.img = img, a.gt = gt, a.grad = grad, a.loss = loss;
    a.counter = ws.counter, a.partial = ws.partial;
    a.n = n;
    a.rgb_weight = cfg.rgb_weight, a.mse_weight = cfg.mse_weight, a.inv_n = (float)(1.0 / (double)n);
    a.g_l1 = (float)((double)cfg.rgb_weight / (double)n), a.g_mse = (float)(2.0 * (double)cfg.mse_weight / (double)n);
    hipLaunchKernelGGL(k_pixel_loss_grad, dim3(l1_blocks(n)), dim3(kSumThreads), 0, s, a);
    FR_HIP(hipGetLastError());
    return FR_OK;
}

// ---------------------------------------------------------------- several small device-to-device copies, one launch
// The per-frame inputs of a captured step (camera block, posed vertices, target image) are copied into the buffers the
// graph was captured with: as separate copies each is a launch-bound 5 us dispatch.
struct CopyArgs {
    int n;
    float* dst[FR_COPY_MAX_SEGMENTS];
    const float* src[FR_COPY_MAX_SEGMENTS];
    unsigned long long count[FR_COPY_MAX_SEGMENTS];   // floats
};

__global__ void __launch_bounds__(256) k_multi_copy(CopyArgs a)
{
    const unsigned long long stride = (unsigned long long)gridDim.x * blockDim.x;
    const unsigned long long t0 = (unsigned long long)blockIdx.x * blockDim.x + threadIdx.x;
    for (int sg = 0; sg < a.n; sg++) {
        const unsigned long long n = a.count[sg];
        const bool wide = ((reinterpret_cast<uintptr_t>(a.dst[sg]) | reinterpret_cast<uintptr_t>(a.src[sg])) & 15) == 0;
        const unsigned long long n4 = wide ? n / 4 : 0;
        for (unsigned long long i = t0; i < n4; i += stride)
            reinterpret_cast<float4*>(a.dst[sg])[i] = reinterpret_cast<const float4*>(a.src[sg])[i];
        for (unsigned long long e = 4 * n4 + t0; e < n; e += stride) a.dst[sg][e] = a.src[sg][e];
    }
}

int launch_multi_copy(int n_seg, float* const* dst, const float* const* src, const unsigned long long* count, hipStream_t s)
{
    CopyArgs a;
    a.n = n_seg;
    unsigned long long most = 0;
    for (int i = 0; i < FR_COPY_MAX_SEGMENTS; i++) {
        a.dst[i] = i < n_seg ? dst[i] : nullptr, a.src[i] = i < n_seg ? src[i] : nullptr, a.count[i] = i < n_seg ? count[i] : 0ull;
        most = a.count[i] > most ? a.count[i] : most;
    }
    if (most == 0) return FR_OK;
    unsigned long long blocks = (most / 4 + 255) / 256;
    blocks = blocks < 1 ? 1 : (blocks > 2048 ? 2048 : blocks);
    hipLaunchKernelGGL(k_multi_copy, dim3((unsigned)blocks), dim3(256), 0, s, a);
    FR_HIP(hipGetLastError());
    return FR_OK;
}

// ---------------------------------------------------------------- scaled sum of up to four equally long arrays
// dst = scale * (src[0] + ... + src[n-1]): the mean of the gradient buffers of the views a rank rendered in flight
// together, written into the exchange buffer of the all-reduce in one pass (three PyTorch kernels otherwise: 142 MB of
// traffic instead of 94 at 23.6 MB per buffer, on a GPU that is busy rendering the next step's frames).  dst may be one
// of the sources (every element is read before it is written, by the same thread): dst += ... for local accumulation.
struct SumArgs {
    int n;
    const float* src[FR_ADAM_MAX_GRADS];
};

__global__ void __launch_bounds__(256) k_scaled_sum(SumArgs a, float* dst, unsigned long long count, float scale)
{
    const unsigned long long n4 = count / 4, stride = (unsigned long long)gridDim.x * blockDim.x;
    const unsigned long long t0 = (unsigned long long)blockIdx.x * blockDim.x + threadIdx.x;
    for (unsigned long long i = t0; i < n4; i += stride) {
        float4 r = reinterpret_cast<const float4*>(a.src[0])[i];
#pragma unroll
        for (int k = 1; k < FR_ADAM_MAX_GRADS; k++) {
            if (k < a.n) {
                const float4 t = reinterpret_cast<const float4*>(a.src[k])[i];
                r.x += t.x, r.y += t.y, r.z += t.z, r.w += t.w;
            }
        }
        reinterpret_cast<float4*>(dst)[i] = make_float4(r.x * scale, r.y * scale, r.z * scale, r.w * scale);
    }
    for (unsigned long long e = 4 * n4 + t0; e < count; e += stride) {
        float r = a.src[0][e];
        for (int k = 1; k < a.n; k++) r += a.src[k][e];
        dst[e] = r * scale;
    }
}

int launch_scaled_sum(int n_src, const float* const* src, float* dst, unsigned long long count, float scale, hipStream_t s)
{
    if (count == 0) return FR_OK;
    SumArgs a;
    a.n = n_src;
    for (int k = 0; k < FR_ADAM_MAX_GRADS; k++) a.src[k] = k < n_src ? src[k] : src[0];
    unsigned long long blocks = (count / 4 + 255) / 256;
    blocks = blocks < 1 ? 1 : (blocks > 4096 ? 4096 : blocks);
    hipLaunchKernelGGL(k_scaled_sum, dim3((unsigned)blocks), dim3(256), 0, s, a, dst, count, scale);
    FR_HIP(hipGetLastError());
    return FR_OK;
}

// ---------------------------------------------------------------- GaussianAvatars' scale / xyz regularisers, one launch
// reference: GaussianAvatarsLoss.accumulate_gradients (train/loss.py:367-379) on the raw local parameters
// (model/baseline/gaussianavatars.py:196-197):
//     scale_loss = relu(exp(_scaling) - threshold_scale).norm(dim=1).mean()
//     xyz_loss   = relu(_xyz.norm(dim=1) - threshold_xyz).mean()
// in PyTorch a dozen launch-bound kernels and their autograd twins on every step.  Here lane = Gaussian: the row's two loss
// terms, and weight x their gradients ADDED into the caller's gradient rows by the lane that owns the row (no atomics).
// Sub-gradients are autograd's: relu passes a gradient where its input is > 0, norm's backward gives 0 at norm 0 — so a
// component with exp(s) <= threshold, a row clipped to zero and a row with |xyz| <= threshold add nothing, and no division
// by a zero norm is evaluated.  The loss sums are reduced as k_l1_loss_grad's: per-workgroup partials, added up in index
// order by the workgroup that finishes last, which also puts the partials back to zero.
constexpr unsigned kRegMaxBlocks = 1024;

struct RegArgs {
    const float* scaling;
    const float* xyz;
    float* d_scaling;     // null: no gradient traffic for the term (also what a zero weight gives)
    float* d_xyz;
    float* partial;       // [2][kRegMaxBlocks]
    unsigned* counter;
    float* loss;          // {scale_loss, xyz_loss}, unweighted
    int P;
    float g_scale, g_xyz; // weight / P
    float thr_scale, thr_xyz, inv_P;
};

__global__ void __launch_bounds__(256) k_gaussian_regularise(RegArgs a)
{
    const float* __restrict__ scaling = a.scaling;
    const float* __restrict__ xyz = a.xyz;
    float* __restrict__ d_scaling = a.d_scaling;
    float* __restrict__ d_xyz = a.d_xyz;
    const unsigned stride = gridDim.x * blockDim.x;
    float acc[2] = {0.f, 0.f};   // scale, xyz
    for (unsigned i = blockIdx.x * blockDim.x + threadIdx.x; i < (unsigned)a.P; i += stride) {
        const size_t o = (size_t)i * 3;
        const float e0 = act_exp(scaling[o]), e1 = act_exp(scaling[o + 1]), e2 = act_exp(scaling[o + 2]);
        const float c0 = fmaxf(e0 - a.thr_scale, 0.f), c1 = fmaxf(e1 - a.thr_scale, 0.f), c2 = fmaxf(e2 - a.thr_scale, 0.f);
        const float ns = sqrtf((c0 * c0 + c1 * c1) + c2 * c2);
        acc[0] += ns;
        if (d_scaling && ns > 0.f) {       // (c_k == 0 where exp(s_k) <= threshold: that component adds an exact 0)
            const float k = a.g_scale / ns;
            d_scaling[o] += k * c0 * e0;
            d_scaling[o + 1] += k * c1 * e1;
            d_scaling[o + 2] += k * c2 * e2;
        }
        const float x = xyz[o], y = xyz[o + 1], z = xyz[o + 2];
        const float nx = sqrtf((x * x + y * y) + z * z);
        const float over = nx - a.thr_xyz;
        acc[1] += fmaxf(over, 0.f);
        if (d_xyz && over > 0.f && nx > 0.f) {
            const float k = a.g_xyz / nx;
            d_xyz[o] += k * x;
            d_xyz[o + 1] += k * y;
            d_xyz[o + 2] += k * z;
        }
    }
    if (!sum_over_workgroups(acc, a.partial, kRegMaxBlocks, a.counter, blockIdx.x, gridDim.x)) return;
    a.loss[0] = acc[0] * a.inv_P;
    a.loss[1] = acc[1] * a.inv_P;
}

size_t regularise_workspace_bytes() { return done_workspace_bytes(2 * kRegMaxBlocks); }

int launch_gaussian_regularise(const fr_regularise_config& cfg, int P, const float* scaling, const float* xyz, float* d_scaling,
                               float* d_xyz, float* loss, void* workspace, hipStream_t s)
{
    if (P <= 0) return FR_OK;
    const unsigned blocks = capped_blocks((unsigned)P, kSumThreads, kRegMaxBlocks);
    const DoneWorkspace ws = done_workspace(workspace);
    RegArgs a;
    a.scaling = scaling, a.xyz = xyz;
    a.d_scaling = cfg.scale_weight != 0.f ? d_scaling : nullptr;   // a zero weight: the array is not touched
    a.d_xyz = cfg.xyz_weight != 0.f ? d_xyz : nullptr;
    a.counter = ws.counter, a.partial = ws.partial;
    a.loss = loss, a.P = P;
    a.inv_P = (float)(1.0 / (double)P);
    a.g_scale = (float)((double)cfg.scale_weight / (double)P), a.g_xyz = (float)((double)cfg.xyz_weight / (double)P);
    a.thr_scale = cfg.threshold_scale, a.thr_xyz = cfg.threshold_xyz;
    hipLaunchKernelGGL(k_gaussian_regularise, dim3(blocks), dim3(256), 0, s, a);
    FR_HIP(hipGetLastError());
    return FR_OK;
}

// ---------------------------------------------------------------- SplattingAvatar's scale term, two launches
// reference: SplattingAvatarLoss.get_scale_loss (train/loss.py:307-315) on get_scaling = exp(_scaling)
// (model/baseline/splattingavatar.py:270):
//     smax, smin = scale.max(-1), scale.min(-1)
//     sel        = (smax > max_scaling) & (smax / smin > scale_threshold)
//     scale_loss = smax[sel].mean() if sel.any() else 0
// The mean's denominator is the number of SELECTED rows, known only once every row has been seen: the first launch reduces
// the sum and the count (k_gaussian_regularise's tail) and stores {scale_loss, count}; the second recomputes every row's
// selection with the same function (scale_row) and ADDS  weight x smax / count  (d smax / d _scaling[argmax] = smax) to the
// row's largest component, by the lane that owns the row.  The count travels as a float: every addend is 0 or 1 and every
// partial result an integer <= P < 2^24 (the entry point refuses more), so it is exact.  No float atomics; with nothing
// selected the second launch returns at once and no 0 / 0 is evaluated.
struct ScaleRow {
    float smax;      // the row's largest activated scale ...
    int arg;         // ... and its component: the FIRST of equal ones (torch.max's gradient goes to one index)
    bool selected;
};

// THE selection of both launches.  Every comparison with a NaN is false and torch.max / torch.min propagate a NaN: a row
// that holds one is not selected (arg and smax are then not used).
__device__ __forceinline__ ScaleRow scale_row(const float* __restrict__ scaling, unsigned i, float max_scaling, float scale_threshold)
{
    const size_t o = (size_t)i * 3;
    const float e0 = act_exp(scaling[o]), e1 = act_exp(scaling[o + 1]), e2 = act_exp(scaling[o + 2]);
    ScaleRow r;
    r.smax = e0, r.arg = 0;
    if (e1 > r.smax) r.smax = e1, r.arg = 1;
    if (e2 > r.smax) r.smax = e2, r.arg = 2;
    const float smin = fminf(e0, fminf(e1, e2));
    const bool numbers = e0 == e0 && e1 == e1 && e2 == e2;
    r.selected = numbers && r.smax > max_scaling && r.smax / smin > scale_threshold;
    return r;
}

struct ScaleTermArgs {
    const float* scaling;
    float* d_scaling;     // the second launch's; never null there
    float* partial;       // [2][kRegMaxBlocks]
    unsigned* counter;
    float* loss;          // {scale_loss, selected rows}
    int P;
    float weight, scale_threshold, max_scaling;
};

__global__ void __launch_bounds__(kSumThreads) k_scale_term_sum(ScaleTermArgs a)
{
    const unsigned stride = gridDim.x * blockDim.x;
    float acc[2] = {0.f, 0.f};   // sum of smax over the selected rows, their number
    for (unsigned i = blockIdx.x * blockDim.x + threadIdx.x; i < (unsigned)a.P; i += stride) {
        const ScaleRow r = scale_row(a.scaling, i, a.max_scaling, a.scale_threshold);
        if (r.selected) acc[0] += r.smax, acc[1] += 1.f;
    }
    if (!sum_over_workgroups(acc, a.partial, kRegMaxBlocks, a.counter, blockIdx.x, gridDim.x)) return;
    a.loss[0] = acc[1] > 0.f ? acc[0] / acc[1] : 0.f;
    a.loss[1] = acc[1];
}

__global__ void __launch_bounds__(kSumThreads) k_scale_term_grad(ScaleTermArgs a)
{
    float* __restrict__ d_scaling = a.d_scaling;
    const float count = a.loss[1];      // (the launch in front of this one stored it)
    if (!(count > 0.f)) return;
    const float g = a.weight / count;
    const unsigned stride = gridDim.x * blockDim.x;
    for (unsigned i = blockIdx.x * blockDim.x + threadIdx.x; i < (unsigned)a.P; i += stride) {
        const ScaleRow r = scale_row(a.scaling, i, a.max_scaling, a.scale_threshold);
        if (r.selected) d_scaling[(size_t)i * 3 + r.arg] += g * r.smax;
    }
}

size_t scale_term_workspace_bytes() { return done_workspace_bytes(2 * kRegMaxBlocks); }

int launch_scale_term(const fr_scale_term_config& cfg, int P, const float* scaling, float* d_scaling, float* loss, void* workspace,
                      hipStream_t s)
{
    if (P <= 0) return FR_OK;
    const unsigned blocks = capped_blocks((unsigned)P, kSumThreads, kRegMaxBlocks);
    const DoneWorkspace ws = done_workspace(workspace);
    ScaleTermArgs a;
    a.scaling = scaling, a.d_scaling = d_scaling;
    a.counter = ws.counter, a.partial = ws.partial;
    a.loss = loss, a.P = P;
    a.weight = cfg.weight, a.scale_threshold = cfg.scale_threshold, a.max_scaling = cfg.max_scaling;
    hipLaunchKernelGGL(k_scale_term_sum, dim3(blocks), dim3(kSumThreads), 0, s, a);
    FR_HIP(hipGetLastError());
    if (d_scaling && cfg.weight != 0.f) {   // (a zero weight, a null array: no gradient traffic)
        hipLaunchKernelGGL(k_scale_term_grad, dim3(blocks), dim3(kSumThreads), 0, s, a);
        FR_HIP(hipGetLastError());
    }
    return FR_OK;
}

}  // namespace fr
