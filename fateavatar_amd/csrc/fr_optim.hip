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

// ---------------------------------------------------------------- the per-pixel image terms and their gradients, one launch each
// Four objectives on the differences d = img - gt.  The reference follows each with loss.backward(): in PyTorch eight (L1: sub,
// abs, mean, fill, sign, mul, ...: 41 us of a 205 us optimisation step at 512 x 512) to about thirty (Huber) launch-bound
// elementwise / reduction kernels with autograd's twins.  Here one pass gives the loss words and the gradient autograd would
// hand to the rasterizer:
//   L1Term       nn.L1Loss(reduction='mean') on the rendered image (model/loss.py:92): mean |d|, gradient sign(d) / n
//   L1WordsTerm  the same with fr_image_loss_grad's outputs, its path for a D-SSIM weight of 0: gradient rgb_weight sign(d) / n
//   HuberTerm    FlashAvatarLoss.get_huber_loss (train/loss.py:217-221) on the image and, with a mouth mask, once more on the
//                masked image and target at weight 40 (:231-239)
//   PixelTerm    SplattingAvatarLoss.accumulate_gradients (train/loss.py:288-304; get_rgb_loss / get_mse_loss :279-283) with
//                rgb_loss 1.0 and mse_loss 10.0 of config/splattingavatar.yaml:13-20: L1 + MSE
// image_term_sweep is the pass they share: float4 pieces on a grid capped at kL1MaxBlocks, a tail in workgroup 0, per-workgroup
// partial sums, and the workgroup that finishes last adds the partials up in index order (deterministic) and hands the totals
// to the term (sum_over_workgroups, fr_common.hpp: every fused loss kernel of the library ends with it).  A term says what one
// difference adds to which of its kSums sums and which gradient word it gives (`one`), what the totals mean (`finish`), and
// whether the partials are put back to zero (kZero: all but the plain L1, whose one row every launch overwrites).  The terms
// whose first sum takes fabsf(d) run the plain L1 kernel's sweep on its grid with its first accumulator: the same addends in
// the same order through the same tree, so loss[1] of L1WordsTerm and of PixelTerm is fr_l1_loss_grad's loss, bit for bit.
constexpr unsigned kL1MaxBlocks = 1024;

struct LossView {   // one image of a (possibly batched) launch
    const float* img;
    const float* gt;
    float* grad;         // or null
    float* partial;      // [kSums][kL1MaxBlocks]
    unsigned* counter;
    float* loss;
};

template <typename Term>
__device__ __forceinline__ void image_term_sweep(const LossView& v, unsigned long long n, const Term& t)
{
    const float* __restrict__ img = v.img;
    const float* __restrict__ gt = v.gt;
    float* __restrict__ grad = v.grad;
    // (kSumThreads is blockDim.x: the launcher's block size, and the one sum_over_workgroups asks for)
    const unsigned long long n4 = n / 4, stride = (unsigned long long)gridDim.x * kSumThreads;
    float acc[Term::kSums] = {};
    for (unsigned long long i = (unsigned long long)blockIdx.x * kSumThreads + threadIdx.x; i < n4; i += stride) {
        const float4 a = reinterpret_cast<const float4*>(img)[i], b = reinterpret_cast<const float4*>(gt)[i];
        const float d[4] = {a.x - b.x, a.y - b.y, a.z - b.z, a.w - b.w};
        float g[4];
#pragma unroll
        for (int k = 0; k < 4; k++) g[k] = t.one(4 * i + k, d[k], acc);
        if (grad) reinterpret_cast<float4*>(grad)[i] = make_float4(g[0], g[1], g[2], g[3]);
    }
    if (blockIdx.x == 0 && threadIdx.x < (unsigned)(n - 4 * n4)) {   // tail of a length that is not a multiple of 4
        const unsigned long long e = 4 * n4 + threadIdx.x;
        const float g = t.one(e, img[e] - gt[e], acc);
        if (grad) grad[e] = g;
    }
    if (!sum_over_workgroups<Term::kSums, Term::kZero>(acc, v.partial, kL1MaxBlocks, v.counter, blockIdx.x, gridDim.x)) return;
    t.finish(acc, v.loss);
}

__device__ __forceinline__ float sign_times(float d, float g) { return d > 0.f ? g : (d < 0.f ? -g : 0.f); }   // torch.sign: 0 at 0

struct L1Term {
    static constexpr int kSums = 1;
    static constexpr bool kZero = false;
    float inv_n;
    __device__ __forceinline__ float one(unsigned long long, float d, float (&acc)[1]) const
    {
        acc[0] += fabsf(d);
        return sign_times(d, inv_n);
    }
    __device__ __forceinline__ void finish(const float (&acc)[1], float* loss) const { *loss = acc[0] * inv_n; }
};

struct L1WordsTerm {   // loss = {rgb_weight x l1, l1, 0}
    static constexpr int kSums = 1;
    static constexpr bool kZero = true;
    float inv_n, g_mag, rgb_weight;   // g_mag = rgb_weight / n
    __device__ __forceinline__ float one(unsigned long long, float d, float (&acc)[1]) const
    {
        acc[0] += fabsf(d);
        return sign_times(d, g_mag);
    }
    __device__ __forceinline__ void finish(const float (&acc)[1], float* loss) const
    {
        const float l1 = acc[0] * inv_n;
        loss[0] = rgb_weight * l1, loss[1] = l1, loss[2] = 0.f;
    }
};

//   h(x) = 0.5 x^2 if |x| < alpha else alpha (|x| - 0.5 alpha);  h'(x) = x if |x| < alpha else alpha sign(x)
struct HuberTerm {   // sums: huber, mouth; loss = {huber + mask_weight x mouth, huber, mouth}
    static constexpr int kSums = 2;
    static constexpr bool kZero = true;
    const float* mask;   // [HW] or null
    unsigned hw;
    float alpha, mask_weight, inv_n;
    // h and h' of one difference x: the value is added to `acc`, the derivative returned
    __device__ __forceinline__ float h(float x, float& acc) const
    {
        const float ax = fabsf(x);
        if (ax < alpha) {
            acc += 0.5f * x * x;
            return x;
        }
        acc += alpha * (ax - 0.5f * alpha);
        return x < 0.f ? -alpha : alpha;
    }
    __device__ __forceinline__ float one(unsigned long long e, float d, float (&acc)[2]) const
    {
        float g = h(d, acc[0]);
        if (mask) {
            const float m = mask[e % hw];   // [1,H,W] broadcast over the channels
            g += mask_weight * m * h(m * d, acc[1]);
        }
        return g * inv_n;
    }
    __device__ __forceinline__ void finish(const float (&acc)[2], float* loss) const
    {
        const float huber = acc[0] * inv_n, mouth = acc[1] * inv_n;
        loss[0] = huber + mask_weight * mouth, loss[1] = huber, loss[2] = mouth;
    }
};

struct PixelTerm {   // sums: l1, mse; loss = {rgb_weight x l1 + mse_weight x mse, l1, mse}
    static constexpr int kSums = 2;
    static constexpr bool kZero = true;
    float rgb_weight, mse_weight, inv_n;
    float g_l1, g_mse;   // rgb_weight / n, 2 mse_weight / n
    // the gradient word  rgb_weight sign(d) / n + mse_weight 2 d / n
    __device__ __forceinline__ float one(unsigned long long, float d, float (&acc)[2]) const
    {
        acc[0] += fabsf(d);
        acc[1] += d * d;
        return sign_times(d, g_l1) + g_mse * d;
    }
    __device__ __forceinline__ void finish(const float (&acc)[2], float* loss) const
    {
        const float l1 = acc[0] * inv_n, mse = acc[1] * inv_n;
        loss[0] = rgb_weight * l1 + mse_weight * mse, loss[1] = l1, loss[2] = mse;
    }
};

// (the *_batch and *_terms kernels: the images of the frames of a batch, same size, one workspace each: grid (x, images))
__global__ void __launch_bounds__(kSumThreads) k_l1_loss_grad(LossView v, unsigned long long n, L1Term t) { image_term_sweep(v, n, t); }
__global__ void __launch_bounds__(kSumThreads) k_l1_loss_grad_batch(BatchOf<LossView> b, unsigned long long n, L1Term t) { image_term_sweep(b.v[blockIdx.y], n, t); }
__global__ void __launch_bounds__(kSumThreads) k_l1_loss_grad_terms(BatchOf<LossView> b, unsigned long long n, L1WordsTerm t) { image_term_sweep(b.v[blockIdx.y], n, t); }
__global__ void __launch_bounds__(kSumThreads) k_huber_loss_grad(LossView v, unsigned long long n, HuberTerm t) { image_term_sweep(v, n, t); }
__global__ void __launch_bounds__(kSumThreads) k_pixel_loss_grad(LossView v, unsigned long long n, PixelTerm t) { image_term_sweep(v, n, t); }

size_t l1_workspace_bytes() { return done_workspace_bytes(kL1MaxBlocks); }
size_t huber_workspace_bytes() { return done_workspace_bytes(HuberTerm::kSums * kL1MaxBlocks); }
size_t pixel_loss_workspace_bytes() { return done_workspace_bytes(PixelTerm::kSums * kL1MaxBlocks); }

// a float4 per thread and sweep: what the sweep takes per workgroup
static unsigned l1_blocks(unsigned long long n) { return capped_blocks(n / 4, kSumThreads, kL1MaxBlocks); }
static float over_n(double x, unsigned long long n) { return n ? (float)(x / (double)n) : 0.f; }   // (n == 0 launches nothing)

// `kernel` takes one LossView (n_images = 1) or a BatchOf<> of them
template <typename Views, typename Term>
static int launch_image_term(void (*kernel)(Views, unsigned long long, Term), int n_images, unsigned long long n, const float* const* img,
                             const float* const* gt, float* const* grad, float* const* loss, void* const* workspace, const Term& t,
                             hipStream_t s)
{
    if (n == 0 || n_images <= 0) return FR_OK;
    BatchOf<LossView> b;
    for (int k = 0; k < kMaxBatch; k++) {
        const int j = k < n_images ? k : 0;   // (unused entries: never indexed, blockIdx.y < n_images)
        const DoneWorkspace ws = done_workspace(workspace[j]);
        b.v[k] = LossView{img[j], gt[j], grad ? grad[j] : nullptr, ws.partial, ws.counter, loss[j]};
    }
    const dim3 grid(l1_blocks(n), (unsigned)n_images);
    if constexpr (std::is_same<Views, LossView>::value) hipLaunchKernelGGL(kernel, grid, dim3(kSumThreads), 0, s, b.v[0], n, t);
    else hipLaunchKernelGGL(kernel, grid, dim3(kSumThreads), 0, s, b, n, t);
    FR_HIP(hipGetLastError());
    return FR_OK;
}

int launch_l1_loss_grad(unsigned long long n, const float* img, const float* gt, float* grad, float* loss, void* workspace,
                        hipStream_t s)
{
    return launch_image_term(k_l1_loss_grad, 1, n, &img, &gt, &grad, &loss, &workspace, L1Term{over_n(1.0, n)}, s);
}

int launch_l1_loss_grad_batch(int n_images, unsigned long long n, const float* const* img, const float* const* gt, float* const* grad,
                              float* const* loss, void* const* workspace, hipStream_t s)
{
    return launch_image_term(k_l1_loss_grad_batch, n_images, n, img, gt, grad, loss, workspace, L1Term{over_n(1.0, n)}, s);
}

int launch_l1_loss_grad_terms(int n_images, unsigned long long n, float rgb_weight, const float* const* img, const float* const* gt,
                              float* const* grad, float* const* loss, void* const* workspace, hipStream_t s)
{
    const L1WordsTerm t{over_n(1.0, n), over_n(rgb_weight, n), rgb_weight};
    return launch_image_term(k_l1_loss_grad_terms, n_images, n, img, gt, grad, loss, workspace, t, s);
}

int launch_huber_loss_grad(const fr_huber_config& cfg, int C, int H, int W, const float* img, const float* gt, const float* mask,
                           float* grad, float* loss, void* workspace, hipStream_t s)
{
    const unsigned long long hw = (unsigned long long)H * (unsigned long long)W, n = hw * (unsigned long long)C;
    const HuberTerm t{mask, (unsigned)hw, cfg.alpha, mask ? cfg.mask_weight : 0.f, over_n(1.0, n)};
    return launch_image_term(k_huber_loss_grad, 1, n, &img, &gt, &grad, &loss, &workspace, t, s);
}

int launch_pixel_loss_grad(const fr_pixel_loss_config& cfg, int C, int H, int W, const float* img, const float* gt, float* grad,
                           float* loss, void* workspace, hipStream_t s)
{
    const unsigned long long n = (unsigned long long)H * (unsigned long long)W * (unsigned long long)C;
    const PixelTerm t{cfg.rgb_weight, cfg.mse_weight, over_n(1.0, n), over_n(cfg.rgb_weight, n), over_n(2.0 * cfg.mse_weight, n)};
    return launch_image_term(k_pixel_loss_grad, 1, n, &img, &gt, &grad, &loss, &workspace, t, s);
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

// ---------------------------------------------------------------- FateAvatar's scale-ratio term, one launch
// reference: FateAvatarLoss.accumulate_gradients (train/loss.py:144-151) on model_outputs['scale'] = exp(_scaling), the RAW
// parameter (model/fateavatar.py:282: not the face-resized scale the rasterizer sees):
//     ratio      = scale.max(-1) / scale.min(-1)
//     scale_loss = relu(ratio - scale_threshold).mean()
// The mean's denominator is P, known at launch: unlike SplattingAvatar's term above, ONE launch gives the loss and the
// gradient.  Lane = Gaussian: the row's relu(ratio - threshold) and, over the threshold,  +weight / P x ratio  ADDED to its
// largest component's gradient and  -weight / P x ratio  to its smallest (d ratio / d _scaling[argmax] = ratio, [argmin] =
// -ratio), by the lane that owns the row (no atomics).  The ratio is the reference's float32 quotient of the two activated
// components, not exp(smax - smin).  Sub-gradients are autograd's: relu passes nothing at exactly 0; max / min give their
// gradient to ONE index, the FIRST of equal components (scale_row's rule); where argmax == argmin (three equal components)
// the two contributions are formed in registers and cancel to an exact 0 in one store.  A row whose ratio is not finite — a
// NaN component, exp overflowing, the smallest component underflowing to 0 — adds nothing to the loss, the count or the
// gradient (a non-finite Gaussian is dropped from a frame the same way; stock PyTorch would make the loss NaN or inf).  The
// count of rows over the threshold travels as a float, exact below 2^24 rows (the entry point refuses more).
struct ScaleRatioArgs {
    const float* scaling;
    float* d_scaling;     // null: no gradient traffic (also what a zero weight gives)
    float* partial;       // [2][kRegMaxBlocks]
    unsigned* counter;
    float* loss;          // {scale_loss, rows over the threshold}, unweighted
    int P;
    float g, scale_threshold;   // g = weight / P
};

__global__ void __launch_bounds__(kSumThreads) k_scale_ratio_term(ScaleRatioArgs a)
{
    const float* __restrict__ scaling = a.scaling;
    float* __restrict__ d_scaling = a.d_scaling;
    const unsigned stride = gridDim.x * blockDim.x;
    float acc[2] = {0.f, 0.f};   // sum of relu(ratio - threshold), rows over the threshold
    for (unsigned i = blockIdx.x * blockDim.x + threadIdx.x; i < (unsigned)a.P; i += stride) {
        const size_t o = (size_t)i * 3;
        const float e0 = act_exp(scaling[o]), e1 = act_exp(scaling[o + 1]), e2 = act_exp(scaling[o + 2]);
        float smax = e0, smin = e0;
        int amax = 0, amin = 0;
        if (e1 > smax) smax = e1, amax = 1;
        if (e2 > smax) smax = e2, amax = 2;
        if (e1 < smin) smin = e1, amin = 1;
        if (e2 < smin) smin = e2, amin = 2;
        const float ratio = smax / smin;
        // (every comparison with a NaN is false: a NaN component, inf / inf and 0 / 0 fail the last one; x / 0 the one before)
        const bool finite = e0 == e0 && e1 == e1 && e2 == e2 && fabsf(ratio) < INFINITY;
        if (!finite || !(ratio > a.scale_threshold)) continue;
        acc[0] += ratio - a.scale_threshold, acc[1] += 1.f;
        if (!d_scaling) continue;
        const float g = a.g * ratio;
        if (amax == amin) {
            d_scaling[o + amax] += g - g;
        } else {
            d_scaling[o + amax] += g;
            d_scaling[o + amin] -= g;
        }
    }
    if (!sum_over_workgroups(acc, a.partial, kRegMaxBlocks, a.counter, blockIdx.x, gridDim.x)) return;
    a.loss[0] = acc[0] / (float)a.P;
    a.loss[1] = acc[1];
}

size_t scale_ratio_workspace_bytes() { return done_workspace_bytes(2 * kRegMaxBlocks); }

int launch_scale_ratio_term(const fr_scale_ratio_config& cfg, int P, const float* scaling, float* d_scaling, float* loss,
                            void* workspace, hipStream_t s)
{
    if (P <= 0) return FR_OK;
    const unsigned blocks = capped_blocks((unsigned)P, kSumThreads, kRegMaxBlocks);
    const DoneWorkspace ws = done_workspace(workspace);
    ScaleRatioArgs a;
    a.scaling = scaling;
    a.d_scaling = cfg.weight != 0.f ? d_scaling : nullptr;   // a zero weight: the array is not touched
    a.counter = ws.counter, a.partial = ws.partial;
    a.loss = loss, a.P = P;
    a.g = (float)((double)cfg.weight / (double)P), a.scale_threshold = cfg.scale_threshold;
    hipLaunchKernelGGL(k_scale_ratio_term, dim3(blocks), dim3(kSumThreads), 0, s, a);
    FR_HIP(hipGetLastError());
    return FR_OK;
}

}  // namespace fr
