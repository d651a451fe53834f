// FlashAvatar's deformation MLP, forward and backward, on gfx950's exact-f32 MFMA (fr_mlp_forward / fr_mlp_backward,
// include/fr_rasterizer.h).
//
// reference: `MLP` (model/baseline/flashavatar.py:434-464) fed by `forward` (:238-240):
//     h = cat([embedded canonical point, condition.expand(N, -1)], -1);  for fc in fcs: h = relu(fc(h));  out = output_linear(h)
// nn.Linear forward and backward through the vendor BLAS, seven of each per frame.
//
// ONE GEMM kernel, four instantiations, a launch per layer and product:
//     forward     H_l     = relu(H_{l-1} W_l^T + b_l)        A = H [N,K] (k contiguous), B = W [256,K] (k contiguous)
//     output      out     = H_{L-1} W_out^T + b_out          the same without the ReLU (D_out <= 16 of the tile's 64 columns are live)
//     backward    dZ_{l-1} = (dZ_l W_l) * [H_{l-1} > 0]      A = dZ [N,K] (k contiguous), B = W [K,256] (n contiguous)
//     weights     dW_l    = dZ_l^T H_{l-1}                   A = dZ (m contiguous), B = H (n contiguous), K = the points, split
// The condition half of layer 0's input is the same for every point, so it is folded into the bias by k_mlp_cond_bias
// (256 dot products of Dc terms) and layer 0's GEMM runs over E's De columns alone; backwards, dW_0's condition columns and
// d_cond come from db_0 (k_mlp_cond_grad).
//
// Tiling.  A workgroup is 4 waves in a 2 x 2 arrangement, each wave TM x TN accumulator tiles of 32 x 32
// (mfma_f32_32x32x2f32: 16 accumulator registers per tile, statically indexed).  The forward and backward-data products use
// 128 points x 64 columns (TM = 2, TN = 1: 32 accumulator registers), K in steps of 32 through LDS.  Both operands are stored
// k-major in LDS ([32][tile + 33] floats, 33 KB for the 128 x 64 tile): an MFMA operand read is then 32 consecutive words
// for each of the two k of the instruction, and the odd row stride keeps the TRANSPOSING store of a k-contiguous operand (32
// lanes = 32 k of one row) off a common bank.  Global loads of the next K step are issued into registers before the MFMAs of
// the current one (one step of software pipelining, 16 + 8 staging registers).
// Weight traffic: a 128 x 64 workgroup reads a QUARTER of the layer's 256 KB weight matrix (its 64 output columns) once per
// 128 points: 64 KB per workgroup per layer against 2 x 128 x 64 x 256 = 4.2 MFLOP, 64 FLOP per L2 byte of weights, and
// 128 KB of activations (32 FLOP per byte of those).  All of a layer's weights stay in the L2.  (128 x 128 tiles halve the
// activation reads but leave 16 384 points with ONE workgroup per CU: measured slower at both sizes, EXPERIMENTS.md.)
// The weight-gradient product is split over the points in chunks of FR_MLP_CHUNK = 256: a 64 x 64 tile per workgroup
// (TM = TN = 1) and one grid z-plane per chunk, each writing its own partial [256 x in | bias] (k_mlp_colsum adds the bias
// row: column sums of dZ, four row phases per column combined in a fixed order).  k_mlp_reduce then adds the chunks'
// partials in chunk order into d_weights: no float atomics anywhere, the same bits on every launch and graph replay.
// The partial buffer is one layer's and is reused by the next (the launches are stream ordered).
//
// Raggedness: every tile load is bounds-checked and zero-filled (rows past M or N, k past the chunk's end), every store is
// bounds-checked: no caller pads.  Rows of E are De floats (51 in the reference: not 16-byte aligned), so global loads are
// single dwords, coalesced along the contiguous index.
// FAST flags (FMA contraction): nothing here mirrors a reference operation order; the products are MFMA either way.
#include "fr_common.hpp"

namespace fr {

constexpr int kMlpW = FR_MLP_WIDTH;
constexpr int kMlpBK = 32;          // K step through LDS
constexpr int kMlpPad = 33;         // LDS row = tile + 33 floats (odd; the instruction's second k lands 33 banks on)
constexpr int kMlpThreads = 256;
constexpr int kMlpChunk = FR_MLP_CHUNK;
static_assert(FR_MLP_POINT_TILE == 128, "the forward tile is 2 x 2 waves of 2 x 1 MFMA tiles: 128 points x 64 columns");

enum { MLP_EPI_PLAIN = 0, MLP_EPI_BIAS_RELU = 1, MLP_EPI_BIAS = 2, MLP_EPI_MASK = 3 };

typedef float f32x16 __attribute__((ext_vector_type(16)));

struct MlpGemmArgs {
    const float* A;      // A(m, k): A_KC ? A[m * lda + k] : A[k * lda + m]
    const float* B;      // B(k, n): B_KC ? B[n * ldb + k] : B[k * ldb + n]
    float* C;            // C[z * c_plane + m * ldc + n]
    const float* aux;    // BIAS*: [N] per column; MASK: [M, ldc], the result is kept where aux > 0
    int M, N, K;
    int lda, ldb, ldc;
    int k_chunk;         // plane z of the grid sums k in [z * k_chunk, min(K, (z + 1) * k_chunk))
    unsigned c_plane;
};

// one operand tile's global -> register fetch: ROWS x kMlpBK values, kMlpThreads threads
template <int ROWS, bool KC>
__device__ __forceinline__ void mlp_fetch(float (&r)[ROWS * kMlpBK / kMlpThreads], const float* __restrict__ src, int ld, int row0,
                                          int n_rows, int k0, int k_end, unsigned t)
{
    constexpr int PER = ROWS * kMlpBK / kMlpThreads;
#pragma unroll
    for (int i = 0; i < PER; i++) {
        int row, k;
        if (KC) {   // 32 lanes = 32 consecutive k of one row
            k = (int)(t & 31u);
            row = (int)(t >> 5) + i * (kMlpThreads / 32);
        } else {    // ROWS lanes = consecutive rows of one k
            row = (int)(t % ROWS);
            k = (int)(t / ROWS) + i * (kMlpThreads / ROWS);
        }
        const int gr = row0 + row, gk = k0 + k;
        float v = 0.f;
        if (gr < n_rows && gk < k_end) v = KC ? src[(size_t)gr * ld + gk] : src[(size_t)gk * ld + gr];
        r[i] = v;
    }
}

template <int ROWS, bool KC>
__device__ __forceinline__ void mlp_stage(const float (&r)[ROWS * kMlpBK / kMlpThreads], float (*lds)[ROWS + kMlpPad], unsigned t)
{
    constexpr int PER = ROWS * kMlpBK / kMlpThreads;
#pragma unroll
    for (int i = 0; i < PER; i++) {
        int row, k;
        if (KC) {
            k = (int)(t & 31u);
            row = (int)(t >> 5) + i * (kMlpThreads / 32);
        } else {
            row = (int)(t % ROWS);
            k = (int)(t / ROWS) + i * (kMlpThreads / ROWS);
        }
        lds[k][row] = r[i];
    }
}

template <int TM, int TN, bool A_KC, bool B_KC, int EPI>
__global__ void __launch_bounds__(kMlpThreads) k_mlp_gemm(MlpGemmArgs g)
{
    constexpr int BM = 64 * TM, BN = 64 * TN;
    __shared__ float As[kMlpBK][BM + kMlpPad];
    __shared__ float Bs[kMlpBK][BN + kMlpPad];
    const float* __restrict__ A = g.A;
    const float* __restrict__ B = g.B;
    const unsigned t = threadIdx.x, lane = t & 63u, wave = t >> 6;
    const int lr = (int)(lane & 31u), lh = (int)(lane >> 5);
    const int wm = (int)(wave >> 1) * 32 * TM, wn = (int)(wave & 1u) * 32 * TN;
    const int m0 = (int)blockIdx.x * BM, n0 = (int)blockIdx.y * BN;
    const int k_begin = (int)blockIdx.z * g.k_chunk;
    const int k_end = min(g.K, k_begin + g.k_chunk);

    f32x16 acc[TM][TN];
#pragma unroll
    for (int i = 0; i < TM; i++)
#pragma unroll
        for (int j = 0; j < TN; j++)
#pragma unroll
            for (int r = 0; r < 16; r++) acc[i][j][r] = 0.f;

    float ra[BM * kMlpBK / kMlpThreads], rb[BN * kMlpBK / kMlpThreads];
    mlp_fetch<BM, A_KC>(ra, A, g.lda, m0, g.M, k_begin, k_end, t);
    mlp_fetch<BN, B_KC>(rb, B, g.ldb, n0, g.N, k_begin, k_end, t);
    for (int k0 = k_begin; k0 < k_end; k0 += kMlpBK) {
        __syncthreads();    // (the previous step's operand reads are done)
        mlp_stage<BM, A_KC>(ra, As, t);
        mlp_stage<BN, B_KC>(rb, Bs, t);
        __syncthreads();
        if (k0 + kMlpBK < k_end) {
            mlp_fetch<BM, A_KC>(ra, A, g.lda, m0, g.M, k0 + kMlpBK, k_end, t);
            mlp_fetch<BN, B_KC>(rb, B, g.ldb, n0, g.N, k0 + kMlpBK, k_end, t);
        }
#pragma unroll
        for (int kk = 0; kk < kMlpBK; kk += 2) {
            float a[TM], b[TN];
#pragma unroll
            for (int i = 0; i < TM; i++) a[i] = As[kk + lh][wm + i * 32 + lr];
#pragma unroll
            for (int j = 0; j < TN; j++) b[j] = Bs[kk + lh][wn + j * 32 + lr];
#pragma unroll
            for (int i = 0; i < TM; i++)
#pragma unroll
                for (int j = 0; j < TN; j++) acc[i][j] = __builtin_amdgcn_mfma_f32_32x32x2f32(a[i], b[j], acc[i][j], 0, 0, 0);
        }
    }

    // C/D map of the 32 x 32 tile: column = lane & 31, row = (r & 3) + 8 (r >> 2) + 4 (lane >> 5)
    float* __restrict__ C = g.C + (size_t)blockIdx.z * g.c_plane;
    const float* __restrict__ aux = g.aux;
#pragma unroll
    for (int j = 0; j < TN; j++) {
        const int col = n0 + wn + j * 32 + lr;
        if (col >= g.N) continue;
        float bias = 0.f;
        if (EPI == MLP_EPI_BIAS_RELU || EPI == MLP_EPI_BIAS) bias = aux[col];
#pragma unroll
        for (int i = 0; i < TM; i++) {
#pragma unroll
            for (int r = 0; r < 16; r++) {
                const int row = m0 + wm + i * 32 + (r & 3) + 8 * (r >> 2) + 4 * lh;
                if (row >= g.M) continue;
                const size_t o = (size_t)row * g.ldc + col;
                float v = acc[i][j][r];
                if (EPI == MLP_EPI_BIAS_RELU) v = fmaxf(v + bias, 0.f);
                if (EPI == MLP_EPI_BIAS) v = v + bias;
                if (EPI == MLP_EPI_MASK) v = aux[o] > 0.f ? v : 0.f;
                C[o] = v;
            }
        }
    }
}

// bias0[j] = b0[j] + sum_i W0[j, De + i] cond[i]   (ascending i, one fmaf chain per unit)
__global__ void __launch_bounds__(kMlpW) k_mlp_cond_bias(const float* __restrict__ W0, int De, int Dc, const float* __restrict__ cond,
                                                       float* __restrict__ bias0)
{
    const int j = (int)threadIdx.x, in0 = De + Dc;
    float s = W0[(size_t)kMlpW * in0 + j];
    for (int i = 0; i < Dc; i++) s = fmaf(W0[(size_t)j * in0 + De + i], cond[i], s);
    bias0[j] = s;
}

// dW0[:, De:] = db0 (x) cond and d_cond = W0[:, De:]^T db0 (ascending j), from the db0 k_mlp_reduce has just written
__global__ void __launch_bounds__(kMlpW) k_mlp_cond_grad(const float* __restrict__ W0, float* __restrict__ dW0, int De, int Dc,
                                                       const float* __restrict__ cond, float* __restrict__ d_cond)
{
    const int j = (int)threadIdx.x, in0 = De + Dc;
    const float* __restrict__ db0 = dW0 + (size_t)kMlpW * in0;
    const float d = db0[j];
    for (int i = 0; i < Dc; i++) dW0[(size_t)j * in0 + De + i] = d * cond[i];
    if (d_cond && j < Dc) {
        // eight interleaved chains of 32 units, combined as a fixed tree (a single chain of 256 carries about twice the error)
        float s[8] = {0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f};
        for (int u = 0; u < kMlpW; u += 8)
#pragma unroll
            for (int q = 0; q < 8; q++) s[q] = fmaf(W0[(size_t)(u + q) * in0 + De + j], db0[u + q], s[q]);
        d_cond[j] = ((s[0] + s[1]) + (s[2] + s[3])) + ((s[4] + s[5]) + (s[6] + s[7]));
    }
}

// the bias row of a chunk's partial: column sums of dZ over the chunk's points.  Workgroup (chunk, 64-column group): four row
// phases of 64 columns, each an ascending sum over every fourth row, combined as ((p0 + p1) + p2) + p3.
__global__ void __launch_bounds__(kMlpThreads) k_mlp_colsum(const float* __restrict__ dZ, int ld, int width, int N, float* __restrict__ partial,
                                                          unsigned plane, unsigned bias_offset)
{
    __shared__ float part[4][64];
    const int c = (int)(blockIdx.y * 64u + (threadIdx.x & 63u)), phase = (int)(threadIdx.x >> 6);
    const int n_begin = (int)blockIdx.x * kMlpChunk, n_end = min(N, n_begin + kMlpChunk);
    float s = 0.f;
    if (c < width)
        for (int n = n_begin + phase; n < n_end; n += 4) s += dZ[(size_t)n * ld + c];
    part[phase][threadIdx.x & 63u] = s;
    __syncthreads();
    if (phase == 0 && c < width) {
        const unsigned k = threadIdx.x;
        partial[(size_t)blockIdx.x * plane + bias_offset + c] = ((part[0][k] + part[1][k]) + part[2][k]) + part[3][k];
    }
}

// d_weights' layer = the chunks' partials added in chunk order.  A partial is [rows x cols | rows]; the layer's weight rows
// are `ldo` floats apart (layer 0: cols = De of ldo = De + Dc, the rest is k_mlp_cond_grad's) and its bias follows them.
__global__ void __launch_bounds__(kMlpThreads) k_mlp_reduce(const float* __restrict__ partial, unsigned plane, int n_chunks, int rows, int cols,
                                                          int ldo, float* __restrict__ d_layer)
{
    const unsigned i = blockIdx.x * blockDim.x + threadIdx.x, n_w = (unsigned)(rows * cols);
    if (i >= n_w + (unsigned)rows) return;
    float s = 0.f;
    for (int c = 0; c < n_chunks; c++) s += partial[(size_t)c * plane + i];
    const size_t o = i < n_w ? (size_t)(i / (unsigned)cols) * ldo + i % (unsigned)cols : (size_t)rows * ldo + (i - n_w);
    d_layer[o] = s;
}

struct MlpWorkspace {
    float* H[FR_MLP_MAX_LAYERS];
    float* dZ[2];
    float* partial;
    float* bias0;
};

static int mlp_chunks(int N) { return (N + kMlpChunk - 1) / kMlpChunk; }
static constexpr unsigned kMlpPlane = (unsigned)((kMlpW + 1) * kMlpW);    // floats of one chunk's partial

size_t mlp_workspace_bytes(int N, int L)
{
    const size_t act = align_up((size_t)N * kMlpW * sizeof(float), 256);
    return (size_t)(L + 2) * act + align_up((size_t)mlp_chunks(N) * kMlpPlane * sizeof(float), 256) + align_up(kMlpW * sizeof(float), 256);
}

static MlpWorkspace mlp_workspace(void* ws, int N, int L)
{
    const size_t act = align_up((size_t)N * kMlpW * sizeof(float), 256);
    char* p = static_cast<char*>(ws);
    MlpWorkspace w{};
    for (int l = 0; l < L; l++) w.H[l] = reinterpret_cast<float*>(p), p += act;
    for (int k = 0; k < 2; k++) w.dZ[k] = reinterpret_cast<float*>(p), p += act;
    w.partial = reinterpret_cast<float*>(p), p += align_up((size_t)mlp_chunks(N) * kMlpPlane * sizeof(float), 256);
    w.bias0 = reinterpret_cast<float*>(p);
    return w;
}

// the flat buffer's layer l (0 .. L; L = the output layer): offset of its weight, its input and output widths
static size_t mlp_layer_offset(const fr_mlp& m, int l)
{
    const size_t in0 = (size_t)(m.De + m.Dc);
    return l == 0 ? 0 : (in0 + 1) * kMlpW + (size_t)(l - 1) * (kMlpW + 1) * kMlpW;
}
static size_t mlp_weight_floats(const fr_mlp& m) { return mlp_layer_offset(m, m.L) + (size_t)(kMlpW + 1) * m.D_out; }

template <int TM, int TN, bool A_KC, bool B_KC, int EPI>
static void mlp_gemm(const MlpGemmArgs& g, int planes, hipStream_t s)
{
    const dim3 grid((unsigned)((g.M + 64 * TM - 1) / (64 * TM)), (unsigned)((g.N + 64 * TN - 1) / (64 * TN)), (unsigned)planes);
    hipLaunchKernelGGL((k_mlp_gemm<TM, TN, A_KC, B_KC, EPI>), grid, dim3(kMlpThreads), 0, s, g);
}

int launch_mlp_forward(const fr_mlp& m, float* out, void* workspace, hipStream_t s)
{
    if (m.N == 0) return FR_OK;
    const MlpWorkspace w = mlp_workspace(workspace, m.N, m.L);
    const int in0 = m.De + m.Dc;
    hipLaunchKernelGGL(k_mlp_cond_bias, dim3(1), dim3(kMlpW), 0, s, m.weights, m.De, m.Dc, m.cond, w.bias0);
    for (int l = 0; l < m.L; l++) {
        const float* W = m.weights + mlp_layer_offset(m, l);
        MlpGemmArgs g{};
        g.A = l == 0 ? m.E : w.H[l - 1], g.lda = l == 0 ? m.De : kMlpW;
        g.B = W, g.ldb = l == 0 ? in0 : kMlpW;
        g.C = w.H[l], g.ldc = kMlpW;
        g.aux = l == 0 ? w.bias0 : W + (size_t)kMlpW * kMlpW;
        g.M = m.N, g.N = kMlpW, g.K = l == 0 ? m.De : kMlpW, g.k_chunk = g.K, g.c_plane = 0;
        mlp_gemm<2, 1, true, true, MLP_EPI_BIAS_RELU>(g, 1, s);
    }
    const float* W = m.weights + mlp_layer_offset(m, m.L);
    MlpGemmArgs g{};
    g.A = w.H[m.L - 1], g.lda = kMlpW, g.B = W, g.ldb = kMlpW, g.C = out, g.ldc = m.D_out;
    g.aux = W + (size_t)m.D_out * kMlpW;
    g.M = m.N, g.N = m.D_out, g.K = kMlpW, g.k_chunk = g.K, g.c_plane = 0;
    mlp_gemm<2, 1, true, true, MLP_EPI_BIAS>(g, 1, s);
    FR_HIP(hipGetLastError());
    return FR_OK;
}

int launch_mlp_backward(const fr_mlp& m, const float* d_out, float* d_weights, float* d_cond, void* workspace, hipStream_t s)
{
    if (m.N == 0) {
        FR_HIP(hipMemsetAsync(d_weights, 0, mlp_weight_floats(m) * sizeof(float), s));
        if (d_cond && m.Dc > 0) FR_HIP(hipMemsetAsync(d_cond, 0, (size_t)m.Dc * sizeof(float), s));
        return FR_OK;
    }
    const MlpWorkspace w = mlp_workspace(workspace, m.N, m.L);
    const int in0 = m.De + m.Dc, chunks = mlp_chunks(m.N);
    const float* dZ = d_out;
    int rows = m.D_out;     // the width of layer l's output = dZ's row length
    for (int l = m.L; l >= 0; l--) {
        const float* W = m.weights + mlp_layer_offset(m, l);
        float* dW = d_weights + mlp_layer_offset(m, l);
        const float* Hin = l == 0 ? m.E : w.H[l - 1];
        const int cols = l == 0 ? m.De : kMlpW, ldh = cols, ldo = l == 0 ? in0 : kMlpW;
        // dW_l = dZ_l^T H_{l-1} and db_l, chunk by chunk, then the chunks in order
        MlpGemmArgs g{};
        g.A = dZ, g.lda = rows, g.B = Hin, g.ldb = ldh, g.C = w.partial, g.ldc = cols, g.aux = nullptr;
        g.M = rows, g.N = cols, g.K = m.N, g.k_chunk = kMlpChunk, g.c_plane = kMlpPlane;
        mlp_gemm<1, 1, false, false, MLP_EPI_PLAIN>(g, chunks, s);
        hipLaunchKernelGGL(k_mlp_colsum, dim3((unsigned)chunks, (unsigned)((rows + 63) / 64)), dim3(kMlpThreads), 0, s, dZ, rows, rows, m.N,
                           w.partial, kMlpPlane, (unsigned)(rows * cols));
        const unsigned n_out = (unsigned)(rows * cols + rows);
        hipLaunchKernelGGL(k_mlp_reduce, dim3((n_out + kMlpThreads - 1) / kMlpThreads), dim3(kMlpThreads), 0, s, w.partial, kMlpPlane, chunks,
                           rows, cols, ldo, dW);
        if (l == 0) {
            if (m.Dc > 0) hipLaunchKernelGGL(k_mlp_cond_grad, dim3(1), dim3(kMlpW), 0, s, W, dW, m.De, m.Dc, m.cond, d_cond);
            break;
        }
        // dZ_{l-1} = (dZ_l W_l) * [H_{l-1} > 0]
        float* next = w.dZ[l & 1];
        MlpGemmArgs h{};
        h.A = dZ, h.lda = rows, h.B = W, h.ldb = kMlpW, h.C = next, h.ldc = kMlpW, h.aux = Hin;
        h.M = m.N, h.N = kMlpW, h.K = rows, h.k_chunk = rows, h.c_plane = 0;
        mlp_gemm<2, 1, true, false, MLP_EPI_MASK>(h, 1, s);
        dZ = next, rows = kMlpW;
    }
    FR_HIP(hipGetLastError());
    return FR_OK;
}

}  // namespace fr
