// FateAvatar's mesh terms and their gradient with respect to the posed vertices, one launch (fr_mesh_terms,
// include/fr_rasterizer.h).
//
// reference: FateAvatarLoss.get_laplacian_smoothing_loss and flame_loss (train/loss.py:112-121, :166-180, :192-197) —
//     L = meshes.laplacian_packed().to_dense()                       (V x V floats: 100.9 MB at V = 5023)
//     laplacian_loss = ((bmm(L, verts) - bmm(L, verts_orig)) ** 2).sum(-1, keepdim=True).mean()
//     flame_loss     = ((verts - verts_orig) ** 2).mean()
// three dense products per step (two forward, one backward).  L has V + 2 E non-zeros (35 071 of 25 230 529): here it is a
// CSR adjacency (binding.mesh_laplacian), L[i,i] = -1, L[i,j] = 1 / deg(i) for a neighbour j.
//
// A GROUP OF EIGHT LANES = one vertex.  With d = verts - verts_orig (the DIFFERENCE first: L verts and L verts_orig agree in
// their leading digits)
//     r_k = -d_k + (sum_{j in N(k)} d_j) * (1 / deg(k))        (ascending j; an empty row: r_k = -d_k)
//     g_i = -r_i + sum_{j in N(i)} r_j * (1 / deg(j))           (= (L^T r)_i: the adjacency is symmetric)
//     d_verts[i] += c_lap * g_i + c_flame * d_i                 (c_lap = weight * 2 / V, c_flame = weight * 2 / (3 V))
// The group RECOMPUTES r_j of the vertex's neighbours from d (the two-ring of i: about 36 rows of d on the head template, a few
// hundred at the eyeball poles, all of it in 60 KB the L2 holds): no workgroup depends on another one's r, so there is one
// launch and no grid barrier.  The 1 + deg(i) terms of g_i (i itself, then its neighbours) are dealt out to the group's lanes
// round-robin and the lanes' sums added up by a shuffle tree in a fixed order; lane 0 of the group is the only one that
// writes row i (a read-modify-write, no float atomics).  (One lane per vertex is the same arithmetic as ONE dependent chain
// of 6 x 32 gathers at a pole, and the launch waits for its slowest lane: 61 us on the MI355X against 100 ns of traffic.)
// The two loss sums go through per-workgroup partials added up in index order by the workgroup that finishes last
// (sum_over_workgroups, fr_common.hpp): the same bits on every launch and every replay.
//
// Roundings (what tests/test_gpu_mesh_terms.py holds the kernel to; eps = 2^-24, first order):
//     r_k: d_j 1, the sum's deg - 1 additions, 1 / deg 1, the product 1, the subtraction 1         -> (deg_k + 3) eps M^r_k
//     g_i: r_j as above (deg_j + 3), its 1 / deg(j) and product 2, at most deg_i additions of two non-zero terms (a lane's
//          own terms one after the other, then the tree; adding a lane's empty 0 is exact), c_lap and its product 2; the
//          flame term's constant, product and addition 3                                            -> (deg_i + deg_j + 10) eps
//     then the read-modify-write's own rounding.
//     loss: squares and the row's two additions 3, wave 6, the workgroup's four waves 2, the partials' wave 6 and four waves
//           2, 1 / V and its product 2: 21 (+ one per further partial of a lane: none up to 8 192 vertices; + one per
//           further visit of a group: none up to 32 768)
// Built with the STRICT flags: no FMA contraction, or the counts above would not describe the code.
#include "fr_common.hpp"

namespace fr {

constexpr unsigned kMeshMaxBlocks = 1024;
constexpr unsigned kMeshThreads = kSumThreads;   // (sum_over_workgroups' workgroup)
constexpr unsigned kMeshGroup = 8;           // lanes per vertex (a power of two that divides the wave)

struct MeshTermsArgs {
    const float* verts;
    const float* orig;
    const int* row_ptr;
    const int* col;
    float* d_verts;       // null: losses only
    float* partial;       // [2][kMeshMaxBlocks]
    unsigned* counter;
    float* loss;          // {laplacian_loss, flame_loss}, unweighted
    int V;
    float c_lap, c_flame; // weight * 2 / V, weight * 2 / (3 V); 0: that term's gradient arithmetic is skipped
    float inv_V, inv_3V;
};

struct Vec3 {
    float x, y, z;
};

__device__ __forceinline__ Vec3 mesh_diff(const float* __restrict__ verts, const float* __restrict__ orig, int k)
{
    const size_t o = (size_t)k * 3;
    return Vec3{verts[o] - orig[o], verts[o + 1] - orig[o + 1], verts[o + 2] - orig[o + 2]};
}

// r_k and 1 / deg(k) (0 for an empty row, which divides by nothing); `d` = d_k
__device__ __forceinline__ Vec3 mesh_row(const float* __restrict__ verts, const float* __restrict__ orig,
                                         const int* __restrict__ row_ptr, const int* __restrict__ col, int k, Vec3 d, float& inv_deg)
{
    const int b = row_ptr[k], e = row_ptr[k + 1];
    float sx = 0.f, sy = 0.f, sz = 0.f;
    for (int p = b; p < e; p++) {
        const Vec3 n = mesh_diff(verts, orig, col[p]);
        sx += n.x, sy += n.y, sz += n.z;
    }
    if (e <= b) {
        inv_deg = 0.f;
        return Vec3{-d.x, -d.y, -d.z};
    }
    inv_deg = 1.0f / (float)(e - b);
    return Vec3{sx * inv_deg - d.x, sy * inv_deg - d.y, sz * inv_deg - d.z};
}

__global__ void __launch_bounds__(kMeshThreads) k_mesh_terms(MeshTermsArgs a)
{
    const float* __restrict__ verts = a.verts;
    const float* __restrict__ orig = a.orig;
    const int* __restrict__ row_ptr = a.row_ptr;
    const int* __restrict__ col = a.col;
    float* const d_verts = a.d_verts;
    const unsigned sub = threadIdx.x & (kMeshGroup - 1);
    const unsigned group = (blockIdx.x * blockDim.x + threadIdx.x) / kMeshGroup, n_groups = gridDim.x * blockDim.x / kMeshGroup;
    const bool lap_grad = d_verts && a.c_lap != 0.f;
    float acc[2] = {0.f, 0.f};   // laplacian, flame
    // (the trip count is the same for every lane of the launch: the shuffles below run with whole waves)
    for (unsigned base = 0; base < (unsigned)a.V; base += n_groups) {
        const unsigned i = base + group;
        float gx = 0.f, gy = 0.f, gz = 0.f;
        Vec3 d = Vec3{0.f, 0.f, 0.f};
        if (i < (unsigned)a.V) {
            const int b = row_ptr[i];
            const unsigned terms = lap_grad ? 1u + (unsigned)(row_ptr[i + 1] - b) : 1u;    // i itself, then its neighbours
            for (unsigned m = sub; m < terms; m += kMeshGroup) {
                if (m == 0) {
                    d = mesh_diff(verts, orig, (int)i);
                    float inv_i;
                    const Vec3 r = mesh_row(verts, orig, row_ptr, col, (int)i, d, inv_i);
                    acc[0] += (r.x * r.x + r.y * r.y) + r.z * r.z;
                    acc[1] += (d.x * d.x + d.y * d.y) + d.z * d.z;
                    gx -= r.x, gy -= r.y, gz -= r.z;
                } else {
                    const int j = col[b + (int)m - 1];
                    float inv_j;
                    const Vec3 rj = mesh_row(verts, orig, row_ptr, col, j, mesh_diff(verts, orig, j), inv_j);
                    gx += rj.x * inv_j, gy += rj.y * inv_j, gz += rj.z * inv_j;
                }
            }
        }
        for (int off = kMeshGroup / 2; off > 0; off >>= 1) {
            gx += __shfl_down(gx, off, kMeshGroup);
            gy += __shfl_down(gy, off, kMeshGroup);
            gz += __shfl_down(gz, off, kMeshGroup);
        }
        if (d_verts && sub == 0 && i < (unsigned)a.V) {
            float ax = 0.f, ay = 0.f, az = 0.f;
            if (lap_grad) ax = a.c_lap * gx, ay = a.c_lap * gy, az = a.c_lap * gz;
            if (a.c_flame != 0.f) ax += a.c_flame * d.x, ay += a.c_flame * d.y, az += a.c_flame * d.z;
            if (ax != 0.f || ay != 0.f || az != 0.f) {   // (a row that gets nothing keeps its bits, a -0 included)
                const size_t o = (size_t)i * 3;
                d_verts[o] += ax, d_verts[o + 1] += ay, d_verts[o + 2] += az;
            }
        }
    }
    if (!sum_over_workgroups(acc, a.partial, kMeshMaxBlocks, a.counter, blockIdx.x, gridDim.x)) return;
    a.loss[0] = acc[0] * a.inv_V;
    a.loss[1] = acc[1] * a.inv_3V;
}

size_t mesh_terms_workspace_bytes() { return done_workspace_bytes(2 * kMeshMaxBlocks); }

int launch_mesh_terms(const fr_mesh_terms_config& cfg, int V, const float* verts, const float* verts_orig, const int* row_ptr,
                      const int* col, float* d_verts, float* loss, void* workspace, hipStream_t s)
{
    if (V <= 0) return FR_OK;
    const unsigned blocks = capped_blocks((unsigned)V, kMeshThreads / kMeshGroup, kMeshMaxBlocks);
    const DoneWorkspace ws = done_workspace(workspace);
    MeshTermsArgs a;
    a.verts = verts, a.orig = verts_orig, a.row_ptr = row_ptr, a.col = col;
    // both weights 0: the gradient array is not touched at all
    a.d_verts = (cfg.laplacian_weight != 0.f || cfg.flame_weight != 0.f) ? d_verts : nullptr;
    a.counter = ws.counter, a.partial = ws.partial;
    a.loss = loss, a.V = V;
    a.c_lap = (float)((double)cfg.laplacian_weight * 2.0 / (double)V);
    a.c_flame = (float)((double)cfg.flame_weight * 2.0 / (3.0 * (double)V));
    a.inv_V = (float)(1.0 / (double)V), a.inv_3V = (float)(1.0 / (3.0 * (double)V));
    hipLaunchKernelGGL(k_mesh_terms, dim3(blocks), dim3(kMeshThreads), 0, s, a);
    FR_HIP(hipGetLastError());
    return FR_OK;
}

}  // namespace fr
