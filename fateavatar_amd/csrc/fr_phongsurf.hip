// SplattingAvatar's CPU submodule simple_phongsurf on gfx950: the walk on the triangle mesh and the Phong-surface fit.
//
// reference (paths relative to submodules/simple_phongsurf/simple_phongsurf/):
//   * the walk — Triwalk::updateSurfacePointsImpl (src/triangle_walk_py.cpp:62-79) around walkSurfacePoint / walkCrossEdge /
//     walkToNeighbor / finalize (src/triangle_walk.cpp:240-386): C++ on the host, one point at a time, behind a device -> host
//     copy and in front of a copy back.  Here k_triwalk: one thread per point, the recursion a loop.
//   * the fit — PhongSurfacePy3d.update_corres_spt (phongsurf_py3d.py:151-185) with method 'uvd': per outer round up to
//     `inner_loop` Adam iterations of an autograd graph (solve_delta_vwd, :256-309; ~40 launches each), then the walk.  Here two
//     launches per round: k_phong_fit_count runs every point's whole trajectory in registers and counts, per iteration, the
//     points whose step was longer than 5e-4 (the loop's one coupling between points, :298-303); k_phong_fit_walk reads the
//     counters, takes the iteration the reference would have stopped at, runs the trajectory again up to it (the same
//     arithmetic: the same bits) and walks by the result.
// No float atomics (integer counters only), no host synchronisation, no copy: capturable, and the same bits on every run.
// A point's barycentrics and shifts are three NAMED scalars rotated with selects: an array indexed by (edge + j) % 3 would
// live in scratch.  Built without FMA contraction (the walk's float32 operations are the host code's, one by one).
#include "fr_common.hpp"

namespace fr {

constexpr int kWalkMaxCrossings = 256;   // decay 0.9: the remaining shift is below 1e-11 of its start by then
constexpr int kFitThreads = 128;
constexpr int kFitMaxInner = 512;

struct B3 {
    float x, y, z;
};

__device__ __forceinline__ float sel3(int e, float a, float b, float c) { return e == 0 ? a : (e == 1 ? b : c); }
// (b[e], b[e + 1], b[e + 2]) — reorderBarycentric (triangle_walk.cpp:131-137)
__device__ __forceinline__ B3 rot3(int e, const B3& b) { return B3{sel3(e, b.x, b.y, b.z), sel3(e, b.y, b.z, b.x), sel3(e, b.z, b.x, b.y)}; }
// out[(e + j) % 3] = p[j]
__device__ __forceinline__ B3 unrot3(int e, const B3& p) { return B3{sel3(e, p.x, p.z, p.y), sel3(e, p.y, p.x, p.z), sel3(e, p.z, p.y, p.x)}; }

// isBaryInside (:21-28)
__device__ __forceinline__ bool bary_inside(const B3& b, float tol)
{
    return b.x >= -tol && b.x <= 1 + tol && b.y >= -tol && b.y <= 1 + tol && b.z >= -tol && b.z <= 1 + tol;
}

// calcLineIntersectBarycentric (:32-86): line p1-p2 with line p3-p4, in double on float inputs; t12 is stored as float.  The
// last test reads t12[0] twice, as the reference does (:72).
__device__ __forceinline__ bool line_intersect(const B3& p1, const B3& p2, const B3& p3, const B3& p4, float& t0, float& t1, B3& hit)
{
    const double eps = 1e-7;   // PARALLEL_EPS
    const double u1 = p1.x, v1 = p1.y, w1 = p1.z, u2 = p2.x, v2 = p2.y, w2 = p2.z;
    const double u3 = p3.x, v3 = p3.y, w3 = p3.z, u4 = p4.x, v4 = p4.y, w4 = p4.z;
    t0 = 0.f, t1 = 0.f;
    if (fabs(u1 - u2) > eps && fabs(u4 - u3) > eps) {
        if (fabs(v1 - v2) > eps && fabs(v4 - v3) > eps) {
            t0 = (float)((u1 * (v4 - v3) + u3 * (v1 - v4) + u4 * (v3 - v1)) / ((u1 - u2) * (v4 - v3) - (u4 - u3) * (v1 - v2)));
            t1 = (float)((u1 * (v2 - v3) + u2 * (v3 - v1) + u3 * (v1 - v2)) / ((u1 - u2) * (v4 - v3) - (u4 - u3) * (v1 - v2)));
        } else if (fabs(w1 - w2) > eps && fabs(w4 - w3) > eps) {
            t0 = (float)((u1 * (w4 - w3) + u3 * (w1 - w4) + u4 * (w3 - w1)) / ((u1 - u2) * (w4 - w3) - (u4 - u3) * (w1 - w2)));
            t1 = (float)((u1 * (w2 - w3) + u2 * (w3 - w1) + u3 * (w1 - w2)) / ((u1 - u2) * (w4 - w3) - (u4 - u3) * (w1 - w2)));
        }
    } else if (fabs(v1 - v2) > eps && fabs(v4 - v3) > eps && fabs(w1 - w2) > eps && fabs(w4 - w3) > eps) {
        t0 = (float)((v1 * (w4 - w3) + v3 * (w1 - w4) + v4 * (w3 - w1)) / ((v1 - v2) * (w4 - w3) - (v4 - v3) * (w1 - w2)));
        t1 = (float)((v1 * (w2 - w3) + v2 * (w3 - w1) + v3 * (w1 - w2)) / ((v1 - v2) * (w4 - w3) - (v4 - v3) * (w1 - w2)));
    }
    if (t0 >= 0 && t0 <= 1.0 && t1 >= 0 && t0 <= 1.0) {
        hit.x = (float)(u1 + (double)t0 * (u2 - u1));
        hit.y = (float)(v1 + (double)t0 * (v2 - v1));
        hit.z = (float)(w1 + (double)t0 * (w2 - w1));
        return true;
    }
    t0 = 0.f, t1 = 0.f;
    hit = p1;
    return false;
}

__device__ __forceinline__ B3 unit3(int j) { return B3{j == 0 ? 1.f : 0.f, j == 1 ? 1.f : 0.f, j == 2 ? 1.f : 0.f}; }

// findCrossingEdge (:93-113)
__device__ __forceinline__ int find_crossing_edge(const B3& p, const B3& q)
{
    int found = -1;
#pragma unroll
    for (int j = 2; j >= 0; j--) {   // (descending, so that the LOWEST crossing edge is what remains)
        float t0, t1;
        B3 hit;
        line_intersect(unit3(j), unit3((j + 1) % 3), p, q, t0, t1, hit);
        if (t0 >= 0.0 && t0 <= 1.0 && (double)t1 > 1e-5 && t1 <= 1.0) found = j;
    }
    return found;
}

// findOnEdgeIndex (:120-129)
__device__ __forceinline__ int find_on_edge(const B3& p)
{
    if ((double)fabsf(p.x) < 1e-5) return 1;
    if ((double)fabsf(p.y) < 1e-5) return 2;
    if ((double)fabsf(p.z) < 1e-5) return 0;
    return -1;
}

// resetBaryToZero (:140-147)
__device__ __forceinline__ void reset_to_zero(B3& b, int idx)
{
    B3 r = rot3(idx, b);
    const float v = r.x;
    r.x = 0.f;
    r.y += v / 2.f;
    r.y = fminf(fmaxf(0.f, r.y), 1.f);
    r.z = 1.f - r.y;
    b = unrot3(idx, r);
}

// resetBaryOnEdge (:150-162)
__device__ __forceinline__ void reset_on_edge(B3& b)
{
    int idx = 0;
    float m = b.x;
    if (fabsf(b.y) < fabsf(m)) m = b.y, idx = 1;
    if (fabsf(b.z) < fabsf(m)) m = b.z, idx = 2;
    reset_to_zero(b, idx);
}

// resetBaryToInside (:165-173).  The reference's `while` does not end for a coordinate that is not finite, or for (1 + e, 0, 0)
// where nothing is negative: two passes, then the point is clamped (`clamped` is set; no input of the tests gets there).
__device__ __forceinline__ void reset_to_inside(B3& b, int& clamped)
{
#pragma unroll
    for (int pass = 0; pass < 2; pass++) {
        if (bary_inside(b, 0.f)) return;
        if (b.x < 0.f) reset_to_zero(b, 0);
        if (b.y < 0.f) reset_to_zero(b, 1);
        if (b.z < 0.f) reset_to_zero(b, 2);
    }
    if (bary_inside(b, 0.f)) return;
    clamped = 1;
    b.x = fminf(fmaxf(b.x, 0.f), 1.f);
    b.y = fminf(fmaxf(b.y, 0.f), 1.f - b.x);
    b.z = 1.f - b.x - b.y;
}

__device__ __forceinline__ bool finite3(float a, float b, float c) { return isfinite(a) && isfinite(b) && isfinite(c); }

// walkSurfacePoint / walkCrossEdge / walkToNeighbor / finalize (:240-386) as one loop: every `continue` is one of the
// reference's recursive calls.  `f`, `b` in-out; `s` the shift.  `nbr[3 f + j]` = 4 g + k of the face and edge behind edge j, or -1.
__device__ __forceinline__ void walk_point(const int* __restrict__ nbr, int F, int& f, B3& b, B3 s, float decay, int& capped, int& clamped)
{
    for (int crossings = 0;; crossings++) {
        const B3 q = {b.x + s.x, b.y + s.y, b.z + s.z};
        if (bary_inside(q, 1e-3f)) {          // the end point is inside this triangle (:280-286)
            b = q;
            reset_to_inside(b, clamped);
            return;
        }
        if (crossings >= kWalkMaxCrossings) {
            capped = 1;
            return;
        }
        if (!bary_inside(b, 1e-3f) && find_on_edge(b) == -1) {   // (:289-299)
            reset_to_inside(b, clamped);
            s = B3{(q.x - b.x) * decay, (q.y - b.y) * decay, (q.z - b.z) * decay};
            continue;
        }
        int e = find_crossing_edge(b, q);      // (:302-313)
        if (e == -1) e = find_on_edge(b);
        if (e == -1) return;
        // walkCrossEdge (:318-367)
        float t0, t1;
        B3 hit;
        if (!line_intersect(unit3(e), unit3(e == 2 ? 0 : e + 1), b, q, t0, t1, hit)) return;   // parallel: stop
        const int n = nbr[3 * f + e];
        if (n < 0 || (n >> 2) >= F) {          // no neighbour: stop on the edge
            b = hit;
            return;
        }
        const B3 remain = {q.x - hit.x, q.y - hit.y, q.z - hit.z};
        const B3 ri = rot3(e, hit), rs = rot3(e, remain);
        // walkToNeighbor (:369-386): AB of this triangle is BA of the neighbour; finalize (:240-260)
        B3 p, pq;
        p.x = ri.y, p.y = ri.x, p.z = 1.0f - p.x - p.y;
        pq.x = p.x + (-rs.x), pq.y = p.y + (-rs.y), pq.z = 1.0f - pq.x - pq.y;
        const B3 sh = {pq.x - p.x, pq.y - p.y, pq.z - p.z};
        f = n >> 2;
        b = unrot3(n & 3, p);
        s = unrot3(n & 3, sh);
        reset_on_edge(b);
        s = B3{s.x * decay, s.y * decay, s.z * decay};
    }
}

// updateSurfacePointsImpl (triangle_walk_py.cpp:62-79) for one point: (u, v) and the shift come as doubles made from floats,
// the third coordinates are formed in double and rounded.  Writes face, (u, v) and 1 - u - v (splattingavatar.py:677).
__device__ __forceinline__ void walk_and_store(const int* __restrict__ nbr, int F, int i, int f, float u, float v, float du, float dv,
                                               float decay, int* face_index, float* bary, int* status)
{
    B3 b = {u, v, (float)(1.0 - (double)u - (double)v)};
    const B3 s = {du, dv, (float)(0.0 - (double)du - (double)dv)};
    int capped = 0, clamped = 0;
    walk_point(nbr, F, f, b, s, decay, capped, clamped);
    if (capped) atomicAdd(status + 0, 1);
    if (clamped) atomicAdd(status + 1, 1);
    face_index[i] = f;
    bary[3 * i] = b.x, bary[3 * i + 1] = b.y, bary[3 * i + 2] = 1.0f - b.x - b.y;
}

__global__ void __launch_bounds__(kFitThreads) k_triwalk(const int* __restrict__ nbr, int F, int n, int* face_index, float* bary,
                                                         const float* __restrict__ delta, int delta_stride, float decay, int* status)
{
    const int i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= n) return;
    const int f = face_index[i];
    const float u = bary[3 * i], v = bary[3 * i + 1];
    const float du = delta[(size_t)i * delta_stride], dv = delta[(size_t)i * delta_stride + 1];
    if (f < 0 || f >= F || !finite3(u, v, bary[3 * i + 2]) || !finite3(du, dv, 0.f)) {   // left exactly as it was
        atomicAdd(status + 2, 1);
        return;
    }
    walk_and_store(nbr, F, i, f, u, v, du, dv, decay, face_index, bary, status);
}

// ---------------------------------------------------------------- the fit
struct V3 {
    float x, y, z;
};
__device__ __forceinline__ V3 ld3(const float* __restrict__ p, int i) { return V3{p[3 * i], p[3 * i + 1], p[3 * i + 2]}; }
__device__ __forceinline__ float dot3(const V3& a, const V3& b) { return a.x * b.x + a.y * b.y + a.z * b.z; }

struct FitPoint {   // 18 floats of mesh data, the query, the start
    V3 v0, v1, v2, n0, n1, n2, q;
    float u, v;
};

struct FitState {   // delta and its Adam moments
    float d[3], m[3], s[3];
    double b1p, b2p;   // beta^t
};

__device__ __forceinline__ V3 interp(const V3& a, const V3& b, const V3& c, float u, float v, float w)
{
    return V3{a.x * u + b.x * v + c.x * w, a.y * u + b.y * v + c.y * w, a.z * u + b.z * v + c.z * w};
}

// delta = (0, 0, |V(uv) - q|) (phongsurf_py3d.py:259-262), zero moments
__device__ __forceinline__ void fit_init(const FitPoint& p, FitState& st)
{
    const V3 c = interp(p.v0, p.v1, p.v2, p.u, p.v, 1.0f - p.u - p.v);
    const V3 r = {c.x - p.q.x, c.y - p.q.y, c.z - p.q.z};
#pragma unroll
    for (int k = 0; k < 3; k++) st.d[k] = st.m[k] = st.s[k] = 0.f;
    st.d[2] = sqrtf(dot3(r, r));
    st.b1p = st.b2p = 1.0;
}

// One iteration of :276-303: the gradient of mean((10 V(uv + d_uv) + 10 n_hat(uv + d_uv) d_d - 10 q)^2) over all 3 n numbers,
// autograd's chain by hand, then torch.optim.Adam's update (lr 0.01, betas 0.9 / 0.999, eps 1e-8; bias corrections in double on
// the step count, as torch forms them on the host).  Returns |delta - delta_prev| > 5e-4.
__device__ __forceinline__ bool fit_iterate(const FitPoint& p, FitState& st, float two_over_3n)
{
    const float u = p.u + st.d[0], v = p.v + st.d[1], w = 1.0f - u - v, dd = st.d[2];
    const V3 cv = interp(p.v0, p.v1, p.v2, u, v, w), nr = interp(p.n0, p.n1, p.n2, u, v, w);
    const float len = fmaxf(sqrtf(dot3(nr, nr)), 1e-12f);
    const V3 nh = {nr.x / len, nr.y / len, nr.z / len};
    // match = 10 V + (10 n_hat) d ; gm = d loss / d match = 2 (match - target) / (3 n)
    const V3 n10 = {nh.x * 10.f, nh.y * 10.f, nh.z * 10.f};
    const V3 gm = {((cv.x * 10.f + n10.x * dd) - p.q.x * 10.f) * two_over_3n, ((cv.y * 10.f + n10.y * dd) - p.q.y * 10.f) * two_over_3n,
                   ((cv.z * 10.f + n10.z * dd) - p.q.z * 10.f) * two_over_3n};
    const float g_d = dot3(gm, n10);
    // through 10 n_hat d -> n_hat = N / max(|N|, eps) -> N = sum bary_k N_k ; through 10 V -> V = sum bary_k V_k
    const V3 gh = {gm.x * dd * 10.f, gm.y * dd * 10.f, gm.z * dd * 10.f};
    const float along = dot3(nh, gh);
    const V3 gn = {(gh.x - nh.x * along) / len, (gh.y - nh.y * along) / len, (gh.z - nh.z * along) / len};
    const V3 gv = {gm.x * 10.f, gm.y * 10.f, gm.z * 10.f};
    const float gb0 = dot3(p.v0, gv) + dot3(p.n0, gn), gb1 = dot3(p.v1, gv) + dot3(p.n1, gn), gb2 = dot3(p.v2, gv) + dot3(p.n2, gn);
    const float g[3] = {gb0 - gb2, gb1 - gb2, g_d};
    st.b1p *= 0.9, st.b2p *= 0.999;
    const float step_size = (float)(0.01 / (1.0 - st.b1p)), bc2_sqrt = (float)sqrt(1.0 - st.b2p);
    float c2 = 0.f;
#pragma unroll
    for (int k = 0; k < 3; k++) {
        st.m[k] = st.m[k] + 0.1f * (g[k] - st.m[k]);                       // exp_avg.lerp_(grad, 1 - beta1)
        st.s[k] = st.s[k] * 0.999f + (0.001f * g[k]) * g[k];               // exp_avg_sq.mul_(beta2).addcmul_(grad, grad, value=1 - beta2)
        const float denom = sqrtf(st.s[k]) / bc2_sqrt + 1e-8f;
        const float nd = st.d[k] + (-step_size * st.m[k]) / denom;        // param.addcdiv_(exp_avg, denom, value=-step_size)
        const float ch = nd - st.d[k];
        c2 += ch * ch;
        st.d[k] = nd;
    }
    return sqrtf(c2) > 5e-4f;
}

struct FitArgs {
    const float* verts;      // [V,3] canonical
    const float* normals;    // [V,3]
    const int* faces;        // [F,3]
    const int* nbr;          // [F,3]
    int V, F, n;
    const float* query;      // [n,3]
    int* face_index;         // [n]   in-out
    float* bary;             // [n,3] in-out
    int inner;
    float decay, two_over_3n;
    int* counters;           // [inner] of this round
    int* status;             // [4]
    float* delta_out;        // [n,3] or null
};

// false: the point is left as it is (face out of range, a vertex index out of range, or something not finite)
__device__ __forceinline__ bool fit_load(const FitArgs& a, int i, int& f, FitPoint& p)
{
    f = a.face_index[i];
    if (f < 0 || f >= a.F) return false;
    const int i0 = a.faces[3 * f], i1 = a.faces[3 * f + 1], i2 = a.faces[3 * f + 2];
    if (i0 < 0 || i0 >= a.V || i1 < 0 || i1 >= a.V || i2 < 0 || i2 >= a.V) return false;
    p.v0 = ld3(a.verts, i0), p.v1 = ld3(a.verts, i1), p.v2 = ld3(a.verts, i2);
    p.n0 = ld3(a.normals, i0), p.n1 = ld3(a.normals, i1), p.n2 = ld3(a.normals, i2);
    p.q = ld3(a.query, i);
    p.u = a.bary[3 * i], p.v = a.bary[3 * i + 1];
    return finite3(p.u, p.v, a.bary[3 * i + 2]) && finite3(p.q.x, p.q.y, p.q.z);
}

// pass A: every point's whole trajectory; counters[it] += number of points with change > 5e-4 in iteration it (a ballot per
// wave, an LDS counter per workgroup, one integer atomic per workgroup and iteration)
__global__ void __launch_bounds__(kFitThreads) k_phong_fit_count(FitArgs a)
{
    __shared__ int s_cnt[kFitMaxInner];
    for (int k = threadIdx.x; k < a.inner; k += blockDim.x) s_cnt[k] = 0;
    __syncthreads();
    const int i = blockIdx.x * blockDim.x + threadIdx.x;
    int f;
    FitPoint p;
    const bool live = i < a.n && fit_load(a, i, f, p);
    FitState st;
    if (live) fit_init(p, st);
    for (int it = 0; it < a.inner; it++) {
        const bool moved = live && fit_iterate(p, st, a.two_over_3n);
        const unsigned long long mask = __ballot(moved);
        if ((threadIdx.x & (kWave - 1)) == 0 && mask) atomicAdd(&s_cnt[it], __popcll(mask));
    }
    __syncthreads();
    for (int k = threadIdx.x; k < a.inner; k += blockDim.x)
        if (s_cnt[k]) atomicAdd(a.counters + k, s_cnt[k]);
}

// pass B: the iteration the loop ends after (the first whose counter is 0, :302-303), the trajectory again up to it, the walk
__global__ void __launch_bounds__(kFitThreads) k_phong_fit_walk(FitArgs a)
{
    __shared__ int s_stop;
    if (threadIdx.x == 0) s_stop = a.inner - 1;
    __syncthreads();
    for (int k = threadIdx.x; k < a.inner; k += blockDim.x)
        if (a.counters[k] == 0) atomicMin(&s_stop, k);
    __syncthreads();
    const int stop = s_stop;
    const int i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i == 0) a.status[3] = stop + 1;
    if (i >= a.n) return;
    int f;
    FitPoint p;
    if (!fit_load(a, i, f, p)) {
        atomicAdd(a.status + 2, 1);
        return;
    }
    FitState st;
    fit_init(p, st);
    for (int it = 0; it <= stop; it++) fit_iterate(p, st, a.two_over_3n);
    if (a.delta_out) a.delta_out[3 * i] = st.d[0], a.delta_out[3 * i + 1] = st.d[1], a.delta_out[3 * i + 2] = st.d[2];
    if (!finite3(st.d[0], st.d[1], 0.f)) {
        atomicAdd(a.status + 2, 1);
        return;
    }
    walk_and_store(a.nbr, a.F, i, f, p.u, p.v, st.d[0], st.d[1], a.decay, a.face_index, a.bary, a.status);
}

__global__ void __launch_bounds__(256) k_zero_words(int* p, int n)
{
    for (int i = blockIdx.x * blockDim.x + threadIdx.x; i < n; i += gridDim.x * blockDim.x) p[i] = 0;
}

int launch_triwalk(const int* nbr, int F, int n, int* face_index, float* bary, const float* delta, int delta_stride, float decay,
                   int* status, hipStream_t s)
{
    if (n <= 0) return FR_OK;
    hipLaunchKernelGGL(k_triwalk, dim3((n + kFitThreads - 1) / kFitThreads), dim3(kFitThreads), 0, s, nbr, F, n, face_index, bary, delta,
                       delta_stride, decay, status);
    FR_HIP(hipGetLastError());
    return FR_OK;
}

int launch_phong_fit(const float* verts, const float* normals, const int* faces, const int* nbr, int V, int F, int n, const float* query,
                     int* face_index, float* bary, int outer_loop, int inner_loop, float decay, int* work, int* status, float* delta_out,
                     hipStream_t s)
{
    if (n <= 0) return FR_OK;
    // (a kernel, not hipMemsetAsync: fr_common.hpp, launch_zero, on memset nodes of captured graphs)
    hipLaunchKernelGGL(k_zero_words, dim3(8), dim3(256), 0, s, work, outer_loop * inner_loop + 4);
    FitArgs a = {verts, normals, faces, nbr, V, F, n, query, face_index, bary, inner_loop, decay, (float)(2.0 / (3.0 * (double)n)),
                 work, status, delta_out};
    const dim3 grid((n + kFitThreads - 1) / kFitThreads), block(kFitThreads);
    for (int r = 0; r < outer_loop; r++) {
        a.counters = work + (size_t)r * inner_loop;
        hipLaunchKernelGGL(k_phong_fit_count, grid, block, 0, s, a);
        hipLaunchKernelGGL(k_phong_fit_walk, grid, block, 0, s, a);
    }
    FR_HIP(hipGetLastError());
    return FR_OK;
}

}  // namespace fr
