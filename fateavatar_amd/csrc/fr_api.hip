// extern "C" entry points declared in include/fr_rasterizer.h.  Argument checking, handle
// lifetime, error strings; the work is in fr_preprocess.hip / fr_tile_sort.hip / fr_blend_fwd.hip /
// fr_blend_bwd.hip / fr_preprocess_bwd.hip / fr_knn.hip.
#include "fr_common.hpp"
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <new>

namespace fr {

thread_local char g_err[512] = "";

int fail_hip(hipError_t e, const char* what, const char* file, int line)
{
    snprintf(g_err, sizeof(g_err), "HIP error %d (%s) at %s:%d in `%s`", (int)e, hipGetErrorString(e), file, line, what);
    return FR_ERR_HIP;
}
int fail_msg(int code, const char* msg)
{
    snprintf(g_err, sizeof(g_err), "%s", msg);
    return code;
}

// (also what a frame rendered from its binding is checked with, before anything is enqueued)
static int check_binding(const fr_binding* b)
{
    if (!b || b->N < 0 || b->V < 0 || b->F < 0) return fail_msg(FR_ERR_INVALID_ARGUMENT, "fr_binding: null or negative sizes");
    if (b->mode != FR_BIND_SHELL && b->mode != FR_BIND_FACE_LOCAL && b->mode != FR_BIND_PHONG && b->mode != FR_BIND_DEFORM)
        return fail_msg(FR_ERR_INVALID_ARGUMENT,
                        "fr_binding: unknown mode (FR_BIND_SHELL, FR_BIND_FACE_LOCAL, FR_BIND_PHONG or FR_BIND_DEFORM)");
    if (b->N == 0) return FR_OK;
    if (b->mode == FR_BIND_DEFORM && (!b->face_index || !b->bary || !b->local_xyz || !b->rotation || !b->scaling))
        return fail_msg(FR_ERR_INVALID_ARGUMENT,
                        "fr_binding: FR_BIND_DEFORM needs face_index, bary, deform [N,10] (in local_xyz), rotation and scaling");
    if (!b->verts || !b->faces || !b->face_index || !b->rotation || !b->scaling)
        return fail_msg(FR_ERR_INVALID_ARGUMENT, "fr_binding: missing array");
    if (b->mode == FR_BIND_FACE_LOCAL) {
        if (!b->local_xyz) return fail_msg(FR_ERR_INVALID_ARGUMENT, "fr_binding: FR_BIND_FACE_LOCAL needs local_xyz");
    } else if (b->mode == FR_BIND_PHONG) {
        const fr_binding_phong* p = reinterpret_cast<const fr_binding_phong*>(b);   // (this mode's descriptor: its `base` is *b)
        if (!b->bary || !p->vert_normals || !p->vert_quats || !p->face_ratio || !b->local_xyz)
            return fail_msg(FR_ERR_INVALID_ARGUMENT,
                            "fr_binding: FR_BIND_PHONG needs bary, vert_normals, vert_quats, face_ratio and uvd (in local_xyz)");
    } else if (b->mode == FR_BIND_DEFORM) {
        // (its own arrays were checked above; offset, face_scale_canonical, shell_len and resize_scale are not read)
    } else if (!b->bary || !b->offset || (b->resize_scale && !b->face_scale_canonical))
        return fail_msg(FR_ERR_INVALID_ARGUMENT, "fr_binding: missing array");
    return FR_OK;
}

static int check_frame(const fr_params* prm, const fr_inputs* in, bool forward)
{
    if (!prm || !in) return fail_msg(FR_ERR_INVALID_ARGUMENT, "null params/inputs");
    if (prm->P < 0 || prm->W <= 0 || prm->H <= 0) return fail_msg(FR_ERR_INVALID_ARGUMENT, "bad P/W/H");
    if (prm->W > 8 * 65535 || prm->H > 8 * 65535) return fail_msg(FR_ERR_UNSUPPORTED, "image larger than 65535 tiles per axis");
    if (prm->D < 0 || prm->D > 3) return fail_msg(FR_ERR_INVALID_ARGUMENT, "SH degree must be 0..3");
    if (prm->P == 0) return FR_OK;
    // opacities are only read by the forward (the backward takes them from the geometry state)
    if (!in->means3D || (forward && !in->opacities) || !in->viewmatrix || !in->projmatrix || !in->campos || !in->background)
        return fail_msg(FR_ERR_INVALID_ARGUMENT, "missing required input pointer");
    // exactly one of shs / colors_precomp, exactly one of (scales+rotations) / cov3D_precomp
    // (the reference enforces this in Python: diff_gaussian_rasterization/__init__.py:191-195)
    if ((in->shs == nullptr) == (in->colors_precomp == nullptr))
        return fail_msg(FR_ERR_INVALID_ARGUMENT, "provide exactly one of shs / colors_precomp");
    const bool sr = in->scales && in->rotations;
    if ((in->scales == nullptr) != (in->rotations == nullptr) || (sr == (in->cov3D_precomp != nullptr)))
        return fail_msg(FR_ERR_INVALID_ARGUMENT, "provide exactly one of scales+rotations / cov3D_precomp");
    if ((prm->flags & FR_FLAG_RAW_ACTIVATIONS) && !sr)
        return fail_msg(FR_ERR_INVALID_ARGUMENT, "FR_FLAG_RAW_ACTIVATIONS needs scales + rotations");
    if (in->shs && prm->M < (prm->D + 1) * (prm->D + 1))
        return fail_msg(FR_ERR_INVALID_ARGUMENT, "M smaller than (D+1)^2");
    if (prm->aux && prm->aux->binding) {
        const fr_binding& b = *prm->aux->binding;
        if (!(prm->flags & FR_FLAG_RAW_ACTIVATIONS) || !sr)
            return fail_msg(FR_ERR_INVALID_ARGUMENT, "fr_aux::binding needs FR_FLAG_RAW_ACTIVATIONS and scales + rotations");
        if (b.N != prm->P) return fail_msg(FR_ERR_INVALID_ARGUMENT, "fr_aux::binding: N must equal P");
        const int rc = check_binding(&b);
        if (rc) return rc;
        if (!forward && b.mode == FR_BIND_PHONG && prm->aux->d_verts)
            return fail_msg(FR_ERR_INVALID_ARGUMENT, "fr_aux::d_verts: a FR_BIND_PHONG binding has no vertex gradient");
    }
    return FR_OK;
}

__global__ void __launch_bounds__(256) k_zero16(uint4* p, size_t n16)
{
    const size_t stride = (size_t)gridDim.x * blockDim.x;
    for (size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x; i < n16; i += stride) p[i] = make_uint4(0u, 0u, 0u, 0u);
}

int launch_zero(void* ptr, size_t bytes, hipStream_t s)
{
    const size_t n16 = (bytes + 15) / 16;
    if (n16 == 0) return FR_OK;
    size_t blocks = (n16 + 255) / 256;
    if (blocks > 2048) blocks = 2048;
    hipLaunchKernelGGL(k_zero16, dim3((unsigned)blocks), dim3(256), 0, s, static_cast<uint4*>(ptr), n16);
    FR_HIP(hipGetLastError());
    return FR_OK;
}

bool note_capture(fr_handle_impl* h, hipStream_t s)
{
    hipStreamCaptureStatus st = hipStreamCaptureStatusNone;
    (void)hipStreamIsCapturing(s, &st);
    if (st != hipStreamCaptureStatusNone) h->captured = true;
    return st != hipStreamCaptureStatusNone;
}

int release_buffer(fr_handle_impl* h, void* p, hipStream_t s)
{
    if (!p) return FR_OK;
    if (h->captured) {   // a captured graph may replay on it: kept until fr_destroy
        h->retired.push_back(p);
        return FR_OK;
    }
    // (frames in flight still hold the old pointer in kernels already enqueued on this stream: free behind them)
    FR_HIP(hipStreamSynchronize(s));
    FR_HIP(hipFree(p));
    return FR_OK;
}

int ensure_accum(fr_handle_impl* h, size_t P, hipStream_t s)
{
    if (P <= h->accum_rows) return FR_OK;
    {
        int rc = release_buffer(h, h->accum, s);
        if (rc) return rc;
    }
    h->accum = nullptr, h->accum_rows = 0;
    const size_t rows = P + P / 4 + 1024;
    FR_HIP(hipMalloc(reinterpret_cast<void**>(&h->accum), rows * kAccumStride * sizeof(float)));
    h->accum_rows = rows;
    return launch_zero(h->accum, rows * kAccumStride * sizeof(float), s);
}

}  // namespace fr

using namespace fr;

extern "C" {

const char* fr_last_error(void) { return g_err; }
const char* fr_version(void) { return "fateavatar_amd rasterizer 0.1 (gfx950, wave64, 8x8 tiles)"; }

int fr_create(fr_handle** out)
{
    if (!out) return fail_msg(FR_ERR_INVALID_ARGUMENT, "null out");
    fr_handle_impl* h = new (std::nothrow) fr_handle_impl();
    if (!h) return fail_msg(FR_ERR_HIP, "out of host memory");
    FR_HIP(hipGetDevice(&h->device));
    FR_HIP(hipHostMalloc(reinterpret_cast<void**>(&h->host_counts), 64, hipHostMallocMapped));
    memset(h->host_counts, 0, 64);
    FR_HIP(hipHostGetDevicePointer(reinterpret_cast<void**>(&h->host_counts_dev), h->host_counts, 0));
    FR_HIP(hipEventCreateWithFlags(&h->counts_ready, hipEventDisableTiming));
    FR_HIP(hipEventCreateWithFlags(&h->frame_done, hipEventDisableTiming));
    FR_HIP(hipEventCreateWithFlags(&h->bwd_done, hipEventDisableTiming));
    FR_HIP(hipStreamCreateWithFlags(&h->side_stream, hipStreamNonBlocking));
    FR_HIP(hipEventCreateWithFlags(&h->side_fork, hipEventDisableTiming));
    FR_HIP(hipEventCreateWithFlags(&h->side_join, hipEventDisableTiming));
    const char* bf = getenv("FR_BLEND_FWD");
    h->gather_in_chain = !(bf && strcmp(bf, "gather") == 0);
    const char* pf = getenv("FR_DENSE_PAIRS_FWD");
    const char* pb = getenv("FR_DENSE_PAIRS_BWD");
    h->dense_pairs_fwd = pf ? (uint32_t)strtoul(pf, nullptr, 10) : kDensePairsFwd;
    h->dense_pairs_bwd = pb ? (uint32_t)strtoul(pb, nullptr, 10) : kDensePairsBwd;
    if (const char* hp = getenv("FR_HEAVY_PAIRS")) h->heavy_pairs = (uint32_t)strtoul(hp, nullptr, 10);
    if (const char* cs = getenv("FR_CHAIN_SPINS")) h->chain_spins = (uint32_t)strtoul(cs, nullptr, 10);
    const char* ph = getenv("FR_DEBUG_PAIR_HIST");
    h->debug_pair_hist = ph && ph[0] == '1';
    *out = reinterpret_cast<fr_handle*>(h);
    return FR_OK;
}

int fr_destroy(fr_handle* hh)
{
    fr_handle_impl* h = reinterpret_cast<fr_handle_impl*>(hh);
    if (!h) return FR_OK;
    (void)hipEventDestroy(h->counts_ready);
    if (h->frame_done) (void)hipEventDestroy(h->frame_done);
    if (h->bwd_done) (void)hipEventDestroy(h->bwd_done);
    if (h->side_fork) (void)hipEventDestroy(h->side_fork);
    if (h->side_join) (void)hipEventDestroy(h->side_join);
    if (h->side_stream) (void)hipStreamDestroy(h->side_stream);
    for (int st = 0; st < ST_COUNT; st++)
        for (size_t i = 0; i < h->ev[st].start.size(); i++) {
            (void)hipEventDestroy(h->ev[st].start[i]);
            (void)hipEventDestroy(h->ev[st].stop[i]);
        }
    (void)hipHostFree(h->host_counts);
    if (h->tile_counters) (void)hipFree(h->tile_counters);
    if (h->accum) (void)hipFree(h->accum);
    if (h->key_buckets) (void)hipFree(h->key_buckets);
    for (void* p : h->retired) (void)hipFree(p);
    delete h;
    return FR_OK;
}

int fr_profile_enable(fr_handle* hh, int32_t on)
{
    fr_handle_impl* h = reinterpret_cast<fr_handle_impl*>(hh);
    if (!h) return fail_msg(FR_ERR_INVALID_ARGUMENT, "null handle");
    h->profiling = on != 0;
    for (int st = 0; st < ST_COUNT; st++) h->ev[st].used = 0;
    return FR_OK;
}

int fr_profile_read(fr_handle* hh, int32_t stage, double* total_ms, uint32_t* launches)
{
    fr_handle_impl* h = reinterpret_cast<fr_handle_impl*>(hh);
    if (!h || stage < 0 || stage >= ST_COUNT || !total_ms || !launches) return fail_msg(FR_ERR_INVALID_ARGUMENT, "bad argument");
    StageEvents& e = h->ev[stage];
    double tot = 0;
    for (size_t i = 0; i < e.used; i++) {
        float ms = 0;
        FR_HIP(hipEventElapsedTime(&ms, e.start[i], e.stop[i]));
        tot += ms;
    }
    *total_ms = tot;
    *launches = (uint32_t)e.used;
    return FR_OK;
}

size_t fr_geometry_bytes(int32_t P) { return GeomView::bytes((size_t)(P > 0 ? P : 0)); }
size_t fr_image_bytes(int32_t W, int32_t H) { return ImageView::bytes(W, H); }
size_t fr_binning_bytes(uint64_t capacity, int32_t W, int32_t H)
{
    ImageView v = ImageView::make(nullptr, W, H);
    return BinningView::bytes((size_t)capacity, (size_t)v.tiles_x * v.tiles_y);
}

size_t fr_camera_grad_workspace_bytes(void) { return camera_grad_workspace_bytes(); }

size_t fr_planes_bytes(uint64_t capacity, int32_t W, int32_t H)
{
    ImageView v = ImageView::make(nullptr, W, H);
    return PlaneView::bytes((size_t)capacity, (size_t)v.tiles_x * v.tiles_y);
}

int fr_forward(fr_handle* hh, const fr_params* prm, const fr_inputs* in, float* out_color, int32_t* radii,
               void* geometry, void* image, void* binning, uint64_t binning_capacity, fr_counts* counts, void* stream)
{
    // (a batch of one: the same checks, codes and messages; a single view may have P == 0)
    return fr_forward_batch(1, &hh, &prm, &in, &out_color, &radii, &geometry, &image, &binning, &binning_capacity, counts,
                            stream);
}

int fr_forward_batch(int32_t n_views, fr_handle* const* handles, const fr_params* const* prm, const fr_inputs* const* in,
                     float* const* out_color, int32_t* const* radii, void* const* geometry, void* const* image,
                     void* const* binning, const uint64_t* binning_capacity, fr_counts* counts, void* stream)
{
    if (n_views < 1 || n_views > kMaxBatch) return fail_msg(FR_ERR_INVALID_ARGUMENT, "n_views must be 1 .. FR_MAX_BATCH");
    if (!handles || !prm || !in || !out_color || !radii || !geometry || !image || !binning || !binning_capacity)
        return fail_msg(FR_ERR_INVALID_ARGUMENT, "null argument array");
    ForwardCall c[kMaxBatch];
    for (int k = 0; k < n_views; k++) {
        fr_handle_impl* h = reinterpret_cast<fr_handle_impl*>(handles[k]);
        if (!h) return fail_msg(FR_ERR_INVALID_ARGUMENT, "null handle");
        for (int j = 0; j < k; j++)
            if (handles[j] == handles[k]) return fail_msg(FR_ERR_INVALID_ARGUMENT, "the views of a batch need a handle each");
        int rc = check_frame(prm[k], in[k], true);
        if (rc) return rc;
        if (n_views > 1 && prm[k]->P <= 0) return fail_msg(FR_ERR_INVALID_ARGUMENT, "batched views need P > 0");
        if (!out_color[k] || !image[k] || (prm[k]->P > 0 && (!radii[k] || !geometry[k])) || (binning_capacity[k] > 0 && !binning[k]))
            return fail_msg(FR_ERR_INVALID_ARGUMENT, "null output / scratch pointer");
        if (binning_capacity[k] >= (1ull << 32)) return fail_msg(FR_ERR_UNSUPPORTED, "binning capacity must be < 2^32 instances");
        if ((prm[k]->flags ^ prm[0]->flags) & FR_FLAG_FORWARD_ONLY)
            return fail_msg(FR_ERR_INVALID_ARGUMENT, "the views of a batch must agree on FR_FLAG_FORWARD_ONLY");
        if ((prm[k]->flags ^ prm[0]->flags) & FR_FLAG_DEPTH_ALPHA)
            return fail_msg(FR_ERR_INVALID_ARGUMENT, "the views of a batch must agree on FR_FLAG_DEPTH_ALPHA");
        if ((prm[k]->flags & FR_FLAG_DEPTH_ALPHA) && (!prm[k]->aux || !prm[k]->aux->out_depth || !prm[k]->aux->out_alpha || !prm[k]->aux->planes))
            return fail_msg(FR_ERR_INVALID_ARGUMENT, "FR_FLAG_DEPTH_ALPHA needs fr_aux::out_depth, out_alpha and planes");
        c[k] = ForwardCall{h, prm[k], in[k], out_color[k], radii[k], geometry[k], image[k], binning[k], binning_capacity[k],
                           counts ? counts + k : nullptr};
    }
    for (int k = 0; k < n_views; k++) {   // (what fr_backward checks its buffers against)
        c[k].h->last_fwd_flags = prm[k]->flags;
        c[k].h->last_fwd_geometry = geometry[k], c[k].h->last_fwd_binning = binning[k];
    }
    return launch_forward(n_views, c, static_cast<hipStream_t>(stream));
}

int fr_read_counts(fr_handle* hh, fr_counts* counts)
{
    fr_handle_impl* h = reinterpret_cast<fr_handle_impl*>(hh);
    if (!h || !counts) return fail_msg(FR_ERR_INVALID_ARGUMENT, "null argument");
    *counts = *h->host_counts;
    // (valid once the frame's stream has been synchronised: the caller's responsibility.)  A handle driven only with
    // FR_FLAG_NO_WAIT learns here that the pinned slot holds a completed frame's counts: the next eager frame sizes the
    // key buckets from them (word 4) and decides about the big-list sorter.
    h->counts_seen = true;
    return FR_OK;
}

// One view of a backward.  P == 0 passes (fr_backward has nothing to do) unless the view is part of a batch.
static int check_backward(const BackwardCall& c, bool batched)
{
    if (!c.h) return fail_msg(FR_ERR_INVALID_ARGUMENT, "null handle");
    int rc = check_frame(c.prm, c.in, false);
    if (rc) return rc;
    if (c.prm->P == 0) return batched ? fail_msg(FR_ERR_INVALID_ARGUMENT, "batched views need P > 0") : FR_OK;
    if (!c.radii || !c.geometry || !c.image || !c.binning || !c.dL_dpix || !c.grads)
        return fail_msg(FR_ERR_INVALID_ARGUMENT, "null pointer");
    if ((c.h->last_fwd_flags & FR_FLAG_FORWARD_ONLY) && (c.geometry == c.h->last_fwd_geometry || c.binning == c.h->last_fwd_binning))
        return fail_msg(FR_ERR_INVALID_ARGUMENT,
                        "these buffers come from a forward-only frame (FR_FLAG_FORWARD_ONLY), which leaves no backward hand-off: "
                        "render the frame without the flag to differentiate it");
    const fr_aux* aux = c.prm->aux;
    if (aux && (aux->dL_ddepth || aux->dL_dalpha)) {
        if (!(c.prm->flags & FR_FLAG_DEPTH_ALPHA))
            return fail_msg(FR_ERR_INVALID_ARGUMENT, "a depth or alpha gradient needs FR_FLAG_DEPTH_ALPHA");
        if (!(c.h->last_fwd_flags & FR_FLAG_DEPTH_ALPHA) && (c.geometry == c.h->last_fwd_geometry || c.binning == c.h->last_fwd_binning))
            return fail_msg(FR_ERR_INVALID_ARGUMENT,
                            "a depth or alpha gradient for a frame rendered without FR_FLAG_DEPTH_ALPHA: it has no planes to differentiate");
        if (!aux->planes) return fail_msg(FR_ERR_INVALID_ARGUMENT, "FR_FLAG_DEPTH_ALPHA with a plane gradient needs fr_aux::planes");
    }
    if (c.prm->flags & FR_FLAG_CAMERA_GRAD) {
        const fr_aux_camera* cam = reinterpret_cast<const fr_aux_camera*>(aux);   // (under the flag, aux is an fr_aux_camera's base)
        if (!cam || (!cam->d_viewmatrix && !cam->d_projmatrix && !cam->d_campos))
            return fail_msg(FR_ERR_INVALID_ARGUMENT, "FR_FLAG_CAMERA_GRAD needs one of fr_aux_camera::d_viewmatrix, d_projmatrix, d_campos");
        if (!cam->camera_workspace) return fail_msg(FR_ERR_INVALID_ARGUMENT, "FR_FLAG_CAMERA_GRAD needs fr_aux_camera::camera_workspace");
    }
    return FR_OK;
}

int fr_backward(fr_handle* hh, const fr_params* prm, const fr_inputs* in, const int32_t* radii, void* geometry,
                const void* image, const void* binning, const float* dL_dpix, const fr_grads* grads, void* stream)
{
    const BackwardCall c = {reinterpret_cast<fr_handle_impl*>(hh), prm, in, radii, geometry, image, binning, dL_dpix, grads};
    int rc = check_backward(c, false);
    if (rc || prm->P == 0) return rc;
    return launch_backward(1, &c, static_cast<hipStream_t>(stream));
}

int fr_backward_batch(int32_t n_views, fr_handle* const* handles, const fr_params* const* prm, const fr_inputs* const* in,
                      const int32_t* const* radii, void* const* geometry, const void* const* image, const void* const* binning,
                      const float* const* dL_dpix, const fr_grads* const* grads, void* stream)
{
    if (n_views < 1 || n_views > kMaxBatch) return fail_msg(FR_ERR_INVALID_ARGUMENT, "n_views must be 1 .. FR_MAX_BATCH");
    if (!handles || !prm || !in || !radii || !geometry || !image || !binning || !dL_dpix || !grads)
        return fail_msg(FR_ERR_INVALID_ARGUMENT, "null argument array");
    BackwardCall c[kMaxBatch];
    for (int k = 0; k < n_views; k++) {
        for (int j = 0; j < k; j++)   // (never two null handles: the first has failed check_backward)
            if (handles[j] == handles[k]) return fail_msg(FR_ERR_INVALID_ARGUMENT, "the views of a batch need a handle each");
        c[k] = BackwardCall{reinterpret_cast<fr_handle_impl*>(handles[k]), prm[k], in[k], radii[k], geometry[k], image[k],
                            binning[k], dL_dpix[k], grads[k]};
        int rc = check_backward(c[k], true);
        if (rc) return rc;
        if ((prm[k]->flags ^ prm[0]->flags) & FR_FLAG_DEPTH_ALPHA)
            return fail_msg(FR_ERR_INVALID_ARGUMENT, "the views of a batch must agree on FR_FLAG_DEPTH_ALPHA");
        if ((prm[k]->flags ^ prm[0]->flags) & FR_FLAG_CAMERA_GRAD)
            return fail_msg(FR_ERR_INVALID_ARGUMENT, "the views of a batch must agree on FR_FLAG_CAMERA_GRAD");
        for (int j = 0; j < k; j++)
            if ((prm[k]->flags & FR_FLAG_CAMERA_GRAD) && reinterpret_cast<const fr_aux_camera*>(prm[j]->aux)->camera_workspace ==
                                                             reinterpret_cast<const fr_aux_camera*>(prm[k]->aux)->camera_workspace)
                return fail_msg(FR_ERR_INVALID_ARGUMENT, "the views of a batch need a camera_workspace each");
    }
    return launch_backward(n_views, c, static_cast<hipStream_t>(stream));
}

int fr_mark_visible(int32_t P, const float* means3D, const float* viewmatrix, const float* projmatrix, uint8_t* present,
                    void* stream)
{
    (void)projmatrix;  // the reference computes but does not use the projected point (auxiliary.h:149-154)
    if (P < 0 || (P > 0 && (!means3D || !viewmatrix || !present))) return fail_msg(FR_ERR_INVALID_ARGUMENT, "bad argument");
    return launch_mark_visible(P, means3D, viewmatrix, present, static_cast<hipStream_t>(stream));
}

const float* fr_image_final_T(const void* image, int32_t W, int32_t H)
{
    return ImageView::make(const_cast<void*>(image), W, H).final_T;
}
const uint32_t* fr_image_n_contrib(const void* image, int32_t W, int32_t H)
{
    return ImageView::make(const_cast<void*>(image), W, H).n_contrib;
}

const void* fr_debug_geometry_field(const void* geometry, int32_t P, int32_t field)
{
    GeomView g = GeomView::make(const_cast<void*>(geometry), (size_t)(P > 0 ? P : 0));
    switch (field) {
        case 0: return nullptr;   // (pixel-space centres: columns 0-1 of field 8)
        case 1: return nullptr;   // (view-space depth: column 10 of field 8)
        case 2: return nullptr;   // (conic + opacity: columns 2-5 of field 8 hold (-0.5 a, -b, -0.5 c, opacity))
        case 3: return nullptr;   // (colours: columns 6-8 of field 8)
        case 4: return nullptr;   // (Sigma3D is not stored any more: both per-Gaussian kernels compute it)
        case 5: return nullptr;   // (the 8x8-tile rectangle is no longer stored)
        case 6: return g.clamped;
        case 7: return nullptr;   // (the gradient accumulators moved into the handle)
        case 8: return g.rec_tmpl;   // [P][12]: x, y, a', b', c', opacity, r, g, b, id bits, depth, 0
        case 9: return g.dcolor_ddir;   // [9][P], planar
        case 10: return g.opacity_act;
        default: return nullptr;
    }
}

const void* fr_debug_binning_region(const void* binning, uint64_t capacity, int32_t W, int32_t H, int32_t region, size_t* bytes)
{
    if (bytes) *bytes = 0;
    if (W <= 0 || H <= 0) return nullptr;
    const ImageView v = ImageView::make(nullptr, W, H);
    const BinningView b = BinningView::make(const_cast<void*>(binning), (size_t)capacity, (size_t)v.tiles_x * v.tiles_y);
    const void* p = nullptr;
    size_t n = 0;
    switch (region) {
        case 0: p = b.masks, n = b.cap * sizeof(uint2); break;
        case 1: p = b.walks, n = b.unit_cap * kUnit * sizeof(uint2); break;
        case 2: p = b.bwd_units, n = b.unit_cap * sizeof(BwdUnit); break;
        case 3: p = b.unit_state, n = b.unit_cap * kUnit * sizeof(float4); break;
        default: return nullptr;
    }
    if (bytes) *bytes = n;
    return p;
}

int fr_debug_selftest_reduce(const float* in, float* out, void* stream)
{
    return launch_selftest_reduce(in, out, static_cast<hipStream_t>(stream));
}

size_t fr_knn_workspace_bytes(int32_t P) { return knn_workspace_bytes(P); }

int fr_knn_mean_dist2(int32_t P, const float* points, float* out, void* workspace, size_t workspace_bytes, void* stream)
{
    if (P < 0 || (P > 0 && (!points || !out || !workspace))) return fail_msg(FR_ERR_INVALID_ARGUMENT, "bad argument");
    return launch_knn(P, points, out, workspace, workspace_bytes, static_cast<hipStream_t>(stream), 0);
}

int fr_knn_nearest_dist2(int32_t P, const float* points, float* out, void* workspace, size_t workspace_bytes, void* stream)
{
    if (P < 0 || (P > 0 && (!points || !out || !workspace))) return fail_msg(FR_ERR_INVALID_ARGUMENT, "bad argument");
    return launch_knn(P, points, out, workspace, workspace_bytes, static_cast<hipStream_t>(stream), 1);
}

int fr_face_scale(int32_t V, int32_t F, const float* verts, const int32_t* faces, float* out_scale, void* stream)
{
    if (V < 0 || F < 0 || (F > 0 && (!verts || !faces || !out_scale))) return fail_msg(FR_ERR_INVALID_ARGUMENT, "bad argument");
    return launch_face_scale(F, verts, faces, out_scale, static_cast<hipStream_t>(stream));
}

int fr_bind_forward(const fr_binding* b, float* xyz, float* rotation_out, float* scaling_out, void* stream)
{
    int rc = check_binding(b);
    if (rc) return rc;
    if (b->N > 0 && (!xyz || !rotation_out || !scaling_out)) return fail_msg(FR_ERR_INVALID_ARGUMENT, "fr_bind_forward: null output");
    return launch_bind_forward(*b, xyz, rotation_out, scaling_out, static_cast<hipStream_t>(stream));
}

int fr_bind_backward(const fr_binding* b, const float* g_xyz, const float* g_rotation, const float* g_scaling,
                     float* d_verts, float* d_offset, float* d_rotation, float* d_scaling, void* stream)
{
    int rc = check_binding(b);
    if (rc) return rc;
    if (b->mode != FR_BIND_SHELL)
        return fail_msg(FR_ERR_INVALID_ARGUMENT,
                        "fr_bind_backward: the binding is not FR_BIND_SHELL (fr_bind_backward_local / _phong / _deform)");
    return launch_bind_backward(*b, g_xyz, g_rotation, g_scaling, d_verts, d_offset, d_rotation, d_scaling, nullptr,
                                static_cast<hipStream_t>(stream));
}

int fr_bind_backward_local(const fr_binding* b, const float* g_xyz, const float* g_rotation, const float* g_scaling,
                           float* d_verts, float* d_local_xyz, float* d_rotation, float* d_scaling, void* stream)
{
    int rc = check_binding(b);
    if (rc) return rc;
    if (b->mode != FR_BIND_FACE_LOCAL) return fail_msg(FR_ERR_INVALID_ARGUMENT, "fr_bind_backward_local: the binding is not FR_BIND_FACE_LOCAL");
    return launch_bind_backward(*b, g_xyz, g_rotation, g_scaling, d_verts, nullptr, d_rotation, d_scaling, d_local_xyz,
                                static_cast<hipStream_t>(stream));
}

int fr_bind_backward_phong(const fr_binding* b, const float* g_xyz, const float* g_rotation, const float* g_scaling,
                           float* d_verts, float* d_uvd, float* d_rotation, float* d_scaling, void* stream)
{
    int rc = check_binding(b);
    if (rc) return rc;
    if (b->mode != FR_BIND_PHONG) return fail_msg(FR_ERR_INVALID_ARGUMENT, "fr_bind_backward_phong: the binding is not FR_BIND_PHONG");
    if (d_verts) return fail_msg(FR_ERR_INVALID_ARGUMENT, "fr_bind_backward_phong: a FR_BIND_PHONG binding has no vertex gradient");
    return launch_bind_backward(*b, g_xyz, g_rotation, g_scaling, nullptr, nullptr, d_rotation, d_scaling, d_uvd,
                                static_cast<hipStream_t>(stream));
}

int fr_bind_backward_deform(const fr_binding* b, const float* g_xyz, const float* g_rotation, const float* g_scaling,
                            float* d_verts, float* d_deform, float* d_rotation, float* d_scaling, void* stream)
{
    int rc = check_binding(b);
    if (rc) return rc;
    if (b->mode != FR_BIND_DEFORM) return fail_msg(FR_ERR_INVALID_ARGUMENT, "fr_bind_backward_deform: the binding is not FR_BIND_DEFORM");
    return launch_bind_backward(*b, g_xyz, g_rotation, g_scaling, d_verts, nullptr, d_rotation, d_scaling, d_deform,
                                static_cast<hipStream_t>(stream));
}

int fr_phong_frame(int32_t V, int32_t F, const float* verts, const float* cano_verts, const int32_t* faces,
                   const int32_t* vf_offsets, const int32_t* vf_faces, const float* face_area_canonical, float* vert_normals,
                   float* vert_quats, float* face_ratio, void* stream)
{
    if (V < 0 || F < 0) return fail_msg(FR_ERR_INVALID_ARGUMENT, "fr_phong_frame: negative sizes");
    if ((V > 0 || F > 0) && (!verts || !cano_verts || !faces || !vf_offsets || !vf_faces || !face_area_canonical))
        return fail_msg(FR_ERR_INVALID_ARGUMENT, "fr_phong_frame: null input");
    if ((V > 0 && (!vert_normals || !vert_quats)) || (F > 0 && !face_ratio))
        return fail_msg(FR_ERR_INVALID_ARGUMENT, "fr_phong_frame: null output");
    return launch_phong_frame(V, F, verts, cano_verts, faces, vf_offsets, vf_faces, face_area_canonical, vert_normals, vert_quats,
                              face_ratio, static_cast<hipStream_t>(stream));
}

int fr_bind_backward_phong_frame(const fr_binding* b, const float* g_xyz, const float* g_rotation, const float* g_scaling,
                                 float* d_verts, float* d_vert_normals, float* d_vert_quats, float* d_face_ratio, void* stream)
{
    int rc = check_binding(b);
    if (rc) return rc;
    if (b->mode != FR_BIND_PHONG)
        return fail_msg(FR_ERR_INVALID_ARGUMENT, "fr_bind_backward_phong_frame: the binding is not FR_BIND_PHONG");
    return launch_bind_backward_phong_frame(*b, g_xyz, g_rotation, g_scaling, d_verts, d_vert_normals, d_vert_quats, d_face_ratio,
                                            static_cast<hipStream_t>(stream));
}

size_t fr_phong_frame_backward_workspace_bytes(int32_t V, int32_t F)
{
    (void)F;
    return phong_frame_backward_workspace_bytes(V);
}

int fr_phong_frame_backward(int32_t V, int32_t F, const float* verts, const float* cano_verts, const int32_t* faces,
                            const int32_t* vf_offsets, const int32_t* vf_faces, const float* face_area_canonical,
                            const float* d_vert_normals, const float* d_vert_quats, const float* d_face_ratio, float* d_verts,
                            void* workspace, void* stream)
{
    if (V < 0 || F < 0) return fail_msg(FR_ERR_INVALID_ARGUMENT, "fr_phong_frame_backward: negative sizes");
    if (V > 0 && F > 0) {
        if (!verts || !cano_verts || !faces || !vf_offsets || !vf_faces || !face_area_canonical)
            return fail_msg(FR_ERR_INVALID_ARGUMENT, "fr_phong_frame_backward: null mesh array");
        if (!d_verts) return fail_msg(FR_ERR_INVALID_ARGUMENT, "fr_phong_frame_backward: null d_verts");
        if (!workspace) return fail_msg(FR_ERR_INVALID_ARGUMENT, "fr_phong_frame_backward: null workspace (fr_phong_frame_backward_workspace_bytes)");
    }
    return launch_phong_frame_backward(V, F, verts, cano_verts, faces, vf_offsets, vf_faces, face_area_canonical, d_vert_normals,
                                       d_vert_quats, d_face_ratio, d_verts, workspace, static_cast<hipStream_t>(stream));
}

int fr_triwalk(void* stream, const int32_t* faces_nbr, int32_t F, int32_t n, int32_t* face_index, float* bary, const float* delta,
               int32_t delta_stride, float decay, int32_t* status)
{
    if (n < 0 || F < 0 || delta_stride < 2) return fail_msg(FR_ERR_INVALID_ARGUMENT, "fr_triwalk: negative size, or delta_stride < 2");
    if (n > 0 && (!faces_nbr || !face_index || !bary || !delta || !status)) return fail_msg(FR_ERR_INVALID_ARGUMENT, "fr_triwalk: null array");
    return launch_triwalk(faces_nbr, F, n, face_index, bary, delta, delta_stride, decay, status, static_cast<hipStream_t>(stream));
}

int fr_phong_fit(void* stream, const float* cano_verts, const float* cano_normals, const int32_t* faces, const int32_t* faces_nbr,
                 int32_t V, int32_t F, int32_t n, const float* query, int32_t* face_index, float* bary, int32_t outer_loop,
                 int32_t inner_loop, float decay, int32_t* work, int32_t* status, float* delta_out)
{
    if (n < 0 || F < 0 || V < 0) return fail_msg(FR_ERR_INVALID_ARGUMENT, "fr_phong_fit: negative size");
    if (inner_loop < 1 || inner_loop > 512) return fail_msg(FR_ERR_INVALID_ARGUMENT, "fr_phong_fit: inner_loop must be 1 .. 512");
    if (outer_loop < 1 || outer_loop > 8) return fail_msg(FR_ERR_INVALID_ARGUMENT, "fr_phong_fit: outer_loop must be 1 .. 8");
    if (n > 0 && (!cano_verts || !cano_normals || !faces || !faces_nbr || !query || !face_index || !bary || !work || !status))
        return fail_msg(FR_ERR_INVALID_ARGUMENT, "fr_phong_fit: null array");
    return launch_phong_fit(cano_verts, cano_normals, faces, faces_nbr, V, F, n, query, face_index, bary, outer_loop, inner_loop, decay,
                            work, status, delta_out, static_cast<hipStream_t>(stream));
}

// Checks that several entry points share: each caller names itself (`who`) in the message, "<who>: <what>"
static int fail_in(const char* who, const char* what)
{
    snprintf(g_err, sizeof(g_err), "%s: %s", who, what);
    return FR_ERR_INVALID_ARGUMENT;
}
static uintptr_t addr(const void* p) { return reinterpret_cast<uintptr_t>(p); }

// What the two Adam entry points ask, in the order they ask it.  `multi`: the gradients are a list with checks and messages of
// its own; otherwise grads[0] is one of the arrays, checked with them.
static int check_adam(const char* who, bool multi, const fr_adam_config* cfg, const float* param, const float* const* grads, int n_grads,
                      const float* exp_avg, const float* exp_avg_sq, const float* state, uint64_t n)
{
    if (!cfg || cfg->n_segments < 1 || cfg->n_segments > FR_ADAM_MAX_SEGMENTS) return fail_in(who, "1..FR_ADAM_MAX_SEGMENTS segments");
    if (multi && (!grads || n_grads < 1 || n_grads > FR_ADAM_MAX_GRADS)) return fail_in(who, "1..FR_ADAM_MAX_GRADS gradient buffers");
    for (int k = 0; multi && k < n_grads; k++)
        if (n > 0 && (!grads[k] || (addr(grads[k]) & 15))) return fail_in(who, "null or misaligned gradient buffer");
    const float* const grad = multi ? param : grads[0];   // (multi: checked above, `param` stands in)
    if (n > 0 && (!param || !grad || !exp_avg || !exp_avg_sq || !state)) return fail_in(who, "null array");
    uint64_t prev = 0;
    for (int i = 0; i < cfg->n_segments; i++) {
        if (cfg->segment_end[i] < prev) return fail_in(who, "segment ends must ascend");
        prev = cfg->segment_end[i];
    }
    if (prev != n) return fail_in(who, "the last segment must end at n");
    if ((addr(param) | addr(grad) | addr(exp_avg) | addr(exp_avg_sq)) & 15) return fail_in(who, "arrays must be 16-byte aligned");
    if (addr(state) & 7) return fail_in(who, "state must be 8-byte aligned");
    return FR_OK;
}

int fr_adam_step(const fr_adam_config* cfg, float* param, const float* grad, float* exp_avg, float* exp_avg_sq,
                 uint64_t n, float* state, void* stream)
{
    const float* one[1] = {grad};
    const int rc = check_adam("fr_adam_step", false, cfg, param, one, 1, exp_avg, exp_avg_sq, state, n);
    return rc ? rc : launch_adam(*cfg, param, one, 1, exp_avg, exp_avg_sq, n, state, static_cast<hipStream_t>(stream));
}

int fr_adam_step_multi(const fr_adam_config* cfg, float* param, const float* const* grads, int32_t n_grads, float* exp_avg,
                       float* exp_avg_sq, uint64_t n, float* state, void* stream)
{
    const int rc = check_adam("fr_adam_step_multi", true, cfg, param, grads, n_grads, exp_avg, exp_avg_sq, state, n);
    return rc ? rc : launch_adam(*cfg, param, grads, n_grads, exp_avg, exp_avg_sq, n, state, static_cast<hipStream_t>(stream));
}

// One image of a per-pixel term (fr_optim.hip's sweep): is it there, and can it be read as float4 (grad: or null)?  Two questions and
// not one check: the entry points with a configuration ask about that in between.
static bool image_null(const float* img, const float* gt, const float* loss, const void* workspace) { return !img || !gt || !loss || !workspace; }
static bool image_misaligned(const float* img, const float* gt, const float* grad) { return ((addr(img) | addr(gt) | addr(grad)) & 15) != 0; }
// The images of a batched image term, image by image: there (`need`: they are read), aligned (`walk4`: img, gt and grad are
// read as float4; `ws16`: the workspace holds float4 maps), and no workspace met before.
static int check_images(const char* who, int n_images, bool need, bool walk4, bool ws16, const float* const* img, const float* const* gt,
                        float* const* grad, float* const* loss, void* const* workspace)
{
    if (!img || !gt || !loss || !workspace) return fail_in(who, "null argument array");
    for (int k = 0; k < n_images; k++) {
        if (need && image_null(img[k], gt[k], loss[k], workspace[k])) return fail_in(who, "null array");
        if ((walk4 && image_misaligned(img[k], gt[k], grad ? grad[k] : nullptr)) || (ws16 && (addr(workspace[k]) & 15)))
            return fail_in(who, "arrays must be 16-byte aligned");
        for (int j = 0; j < k; j++)
            if (workspace[j] == workspace[k]) return fail_in(who, "one workspace per image");
    }
    return FR_OK;
}

size_t fr_l1_workspace_bytes(void) { return l1_workspace_bytes(); }

int fr_l1_loss_grad(uint64_t n, const float* img, const float* gt, float* grad, float* loss, void* workspace, void* stream)
{
    if (n > 0 && image_null(img, gt, loss, workspace)) return fail_in("fr_l1_loss_grad", "null array");
    if (image_misaligned(img, gt, grad)) return fail_in("fr_l1_loss_grad", "arrays must be 16-byte aligned");
    return launch_l1_loss_grad(n, img, gt, grad, loss, workspace, static_cast<hipStream_t>(stream));
}

int fr_l1_loss_grad_batch(int32_t n_images, uint64_t n, const float* const* img, const float* const* gt, float* const* grad,
                          float* const* loss, void* const* workspace, void* stream)
{
    if (n_images < 1 || n_images > kMaxBatch) return fail_in("fr_l1_loss_grad_batch", "1 .. FR_MAX_BATCH images");
    const int rc = check_images("fr_l1_loss_grad_batch", n_images, n > 0, true, false, img, gt, grad, loss, workspace);
    return rc ? rc : launch_l1_loss_grad_batch(n_images, n, img, gt, grad, loss, workspace, static_cast<hipStream_t>(stream));
}

size_t fr_huber_workspace_bytes(void) { return huber_workspace_bytes(); }

int fr_huber_loss_grad(const fr_huber_config* cfg, int32_t C, int32_t H, int32_t W, const float* img, const float* gt,
                       const float* mask, float* grad, float* loss, void* workspace, void* stream)
{
    if (!cfg || image_null(img, gt, loss, workspace)) return fail_in("fr_huber_loss_grad", "null configuration, img, gt, loss or workspace");
    if (!(cfg->alpha > 0.f)) return fail_in("fr_huber_loss_grad", "alpha must be > 0");
    if (C < 0 || H < 0 || W < 0 || (int64_t)H * W >= (1ll << 31)) return fail_in("fr_huber_loss_grad", "C, H, W >= 0, H x W < 2^31");
    if (image_misaligned(img, gt, grad)) return fail_in("fr_huber_loss_grad", "img, gt and grad must be 16-byte aligned");
    return launch_huber_loss_grad(*cfg, C, H, W, img, gt, mask, grad, loss, workspace, static_cast<hipStream_t>(stream));
}

size_t fr_pixel_loss_workspace_bytes(void) { return pixel_loss_workspace_bytes(); }

int fr_pixel_loss_grad(const fr_pixel_loss_config* cfg, int32_t C, int32_t H, int32_t W, const float* img, const float* gt,
                       float* grad, float* loss, void* workspace, void* stream)
{
    if (!cfg || image_null(img, gt, loss, workspace)) return fail_in("fr_pixel_loss_grad", "null configuration, img, gt, loss or workspace");
    if (C < 0 || H < 0 || W < 0) return fail_in("fr_pixel_loss_grad", "C, H, W >= 0");
    if (image_misaligned(img, gt, grad)) return fail_in("fr_pixel_loss_grad", "img, gt and grad must be 16-byte aligned");
    return launch_pixel_loss_grad(*cfg, C, H, W, img, gt, grad, loss, workspace, static_cast<hipStream_t>(stream));
}

size_t fr_scale_term_workspace_bytes(void) { return scale_term_workspace_bytes(); }

int fr_scale_term(const fr_scale_term_config* cfg, int32_t P, const float* scaling, float* d_scaling, float* loss, void* workspace,
                  void* stream)
{
    if (!cfg || P < 0) return fail_msg(FR_ERR_INVALID_ARGUMENT, "fr_scale_term: null configuration or negative P");
    // (the selected rows are counted in floats: exact below 2^24)
    if (P >= (1 << 24)) return fail_msg(FR_ERR_INVALID_ARGUMENT, "fr_scale_term: P < 2^24");
    if (P > 0 && !scaling) return fail_msg(FR_ERR_INVALID_ARGUMENT, "fr_scale_term: null parameter array");
    if (!workspace || !loss) return fail_msg(FR_ERR_INVALID_ARGUMENT, "fr_scale_term: null workspace or loss");
    return launch_scale_term(*cfg, P, scaling, d_scaling, loss, workspace, static_cast<hipStream_t>(stream));
}

size_t fr_scale_ratio_workspace_bytes(void) { return scale_ratio_workspace_bytes(); }

int fr_scale_ratio_term(const fr_scale_ratio_config* cfg, int32_t P, const float* scaling, float* d_scaling, float* loss,
                        void* workspace, void* stream)
{
    if (!cfg || P < 0) return fail_msg(FR_ERR_INVALID_ARGUMENT, "fr_scale_ratio_term: null configuration or negative P");
    // (the rows over the threshold are counted in floats: exact below 2^24)
    if (P >= (1 << 24)) return fail_msg(FR_ERR_INVALID_ARGUMENT, "fr_scale_ratio_term: P < 2^24");
    if (P > 0 && !scaling) return fail_msg(FR_ERR_INVALID_ARGUMENT, "fr_scale_ratio_term: null parameter array");
    if (!workspace || !loss) return fail_msg(FR_ERR_INVALID_ARGUMENT, "fr_scale_ratio_term: null workspace or loss");
    return launch_scale_ratio_term(*cfg, P, scaling, d_scaling, loss, workspace, static_cast<hipStream_t>(stream));
}

void fr_ssim_window(float out[11])
{
    if (out) ssim_window(out);
}

size_t fr_image_loss_workspace_bytes(int32_t C, int32_t H, int32_t W) { return image_loss_workspace_bytes(C, H, W); }

int fr_image_loss_grad(const fr_image_loss_config* cfg, int32_t n_images, int32_t C, int32_t H, int32_t W, const float* const* img,
                       const float* const* gt, float* const* grad, float* const* loss, void* const* workspace, void* stream)
{
    if (!cfg) return fail_in("fr_image_loss_grad", "null configuration");
    if (n_images < 1 || n_images > kMaxBatch) return fail_in("fr_image_loss_grad", "1 .. FR_MAX_BATCH images");
    if (C < 1 || H < 1 || W < 1 || (int64_t)n_images * C > 65535 || H > (1 << 20) || W > (1 << 20))
        return fail_in("fr_image_loss_grad", "C, H, W >= 1, n_images x C <= 65535, H, W <= 2^20");
    // (the D-SSIM-free path is k_l1_loss_grad's float4 walk)
    const int rc = check_images("fr_image_loss_grad", n_images, true, cfg->dssim_weight == 0.f, true, img, gt, grad, loss, workspace);
    return rc ? rc : launch_image_loss_grad(*cfg, n_images, C, H, W, img, gt, grad, loss, workspace, static_cast<hipStream_t>(stream));
}

size_t fr_regularise_workspace_bytes(void) { return regularise_workspace_bytes(); }

int fr_gaussian_regularise(const fr_regularise_config* cfg, int32_t P, const float* scaling, const float* xyz, float* d_scaling,
                           float* d_xyz, float* loss, void* workspace, void* stream)
{
    if (!cfg || P < 0) return fail_msg(FR_ERR_INVALID_ARGUMENT, "fr_gaussian_regularise: null configuration or negative P");
    if (P > 0 && (!scaling || !xyz)) return fail_msg(FR_ERR_INVALID_ARGUMENT, "fr_gaussian_regularise: null parameter array");
    if (!workspace || !loss) return fail_msg(FR_ERR_INVALID_ARGUMENT, "fr_gaussian_regularise: null workspace or loss");
    return launch_gaussian_regularise(*cfg, P, scaling, xyz, d_scaling, d_xyz, loss, workspace, static_cast<hipStream_t>(stream));
}

size_t fr_mesh_terms_workspace_bytes(void) { return mesh_terms_workspace_bytes(); }

int fr_mesh_terms(const fr_mesh_terms_config* cfg, int32_t V, const float* verts, const float* verts_orig, const int32_t* row_ptr,
                  const int32_t* col, float* d_verts, float* loss, void* workspace, void* stream)
{
    if (!cfg || V < 0) return fail_msg(FR_ERR_INVALID_ARGUMENT, "fr_mesh_terms: null configuration or negative V");
    if (!verts || !verts_orig || !row_ptr) return fail_msg(FR_ERR_INVALID_ARGUMENT, "fr_mesh_terms: null verts, verts_orig or row_ptr");
    if (V > 0 && !col) return fail_msg(FR_ERR_INVALID_ARGUMENT, "fr_mesh_terms: null col");
    if (!workspace || !loss) return fail_msg(FR_ERR_INVALID_ARGUMENT, "fr_mesh_terms: null workspace or loss");
    return launch_mesh_terms(*cfg, V, verts, verts_orig, row_ptr, col, d_verts, loss, workspace, static_cast<hipStream_t>(stream));
}

static const char* point_lbs_invalid(const fr_point_lbs* d)
{
    if (!d || d->N < 0) return "fr_point_lbs: null descriptor or negative N";
    if (d->E < 1 || d->E > FR_LBS_MAX_E || d->J < 1 || d->J > FR_LBS_MAX_J) return "fr_point_lbs: E outside 1 .. FR_LBS_MAX_E or J outside 1 .. FR_LBS_MAX_J";
    if (d->N > 0 && (!d->points || !d->shapedirs || !d->posedirs || !d->weights)) return "fr_point_lbs: null per-point array";
    for (const fr_pose_state* p : {&d->canonical, &d->frame})
        if (!p->betas || !p->pose_feature || !p->transforms) return "fr_point_lbs: null pose state array";
    return nullptr;
}

int fr_point_lbs_forward(const fr_point_lbs* lbs, float* xyz, void* stream)
{
    if (const char* why = point_lbs_invalid(lbs)) return fail_msg(FR_ERR_INVALID_ARGUMENT, why);
    if (lbs->N > 0 && !xyz) return fail_msg(FR_ERR_INVALID_ARGUMENT, "fr_point_lbs_forward: null xyz");
    return launch_point_lbs_forward(*lbs, xyz, static_cast<hipStream_t>(stream));
}

int fr_point_lbs_backward(const fr_point_lbs* lbs, const float* g_xyz, float* d_points, float* d_shapedirs, float* d_posedirs,
                          float* d_weights, void* stream)
{
    if (const char* why = point_lbs_invalid(lbs)) return fail_msg(FR_ERR_INVALID_ARGUMENT, why);
    if (lbs->N > 0 && !g_xyz) return fail_msg(FR_ERR_INVALID_ARGUMENT, "fr_point_lbs_backward: null g_xyz");
    return launch_point_lbs_backward(*lbs, g_xyz, d_points, d_shapedirs, d_posedirs, d_weights, static_cast<hipStream_t>(stream));
}

size_t fr_point_lbs_pose_workspace_bytes(void) { return point_lbs_pose_workspace_bytes(); }

int fr_point_lbs_backward_pose(const fr_point_lbs* lbs, const float* g_xyz, float* d_betas, float* d_pose_feature, float* d_transforms,
                               void* workspace, void* stream)
{
    if (const char* why = point_lbs_invalid(lbs)) return fail_msg(FR_ERR_INVALID_ARGUMENT, why);
    if (lbs->N > 0 && !g_xyz) return fail_msg(FR_ERR_INVALID_ARGUMENT, "fr_point_lbs_backward_pose: null g_xyz");
    if (!workspace || (reinterpret_cast<uintptr_t>(workspace) & 15u))
        return fail_msg(FR_ERR_INVALID_ARGUMENT, "fr_point_lbs_backward_pose: null workspace, or one that is not 16-byte aligned");
    return launch_point_lbs_backward_pose(*lbs, g_xyz, d_betas, d_pose_feature, d_transforms, workspace, static_cast<hipStream_t>(stream));
}

int fr_nearest_vertex(int32_t N, const float* points, int32_t V, const float* verts, int32_t* index, float* dist2, void* stream)
{
    if (N < 0) return fail_msg(FR_ERR_INVALID_ARGUMENT, "fr_nearest_vertex: negative N");
    if (V <= 0 || V > FR_NEAREST_MAX_V) return fail_msg(FR_ERR_INVALID_ARGUMENT, "fr_nearest_vertex: V outside 1 .. FR_NEAREST_MAX_V");
    if (!verts || (N > 0 && (!points || !index))) return fail_msg(FR_ERR_INVALID_ARGUMENT, "fr_nearest_vertex: null points, verts or index");
    return launch_nearest_vertex(N, points, V, verts, index, dist2, static_cast<hipStream_t>(stream));
}

size_t fr_lbs_terms_workspace_bytes(void) { return lbs_terms_workspace_bytes(); }

int fr_lbs_terms(const fr_lbs_terms_config* cfg, int32_t N, int32_t V, int32_t E, int32_t J, const int32_t* index, const float* weights,
                 const float* posedirs, const float* shapedirs, const float* gt_weights, const float* gt_posedirs,
                 const float* gt_shapedirs, float* d_weights, float* d_posedirs, float* d_shapedirs, float* loss, void* workspace,
                 void* stream)
{
    if (!cfg || N < 0) return fail_msg(FR_ERR_INVALID_ARGUMENT, "fr_lbs_terms: null configuration or negative N");
    if (V < 1 || E < 1 || J < 1) return fail_msg(FR_ERR_INVALID_ARGUMENT, "fr_lbs_terms: V, E and J are at least 1");
    if (N > 0 && (!index || !weights || !posedirs || !shapedirs)) return fail_msg(FR_ERR_INVALID_ARGUMENT, "fr_lbs_terms: null index or predicted array");
    if (!gt_weights || !gt_posedirs || !gt_shapedirs) return fail_msg(FR_ERR_INVALID_ARGUMENT, "fr_lbs_terms: null ground-truth table");
    if (!workspace || !loss) return fail_msg(FR_ERR_INVALID_ARGUMENT, "fr_lbs_terms: null workspace or loss");
    return launch_lbs_terms(*cfg, N, V, E, J, index, weights, posedirs, shapedirs, gt_weights, gt_posedirs, gt_shapedirs, d_weights,
                            d_posedirs, d_shapedirs, loss, workspace, static_cast<hipStream_t>(stream));
}

int fr_multi_copy(int32_t n_segments, float* const* dst, const float* const* src, const uint64_t* count, void* stream)
{
    if (n_segments < 0 || n_segments > FR_COPY_MAX_SEGMENTS || (n_segments > 0 && (!dst || !src || !count)))
        return fail_msg(FR_ERR_INVALID_ARGUMENT, "fr_multi_copy: 0..FR_COPY_MAX_SEGMENTS segments");
    unsigned long long cnt[FR_COPY_MAX_SEGMENTS];
    for (int i = 0; i < n_segments; i++) {
        if (count[i] > 0 && (!dst[i] || !src[i])) return fail_msg(FR_ERR_INVALID_ARGUMENT, "fr_multi_copy: null segment");
        cnt[i] = count[i];
    }
    return launch_multi_copy(n_segments, dst, src, cnt, static_cast<hipStream_t>(stream));
}

int fr_scaled_sum(int32_t n_src, const float* const* src, float* dst, uint64_t count, float scale, void* stream)
{
    if (n_src < 1 || n_src > FR_ADAM_MAX_GRADS || !src || (count > 0 && !dst))
        return fail_msg(FR_ERR_INVALID_ARGUMENT, "fr_scaled_sum: 1..FR_ADAM_MAX_GRADS sources");
    uintptr_t bits = reinterpret_cast<uintptr_t>(dst);
    for (int k = 0; k < n_src; k++) {
        if (count > 0 && !src[k]) return fail_msg(FR_ERR_INVALID_ARGUMENT, "fr_scaled_sum: null source");
        bits |= reinterpret_cast<uintptr_t>(src[k]);
    }
    if (bits & 15) return fail_msg(FR_ERR_INVALID_ARGUMENT, "fr_scaled_sum: arrays must be 16-byte aligned");
    return launch_scaled_sum(n_src, src, dst, count, scale, static_cast<hipStream_t>(stream));
}

size_t fr_mlp_workspace_bytes(int32_t N, int32_t L)
{
    if (N < 0 || L < 1 || L > FR_MLP_MAX_LAYERS) return 0;
    return mlp_workspace_bytes(N, L);
}

static int mlp_check(const fr_mlp* m, const void* workspace, const char*& why)
{
    why = nullptr;
    if (!m) why = "null descriptor";
    else if (m->N < 0) why = "negative N";
    else if (m->L < 1 || m->L > FR_MLP_MAX_LAYERS) why = "1 <= L <= FR_MLP_MAX_LAYERS";
    else if (m->De < 1 || m->Dc < 0 || m->De + m->Dc > FR_MLP_WIDTH) why = "De >= 1, Dc >= 0, De + Dc <= FR_MLP_WIDTH";
    else if (m->D_out < 1 || m->D_out > FR_MLP_MAX_OUT) why = "1 <= D_out <= FR_MLP_MAX_OUT";
    else if (!workspace) why = "null workspace";
    else if (reinterpret_cast<uintptr_t>(workspace) & 255) why = "the workspace must be 256-byte aligned";
    else if (m->N > 0 && (!m->E || !m->weights || (m->Dc > 0 && !m->cond))) why = "null E, weights or cond";
    return why ? FR_ERR_INVALID_ARGUMENT : FR_OK;
}

int fr_mlp_forward(const fr_mlp* mlp, float* out, void* workspace, void* stream)
{
    const char* why;
    if (mlp_check(mlp, workspace, why) != FR_OK) {
        snprintf(g_err, sizeof(g_err), "fr_mlp_forward: %s", why);
        return FR_ERR_INVALID_ARGUMENT;
    }
    if (mlp->N > 0 && !out) return fail_msg(FR_ERR_INVALID_ARGUMENT, "fr_mlp_forward: null out");
    return launch_mlp_forward(*mlp, out, workspace, static_cast<hipStream_t>(stream));
}

int fr_mlp_backward(const fr_mlp* mlp, const float* d_out, float* d_weights, float* d_cond, void* workspace, void* stream)
{
    const char* why;
    if (mlp_check(mlp, workspace, why) != FR_OK) {
        snprintf(g_err, sizeof(g_err), "fr_mlp_backward: %s", why);
        return FR_ERR_INVALID_ARGUMENT;
    }
    if (!d_weights || (mlp->N > 0 && !d_out)) return fail_msg(FR_ERR_INVALID_ARGUMENT, "fr_mlp_backward: null d_out or d_weights");
    return launch_mlp_backward(*mlp, d_out, d_weights, d_cond, workspace, static_cast<hipStream_t>(stream));
}

size_t fr_flame_workspace_bytes(int32_t V, int32_t NE)
{
    if (V < 0 || NE < 1 || NE > FR_FLAME_MAX_E) return 0;
    return flame_workspace_bytes(V, NE);
}

size_t fr_flame_workspace_zeroed_bytes(void) { return flame_workspace_zeroed_bytes(); }

static const char* flame_invalid(const fr_flame* f, const void* workspace)
{
    if (!f || f->V < 0 || f->NS < 0) return "fr_flame: null descriptor, or negative V or NS";
    if (f->NE < 1 || f->NE > FR_FLAME_MAX_E) return "fr_flame: NE outside 1 .. FR_FLAME_MAX_E";
    if (!workspace || (reinterpret_cast<uintptr_t>(workspace) & 15u)) return "fr_flame: null workspace, or one that is not 16-byte aligned";
    if (!f->parents || !f->expression || !f->pose) return "fr_flame: null parents, expression or pose";
    if (f->V > 0 && (!f->v_template || !f->shapedirs || !f->posedirs || !f->J_regressor || !f->lbs_weights))
        return "fr_flame: null model array";
    return nullptr;
}

int fr_flame_forward(const fr_flame* flame, float* verts, float* verts_orig, float* pose_feature, float* transforms, void* workspace,
                     void* stream)
{
    if (const char* why = flame_invalid(flame, workspace)) return fail_msg(FR_ERR_INVALID_ARGUMENT, why);
    if (flame->V > 0 && !verts) return fail_msg(FR_ERR_INVALID_ARGUMENT, "fr_flame_forward: null verts");
    return launch_flame_forward(*flame, verts, verts_orig, pose_feature, transforms, workspace, static_cast<hipStream_t>(stream));
}

int fr_flame_backward(const fr_flame* flame, const float* g_verts, float* d_delta_exp, float* d_delta_posedirs, float* d_delta_vertex,
                      float* d_expression, float* d_pose, void* workspace, void* stream)
{
    if (const char* why = flame_invalid(flame, workspace)) return fail_msg(FR_ERR_INVALID_ARGUMENT, why);
    if (flame->V > 0 && !g_verts) return fail_msg(FR_ERR_INVALID_ARGUMENT, "fr_flame_backward: null g_verts");
    return launch_flame_backward(*flame, g_verts, d_delta_exp, d_delta_posedirs, d_delta_vertex, d_expression, d_pose, workspace,
                                 static_cast<hipStream_t>(stream));
}

size_t fr_vgg_workspace_bytes(const fr_vgg* vgg) { return vgg_invalid(vgg) ? 0 : vgg_workspace_bytes(*vgg); }

int fr_vgg_loss_grad(const fr_vgg* vgg, float weight, int accumulate, float* loss_out, float* d_image, void* workspace, void* stream)
{
    const char* why = vgg_invalid(vgg);
    if (!why && (!vgg->weights_fwd || !vgg->weights_bwd || !vgg->image || !vgg->target)) why = "null weights, image or target";
    if (!why && !loss_out) why = "null loss_out";
    if (!why && !workspace) why = "null workspace";
    if (!why && (reinterpret_cast<uintptr_t>(workspace) & 255)) why = "the workspace must be 256-byte aligned";
    if (!why && ((reinterpret_cast<uintptr_t>(vgg->weights_fwd) | reinterpret_cast<uintptr_t>(vgg->weights_bwd)) & 15))
        why = "the packed weights must be 16-byte aligned";
    if (!why && ((reinterpret_cast<uintptr_t>(vgg->image) | reinterpret_cast<uintptr_t>(vgg->target) |
                  reinterpret_cast<uintptr_t>(loss_out) | reinterpret_cast<uintptr_t>(d_image)) & 3))
        why = "float arrays must be 4-byte aligned";
    if (why) {
        snprintf(g_err, sizeof(g_err), "fr_vgg_loss_grad: %s", why);
        return FR_ERR_INVALID_ARGUMENT;
    }
    return launch_vgg_loss_grad(*vgg, weight, accumulate, loss_out, d_image, workspace, static_cast<hipStream_t>(stream));
}

size_t fr_lpips_workspace_bytes(const fr_vgg* vgg) { return lpips_invalid(vgg) ? 0 : lpips_workspace_bytes(*vgg); }

int fr_lpips_loss_grad(const fr_vgg* vgg, const float* lin, float weight, int accumulate, float* loss_out, float* d_image, void* workspace,
                       void* stream)
{
    const char* why = lpips_invalid(vgg);
    if (!why && (!vgg->weights_fwd || !vgg->weights_bwd || !vgg->image || !vgg->target)) why = "null weights, image or target";
    if (!why && !lin) why = "null lin";
    if (!why && !loss_out) why = "null loss_out";
    if (!why && !workspace) why = "null workspace";
    if (!why && (reinterpret_cast<uintptr_t>(workspace) & 255)) why = "the workspace must be 256-byte aligned";
    if (!why && ((reinterpret_cast<uintptr_t>(vgg->weights_fwd) | reinterpret_cast<uintptr_t>(vgg->weights_bwd) | reinterpret_cast<uintptr_t>(lin)) & 15))
        why = "the packed weights and lin must be 16-byte aligned";
    if (!why && ((reinterpret_cast<uintptr_t>(vgg->image) | reinterpret_cast<uintptr_t>(vgg->target) |
                  reinterpret_cast<uintptr_t>(loss_out) | reinterpret_cast<uintptr_t>(d_image)) & 3))
        why = "float arrays must be 4-byte aligned";
    if (why) {
        snprintf(g_err, sizeof(g_err), "fr_lpips_loss_grad: %s", why);
        return FR_ERR_INVALID_ARGUMENT;
    }
    return launch_lpips_loss_grad(*vgg, lin, weight, accumulate, loss_out, d_image, workspace, static_cast<hipStream_t>(stream));
}

}  // extern "C"
