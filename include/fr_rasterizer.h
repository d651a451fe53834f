/*
 * fr_rasterizer.h — C ABI of the MI355X (gfx950) Gaussian-splat rasterizer.
 *
 * Drop-in boundary for FateAvatar's render path.  Every entry point takes plain
 * DEVICE pointers, sizes and a HIP stream; no torch types, no exceptions across
 * the ABI, integer return codes.  The entry points are what the reference's own
 * torch glue binds (reference paths are relative to
 * submodules/diff-gaussian-rasterization/ and submodules/simple-knn/):
 *
 *   fr_forward        replaces CudaRasterizer::Rasterizer::forward
 *                     (cuda_rasterizer/rasterizer.h:36-60, rasterizer_impl.cu:198-336),
 *                     called from RasterizeGaussiansCUDA (rasterize_points.cu:35-115)
 *   fr_backward       replaces CudaRasterizer::Rasterizer::backward
 *                     (cuda_rasterizer/rasterizer.h:62-85, rasterizer_impl.cu:340-434),
 *                     called from RasterizeGaussiansBackwardCUDA (rasterize_points.cu:117-196)
 *   fr_mark_visible   replaces CudaRasterizer::Rasterizer::markVisible
 *                     (cuda_rasterizer/rasterizer.h:24-29, rasterizer_impl.cu:141-153),
 *                     called from markVisible (rasterize_points.cu:198-217)
 *   fr_bind_forward / fr_bind_backward / fr_face_scale replace the ~40 PyTorch kernels of the mesh
 *                     binding (model/fateavatar.py:225-258, volume_rendering/mesh_compute.py:27-59);
 *                     with FR_BIND_FACE_LOCAL, fr_bind_forward / fr_bind_backward_local replace those of
 *                     GaussianAvatars' binding (model/baseline/gaussianavatars.py:144-171)
 *   fr_phong_frame    SplattingAvatar's per-frame mesh pass (model/baseline/splattingavatar.py:203-215, :819-902): vertex
 *                     normals, per-vertex quaternions, face area ratios in one launch; with FR_BIND_PHONG, fr_bind_forward /
 *                     fr_bind_backward_phong replace its Phong-surface binding (:224-246)
 *   fr_triwalk / fr_phong_fit replace SplattingAvatar's CPU submodule (submodules/simple_phongsurf/simple_phongsurf/):
 *                     Triwalk::updateSurfacePointsImpl (src/triangle_walk_py.cpp:62-79) around walkSurfacePoint
 *                     (src/triangle_walk.cpp:240-386), and PhongSurfacePy3d.update_corres_spt (phongsurf_py3d.py:151-185)
 *   fr_adam_step      replaces torch.optim.Adam.step() over the Gaussian groups (train/optim.py:11-37)
 *   fr_knn_mean_dist2 replaces SimpleKNN::knn (simple_knn.h, simple_knn.cu:186-222),
 *                     called from distCUDA2 (spatial.cu:14-25)
 *   fr_knn_nearest_dist2 replaces pytorch3d knn_points(p, p, K=6).dists[..., 1] in get_init_scale_by_knn
 *                     (model/fateavatar.py:597-608)
 *
 * Differences from the reference interface, all deliberate:
 *   - Scratch is three caller-owned byte buffers sized by fr_*_bytes() instead of
 *     std::function<char*(size_t)> resize callbacks: the caller's allocator stays in
 *     charge (torch caching allocator in the Python host).  The only device memory the
 *     library owns lives in the fr_handle: per-tile counters, the key buckets the counting
 *     pass writes into (tiles x 8 x capacity keys; 34 MB at 512 x 512) and the gradient
 *     accumulators of the blend backward (64 B per Gaussian), all allocated when a size is
 *     first seen and grown on demand.
 *   - The binning buffer has a CAPACITY.  fr_forward never blocks the GPU on the
 *     instance count (the reference does a blocking cudaMemcpy, rasterizer_impl.cu:281):
 *     it enqueues the whole frame, then reads the counts the sort kernel wrote to pinned
 *     host memory.  If the capacity was too small it returns FR_ERR_BINNING_CAPACITY and
 *     the required size; the caller regrows and calls again.
 *   - Work is enqueued on the stream passed in, not on the legacy default stream.
 *   - Tiles are 8x8 pixels = one 64-lane wavefront (the reference uses 16x16 = 256
 *     threads) and per-tile lists only hold Gaussians whose alpha >= 1/255 footprint
 *     touches the tile, clipped to the reference's own 16x16 tile rectangle, so every
 *     pixel blends exactly the sequence the reference blends.  `num_rendered` is still
 *     reported in reference semantics (sum of 16x16 tiles touched).
 */
#ifndef FR_RASTERIZER_H_INCLUDED
#define FR_RASTERIZER_H_INCLUDED

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define FR_OK 0
#define FR_ERR_INVALID_ARGUMENT 1
#define FR_ERR_BINNING_CAPACITY 2 /* binning buffer too small; *instances_needed tells how big */
#define FR_ERR_HIP 3              /* a HIP runtime call failed; see fr_last_error() */
#define FR_ERR_UNSUPPORTED 4

/* Per-device context: pinned count slot, event, and the per-tile binning counters (device memory, kept zero
 * between frames so that a frame needs no zeroing launch), the key buckets and the gradient accumulators.  Calls on
 * one handle must not overlap on the host (one thread at a time); on the device, frames enqueued on one stream are
 * ordered by it and a frame on another stream first waits for the previous frame's event (forward passes wait for the
 * previous forward, backward passes for the previous backward: they share the counters resp. the accumulators).  Frames
 * enqueued while a stream is being CAPTURED are ordered by the capture; replays of the graph by whoever launches them —
 * give frames that are to run concurrently their own handles.  The handle's device memory
 * grows with the tile grid / Gaussian count / longest per-XCD tile sub-list (hipMalloc — not while the stream is being
 * captured into a hipGraph: run one eager frame of that size first; fr_forward on a capturing stream that would have
 * to grow something returns FR_ERR_UNSUPPORTED before enqueuing anything, which leaves the capture valid).  A captured
 * graph holds the handle's buffer pointers: once a frame of the handle has been captured, buffers that a later eager
 * frame outgrows are retired (kept until fr_destroy) instead of freed, so replays stay valid. */
typedef struct fr_handle fr_handle;

/* (defined with fr_bind_forward below) */
typedef struct fr_binding fr_binding;

/* Optional fused side inputs / outputs: per-Gaussian work the caller's step otherwise does
 * with extra kernels around the rasterizer.  Device pointers unless stated otherwise; any member may be NULL. */
typedef struct fr_aux {
    uint8_t* visible;   /* fr_forward  out    [P]: radii > 0, i.e. render()'s visibility_filter (render_3dgs.py:80) */
    float* grad_accum;  /* fr_backward in/out [P]: += ||dL_dmeans2D[i,:2]|| where radii > 0 — xyz_gradient_accum of
                           _add_densification_stats (model/fateavatar.py:734-737) */
    float* denom;       /* fr_backward in/out [P]: += 1 where radii > 0 (same function) */
    /* The frame rendered straight from its MESH BINDING (model/fateavatar.py:225-258; HOST pointer to the descriptor
     * fr_bind_forward takes, binding->N == P).  Needs FR_FLAG_RAW_ACTIVATIONS and scales + rotations.
     * fr_forward: the per-Gaussian kernel evaluates fr_bind_forward's expressions in front of its own work — same bits —
     * and inputs.means3D / rotations / scales are then OUTPUTS of the call: every row is written with the bound values
     * (what the reference assigns to gaussian._xyz / _rotation / _scaling before render()); they are not read.
     * fr_backward (same descriptor, the arrays fr_forward wrote handed back in inputs): the per-Gaussian backward
     * continues through the binding — fr_bind_backward's expressions on the gradients it would have written to
     * dL_dmeans3D / dL_drotations / dL_dscales (which may then be NULL) — and writes d_offset [P], d_rotation [P,4],
     * d_scaling [P,3] (every row; zeros for culled Gaussians) and ADDS dL/dverts into d_verts [V,3] (float atomics; the
     * caller zeroes it).  FR_FLAG_ACCUMULATE does not apply to these four.
     * A descriptor with mode FR_BIND_FACE_LOCAL (model/baseline/gaussianavatars.py:144-171) goes the same way; its backward
     * writes d_local_xyz [P,3] (below) where the shell binding writes d_offset.  So does one with mode FR_BIND_PHONG
     * (model/baseline/splattingavatar.py:224-246): d_local_xyz receives d_uvd, and d_verts must be NULL.  And one with mode
     * FR_BIND_DEFORM (model/baseline/flashavatar.py:242-276): d_local_xyz receives d_deform, TEN floats per row, and d_verts
     * takes b_k g_xyz at the face's three corners. */
    const fr_binding* binding;
    float* d_verts;
    float* d_offset;
    float* d_rotation;
    float* d_scaling;
    /* fr_backward out [1] (device float, or NULL): 1.0f if the frame this backward belongs to overflowed its binning capacity
     * — nothing was blended, every gradient of the call is zero —, else 0.0f.  A step replayed from a hipGraph cannot react on
     * the host before its optimizer kernel runs; fr_adam_config::skip points the update at these words instead (a step
     * whose gradient is partly zeros for that reason is skipped, moments and step count included).  The word is OVERWRITTEN by
     * every backward call: frames that feed one optimizer step need ONE WORD EACH (fr_adam_config::skip takes up to
     * FR_ADAM_MAX_GRADS of them); the views of one fr_backward_batch call must not share a word. */
    float* overflow_out;
    /* fr_backward / fr_backward_batch out [P,3]: a binding with mode FR_BIND_FACE_LOCAL or FR_BIND_PHONG (d_uvd), or out [P,10]:
     * one with mode FR_BIND_DEFORM (d_deform) — only those three modes —, where it takes d_offset's
     * place (every row written, zeros for culled Gaussians; d_offset is then not touched).  It sits behind the binding's
     * other members: the members in front of it keep their offsets, the plane members below stay the struct's last. */
    float* d_local_xyz;
    /* FR_FLAG_DEPTH_ALPHA only (appended: positional construction of the members above is unchanged; all unused without the
     * flag).  fr_forward / fr_forward_batch out [H,W], both required under the flag: out_depth = sum over the pixel's blended
     * Gaussians of z_i alpha_i T_i (z_i the view-space depth of the mean; 0 where nothing is blended), out_alpha = 1 - the final
     * transmittance fr_image_final_T holds (0 where nothing is blended).  Expected depth is out_depth / out_alpha. */
    float* out_depth;
    float* out_alpha;
    /* fr_backward / fr_backward_batch in [H,W]: the planes' upstream gradients.  Either may be NULL (zero); with both NULL the
     * backward is the plain one.  dL/dz reaches dL_dmeans3D through row 2 of the view matrix (and from there fr_aux::binding
     * and FR_FLAG_ACCUMULATE as every means3D gradient); dL_dmeans2D's z stays 0. */
    const float* dL_ddepth;
    const float* dL_dalpha;
    /* fr_planes_bytes(capacity, W, H) bytes of caller-owned device scratch (capacity = the frame's binning capacity), required
     * under the flag: the depth channel's share of the blend hand-off.  The forward fills it and the backward of the same frame
     * reads it, like `binning`: hand the backward the same buffer. */
    void* planes;
} fr_aux;

/* The side block of a backward with FR_FLAG_CAMERA_GRAD: fr_aux with the camera's members behind it.  With the flag set,
 * fr_params::aux MUST point at the `base` member of one of these — fr_backward / fr_backward_batch read the tail through that
 * pointer (as fr_binding_phong extends fr_binding).  fr_aux itself is unchanged, size and layout: callers without the flag
 * neither carry nor read a tail. */
typedef struct fr_aux_camera {
    fr_aux base;
    /* out: dL/d(viewmatrix) [16], dL/d(projmatrix) [16] and dL/d(campos) [3] of fr_inputs, in the storage the kernels read,
     * OVERWRITTEN.  Any of the three may be NULL (not wanted), not all of them. */
    float* d_viewmatrix;
    float* d_projmatrix;
    float* d_campos;
    /* fr_camera_grad_workspace_bytes() bytes of device memory, 16-byte aligned, required: zeroed ONCE by the caller and left
     * zeroed by the kernel.  Launches that may overlap on the device (the views of a batch, other handles) need one each. */
    void* camera_workspace;
} fr_aux_camera;

/* Frame parameters: the scalar arguments of Rasterizer::forward/backward. */
typedef struct fr_params {
    int32_t P;            /* number of Gaussians */
    int32_t D;            /* active SH degree (0..3) */
    int32_t M;            /* SH coefficients stored per Gaussian (shs is [P,M,3]); 0 if no shs */
    int32_t W, H;         /* image size in pixels */
    float tan_fovx, tan_fovy;
    float scale_modifier;
    int32_t prefiltered;  /* accepted for interface parity; the near-plane cull is always applied */
    int32_t debug;        /* !=0: synchronise and check after every stage (auxiliary.h:166-173) */
    int32_t flags;        /* FR_FLAG_* */
    const fr_aux* aux;    /* optional fused side outputs (host pointer to a struct of device pointers), or NULL */
} fr_params;

/* fr_forward does not wait for the frame counts: nothing in the call blocks or touches an event, so it can
 * be captured into a hipGraph.  `counts` is not filled; after the stream has been synchronised read them with
 * fr_read_counts.  If counts.overflow is set the frame's outputs are invalid: rerun with a larger capacity. */
#define FR_FLAG_NO_WAIT 1

/* Fused activations (reference volume_rendering/gaussian_model.py:39-50,105-128):
 * inputs.opacities / scales / rotations hold the RAW parameters and the kernels apply sigmoid / exp /
 * normalize (x / max(|x|, 1e-12)) themselves; fr_backward then returns dL/d(raw) in dL_dopacity, dL_dscales,
 * dL_drotations.  Requires scales + rotations (not cov3D_precomp).  Pass the same flag to fr_backward. */
#define FR_FLAG_RAW_ACTIVATIONS 2

/* fr_forward / fr_forward_batch: a frame NO BACKWARD will follow (evaluation, fps measurement, reenactment, a GUI — the
 * reference renders those under torch.no_grad()).  The forward skips the backward's hand-off: it neither evaluates nor
 * stores the colour's derivative with respect to the view direction, stores no clamp bits and no activated opacities in
 * `geometry`, and no footprint masks, pixel-major walks, backward work list or per-unit entry state in `binning`
 * (fr_debug_geometry_field 6, 9, 10 and fr_debug_binning_region 0 .. 3: they keep whatever they held, i.e. are undefined).
 * The image, radii, fr_aux::visible, the bound means3D / rotations / scales of fr_aux::binding, and the final transmittance
 * and contributor count in `image` (fr_image_final_T / fr_image_n_contrib) are written as by the full forward of the same
 * frame, bit for bit.  All views of a batch must agree on the flag (FR_ERR_INVALID_ARGUMENT otherwise).  The handle
 * remembers the flags and the geometry / binning pointers of its most recent forward: fr_backward / fr_backward_batch
 * handed the geometry or binning buffer of a forward-only frame return FR_ERR_INVALID_ARGUMENT and enqueue nothing.  A
 * forward-only frame leaves the handle as any frame does: a full forward + backward may follow it on the same handle. */
#define FR_FLAG_FORWARD_ONLY 4

/* A frame with per-pixel DEPTH and ALPHA planes next to the image (fr_aux::out_depth / out_alpha; the reference's rasterizer
 * returns neither: silhouette / mask losses, compositing over anything, depth regularisers).  Honoured by fr_forward,
 * fr_forward_batch, fr_backward and fr_backward_batch; combines with FR_FLAG_FORWARD_ONLY, FR_FLAG_RAW_ACTIVATIONS,
 * FR_FLAG_NO_WAIT, FR_FLAG_ACCUMULATE and fr_aux::binding.  The image, radii, fr_aux::visible, final transmittance,
 * contributor counts and bound means3D / rotations / scales are those of the same frame without the flag, bit for bit; the
 * depth is blended as a fourth colour channel (colour z_i, background 0) with the colours' arithmetic.  Under the flag the
 * forward needs fr_aux::out_depth, out_alpha and planes (FR_ERR_INVALID_ARGUMENT otherwise).  The backward takes the planes'
 * gradients in fr_aux::dL_ddepth / dL_dalpha with the flag set (a plane gradient without the flag is FR_ERR_INVALID_ARGUMENT);
 * handed the geometry or binning buffer of the handle's most recent forward while that forward had no planes, it returns
 * FR_ERR_INVALID_ARGUMENT and enqueues nothing.  All views of a batch must agree on the flag.  Scratch sizes of frames without
 * the flag are unchanged; a frame with it needs fr_planes_bytes() more. */
#define FR_FLAG_DEPTH_ALPHA 8

/* fr_backward / fr_backward_batch: also return the gradient of the loss with respect to the frame's CAMERA — the three camera
 * inputs of fr_inputs, viewmatrix [16], projmatrix [16] and campos [3], as independent variables in the storage the kernels
 * read (view-space mean c = sum_r viewmatrix[c + 4 r] m_r + viewmatrix[c + 12]) — in fr_aux_camera::d_viewmatrix /
 * d_projmatrix / d_campos (fr_params::aux then points at an fr_aux_camera's `base`).  The reference's rasterizer returns None for them (diff_gaussian_rasterization/__init__.py:143-153), so its
 * per-frame camera embedding (train/base.py:123,142) never trains.  One more launch between the blend backward and the
 * per-Gaussian backward sums, over the Gaussians with radii > 0,
 *   d viewmatrix[c + 4 r] = dL/dt_c m_r (m = (mean, 1); dL/dt the per-Gaussian backward's, with the reference's stop-gradient
 *                           on guard-band-clamped x / y; + the depth plane's dL/dz for c = 2) + the part through the rotation
 *                           inside the 2D covariance's T = J W,
 *   d projmatrix          through ndc = hom.xy / (hom.w + 1e-7) from dL_dmeans2D,
 *   d campos              = minus the SH colour's share of dL_dmeans3D (0 for a frame with colors_precomp).
 * Entries no kernel reads are written as 0: flat indices 3, 7, 11, 15 of viewmatrix and 2, 6, 10, 14 of projmatrix.  The
 * discrete decisions (culling, tile lists, depth order) get no gradient, and neither do tan_fovx / tan_fovy.  A frame that
 * overflowed its binning capacity writes zeros; fr_backward with P == 0 enqueues nothing and leaves them as they are.  No float atomics: per-workgroup partial sums are added up in index order by
 * the workgroup that finishes last, so the same inputs give the same bits on every call; nothing allocates or synchronises
 * (the call stays capturable).  The fr_grads arrays are those of the same call without the flag, bit for bit, and a call
 * without the flag launches exactly what it did before.  Needs an fr_aux_camera with camera_workspace and at least one of the three
 * outputs (FR_ERR_INVALID_ARGUMENT otherwise); all views of a batch must agree on the flag.  Combines with
 * FR_FLAG_RAW_ACTIVATIONS, FR_FLAG_DEPTH_ALPHA, FR_FLAG_ACCUMULATE (which does not apply to the three arrays) and
 * fr_aux::binding (the bound means3D / scales / rotations the forward wrote come back in fr_inputs).  fr_forward ignores it. */
#define FR_FLAG_CAMERA_GRAD 16

/* fr_backward only: FR_FLAG_ACCUMULATE(k) makes the k-th array of fr_grads (k = position of the pointer in the
 * struct: 0 = dL_dmeans2D ... 7 = dL_drotations) ACCUMULATE: the frame's gradient is added to what the array holds
 * instead of overwriting it (culled Gaussians then touch nothing).  A batch of frames rendered from the same
 * parameters (the reference's batch loop, model/fateavatar.py:251-276, whose gradients autograd sums with one add
 * kernel and one temporary per frame and parameter) accumulates in one buffer: first frame without the flag, the
 * others with it.  FR_FLAG_ACCUMULATE_ALL = every array. */
#define FR_FLAG_ACCUMULATE_SHIFT 8
#define FR_FLAG_ACCUMULATE(k) (1 << (FR_FLAG_ACCUMULATE_SHIFT + (k)))
#define FR_FLAG_ACCUMULATE_ALL (0xFF << FR_FLAG_ACCUMULATE_SHIFT)

/* Device pointers.  NULL = the "empty tensor" of the reference glue
 * (rasterize_points.cu:94-103 passes data_ptr() of empty tensors; kernels branch on nullptr). */
typedef struct fr_inputs {
    const float* background;     /* [3] */
    const float* means3D;        /* [P,3] */
    const float* shs;            /* [P,M,3] or NULL */
    const float* colors_precomp; /* [P,3]   or NULL (exactly one of shs / colors_precomp) */
    const float* opacities;      /* [P] */
    const float* scales;         /* [P,3]   or NULL */
    const float* rotations;      /* [P,4]   or NULL (r,x,y,z; not normalised in-kernel) */
    const float* cov3D_precomp;  /* [P,6]   or NULL (exactly one of scales+rotations / cov3D_precomp) */
    const float* viewmatrix;     /* [16] row-major "transposed" world->view (camera_3dgs.py:53) */
    const float* projmatrix;     /* [16] full projection, same convention (camera_3dgs.py:71) */
    const float* campos;         /* [3] */
} fr_inputs;

/* Gradient outputs of fr_backward (device pointers).  Every non-NULL array is fully written
 * (rows of culled Gaussians are zero), so the caller may pass uninitialised memory; the
 * reference instead requires nine zero-filled tensors (rasterize_points.cu:151-159).
 * NULL = not wanted. */
typedef struct fr_grads {
    float* dL_dmeans2D;   /* [P,3] screen-space mean gradient, NDC-scaled, z = 0 (backward.cu:545-546) */
    float* dL_dcolors;    /* [P,3] */
    float* dL_dopacity;   /* [P]   */
    float* dL_dmeans3D;   /* [P,3] */
    float* dL_dcov3D;     /* [P,6] */
    float* dL_dsh;        /* [P,M,3] */
    float* dL_dscales;    /* [P,3] */
    float* dL_drotations; /* [P,4] */
} fr_grads;

/* What the binning stages report for a frame. */
typedef struct fr_counts {
    uint32_t num_rendered;   /* reference semantics: sum over Gaussians of 16x16 tiles touched */
    uint32_t num_instances;  /* (8x8 tile, Gaussian) instances this implementation bins and sorts */
    uint32_t max_tile_list;  /* longest per-tile list */
    uint32_t overflow;       /* 1 if num_instances exceeded the binning capacity */
} fr_counts;

int fr_create(fr_handle** out);
int fr_destroy(fr_handle* h);
const char* fr_last_error(void);
const char* fr_version(void);

/* Stage timing.  While enabled, every kernel launch of fr_forward / fr_backward is bracketed by HIP
 * events on the stream it is launched on; fr_profile_read sums the elapsed time of one stage over all
 * launches since fr_profile_enable(h, 1) (the stream must have been synchronised by the caller).
 * stage: 0 preprocess_fwd (+ key binning), 1 scan (per-tile totals and range allocation), 2 emit (no launch any more:
 * the preprocess kernel writes the keys), 3 tile_sort, 4 blend_fwd, 5 blend_bwd, 6 preprocess_bwd. */
int fr_profile_enable(fr_handle* h, int32_t on);
int fr_profile_read(fr_handle* h, int32_t stage, double* total_ms, uint32_t* launches);

/* Scratch sizes in bytes.  geometry: per-Gaussian state + gradient accumulators; image: per-pixel
 * final transmittance / contributor count and per-tile ranges; binning: `capacity` instances. */
size_t fr_geometry_bytes(int32_t P);
size_t fr_image_bytes(int32_t W, int32_t H);
size_t fr_binning_bytes(uint64_t capacity, int32_t W, int32_t H);
/* fr_aux::planes of a frame with FR_FLAG_DEPTH_ALPHA whose binning buffer holds `capacity` instances: 512 bytes per blend
 * unit (capacity / 64 + tiles + 1 of them), plus alignment.  Regrow it with the binning buffer. */
size_t fr_planes_bytes(uint64_t capacity, int32_t W, int32_t H);
/* fr_aux_camera::camera_workspace of a backward with FR_FLAG_CAMERA_GRAD (a constant: counters and per-workgroup partial sums). */
size_t fr_camera_grad_workspace_bytes(void);

/* out_color [3,H,W], radii [P] (reference semantics: ceil(3*sigma_max), 0 if culled).
 * Returns FR_OK, or FR_ERR_BINNING_CAPACITY with counts->num_instances = capacity required
 * (outputs are then undefined and the call must be repeated with a larger binning buffer). */
int fr_forward(fr_handle* h, const fr_params* prm, const fr_inputs* in, float* out_color, int32_t* radii,
               void* geometry, void* image, void* binning, uint64_t binning_capacity, fr_counts* counts,
               void* hip_stream);

/* Counts of the most recent frame enqueued through this handle (valid once its stream has been synchronised). */
int fr_read_counts(fr_handle* h, fr_counts* counts);

/* geometry/image/binning: the buffers a successful fr_forward of the same frame filled.
 * dL_dpix [3,H,W]. */
int fr_backward(fr_handle* h, const fr_params* prm, const fr_inputs* in, const int32_t* radii, void* geometry,
                const void* image, const void* binning, const float* dL_dpix, const fr_grads* grads,
                void* hip_stream);

/* ---- several views through ONE launch chain (SURVEY.md §8e / reference model/fateavatar.py:251-276: the frames of a
 * batch are rendered one after the other with shared Gaussians; one frame's kernels leave most of an MI355X idle).
 * fr_forward_batch / fr_backward_batch do exactly what n_views calls of fr_forward / fr_backward would — every view has
 * its own handle, parameter block, inputs (which may or may not share pointers), outputs and scratch buffers, and the
 * results are the same bit for bit (the forward) resp. to atomic-summation order (the backward) — but every kernel of
 * the frame is launched once with a (grid, n_views) grid, so that the views fill the chip together without any stream
 * or hardware-queue arrangement on the caller's side.  1 <= n_views <= FR_MAX_BATCH; batched views need P > 0, distinct
 * handles and the default forward path (FR_BLEND_FWD unset).  `counts` (may be NULL): n_views entries.  Returns
 * FR_ERR_BINNING_CAPACITY if ANY view overflowed its binning capacity (counts[k].overflow says which). */
#define FR_MAX_BATCH 4
int fr_forward_batch(int32_t n_views, fr_handle* const* handles, const fr_params* const* prm, const fr_inputs* const* in,
                     float* const* out_color, int32_t* const* radii, void* const* geometry, void* const* image,
                     void* const* binning, const uint64_t* binning_capacity, fr_counts* counts, void* hip_stream);
int fr_backward_batch(int32_t n_views, fr_handle* const* handles, const fr_params* const* prm, const fr_inputs* const* in,
                      const int32_t* const* radii, void* const* geometry, const void* const* image,
                      const void* const* binning, const float* const* dL_dpix, const fr_grads* const* grads,
                      void* hip_stream);

/* ---- fused Adam over a flat parameter buffer (replaces torch.optim.Adam.step() over the
 * Gaussian parameter groups of train/optim.py:11-37: betas (0.9, 0.999), eps 1e-8, no weight decay, no amsgrad).
 * The buffer is cut into up to FR_ADAM_MAX_SEGMENTS consecutive segments, each with its own learning rate (the
 * reference's param groups); param / grad / exp_avg / exp_avg_sq are device arrays of n floats with the same
 * layout.  `state` is a device array of FR_ADAM_STATE_FLOATS floats owned by the caller, 8-byte aligned, zero-initialised
 * once: {step, 1 - beta1^step, 1 - beta2^step, unused, the same two corrections as DOUBLES in words 4..7 (the values the
 * kernel carries forward: save and restore words 0..7 together), ..., kernel bookkeeping from word 32 on that is zero
 * between calls}; every call advances it on the device (so the call is hipGraph-capturable: nothing step-dependent is a kernel argument) and applies
 *   m = b1 m + (1-b1) g;  v = b2 v + (1-b2) g^2;  p -= lr / (1 - b1^t) * m / (sqrt(v) / sqrt(1 - b2^t) + eps)
 * with g = grad_scale * grad (grad_scale: e.g. 1/world_size after a SUM all-reduce). */
#define FR_ADAM_MAX_SEGMENTS 16
#define FR_ADAM_STATE_FLOATS 576
typedef struct fr_adam_config {
    int32_t n_segments;
    uint64_t segment_end[FR_ADAM_MAX_SEGMENTS]; /* exclusive end offset (in floats) of each segment, ascending; last == n */
    float segment_lr[FR_ADAM_MAX_SEGMENTS];
    /* optional two-rate pattern inside a segment (SH coefficients stored [P,M,3] with the DC term at lr and the
     * rest at lr/20, train/optim.py:49-50): element e (relative to the segment start) uses segment_lr if
     * e % segment_period < segment_split, else segment_lr2.  segment_period == 0: segment_lr everywhere. */
    uint32_t segment_period[FR_ADAM_MAX_SEGMENTS];
    uint32_t segment_split[FR_ADAM_MAX_SEGMENTS];
    float segment_lr2[FR_ADAM_MAX_SEGMENTS];
    double beta1, beta2, eps; /* doubles, like torch's hyper-parameters: 1 - beta is rounded to float from here */
    float grad_scale;
    /* optional: n_skip (0 .. FR_ADAM_MAX_GRADS) device floats; if ANY of them is non-zero when the kernel runs the step does
     * nothing — no parameter, no moment, no step count changes.  Point them at the fr_aux::overflow_out words of the frames
     * whose gradients feed this step; in a data-parallel step keep those words behind the gradients in the exchanged buffer,
     * so that the all-reduce sums them and every rank skips the same steps. */
    const float* skip[4 /* FR_ADAM_MAX_GRADS */];
    int32_t n_skip;
} fr_adam_config;
int fr_adam_step(const fr_adam_config* cfg, float* param, const float* grad, float* exp_avg, float* exp_avg_sq,
                 uint64_t n, float* state, void* hip_stream);
/* The same step with the gradient given as the SUM of n_grads (1 .. FR_ADAM_MAX_GRADS) buffers of n floats: the views of
 * a batch (the reference's `for bs_ in range(bs)` loop, model/fateavatar.py:251-276) each back-propagate into their own
 * buffer, in flight together; grad_scale = 1 / (views x ranks) makes it the batch mean of train/loss.py:92-105. */
#define FR_ADAM_MAX_GRADS 4
int fr_adam_step_multi(const fr_adam_config* cfg, float* param, const float* const* grads, int32_t n_grads,
                       float* exp_avg, float* exp_avg_sq, uint64_t n, float* state, void* hip_stream);

/* ---- the image loss of the optimisation step (reference nn.L1Loss(reduction='mean') on the rendered
 * image, model/loss.py:92, followed by loss.backward()): loss = mean |img - gt| and grad = sign(img - gt) / n (what
 * autograd hands to the rasterizer's backward for a unit upstream gradient) in ONE launch.  `grad` may be NULL.
 * `workspace`: fr_l1_workspace_bytes() bytes of device memory, zeroed ONCE by the caller (the kernel leaves it zeroed).
 * A workspace must NOT be shared by launches that can overlap on the device (other streams, other graphs): the kernel
 * elects its last workgroup and sums per-workgroup partials through it;
 * `loss`: one device float.  All arrays on the device, n floats each. */
size_t fr_l1_workspace_bytes(void);
int fr_l1_loss_grad(uint64_t n, const float* img, const float* gt, float* grad, float* loss, void* workspace,
                    void* hip_stream);
/* The same for the n_images (1 .. FR_MAX_BATCH) images of the frames of a batch (n floats each; the reference's batch loop,
 * model/fateavatar.py:251-276 with train/loss.py:92-105) in ONE launch: image k has its own gt / grad / loss / workspace
 * (distinct workspaces).  `grad` may be NULL (no gradients), or hold NULL entries. */
int fr_l1_loss_grad_batch(int32_t n_images, uint64_t n, const float* const* img, const float* const* gt, float* const* grad,
                          float* const* loss, void* const* workspace, void* hip_stream);

/* ---- L1 + D-SSIM image loss and its gradient with respect to the rendered image in TWO launches (reference:
 * GaussianAvatarsLoss, train/loss.py:351-365, with rgb_weight 0.8 and dssim_weight 0.2 of config/gaussianavatars.yaml:16-20 —
 * the original 3DGS objective; d_ssim is tools/loss_utils/dssim.py:28-56: five grouped F.conv2d with an 11 x 11 Gaussian
 * window of sigma 1.5, zero padding 5, a dozen elementwise kernels, and autograd's backward of all of them):
 *   loss[0] = rgb_weight * loss[1] + dssim_weight * loss[2],  loss[1] = mean |img - gt|,  loss[2] = 1 - mean(ssim_map)
 *   grad    = rgb_weight * sign(img - gt) / N + dssim_weight * d loss[2] / d img,         N = C H W
 * for n_images (1 .. FR_MAX_BATCH) images of C x H x W floats each, every image with its own gt / grad / loss (3 device
 * floats) / workspace (distinct).  `grad` may be NULL, or hold NULL entries: losses only for those images.  The first launch
 * stores three derivative maps of the SSIM map in the workspace and reduces the two sums, the second convolves the maps and
 * writes the gradient (one plain store per pixel); no float atomics, the results are bit-reproducible from launch to launch.
 * A dssim_weight of 0 runs fr_l1_loss_grad's kernel alone: gradient and loss[1] are that entry's, bit for bit (for an
 * rgb_weight of 1), loss[2] is 0; the image arrays must then be 16-byte aligned.
 * `workspace`: fr_image_loss_workspace_bytes(C, H, W) bytes of device memory, 16-byte aligned: counters and per-workgroup
 * partial sums, zeroed ONCE by the caller and left zeroed by the kernels, in front of 12 C H W bytes for the maps, which
 * are written before they are read and need no initial value.  Not to be shared by launches that can overlap on the device.
 * fr_ssim_window: the eleven 1-D taps in the reference's float32 arithmetic (dssim.py:18-20); host only, as is the size query. */
typedef struct fr_image_loss_config {
    float rgb_weight, dssim_weight;       /* reference: 0.8, 0.2 (config/gaussianavatars.yaml) */
} fr_image_loss_config;
void fr_ssim_window(float out[11]);
size_t fr_image_loss_workspace_bytes(int32_t C, int32_t H, int32_t W);
int fr_image_loss_grad(const fr_image_loss_config* cfg, int32_t n_images, int32_t C, int32_t H, int32_t W,
                       const float* const* img, const float* const* gt, float* const* grad, float* const* loss,
                       void* const* workspace, void* hip_stream);

/* ---- FlashAvatar's Huber image term and its gradient with respect to the rendered image in ONE launch (reference:
 * FlashAvatarLoss.get_huber_loss and accumulate_gradients, train/loss.py:217-221, :231-239, with alpha 0.1 and the mouth term's
 * weight 40).  With d = img - gt over the n = C H W floats of an image and
 *   h(x) = 0.5 x^2 if |x| < alpha else alpha (|x| - 0.5 alpha),     h'(x) = x if |x| < alpha else alpha sign(x)
 * and `mask` [H*W] (any values in [0,1]; broadcast over the C channels; NULL: no mouth term):
 *   loss[1] = mean_n h(d),   loss[2] = mean_n h(mask * d)  (0 without a mask),   loss[0] = loss[1] + mask_weight * loss[2]
 *   grad    = (h'(d) + mask_weight * mask * h'(mask * d)) / n          (`grad` may be NULL: losses only)
 * h is C1, so nothing flips at |x| = alpha.  One launch of float4 pieces plus a tail, two per-workgroup partial sums added up in
 * index order by the workgroup that finishes last: no float atomics, the same bits on every run.  `workspace`:
 * fr_huber_workspace_bytes() bytes of device memory, zeroed ONCE by the caller and left zeroed by the kernel; not to be shared
 * by launches that can overlap on the device.  No allocation, no synchronisation: the call can be captured in a graph.  img, gt
 * and grad must be 16-byte aligned (mask need not be).  n == 0 launches nothing and leaves `loss` as it is.  A NULL cfg / img /
 * gt / loss / workspace, or alpha <= 0, is FR_ERR_INVALID_ARGUMENT.  `loss`: three device floats. */
typedef struct fr_huber_config {
    float alpha, mask_weight;             /* reference: 0.1, 40 (train/loss.py:231-239) */
} fr_huber_config;
size_t fr_huber_workspace_bytes(void);
int fr_huber_loss_grad(const fr_huber_config* cfg, int32_t C, int32_t H, int32_t W, const float* img, const float* gt,
                       const float* mask, float* grad, float* loss, void* workspace, void* hip_stream);

/* ---- SplattingAvatar's L1 + MSE image term and its gradient with respect to the rendered image in ONE launch (reference:
 * SplattingAvatarLoss.accumulate_gradients, train/loss.py:288-323, with get_rgb_loss / get_mse_loss :279-283 and rgb_loss 1.0,
 * mse_loss 10.0 of config/splattingavatar.yaml:13-20).  With d = img - gt over the n = C H W floats of an image:
 *   loss[1] = mean_n |d|,   loss[2] = mean_n d^2,   loss[0] = rgb_weight * loss[1] + mse_weight * loss[2]
 *   grad    = rgb_weight * sign(d) / n + mse_weight * 2 d / n     (sign(0) = 0; `grad` may be NULL: losses only)
 * One launch of float4 pieces plus a tail, two per-workgroup partial sums added up in index order by the workgroup that
 * finishes last: no float atomics, the same bits on every run.  The L1 sum takes its addends in fr_l1_loss_grad's order:
 * loss[1] is that entry's loss, bit for bit.  `workspace`: fr_pixel_loss_workspace_bytes() bytes of device memory, zeroed ONCE
 * by the caller and left zeroed by the kernel; not to be shared by launches that can overlap on the device.  No allocation, no
 * synchronisation: the call can be captured in a graph.  img, gt and grad must be 16-byte aligned.  n == 0 launches nothing and
 * leaves `loss` as it is.  A NULL cfg / img / gt / loss / workspace is FR_ERR_INVALID_ARGUMENT.  `loss`: three device floats. */
typedef struct fr_pixel_loss_config {
    float rgb_weight, mse_weight;         /* reference: 1.0, 10.0 (config/splattingavatar.yaml:13-20) */
} fr_pixel_loss_config;
size_t fr_pixel_loss_workspace_bytes(void);
int fr_pixel_loss_grad(const fr_pixel_loss_config* cfg, int32_t C, int32_t H, int32_t W, const float* img, const float* gt,
                       float* grad, float* loss, void* workspace, void* hip_stream);

/* ---- SplattingAvatar's scale term and its gradient in TWO launches (reference: SplattingAvatarLoss.get_scale_loss,
 * train/loss.py:307-315, on get_scaling = exp(_scaling), model/baseline/splattingavatar.py:270).  `scaling`: P rows of 3 raw
 * floats.  With scale = exp(scaling), smax / smin a row's largest / smallest component:
 *   selected   = smax > max_scaling  and  smax / smin > scale_threshold
 *   loss[0]    = mean of smax over the selected rows (0 if there is none),   loss[1] = their number (an exact integer)
 * both UNWEIGHTED, and `weight * smax / loss[1]` is ADDED to d_scaling[row][argmax] of every selected row (read-modify-write
 * by the lane that owns the row, no atomics; the first of equal components takes it).  The first launch reduces sum and
 * count (per-workgroup partials summed in index order by the workgroup that finishes last: the same bits on every run) and
 * stores `loss`; the second recomputes the selection with the same device function and reads the stored count.  A row with
 * a NaN scale is not selected and its gradient row not touched; with no row selected `d_scaling` is not touched and no 0 / 0
 * is evaluated.  `d_scaling` NULL or a weight of 0: the second launch is not made (no gradient traffic).  `workspace`:
 * fr_scale_term_workspace_bytes() bytes of device memory, zeroed ONCE by the caller; the kernel leaves it zeroed; not to be
 * shared by launches that can overlap on the device.  No allocation, no synchronisation: the call can be captured in a graph.
 * P == 0 launches nothing and leaves `loss` as it is; P >= 2^24 is FR_ERR_INVALID_ARGUMENT (the count is summed in floats,
 * exact below that).  `loss`: two device floats. */
typedef struct fr_scale_term_config {
    float weight;                         /* reference: 1.0 (scale_loss, config/splattingavatar.yaml:13-20) */
    float scale_threshold, max_scaling;   /* reference: 10.0, 0.008 */
} fr_scale_term_config;
size_t fr_scale_term_workspace_bytes(void);
int fr_scale_term(const fr_scale_term_config* cfg, int32_t P, const float* scaling, float* d_scaling, float* loss,
                  void* workspace, void* hip_stream);

/* ---- FateAvatar's scale-ratio term and its gradient in ONE launch (reference: FateAvatarLoss.accumulate_gradients,
 * train/loss.py:144-151, on model_outputs['scale'] = exp(_scaling), the RAW parameter, model/fateavatar.py:282).  `scaling`: P
 * rows of 3 raw floats.  With scale = exp(scaling), smax / smin a row's largest / smallest component and ratio = smax / smin
 * (the float32 quotient, as the reference forms it):
 *   loss[0] = mean over ALL P rows of relu(ratio - scale_threshold),   loss[1] = the rows with ratio > scale_threshold
 * both UNWEIGHTED (the count an exact integer), and for every such row `weight / P * ratio` is ADDED to d_scaling[row][argmax]
 * and SUBTRACTED from d_scaling[row][argmin] (read-modify-write by the lane that owns the row, no atomics; nothing anywhere
 * else).  Sub-gradients are autograd's: a ratio exactly at the threshold adds nothing; the FIRST of equal components takes
 * max's / min's gradient; where argmax == argmin (three equal components) the two contributions cancel to an exact 0.  A row
 * whose ratio is not finite (a NaN component, exp overflowing, the smallest component underflowing to 0) adds nothing to the
 * loss, the count or the gradient, where stock PyTorch would make the loss NaN or inf.  Per-workgroup partials summed in
 * index order by the workgroup that finishes last: the same bits on every run.  `d_scaling` NULL or a weight of 0: no
 * gradient traffic.  `workspace`: fr_scale_ratio_workspace_bytes() bytes of device memory, zeroed ONCE by the caller; the
 * kernel leaves it zeroed; not to be shared by launches that can overlap on the device.  No allocation, no synchronisation:
 * the call can be captured in a graph.  P == 0 launches nothing and leaves `loss` as it is; P >= 2^24 is
 * FR_ERR_INVALID_ARGUMENT (the count is summed in floats, exact below that).  `loss`: two device floats. */
typedef struct fr_scale_ratio_config {
    float weight;                         /* reference: 0.1 (scale_loss, config/fateavatar.yaml:13-25) */
    float scale_threshold;                /* reference: 9.0 */
} fr_scale_ratio_config;
size_t fr_scale_ratio_workspace_bytes(void);
int fr_scale_ratio_term(const fr_scale_ratio_config* cfg, int32_t P, const float* scaling, float* d_scaling, float* loss,
                        void* workspace, void* hip_stream);

/* ---- GaussianAvatars' two per-Gaussian regularisers and their gradients in ONE launch (reference:
 * GaussianAvatarsLoss.accumulate_gradients, train/loss.py:367-379, on the raw local parameters,
 * model/baseline/gaussianavatars.py:196-197):
 *   scale_loss = relu(exp(_scaling) - threshold_scale).norm(dim=1).mean()
 *   xyz_loss   = relu(_xyz.norm(dim=1) - threshold_xyz).mean()
 * `scaling`, `xyz`: P rows of 3 raw floats.  The kernel ADDS scale_weight * d scale_loss / d _scaling into `d_scaling`
 * [P,3] and xyz_weight * d xyz_loss / d _xyz into `d_xyz` [P,3] (read-modify-write by the lane that owns the row, no
 * atomics) with autograd's sub-gradients: a component with exp(s) <= threshold, a row whose clipped vector has norm 0 and
 * a row with |xyz| <= threshold add nothing; no division by a zero norm is evaluated.  A weight of 0 leaves that term's
 * array untouched (no traffic); either gradient pointer may be NULL (loss only).  `loss`: two device floats,
 * {scale_loss, xyz_loss}, UNWEIGHTED; bit-reproducible from launch to launch (per-workgroup partials summed in index order
 * by the workgroup that finishes last).  `workspace`: fr_regularise_workspace_bytes() bytes of device memory, zeroed ONCE
 * by the caller; the kernel leaves it zeroed; not to be shared by launches that can overlap on the device.  Nothing
 * depends on the step: the call can be captured in a graph.  P == 0 launches nothing and leaves `loss` as it is. */
typedef struct fr_regularise_config {
    float scale_weight, xyz_weight;       /* reference: 1.0, 0.01 (config/gaussianavatars.yaml) */
    float threshold_scale, threshold_xyz; /* reference: 0.6, 1.0 */
} fr_regularise_config;
size_t fr_regularise_workspace_bytes(void);
int fr_gaussian_regularise(const fr_regularise_config* cfg, int32_t P, const float* scaling, const float* xyz,
                           float* d_scaling, float* d_xyz, float* loss, void* workspace, void* hip_stream);

/* ---- FateAvatar's two mesh terms and their gradient with respect to the posed vertices in ONE launch (reference:
 * FateAvatarLoss.get_laplacian_smoothing_loss and flame_loss, train/loss.py:112-121, :166-180, :192-197, where the uniform
 * Laplacian is a dense V x V matrix applied with bmm).  `row_ptr` [V+1], `col` [row_ptr[V]]: the mesh's adjacency in CSR
 * form, every row ascending and duplicate-free, symmetric (j in row i <=> i in row j), no self-edges; L[i,i] = -1 for every
 * vertex, L[i,j] = 1 / deg(i) for a neighbour j (pytorch3d's Meshes.laplacian_packed()).  With d = verts - verts_orig
 * ([V,3] floats each) and r = L d:
 *   loss[0] = (1/V) sum_i |r_i|^2      ((L verts - L verts_orig)^2 .sum(-1, keepdim=True).mean())
 *   loss[1] = mean over the 3 V entries of d^2
 * both UNWEIGHTED, and the kernel ADDS into `d_verts` [V,3]
 *   laplacian_weight * (2/V) * (-r_i + sum_{j in N(i)} r_j / deg(j)) + flame_weight * (2/(3V)) * d_i
 * by a read-modify-write of the lane that owns the row (it recomputes its neighbours' r_j: no atomics, no second launch).
 * A weight of 0 skips that term's gradient arithmetic; with both weights 0 `d_verts` is not touched; `d_verts` may be NULL
 * (losses only).  An empty row (a vertex no face uses) has r_i = -d_i and divides by nothing.  The losses are
 * bit-reproducible from launch to launch (per-workgroup partials summed in index order by the workgroup that finishes last).
 * `workspace`: fr_mesh_terms_workspace_bytes() bytes of device memory, zeroed ONCE by the caller; the kernel leaves it
 * zeroed; not to be shared by launches that can overlap on the device.  The call can be captured in a graph.  V == 0
 * launches nothing and leaves `loss` as it is.  The kernel cannot validate the CSR arrays: that is the caller's side
 * (binding.mesh_laplacian). */
typedef struct fr_mesh_terms_config {
    float laplacian_weight, flame_weight; /* reference: 1e5, 0 (config/fateavatar.yaml:23) */
} fr_mesh_terms_config;
size_t fr_mesh_terms_workspace_bytes(void);
int fr_mesh_terms(const fr_mesh_terms_config* cfg, int32_t V, const float* verts, const float* verts_orig,
                  const int32_t* row_ptr, const int32_t* col, float* d_verts, float* loss, void* workspace, void* hip_stream);

/* ---- dst = scale * (src[0] + ... + src[n_src - 1]), n_src in 1 .. FR_ADAM_MAX_GRADS arrays of `count` floats, 16-byte
 * aligned: the mean of the gradient buffers of the views a rank rendered in flight together, written into the exchange
 * buffer of the data-parallel all-reduce in one pass.  dst may be one of the sources. */
int fr_scaled_sum(int32_t n_src, const float* const* src, float* dst, uint64_t count, float scale, void* hip_stream);

/* ---- up to FR_COPY_MAX_SEGMENTS device-to-device copies of float arrays in one launch (the per-frame inputs of a
 * captured step: camera block, posed vertices, target image).  Segments must not overlap each other. */
#define FR_COPY_MAX_SEGMENTS 12
int fr_multi_copy(int32_t n_segments, float* const* dst, const float* const* src, const uint64_t* count, void* hip_stream);

/* ---- FateAvatar's mesh binding (reference model/fateavatar.py:225-258 with
 * volume_rendering/mesh_compute.py:27-59 and pytorch3d's matrix_to_quaternion / quaternion_multiply): from the posed
 * mesh and each Gaussian's binding (face index, barycentrics) and raw parameters to what the reference assigns to
 * gaussian._xyz / _rotation / _scaling before render():
 *   xyz = sum_k bary_k v_k + (e1 x e2) * shell_len * tanh(offset);  rotation = standardize(q_face (x) rotation);
 *   scaling = scaling + log(face_scale / face_scale_canonical)   (resize_scale != 0; unchanged otherwise).
 * All pointers are device pointers; one frame per call.
 *
 * fr_binding::mode selects the binding; a zeroed field is FR_BIND_SHELL, the one above.  FR_BIND_FACE_LOCAL is
 * GaussianAvatars' (model/baseline/gaussianavatars.py:144-171): with R = [a0 a1 a2] the face's frame, s its scale and c
 * the mean of its three vertices,
 *   xyz = (R local_xyz) * s + c;  rotation = standardize(normalize(q_face) (x) rotation);  scaling = scaling + log(s)
 * (normalize: q / max(|q|, 1e-12)).  bary, offset, face_scale_canonical, shell_len and resize_scale are then ignored and
 * may be NULL / zero; local_xyz is required.
 *
 * FR_BIND_PHONG is SplattingAvatar's (model/baseline/splattingavatar.py:224-246): a point of the posed mesh's Phong surface.
 * With b = bary and i_k the corners of the Gaussian's face f,
 *   xyz = sum_k b_k verts[i_k] + normalize(sum_k b_k vert_normals[i_k]) * uvd[2]      (:224-233, :246; normalize: eps 1e-12)
 *   rotation = standardize((sum_k b_k vert_quats[i_k]) (x) rotation)                   (:235, :245; the sum is not normalised)
 *   scaling = scaling * face_ratio[f]                                                  (:237, :244: the raw log-scale is MULTIPLIED)
 * vert_normals / vert_quats / face_ratio are fr_phong_frame's outputs for the posed mesh; they travel in struct fr_binding_phong
 * (below), which extends the descriptor for this mode.  The per-Gaussian parameter uvd
 * [N,3] travels in the `local_xyz` member (and its gradient in the backward's d_local_xyz slot): only its third column is
 * read, and the first two columns of its gradient are written as zeros — walking a Gaussian over the mesh (the reference's
 * CPU submodule simple_phongsurf) is outside this library.  face_index, bary, rotation, scaling, local_xyz and the three
 * fr_phong_frame arrays are required; offset, face_scale_canonical, shell_len and resize_scale are ignored.  fr_backward and
 * fr_bind_backward_phong hand NO gradient to the posed vertices in this mode: a d_verts request there is
 * FR_ERR_INVALID_ARGUMENT.  The vertex gradient is two calls of its own, fr_bind_backward_phong_frame and
 * fr_phong_frame_backward (below).
 *
 * FR_BIND_DEFORM is FlashAvatar's (model/baseline/flashavatar.py:242-276, :380-390): the barycentric point moved, turned and
 * stretched by the ten outputs of the caller's deformation MLP for this Gaussian in this frame.  With t = tanh(deform[n]),
 *   xyz = sum_k b_k verts[i_k] + t[0:3]
 *   rotation = rotation (x) (exp(t[3]), t[4], t[5], t[6])      (the Hamilton product as it comes: the PARAMETER is the first
 *                                                               factor and the sign is NOT standardised, quatProduct_batch)
 *   scaling = scaling * exp(t[7:10])                            (the raw log-scale is MULTIPLIED, as in FR_BIND_PHONG)
 * The RAW deform array [N,10] travels in the `local_xyz` member, and its gradient [N,10] in the backward's d_local_xyz slot
 * (fr_aux::d_local_xyz, fr_bind_backward_deform's d_deform): all ten columns are read and written.  face_index, bary,
 * local_xyz, rotation and scaling are required; offset, face_scale_canonical, shell_len and resize_scale are ignored.  The
 * mode HAS a vertex gradient: d_verts[i_k] += b_k g_xyz.
 *
 * The value 3 is unassigned: a descriptor that carries it is refused like any other unknown mode. */
#define FR_BIND_SHELL 0
#define FR_BIND_FACE_LOCAL 1
#define FR_BIND_PHONG 2
#define FR_BIND_DEFORM 4
struct fr_binding {
    int32_t N, V, F;
    const float* verts;                 /* [V,3] posed vertices */
    const int32_t* faces;               /* [F,3] */
    const int32_t* face_index;          /* [N]   face every Gaussian is bound to */
    const float* bary;                  /* [N,3] barycentric coordinates */
    const float* face_scale_canonical;  /* [F]   fr_face_scale of the canonical mesh */
    float shell_len;                    /* cfg_model.normal_offset */
    int32_t resize_scale;
    const float* offset;                /* [N]   raw: tanh is applied here */
    const float* rotation;              /* [N,4] raw quaternion (r,x,y,z) */
    const float* scaling;               /* [N,3] raw log-scale */
    int32_t mode;                       /* FR_BIND_* (appended: a descriptor that ends above, zero-filled, is a shell binding) */
    const float* local_xyz;             /* [N,3] FR_BIND_FACE_LOCAL: position in the face's frame; FR_BIND_PHONG: uvd;
                                         * [N,10] FR_BIND_DEFORM: the raw outputs of the deformation MLP */
};
/* The descriptor of a FR_BIND_PHONG binding: fr_binding with the mode's three arrays behind it.  Wherever a `const fr_binding*`
 * is taken (fr_bind_forward, fr_bind_backward_phong, fr_aux::binding) a descriptor whose mode is FR_BIND_PHONG MUST be the
 * `base` member of one of these — the functions read the tail through that pointer.  fr_binding itself is unchanged: the two
 * other modes neither carry nor read a tail. */
typedef struct fr_binding_phong {
    struct fr_binding base;             /* mode = FR_BIND_PHONG, bary, uvd in local_xyz */
    const float* vert_normals;          /* [V,3] fr_phong_frame's outputs for the posed mesh */
    const float* vert_quats;            /* [V,4] */
    const float* face_ratio;            /* [F]   */
} fr_binding_phong;
int fr_face_scale(int32_t V, int32_t F, const float* verts, const int32_t* faces, float* out_scale, void* hip_stream);
int fr_bind_forward(const fr_binding* b, float* xyz, float* rotation_out, float* scaling_out, void* hip_stream);
/* Gradients of the three outputs in, gradients of offset / rotation / scaling out (fully written), and dL/dverts
 * ADDED into d_verts [V,3] with float atomics (the caller zeroes it).  Any of the seven arrays may be NULL. */
int fr_bind_backward(const fr_binding* b, const float* g_xyz, const float* g_rotation, const float* g_scaling,
                     float* d_verts, float* d_offset, float* d_rotation, float* d_scaling, void* hip_stream);
/* The same for a FR_BIND_FACE_LOCAL binding (any other mode is FR_ERR_INVALID_ARGUMENT): d_local_xyz [N,3] where the shell
 * binding has d_offset. */
int fr_bind_backward_local(const fr_binding* b, const float* g_xyz, const float* g_rotation, const float* g_scaling,
                           float* d_verts, float* d_local_xyz, float* d_rotation, float* d_scaling, void* hip_stream);
/* The same for a FR_BIND_PHONG binding (any other mode is FR_ERR_INVALID_ARGUMENT): d_uvd [N,3] = (0, 0, g_xyz . n_hat),
 * d_rotation through the quaternion product, d_scaling = g_scaling * face_ratio[f].  d_verts must be NULL (the argument keeps
 * the three entry points' shape): the mode has no vertex gradient. */
int fr_bind_backward_phong(const fr_binding* b, const float* g_xyz, const float* g_rotation, const float* g_scaling,
                           float* d_verts, float* d_uvd, float* d_rotation, float* d_scaling, void* hip_stream);
/* The same for a FR_BIND_DEFORM binding (any other mode is FR_ERR_INVALID_ARGUMENT): d_deform [N,10] through tanh, the
 * quaternion product and the two exponentials, d_rotation through the product, d_scaling = g_scaling * exp(t[7:10]), and
 * b_k g_xyz ADDED into d_verts [V,3] at the face's three corners. */
int fr_bind_backward_deform(const fr_binding* b, const float* g_xyz, const float* g_rotation, const float* g_scaling,
                            float* d_verts, float* d_deform, float* d_rotation, float* d_scaling, void* hip_stream);
/* SplattingAvatar's per-frame mesh pass (model/baseline/splattingavatar.py `forward` :203-215, `PerVertQuaternion` :819-902,
 * `calc_face_areas` :781-791, `tbn` :756-765, `calc_per_face_Rt` :795-802) for FR_BIND_PHONG, from the posed verts [V,3], the
 * canonical cano_verts [V,3], faces [F,3], the vertex -> face incidence list in CSR form (vf_offsets [V+1], vf_faces [3F],
 * ascending within a row) and the canonical face areas face_area_canonical [F] (|cross(v2 - v1, v0 - v1)| / 2):
 *   face_ratio [F]     = (area_posed + 1e-4) / (area_canonical + 1e-4)                                   (:899-902)
 *   vert_normals [V,3] = normalize(sum over the vertex's faces of cross(v2 - v1, v0 - v1), eps 1e-6)     (:206, pytorch3d's
 *                        verts_normals_packed)
 *   vert_quats [V,4]   = normalize(sum of area_canonical[f] * q_f, eps 1e-6),  q_f = matrix_to_quaternion(R_posed,f R_cano,f^T)
 *                        with R = tbn(triangle) (:846-881; the reference inverts [R|T] with torch.inverse: tbn is orthonormal)
 * One launch on hip_stream, no allocation, no synchronisation (capturable), and no float atomics: every vertex gathers its
 * faces in the list's order, so the result is the same bits on every run.  Its backward is fr_phong_frame_backward (below). */
int fr_phong_frame(int32_t V, int32_t F, const float* verts, const float* cano_verts, const int32_t* faces,
                   const int32_t* vf_offsets, const int32_t* vf_faces, const float* face_area_canonical, float* vert_normals,
                   float* vert_quats, float* face_ratio, void* hip_stream);

/* ---- The vertex gradient of the FR_BIND_PHONG path: two separate calls behind the ones above, which stay as they are
 * (fr_bind_backward_phong and fr_backward with fr_aux::d_verts keep refusing a d_verts request in that mode: the gradient
 * toward the posed mesh is asked for HERE).  The reference has it from autograd through splattingavatar.py:203-246.
 *
 * fr_bind_backward_phong_frame: per Gaussian n on face f with corners i_k, barycentrics b_k, d = uvd[n,2],
 * nb = sum_k b_k vert_normals[i_k], n_hat = nb / max(|nb|, 1e-12), from the gradients of the bound values:
 *   d_verts[i_k]        += b_k g_xyz
 *   d_vert_normals[i_k] += b_k d (g_xyz - n_hat (n_hat . g_xyz)) / max(|nb|, 1e-12)
 *   d_vert_quats[i_k]   += b_k dq,   dq = the gradient of the quaternion product w.r.t. its first factor sum_k b_k vert_quats[i_k]
 *   d_face_ratio[f]     += sum_c g_scaling[n,c] scaling[n,c]
 * ADDED with float atomics into arrays the caller zeroed ([V,3], [V,3], [V,4], [F]).  Any g_* may be NULL (zero), any output
 * may be NULL.  `b` is the `base` of an fr_binding_phong; any other mode is FR_ERR_INVALID_ARGUMENT.  One launch.
 *
 * fr_phong_frame_backward: the backward of fr_phong_frame.  It takes that call's inputs and the gradients of its three outputs
 * (each may be NULL: zero) and ADDS dL/dverts onto d_verts [V,3] — the thread that owns a vertex reads, adds and stores, so it
 * composes with the call above on the same stream.  Through F.normalize(eps=1e-6) of the per-vertex sums, the face cross
 * product (vertex normals and area ratio), matrix_to_quaternion's selected candidate, M = R_posed R_cano^T and tbn of the posed
 * triangle; the canonical mesh is constant.  Two launches: per vertex the gradients of the two unnormalised sums into
 * `workspace` (fr_phong_frame_backward_workspace_bytes(V, F) bytes, 7 floats per vertex), then per vertex a gather over its
 * incidence row.  No float atomics: the same bits on every launch and graph replay.  A vertex that belongs to no face is not
 * touched.  Neither call allocates, synchronises or copies (capturable). */
int fr_bind_backward_phong_frame(const fr_binding* b, const float* g_xyz, const float* g_rotation, const float* g_scaling,
                                 float* d_verts, float* d_vert_normals, float* d_vert_quats, float* d_face_ratio, void* hip_stream);
size_t fr_phong_frame_backward_workspace_bytes(int32_t V, int32_t F);
int fr_phong_frame_backward(int32_t V, int32_t F, const float* verts, const float* cano_verts, const int32_t* faces,
                            const int32_t* vf_offsets, const int32_t* vf_faces, const float* face_area_canonical,
                            const float* d_vert_normals, const float* d_vert_quats, const float* d_face_ratio, float* d_verts,
                            void* workspace, void* hip_stream);

/* ---- SplattingAvatar's walk on the triangle mesh and Phong-surface fit (the reference's CPU submodule
 * submodules/simple_phongsurf/simple_phongsurf/).  All pointers are device pointers; no call allocates, synchronises or copies
 * to the host (capturable); no float atomics: the same inputs give the same bits on every run.  NOTE the stream comes FIRST.
 *
 * faces_nbr [F,3]: entry [f, j] describes the directed edge faces[f,j] -> faces[f,(j+1)%3]: 4 g + k of the face g and edge k that
 * carry the reversed edge, or -1 (initTriangleNeighbor, src/triangle_walk.cpp:176-237).
 *
 * fr_triwalk: Triwalk::updateSurfacePointsImpl (src/triangle_walk_py.cpp:62-79) around walkSurfacePoint / walkCrossEdge /
 * walkToNeighbor / finalize (src/triangle_walk.cpp:240-386), one thread per point: point i starts on face face_index[i] at
 * (u, v) = bary[i, :2] and is shifted by (delta[i * delta_stride], delta[i * delta_stride + 1]) barycentric units, crossing into
 * neighbouring faces with the remaining shift multiplied by `decay` (cross_triangle_decay, 0.9) per crossing.  face_index and
 * bary are updated in place; bary[i, 2] = 1 - u - v.  Precisions, tolerances and the `t12[0] <= 1.0` typo of :72 are the
 * reference's.  Where the reference's recursion would not end, the loop does, and counts it in status [4] (ADDED to; the
 * caller zeroes it): status[0] points stopped after 256 crossings; status[1] points whose resetBaryToInside (:165-173) did not
 * settle in two passes and were clamped; status[2] points left exactly as they were because their delta or barycentrics were
 * not finite or their face was out of range.
 *
 * fr_phong_fit: PhongSurfacePy3d.update_corres_spt (phongsurf_py3d.py:151-185) with method 'uvd', N = None, max_dist = inf:
 * outer_loop (1 .. 8) rounds of solve_delta_vwd (:256-309; at most inner_loop, 1 .. 512, iterations of torch.optim.Adam at
 * lr 0.01 on mean((10 V(uv + d) + 10 n_hat(uv + d) d_d - 10 q)^2), ended after the first iteration in which no point of the
 * batch moved by more than 5e-4) followed by the walk by d_uv.  Two launches per round: the first runs every trajectory and
 * counts the moving points per iteration into work[round * inner_loop + it], the second takes the stopping iteration from the
 * counters, runs the trajectories again up to it and walks.  work: int32 [outer_loop * inner_loop + 4], zeroed by the call
 * (the last four words are reserved); status[3] = the iteration count of the last round; status[0..2] as fr_triwalk.
 * delta_out [n,3] (may be NULL): the last round's (d_u, d_v, d_d), for tests. */
int fr_triwalk(void* hip_stream, const int32_t* faces_nbr, int32_t F, int32_t n, int32_t* face_index, float* bary,
               const float* delta, int32_t delta_stride, float decay, int32_t* status);
int fr_phong_fit(void* hip_stream, const float* cano_verts, const float* cano_normals, const int32_t* faces,
                 const int32_t* faces_nbr, int32_t V, int32_t F, int32_t n, const float* query, int32_t* face_index, float* bary,
                 int32_t outer_loop, int32_t inner_loop, float decay, int32_t* work, int32_t* status, float* delta_out);

/* ---- Gaussian attributes looked up in UV attribute maps: the per-frame front end of a BAKED FateAvatar (reference
 * model/uv_decoder.py:179-202, `UVSampling._texture_look_up`: F.grid_sample(texture, 2 uv - 1, mode="bilinear",
 * padding_mode="border", align_corners=True) once per attribute map, behind the per-texture activations of :133-156;
 * callers `_gather_attribute` :85-107, `_gather_attribute_from_texture_dict` :109-131, `UVDecoder.forward` :387-542,
 * `render_from_texture_dict` :564-690, `_export_avatar_model` :342-385).
 * Up to FR_TEX_MAX_LAYERS planar [C,H,W] float textures of ONE common H x W, C <= 4 each, are sampled at uv [N,2] in one
 * launch: out[n, c] = sum over the four corners of w * act(texture[c, y, x]), row-major [N,C].  u is x (width), v is y
 * (height), no flip; coordinates outside [0,1] clip to the border.  The activation is applied to the TEXEL (what activating
 * the whole texture and then sampling gives):
 *   FR_TEX_ACT_IDENTITY      t
 *   FR_TEX_ACT_TANH_SCALE    tanh(t) * a0                         (colour: a0 = 0.5 / C0, :134-138; offset: a0 = 1, :152-156)
 *   FR_TEX_ACT_SOFTPLUS_CAP  a1 - softplus(-(t + a0) + a1)        (scaling: a0 = mean, a1 = max, :140-149; softplus with
 *                                                                 torch's defaults: beta 1, linear above 20)
 * All pointers are device pointers.  No call allocates or synchronises: each can be captured in a HIP graph. */
#define FR_TEX_MAX_LAYERS 8
#define FR_TEX_ACT_IDENTITY 0
#define FR_TEX_ACT_TANH_SCALE 1
#define FR_TEX_ACT_SOFTPLUS_CAP 2
typedef struct fr_tex_layer {
    const float* texture;   /* [C,H,W] raw (not activated) texture */
    float* out;             /* forward:  [N,C] looked-up values */
    const float* d_out;     /* backward: [N,C] gradient of `out` */
    float* d_texture;       /* backward: [C,H,W] gradient of `texture`, every texel written */
    int32_t channels;       /* C: 1 .. 4 */
    int32_t activation;     /* FR_TEX_ACT_* */
    float a0, a1;
} fr_tex_layer;
/* corners[n, k] = texel index (y * W + x) of corner k of point n (k = 0 .. 3: (y0,x0), (y0,x1), (y1,x0), (y1,x1), the order
 * in which the look-up sums them), or -1 for a corner past the last row / column (weight 0, never read).  The plan of the
 * backward is these indices inverted, once per UV set. */
int fr_texture_corners(int32_t N, const float* uv, int32_t H, int32_t W, int32_t* corners, void* hip_stream);
int fr_texture_lookup(int32_t N, const float* uv, int32_t H, int32_t W, int32_t n_layers, const fr_tex_layer* layers,
                      void* hip_stream);
/* The backward as a GATHER per texel.  row_start [H*W + 1] and entries [row_start[H*W]] are the CSR of the plan: the
 * entries of texel t are entries[row_start[t] .. row_start[t+1]), each 4 * point + corner, for every corner
 * fr_texture_corners reported on t.  d_texture[c, y, x] = act'(texture[c, y, x]) * sum over the texel's entries, in list
 * order, of w(uv[point], corner) * d_out[point, c] — STORED for every texel of every layer (0 where no point lands): no
 * zero fill beforehand, no float atomics, the same bits on every run.  `texture` may be NULL for an identity layer.  uv
 * gets no gradient (the reference's coordinates are buffers). */
int fr_texture_lookup_backward(int32_t N, const float* uv, int32_t H, int32_t W, const int32_t* row_start,
                               const int32_t* entries, int32_t n_layers, const fr_tex_layer* layers, void* hip_stream);

/* ---- Neural baking: the decoder's packed output decoded into the five attribute arrays, one launch per direction
 * (reference `UVDecoder.forward`, model/uv_decoder.py:387-542 -> `_gather_attribute` :85-107 on the channel slices of
 * :225-245, `UVDecoderLoss` train/loss.py:522-677).  `tex_out`: planar [11,H,W] floats — colour 0:3, opacity 3:4, scaling
 * 4:7, rotation 7:10, offset 10:11.  Outputs row-major: colour [N,3] = tanh(t) * 0.5 / C0, opacity [N,1] = t, scaling [N,3] =
 * max_scaling - softplus(-(t + mean_scaling) + max_scaling), offset [N,1] = tanh(t) — these four rows are those of
 * fr_texture_lookup with the matching FR_TEX_ACT_*, bit for bit — and rotation [N,4]: per corner texel a = tanh(t) * 2 pi over
 * the three channels, theta = |a|, q = (cos(theta / 2), a * s) with s = sin(theta / 2) / theta (theta < 1e-6: 0.5 - theta^2 /
 * 48), emitted as (q[3], q[0], q[1], q[2]) (`_rotation_activation`, uv_decoder.py:158-174, as it runs), then the four
 * components interpolated: what activating the whole map and sampling it gives, without the activated map.  The rotation
 * rows are read and written sixteen bytes at a time: 16-byte aligned arrays.  Argument checks run before the first HIP call;
 * N == 0 is FR_OK and launches nothing.  No call allocates or synchronises: each can be captured in a HIP graph. */
int fr_bake_decode(int32_t N, const float* uv, int32_t H, int32_t W, const float* tex_out, float mean_scaling,
                   float max_scaling, float* color, float* opacity, float* scaling, float* rotation, float* offset,
                   void* hip_stream);
/* The backward as a gather per texel over the CSR of fr_texture_lookup_backward, walked ONCE: the twelve gradient channels
 * are summed in list order, taken through the per-texel Jacobians (rotation: the 4 -> 3 transpose through the quaternion map
 * and the tanh; at a texel whose three rotation channels are 0 the Taylor branch is taken and nothing divides by theta: every
 * non-zero entry of d out / d t is pi there) and STORED for every texel of d_tex_out [11,H,W]: no zero fill, no float atomics,
 * the same bits on every run.  A NULL d_* array stands for a zero gradient.  Entries whose point is not in 0 .. N - 1 are
 * skipped. */
int fr_bake_decode_backward(int32_t N, const float* uv, int32_t H, int32_t W, const int32_t* row_start,
                            const int32_t* entries, const float* tex_out, float mean_scaling, float max_scaling,
                            const float* d_color, const float* d_opacity, const float* d_scaling, const float* d_rotation,
                            const float* d_offset, float* d_tex_out, void* hip_stream);
/* The baking objective's rotation term and its gradient in ONE launch (train/loss.py:612-617 on raw_rot =
 * quaternion_to_axis_angle(decode_rotation), uv_decoder.py:516; pytorch3d 0.7.7's formula, element 0 of a row taken for the
 * real part): n = |q[1:]|, half = atan2(n, q[0]), ang = 2 half, s = sin(half) / ang (|ang| < 1e-6: 0.5 - ang^2 / 48), raw =
 * q[1:] / s;  loss[0] = mean(raw[:,0]^2) + mean(raw[:,2]^2), UNWEIGHTED, and weight x its gradient is ADDED to the rows of
 * d_rotation [N,4] by the lane that owns the row (NULL, or a weight of 0: no gradient traffic).  |q[1:]| = 0 passes no
 * gradient through the norm.  Per-workgroup partials summed in index order by the workgroup that finishes last: the same
 * bits on every run.  `workspace`: fr_rot_term_workspace_bytes() bytes of device memory, zeroed ONCE by the caller, left
 * zeroed; not to be shared by launches that can overlap.  16-byte aligned rows.  N == 0 launches nothing and leaves `loss`. */
size_t fr_rot_term_workspace_bytes(void);
int fr_rot_term(float weight, int32_t N, const float* rotation, float* d_rotation, float* loss, void* workspace,
                void* hip_stream);

/* present[i] = view-space z of means3D[i] > 0.2 (auxiliary.h:154). */
int fr_mark_visible(int32_t P, const float* means3D, const float* viewmatrix, const float* projmatrix,
                    uint8_t* present, void* hip_stream);

/* Per-pixel auxiliaries of the last forward held in `image` (device pointers into it). */
const float* fr_image_final_T(const void* image, int32_t W, int32_t H);
const uint32_t* fr_image_n_contrib(const void* image, int32_t W, int32_t H);

/* Test/diagnostic accessor: device pointer of one per-Gaussian array inside a geometry buffer filled by
 * fr_forward.  field: 6 clamped (uint8 bitmask), 8 the blend-record
 * template (12 floats: x, y, a', b', c', opacity, r, g, b, id bits, depth, 0 — the pixel-space centre, the view-space
 * depth and the colour that fields 0, 1 and 3 used to hold are its columns 0-1, 10 and 6-8; 2 was conic_opacity (the
 * conic as (-0.5 a, -b, -0.5 c) and the opacity are columns 2-5; the backward inverts its own 2D covariance), 4 was cov3D, which is no
 * longer stored (both per-Gaussian kernels compute it); 5 was the tile rectangle, 7 the gradient accumulators: they
 * live in the handle now), 9 the colour's derivative with respect to the view direction (9 floats: dR/dx, dG/dx, dB/dx,
 * then /dy, /dz; written for frames rendered from SH coefficients), 10 the activated opacity (float).  NULL for any other
 * field. */
const void* fr_debug_geometry_field(const void* geometry, int32_t P, int32_t field);

/* Test/diagnostic accessor: device pointer and size (*bytes, may be NULL) of one region of the backward's hand-off inside a
 * binning buffer of `capacity` instances for a W x H image (fr_binning_bytes(capacity, W, H) bytes): 0 the footprint masks
 * (8 bytes per instance), 1 the pixel-major walks (512 bytes per blend unit), 2 the backward's work list (32 bytes per unit),
 * 3 the per-unit entry state (1 KB per unit).  A forward-only frame (FR_FLAG_FORWARD_ONLY) writes none of them.  NULL (and
 * *bytes = 0) for any other region. */
const void* fr_debug_binning_region(const void* binning, uint64_t capacity, int32_t W, int32_t H, int32_t region, size_t* bytes);

/* Test hook for the wave reduce-scatter used by the blend backward: in[64*36] (lane-major), out[64]:
 * out[l] = sum over lanes of in[lane*36 + bitrev6(l)] for bitrev6(l) < 36. */
int fr_debug_selftest_reduce(const float* in, float* out, void* hip_stream);

/* simple-knn: out[i] = mean of the 3 smallest squared distances from points[i] to the other points. */
size_t fr_knn_workspace_bytes(int32_t P);
int fr_knn_mean_dist2(int32_t P, const float* points, float* out, void* workspace, size_t workspace_bytes,
                      void* hip_stream);
/* out[i] = squared distance from points[i] to the nearest OTHER point (FLT_MAX if P == 1): the quantity
 * FateAvatar.get_init_scale_by_knn takes from pytorch3d's knn_points(p, p, K=6).dists[..., 1]
 * (model/fateavatar.py:597-608).  Same workspace as fr_knn_mean_dist2. */
int fr_knn_nearest_dist2(int32_t P, const float* points, float* out, void* workspace, size_t workspace_bytes,
                         void* hip_stream);

/* ---- MonoGaussianAvatar's point deformation: every point carries its own blendshapes and skinning weights and is moved by
 * FLAME's linear blend skinning (reference: FLAME.forward_pts, flame/FLAME.py:207-237, over flame/lbs.py:103-188; the caller
 * is model/baseline/monogaussianavatar.py:345-359).  One launch per direction where the reference expands the expression
 * vector, the pose feature and the bone transforms per point, inverts N 4x4 matrices and differentiates the lot forward-mode.
 * Per point, with h = (p, 1), a pose state (betas [E], pose_feature [36], transforms [J,16] row-major 4x4) for the canonical
 * pose (c) and one for the frame:
 *   T_c = sum_j w_j A^c_j                  z = T_c^-1 h                (a 4-vector: z[3] = 1 / sum_j w_j)
 *   x   = z[:3] + S (beta - beta_c) + P^T (phi - phi_c)                (S = shapedirs [3,E], P = posedirs [36,3] of the point)
 *   xyz = (sum_j w_j A_j (x, 1))[:3]                                   (no division by the homogeneous coordinate)
 * PRECONDITION, not checked on the device: every bone matrix has the last row (0, 0, 0, 1).  The weights are taken as given:
 * they need not sum to 1.  The backward takes g_xyz [N,3] and writes EVERY row of d_points [N,3], d_shapedirs [N,3,E],
 * d_posedirs [N,36,3] and d_weights [N,J]; any of them may be NULL, and what is written does not depend on which are.  The
 * pose states get no gradient.  All pointers are device pointers; no call allocates, synchronises or uses float atomics:
 * the same bits on every launch, and both calls can be captured in a graph (the pose states are read at run time).
 * N == 0 launches nothing.  E outside 1 .. FR_LBS_MAX_E or J outside 1 .. FR_LBS_MAX_J is FR_ERR_INVALID_ARGUMENT. */
#define FR_LBS_MAX_E 64
#define FR_LBS_MAX_J 8
#define FR_LBS_POSE_FEATURES 36
typedef struct fr_pose_state {
    const float* betas;        /* [E] expression coefficients */
    const float* pose_feature; /* [FR_LBS_POSE_FEATURES] */
    const float* transforms;   /* [J,16] */
} fr_pose_state;
typedef struct fr_point_lbs {
    int32_t N, E, J;
    const float* points;    /* [N,3] */
    const float* shapedirs; /* [N,3,E] */
    const float* posedirs;  /* [N,FR_LBS_POSE_FEATURES,3] */
    const float* weights;   /* [N,J] */
    fr_pose_state canonical, frame;
} fr_point_lbs;
int fr_point_lbs_forward(const fr_point_lbs* lbs, float* xyz, void* hip_stream);
int fr_point_lbs_backward(const fr_point_lbs* lbs, const float* g_xyz, float* d_points, float* d_shapedirs, float* d_posedirs,
                          float* d_weights, void* hip_stream);

/* ---- the gradient of the same deformation to the FRAME's pose state (the reference's tracking optimisation of `expression`
 * and `flame_pose` reaches the image only through it, model/baseline/monogaussianavatar.py:162-186): one launch that sums over
 * the points, with g = g_xyz, T = sum_j w_j A_j, d_x = T[:3,:3]^T g and x as above,
 *   d_betas[l]          = sum_n sum_k S_n[k,l] d_x_n[k]                       (E sums)
 *   d_pose_feature[i]   = sum_n sum_k P_n[i,k] d_x_n[k]                       (36 sums)
 *   d_transforms[j,r,c] = sum_n w_nj g_n[r] (x_n, 1)[c],  r < 3, c < 4        (12 J sums; the last row of every bone is written 0)
 * PRECONDITION as above: every bone matrix has the last row (0, 0, 0, 1) — it is a constant, so its gradient is 0 and nothing
 * else is computed for it.  The canonical state gets no gradient (it is a constant buffer in the reference).  Any of the three
 * outputs may be NULL, what the others receive does not depend on which are, and EVERY element of a non-NULL output is
 * written.  Sums as fr_lbs_terms: per-workgroup partials added up in workgroup-index order by the workgroup that finishes
 * last, no float atomics, the same bits on every launch; it can be captured in a graph.  `workspace`:
 * fr_point_lbs_pose_workspace_bytes() bytes, 16-byte aligned, zeroed ONCE by the caller, left zeroed, not shared by launches
 * that can overlap.  N == 0 launches nothing (the outputs are left as they are).  The descriptor is checked as by
 * fr_point_lbs_backward; a NULL g_xyz with N > 0 or a NULL workspace is FR_ERR_INVALID_ARGUMENT. */
size_t fr_point_lbs_pose_workspace_bytes(void);
int fr_point_lbs_backward_pose(const fr_point_lbs* lbs, const float* g_xyz, float* d_betas, float* d_pose_feature,
                               float* d_transforms, void* workspace, void* hip_stream);

/* ---- index[i] = the vertex nearest to points[i], brute force against V <= FR_NEAREST_MAX_V vertices held in LDS (reference:
 * pytorch3d's knn_points(p, verts, K=1), train/loss.py:231-233).  The squared distance is (dx*dx + dy*dy) + dz*dz in float32
 * without contraction, d = point - vertex; ties go to the LOWEST index.  `dist2` [N] may be NULL.  V <= 0 or
 * V > FR_NEAREST_MAX_V is FR_ERR_INVALID_ARGUMENT; N == 0 launches nothing. */
#define FR_NEAREST_MAX_V 8192
int fr_nearest_vertex(int32_t N, const float* points, int32_t V, const float* verts, int32_t* index, float* dist2,
                      void* hip_stream);

/* ---- the three blendshape terms of MonoGaussianAvatarLoss in ONE launch (reference: train/loss.py:418-445, :472-515): with
 * v = index[i] (clamped to 0 .. V-1) the plain mean squared errors
 *   loss[0] = mean (weights [N,J]     - gt_weights [V,J][v])^2
 *   loss[1] = mean (posedirs [N,36,3] - gt_posedirs [V,36,3][v])^2
 *   loss[2] = mean (shapedirs [N,3,E] - gt_shapedirs [V,3,E][v])^2
 * UNWEIGHTED, and the kernel ADDS weight_k * 2 (pred - gt) / count_k into d_weights / d_posedirs / d_shapedirs by a
 * read-modify-write of the lane that owns the element (so that it lands on what fr_point_lbs_backward wrote; no atomics).  A
 * weight of 0 leaves that array untouched; a NULL gradient pointer means that term's loss only.  The caller pads the ghost
 * bone's column and transposes FLAME's [36, 3V] pose basis.  Sums and workspace as fr_gaussian_regularise: per-workgroup
 * partials summed in index order by the workgroup that finishes last (the same bits on every launch); `workspace`:
 * fr_lbs_terms_workspace_bytes() bytes, zeroed ONCE by the caller, left zeroed, not shared by launches that can overlap.
 * `loss`: three device floats.  N == 0 launches nothing and leaves `loss` as it is. */
typedef struct fr_lbs_terms_config {
    float weights_weight, posedirs_weight, shapedirs_weight;
} fr_lbs_terms_config;
size_t fr_lbs_terms_workspace_bytes(void);
int fr_lbs_terms(const fr_lbs_terms_config* cfg, int32_t N, int32_t V, int32_t E, int32_t J, const int32_t* index,
                 const float* weights, const float* posedirs, const float* shapedirs, const float* gt_weights,
                 const float* gt_posedirs, const float* gt_shapedirs, float* d_weights, float* d_posedirs, float* d_shapedirs,
                 float* loss, void* workspace, void* hip_stream);

/* ---- FlashAvatar's deformation MLP (reference: `MLP`, model/baseline/flashavatar.py:434-464, fed by :238-240): L hidden ReLU
 * layers (1 <= L <= FR_MLP_MAX_LAYERS) of width FR_MLP_WIDTH and a linear output layer of D_out <= FR_MLP_MAX_OUT columns, all
 * float32: the products are exact-f32 MFMA (a k-ordered fmaf chain), everything else plain f32.
 *   input row of point n = [E[n, 0:De] | cond[0:Dc]]   (E: a per-point constant; cond: ONE vector per frame; De >= 1, Dc >= 0,
 *                                                       De + Dc <= FR_MLP_WIDTH)
 * The broadcast half is never materialised: layer 0 is relu(E W0[:, :De]^T + (W0[:, De:] cond + b0)).
 * `weights`: ONE flat buffer in torch's nn.Linear layout — per layer `weight` [out, in] row-major then `bias` [out], layers in
 * order (in = De + Dc for layer 0, FR_MLP_WIDTH after it; out = FR_MLP_WIDTH, D_out for the last): a checkpoint's
 * deformNet.fcs.{i}.weight/bias and deformNet.output_linear.* copy in and out without a transpose.  `d_weights` has the same
 * layout.
 * fr_mlp_forward writes the RAW outputs `out` [N, D_out] (no tanh) and saves every hidden layer's post-ReLU activations in the
 * workspace.  fr_mlp_backward (after a forward with the same descriptor and workspace) computes, last layer first,
 *   dZ_l = dH_l * [H_l > 0],  dH_{l-1} = dZ_l W_l,  dW_l = dZ_l^T H_{l-1},  db_l = sum_n dZ_l,
 *   dW_0[:, De:] = db_0 (x) cond,  d_cond = W_0[:, De:]^T db_0     (`d_cond` [Dc] may be NULL)
 * and OVERWRITES d_weights (every element; nothing is accumulated).  E gets no gradient (a registered buffer in the reference).
 * The sums over n run in chunks of FR_MLP_CHUNK points, each a k-ordered chain, and a second launch adds the chunks' partials
 * in chunk order: no float atomics, the same bits on every launch and every graph replay.  Ragged sizes (N against the
 * FR_MLP_POINT_TILE-point tile, De against the MFMA's K step, D_out, the last chunk) are handled inside the kernels.
 * N == 0 launches no kernel: the forward writes nothing, the backward zeroes d_weights and d_cond.  Sizes outside the limits,
 * a NULL workspace, or a NULL array that N > 0 needs are FR_ERR_INVALID_ARGUMENT.
 * `workspace`: fr_mlp_workspace_bytes(N, L) bytes, 256-byte aligned, the caller's, not shared by launches that can overlap:
 *     (L + 2) * r256(N * FR_MLP_WIDTH * 4)                             the saved activations and two dZ buffers
 *   + r256(ceil(N / FR_MLP_CHUNK) * (FR_MLP_WIDTH + 1) * FR_MLP_WIDTH * 4)   one layer's split-N partials (weight and bias)
 *   + r256(FR_MLP_WIDTH * 4)                                           layer 0's bias with the condition folded in
 * with r256 = round up to 256 (151.1 MB at N = 16 384, L = 6). */
#define FR_MLP_WIDTH 256
#define FR_MLP_MAX_LAYERS 8
#define FR_MLP_MAX_OUT 16
#define FR_MLP_POINT_TILE 128
#define FR_MLP_CHUNK 256
typedef struct fr_mlp {
    int32_t N, L, De, Dc, D_out;
    const float* E;       /* [N, De] */
    const float* cond;    /* [Dc] (may be NULL if Dc == 0) */
    const float* weights; /* flat, as above */
} fr_mlp;
size_t fr_mlp_workspace_bytes(int32_t N, int32_t L);
int fr_mlp_forward(const fr_mlp* mlp, float* out, void* workspace, void* hip_stream);
int fr_mlp_backward(const fr_mlp* mlp, const float* d_out, float* d_weights, float* d_cond, void* workspace, void* hip_stream);

/* ---- FLAME's linear blend skinning with FateAvatar's personalised deltas, for ONE frame (reference:
 * FLAME.forward_with_delta_blendshape, flame/FLAME.py:156-204, over lbs(), flame/lbs.py:24-101; the caller is
 * model/fateavatar.py:212-223 with the `bs` optimizer group of train/optim.py:27-33).  V vertices, NS shape and NE expression
 * columns (L = NS + NE), FR_FLAME_JOINTS joints with parents[i] < i (parents[0] is not read), FR_FLAME_POSE_FEATURES pose
 * features:
 *   v_shaped = (v_template + delta_vertex) + (shapedirs[:, :, NS:] + delta_exp) expression
 *   Jnt      = J_regressor v_shaped
 *   R_j      = batch_rodrigues(pose[3j : 3j + 3])         (angle = |r + 1e-8|, dir = r / angle, as the reference)
 *   phi      = (R_1 .. R_4 - I).flatten()
 *   v_posed  = v_shaped + phi (posedirs + delta_posedirs)
 *   A        = batch_rigid_transform(R, Jnt, parents)
 *   verts    = (sum_j w_vj A_j) (v_posed, 1)
 * The reference multiplies the NS shape columns by exact zeros: they are not read, their gradient is exactly 0, and the trained
 * part of `delta_shapedirs` [V,3,L] is its expression slice `delta_exp` [V,3,NE] alone.  Any of the three deltas may be NULL:
 * zeros.  fr_flame_forward writes `verts` [V,3], `pose_feature` [36] and `transforms` [5,16] (row-major 4x4, last rows
 * (0,0,0,1); these two may be NULL) and, if `verts_orig` is not NULL, the mesh WITHOUT the deltas (joint sums of its own) there.
 * fr_flame_backward (after a forward with the same descriptor and workspace) takes g_verts [V,3] = dLoss/dverts and writes
 * EVERY element of d_delta_exp [V,3,NE], d_delta_posedirs [36,3V], d_delta_vertex [V,3], d_expression [NE] and d_pose [15]
 * (stored, not accumulated); any of them may be NULL, and what the others receive does not depend on which are.
 * Two launches per call.  The sums over the vertices (the joints; d_A, d_phi; d_expression) are per-workgroup partials added up
 * in workgroup-index order by the workgroup that finishes last: no float atomics, the same bits on every launch and every graph
 * replay.  Nothing allocates or synchronises; both calls can be captured.  V == 0 launches nothing.  NE outside
 * 1 .. FR_FLAME_MAX_E, negative V or NS, a NULL required pointer or a NULL / misaligned workspace is FR_ERR_INVALID_ARGUMENT.
 * Inputs are assumed finite.
 * `workspace`: fr_flame_workspace_bytes(V, NE) bytes, 16-byte aligned, not shared by launches that can overlap.  Its first
 * fr_flame_workspace_zeroed_bytes() bytes (counters and partials) are zeroed ONCE by the caller and left zeroed by every call;
 * the rest is the frame's state (phi, A, the chain, v_posed, d_v_posed), which a forward overwrites and the backward reads. */
#define FR_FLAME_MAX_E 128
#define FR_FLAME_JOINTS 5
#define FR_FLAME_POSE_FEATURES 36
typedef struct fr_flame {
    int32_t V, NS, NE;
    const int32_t* parents;      /* [5], device */
    const float* v_template;     /* [V,3] */
    const float* shapedirs;      /* [V,3,NS+NE] */
    const float* posedirs;       /* [36,3V] */
    const float* J_regressor;    /* [5,V] */
    const float* lbs_weights;    /* [V,5] */
    const float* delta_exp;      /* [V,3,NE] or NULL */
    const float* delta_posedirs; /* [36,3V] or NULL */
    const float* delta_vertex;   /* [V,3] or NULL */
    const float* expression;     /* [NE] */
    const float* pose;           /* [15] */
} fr_flame;
size_t fr_flame_workspace_bytes(int32_t V, int32_t NE);
size_t fr_flame_workspace_zeroed_bytes(void);
int fr_flame_forward(const fr_flame* flame, float* verts, float* verts_orig, float* pose_feature, float* transforms,
                     void* workspace, void* hip_stream);
int fr_flame_backward(const fr_flame* flame, const float* g_verts, float* d_delta_exp, float* d_delta_posedirs,
                      float* d_delta_vertex, float* d_expression, float* d_pose, void* workspace, void* hip_stream);

/* ---- FateAvatar's VGG perceptual term (reference: VGGPerceptualLoss.forward, tools/loss_utils/vgg_feature.py:24-47, at
 * weight 0.1 in train/loss.py): a frozen stack of 3 x 3 convolutions run on the rendered image and on its target, and the
 * mean absolute difference of chosen layer outputs, with the gradient to the rendered image.  The stack is a descriptor, not
 * VGG-16 hard-wired: n_layers <= FR_VGG_MAX_LAYERS layers, each conv3x3(c_in -> c_out, padding 1) + bias + ReLU with
 *   pool_before  a 2 x 2 / stride 2 max-pool on the layer's input (not on layer 0),
 *   tap_after    the layer's output is a feature the loss compares (the LAST layer must be one: nothing else reaches it).
 * Layer 0 has c_in = 3; every later c_in equals the previous c_out and is a multiple of 32; every c_out is a multiple of 64;
 * size_h and size_w are divisible by 2^(number of pools) and at most 32767.  Anything else is FR_ERR_INVALID_ARGUMENT.
 *   x      = resize((image - mean) / std),  x_gt = the same of `target`      image, target: [3,H,W] planar, size: size_h x size_w
 *   a_l    = relu(conv(pool?(a_{l-1}), W_l) + b_l)                            for both images
 *   term_t = mean |a_l - a_l_gt| over the layer's c_out h_l w_l elements      for the t-th layer with tap_after
 * The resize is F.interpolate(mode='bilinear', align_corners=False): source coordinate (o + 0.5) in / out - 0.5 clamped at 0,
 * upper tap clamped at the edge, no antialiasing; size == (H, W) is the exact identity.  The max-pool's gradient goes to the
 * first maximum of the window in row-major order (torch's rule); sign(0) = 0 in the terms' gradient.
 * Every activation is NHWC with the two images stacked: row m = (image i, y, x) = i h w + y w + x, channels contiguous; image 0
 * is the rendered one, image 1 the target.
 * Weights are packed ONCE by the caller (the network is frozen; fateavatar_amd/perceptual.py does it with torch permutes):
 *   weights_fwd   per layer, in order: [9 c_in][c_out] with row k = (3 ky + kx) c_in + ci holding W[co, ci, ky, kx], then the
 *                 bias [c_out]                                         (the GEMM's B operand: K tap-major, channel-minor)
 *   weights_bwd   per layer, in order: [9 c_out][c_in] with row k = (3 ky + kx) c_out + co holding W[co, ci, 2 - ky, 2 - kx]
 *                 (taps flipped, c_in / c_out exchanged: the data gradient is the same gathered GEMM over this packing)
 * fr_vgg_loss_grad writes loss_out[0] = the unweighted sum of the terms and loss_out[1 .. T] = the terms, and, unless d_image
 * is NULL (forward only), d_image [3,H,W] = weight * dLoss/dimage: stored when `accumulate` is 0, added to what is there when
 * it is 1.  The products are exact-f32 MFMA (layer 0 and its gradient: plain f32); no float atomics anywhere: the same bits on
 * every launch and every graph replay.  Nothing allocates or synchronises.
 * A GEMM of M rows (the pixels: of both images forward, of image 0 in the gradient) and N columns (c_out forward, c_in in the
 * gradient) whose grid of 64 x 64 tiles is too small for the device is SPLIT over the nine taps into s planes — with
 * t = ceil(M / 64) ceil(N / 64): s = 1 if t >= 256, else 3 if 3 t >= 256, else 9 — whose partial products a second launch adds
 * in plane order before the epilogue.  s depends on the shape alone.
 * `tile`: FR_VGG_TILE_AUTO (the GEMM's tile is the library's choice: 64 x 64), FR_VGG_TILE_64 or FR_VGG_TILE_128 (128 x 64
 * forced; the results do not depend on the tile, bit for bit), optionally + FR_VGG_NO_SPLIT (no GEMM is split: another
 * summation order, so other low bits).  For measurement and tests.
 * `workspace`: fr_vgg_workspace_bytes() bytes (0 for an invalid descriptor), 256-byte aligned, the caller's, not shared by
 * launches that can overlap.  With r256 = round up to 256 and h_l x w_l layer l's OUTPUT extent, in this order:
 *     r256(FR_VGG_REDUCE_BYTES)                         counters and partials of the terms' sums: ZERO before the first call,
 *                                                       left zeroed by every call
 *   + r256(2 size_h size_w 3 * 4)                       x: the normalised, resized images
 *   + sum over l of r256(2 h_l w_l c_out_l * 4)         a_l: every layer's post-ReLU output, both images (what the backward's
 *                                                       masks, argmaxes and signs are read from)
 *   + r256(max over pooled l of 2 h_l w_l c_in_l * 4)   the pooled input of the layer being computed
 *   + 2 r256(max over l of h_l w_l c_out_l * 4)         two gradient buffers (image 0 only), used alternately
 *   + r256(max over pooled l of h_l w_l c_in_l * 4)     a pooled layer's input gradient before it is routed to the argmaxes
 *   + r256(max over the split GEMMs of s M N * 4)       the planes of the GEMM being computed (layers l >= 1: forward
 *                                                       M = 2 h_l w_l, N = c_out_l; gradient M = h_l w_l, N = c_in_l)
 * (152.1 MB for VGG-16 at 224^2.)  `weights_fwd` and `weights_bwd` are 16-byte aligned. */
#define FR_VGG_MAX_LAYERS 16
#define FR_VGG_LOSS_BLOCKS 1024
#define FR_VGG_REDUCE_BYTES ((16 + 1) * 32 * 4 + FR_VGG_LOSS_BLOCKS * 4)
#define FR_VGG_TILE_AUTO 0
#define FR_VGG_TILE_64 1
#define FR_VGG_TILE_128 2
#define FR_VGG_NO_SPLIT 4
typedef struct fr_vgg_layer {
    int32_t c_in, c_out, pool_before, tap_after;
} fr_vgg_layer;
typedef struct fr_vgg {
    int32_t n_layers, H, W, size_h, size_w, tile;
    float mean[3], std[3];
    fr_vgg_layer layers[FR_VGG_MAX_LAYERS];
    const float* weights_fwd; /* packed, as above */
    const float* weights_bwd;
    const float* image;       /* [3,H,W] */
    const float* target;      /* [3,H,W] */
} fr_vgg;
size_t fr_vgg_workspace_bytes(const fr_vgg* vgg);
int fr_vgg_loss_grad(const fr_vgg* vgg, float weight, int accumulate, float* loss_out, float* d_image, void* workspace,
                     void* hip_stream);

/* ---- The LPIPS term over the same descriptor (reference: lpips.LPIPS(net='vgg') called with normalize=True, in
 * FlashAvatar's objective at weight 0.05 after step 15 000 and SplattingAvatar's at 0.01, train/loss.py:203-323, and the
 * evaluation metric, train/metrics.py:69).  Its input (2x - 1 - shift) / scale equals (x - mean) / std with the ImageNet
 * statistics, i.e. the descriptor's `mean` / `std`; its trunk is vgg16.features[:30]: 13 layers, 4 pools, 5 taps; it does
 * not resize (size == (H, W)), though the descriptor may.  Per tap, with a / b the rendered / target feature [h,w,C]:
 *   n_a(p) = sqrt(sum_c a_c(p)^2),  a^ = a / (n_a + 1e-10)   (the same for b),
 *   term   = (1 / (h w)) sum_p sum_c lin_c (a^_c - b^_c)^2,   the loss = the sum of the terms,
 *   dterm/da_c = r g_c - a^_c T / n_a   with g_c = 2 lin_c (a^_c - b^_c) / (h w), r = 1 / (n_a + 1e-10), T = sum_c g_c a^_c.
 * DEAD PIXELS, a deviation from stock autograd: where n_a(p) == 0 autograd yields NaN (sqrt's backward at 0 is inf x 0).  Here
 * n == 0 makes the hat vector 0, the pixel contributes sum_c lin_c b^_c^2, its gradient is exactly 0 (every unit behind it is
 * a ReLU at 0, whose mask passes nothing anyway), and nothing non-finite is ever produced.
 * `lin`: the taps' [c_out] vectors concatenated in tap order, 16-byte aligned; a tapped layer has c_out <= 512.  loss_out is
 * [1 + T] as above; `weight`, `accumulate`, d_image == NULL and `tile` mean what they mean for fr_vgg_loss_grad, and the same
 * bits come out of every launch and replay (a wave per pixel, fixed-order sums, no float atomics).
 * The tap gradient is MATERIALISED, not recomputed in the epilogues: a small kernel writes a tap's seed (already behind the
 * ReLU mask) from the two saved activations, the pixel's three scalars and lin — the LAST tap's into a gradient buffer, from
 * which the backward starts on the plain fetch; an earlier tap's into ONE seed buffer just ahead of the GEMM whose epilogue
 * (in-kernel, split-reduce or un-pool) adds it.  The L1 kernels are the same templates with the other term kind.
 * `workspace`: fr_lpips_workspace_bytes() bytes = the fr_vgg_workspace_bytes() layout, unchanged, followed by
 *   + sum over the taps of r256(3 h_l w_l * 4)                         per pixel (r_a, r_b, T / n_a), all 0 at a dead pixel
 *   + r256(max over the taps but the last of h_l w_l c_out_l * 4)      the seed buffer
 * (763.4 MB + 4.2 MB + 67.1 MB = 834.7 MB for the 13-layer trunk at 512^2; 168.2 MB at 224^2.) */
size_t fr_lpips_workspace_bytes(const fr_vgg* vgg);
int fr_lpips_loss_grad(const fr_vgg* vgg, const float* lin, float weight, int accumulate, float* loss_out, float* d_image,
                       void* workspace, void* hip_stream);

#ifdef __cplusplus
}
#endif
#endif
