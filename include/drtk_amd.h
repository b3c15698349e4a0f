/* drtk_amd -- C ABI of the MI355X-native rasterize -> render -> interpolate -> edge_grad hot path.
 *
 * This is the drop-in boundary below the torch-operator layer.  The reference (facebookresearch/
 * DRTK) has no extern "C" surface of its own: its extensions are reached through the torch
 * dispatcher, whose CUDA-key implementations are the C++ host launchers cited on every entry
 * below.  Each function here replaces exactly one of those launchers (same inputs, outputs and
 * semantics, contiguous layouts, raw device pointers, an explicit HIP stream) so that the
 * torch-op shim (drtk_amd/csrc/torch_ops/<op>.cpp), a ctypes caller or a C program can all drive the
 * same kernels.  INTEGRATION.md shows the binding a reference maintainer would add.
 *
 * Conventions
 *   - all pointers are DEVICE pointers (hipMalloc / torch caching allocator), tensors contiguous:
 *       v, v_pix        [N,V,3]        vi         [N,F,3] int32, batch stride `vi_sN` elements
 *                                                 (0 = one [F,3] topology shared by all views)
 *       index_img       [N,H,W] int32  (-1 = empty)
 *       depth_img       [N,H,W]        bary_img   [N,3,H,W]   (planar)
 *       attrs           [N,V,C]        img / out  [N,C,H,W]   (planar)
 *   - alignment: tensor pointers need the alignment of their ELEMENT type only (4 bytes for float / int32, 8 for
 *     double) -- a contiguous view at any element offset of a larger buffer is fine, for inputs and for outputs.
 *     The kernels take their 16-byte vector paths when a tensor happens to be 16-byte aligned (every hipMalloc /
 *     torch allocation is) and the image width allows it; otherwise they fall back to scalar accesses or rely on
 *     the platform's support for dword-aligned wide accesses (tests/test_gpu_parity.py, ..._odd_element_offsets).
 *     WORKSPACES must be 16-byte aligned (they hold 64-bit counters updated atomically); this is checked:
 *     DRTK_ERR_INVALID_ARGUMENT otherwise.
 *   - `dtype` selects float or double for every floating tensor of the call (the reference
 *     dispatches float/double only: src/include/kernel_utils.h:35-57); indices are int32.
 *   - N (views) is unbounded on the path's operators: a launch takes 65 535 views (the view is blockIdx.y), a larger
 *     batch is executed as consecutive slices by the entry point itself -- views are independent, results identical
 *     (the reference's grid-stride kernels take any N: render_kernel.cu:349-377).  H * W < 2^31 per view (in-plane
 *     offsets are 32-bit); the two normal-matrix operators, which accumulate all views into one array, keep N <= 65 535.
 *   - `stream` is a hipStream_t (NULL = the null stream).  No call synchronises the device or
 *     allocates memory; all work is enqueued on `stream`.
 *   - return value: DRTK_OK or a negative drtk_status_t; drtk_amd_status_string() explains it.
 *     Argument validation mirrors the reference's TORCH_CHECKs where it can be expressed on raw
 *     sizes; tensor-level checks (dtype, device, ndim) live in the torch shim.
 *   - reproducibility: forward outputs and per-pixel gradients are bit-identical from run to run; per-VERTEX
 *     gradients (grad_v, attr_grad, grad_v_pix) are accumulated with float atomics in varying order and agree to
 *     ~1e-7 of their largest value between runs, like the reference's atomicAdd scatter.
 *   - knife-edge decisions: float arithmetic follows the reference's HOST source in its written order under IEEE
 *     rules (no contraction, correctly rounded / and sqrt), i.e. what a strict build of its CPU kernels evaluates.
 *     Where the reference decides on a quantity that is zero up to rounding -- the sign get_dp_dr takes from `d`
 *     where two DIFFERENT surfaces meet in the image with face normals equal to ~1e-8 yet not bit-identical
 *     (edge_grad_kernel_cpu.cpp:113-137; d ~ 1e-9 in exact arithmetic, the output of that pixel is +-max_dp_dr * ...;
 *     exact instanced copies give d == 0 and generic offsets |d| ~ 1e-6: both signed stably) -- its own builds
 *     differ from one another at that pixel: the shipped host
 *     build is -O3 --fast-math (setup.py:23-24), the CUDA build normalises with ::rnorm3df where the host divides by
 *     sqrt (cuda_math_helper.h:173-176).  Expect differences of 2 * max_dp_dr at a few such silhouette pixels when
 *     comparing against those (about 1 in 150 of the small two-object float32 test scenes has one); against the
 *     strict evaluation there are none (profiles/NOTES.md section 3).
 *   - thread-safety: re-entrant; no global mutable state except the rasterizer's depth-order setting (one atomic int).
 */
#ifndef DRTK_AMD_H
#define DRTK_AMD_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

/* The library is built with -fvisibility=hidden and a linker version script (drtk_amd/csrc/exports.map): the functions
 * declared between this push and its pop are its ENTIRE dynamic symbol table (tests/test_host_logic.py checks nm -D). */
#if defined(__GNUC__) || defined(__clang__)
#pragma GCC visibility push(default)
#endif

#define DRTK_AMD_VERSION_MAJOR 0
#define DRTK_AMD_VERSION_MINOR 4

/* DRTK_F16 (IEEE half, storage only) is accepted by drtk_amd_filter2d alone; every other entry point answers it with
 * DRTK_ERR_INVALID_ARGUMENT. */
typedef enum { DRTK_F32 = 0, DRTK_F64 = 1, DRTK_F16 = 2 } drtk_dtype_t;

typedef enum {
  DRTK_OK = 0,
  DRTK_ERR_INVALID_ARGUMENT = -1, /* bad size / null pointer / unknown dtype */
  DRTK_ERR_WORKSPACE_TOO_SMALL = -2,
  DRTK_ERR_LAUNCH = -3,       /* hipGetLastError() after a launch was not hipSuccess */
  DRTK_ERR_UNSUPPORTED = -4,  /* reserved */
  DRTK_ERR_TOO_MANY_VERTICES = -5 /* V >= 2^28, rasterize_kernel.cu:459-462 */
} drtk_status_t;

typedef void* drtk_stream_t; /* hipStream_t */

const char* drtk_amd_status_string(int status);
/* "major.minor (gfx950)" */
const char* drtk_amd_version(void);

/* ------------------------------------------------------------------------------------------
 * rasterize        replaces rasterize_cuda            (src/rasterize/rasterize_kernel.cu:417-563)
 *
 * Z-buffer rasterization of N views.  Writes index_img (triangle id, -1 where empty; lower id
 * wins depth ties) and depth_img (ALWAYS float32, 0 where empty, rasterize_kernel.cu:481) --
 * bit-exact with the reference's arithmetic (rasterize_kernel.cu:69-166).
 * The depth's summation order is the one the reference's source spells, evaluated strictly.  A reference
 * build compiled with -ffast-math (its setup.py:22-24) associates that sum differently: the library's DEPTH-ORDER
 * SETTING (drtk_amd_set_depth_order below, or DRTK_AMD_DEPTH_ORDER=fastmath in the environment) makes every later
 * rasterize call evaluate it in the order such a build was observed to use, for deployments that must match one bit
 * for bit.
 * `workspace` holds the tile bins; query its size first.
 * `wireframe != 0` selects the line mode (rasterize_kernel.cu:170-400: edges whose bit is set in the top
 * nibble of vi[...,0] are drawn by the diamond rule, the triangles themselves only occlude); it needs the
 * workspace of drtk_amd_rasterize_lines_workspace_bytes (a packed [N,H,W] 64-bit buffer) instead.
 */
typedef enum {
  DRTK_DEPTH_ORDER_STRICT = 0,  /* s = dinv0 (e0/|den|) + dinv1 (e1/|den|) + dinv2 (e2/|den|): rasterize_kernel.cu:148-153 as written */
  DRTK_DEPTH_ORDER_FASTMATH = 1 /* s = ((e1 dinv1 + e0 dinv0) + e2 dinv2) (1/|den|): the host build of setup.py:22-24 (-O3 --fast-math) */
} drtk_depth_order_t;
/* The one library-level setting (everything else is re-entrant and stateless): which of the two orders
 * drtk_amd_rasterize launches from now on.  Initial value: DRTK_DEPTH_ORDER_FASTMATH if the environment holds
 * DRTK_AMD_DEPTH_ORDER=fastmath when the setting is first read or written, else DRTK_DEPTH_ORDER_STRICT.  The torch
 * operators (torch.ops.rasterize_ext.rasterize, drtk.rasterize) call the same entry point and follow it.
 * Set it before the first rasterize call of a deployment; a change is atomic and affects later launches only.
 * The order is part of the kernel a call launches: a captured graph (hipGraph, torch.cuda.graph) replays the order that
 * was active when it was captured, whatever is set afterwards.  The setting is process-wide: one value shared by every
 * thread and stream that uses the library. */
int drtk_amd_set_depth_order(int order); /* DRTK_OK, or DRTK_ERR_INVALID_ARGUMENT for anything but the two values */
int drtk_amd_get_depth_order(void);      /* a drtk_depth_order_t */
int drtk_amd_rasterize_workspace_bytes(int64_t N, int64_t F, int64_t H, int64_t W, size_t* bytes);
int drtk_amd_rasterize_lines_workspace_bytes(int64_t N, int64_t H, int64_t W, size_t* bytes);
int drtk_amd_rasterize(
    drtk_dtype_t dtype, const void* v, const int32_t* vi, int64_t N, int64_t V, int64_t F,
    int64_t vi_sN, int64_t H, int64_t W, int wireframe, float* depth_img, int32_t* index_img,
    void* workspace, size_t workspace_bytes, drtk_stream_t stream);

/* ------------------------------------------------------------------------------------------
 * rasterize_layers     (no counterpart in the reference: its z-buffer keeps the nearest fragment only)
 *
 * The `num_layers` nearest triangles of every pixel in one call (depth peeling), triangle mode only.  The FRAGMENTS of
 * a pixel are the triangles drtk_amd_rasterize would consider covering its centre (same culling, top-left rule, exact
 * arithmetic, depth expression under the current depth-order setting), each with the key
 * (float32 depth bits << 32) | triangle id, an unsigned 64-bit number.  Layer k (0-based) of a pixel is its fragment
 * with the k-th smallest key:
 *     index_img [N,K,H,W] int32   its id, -1 where the pixel has fewer than k + 1 fragments
 *     depth_img [N,K,H,W] float32 its depth, 0 there
 * Layer 0 is drtk_amd_rasterize bit for bit; keys increase strictly with k, empty layers trail; fragments of equal
 * depth all appear, lower id first.  Deterministic.  1 <= num_layers <= DRTK_AMD_MAX_RASTER_LAYERS, checked before
 * anything else.  The workspace holds the tile bins, built once per call and shared by all layers (same size as
 * drtk_amd_rasterize's); the call only enqueues (num_layers raster launches) and can be captured into a graph.
 * To shade the layers, fold them into the batch: index_img viewed as [N*K,H,W] with every view's vertices
 * repeated K times goes through render / interpolate unchanged ("layers").
 */
#define DRTK_AMD_MAX_RASTER_LAYERS 8
int drtk_amd_rasterize_layers_workspace_bytes(int64_t N, int64_t F, int64_t H, int64_t W, int num_layers, size_t* bytes);
int drtk_amd_rasterize_layers(
    drtk_dtype_t dtype, const void* v, const int32_t* vi, int64_t N, int64_t V, int64_t F,
    int64_t vi_sN, int64_t H, int64_t W, int num_layers, float* depth_img, int32_t* index_img,
    void* workspace, size_t workspace_bytes, drtk_stream_t stream);

/* ------------------------------------------------------------------------------------------
 * render           replaces render_cuda               (src/render/render_kernel.cu:283-380)
 * Perspective-correct barycentrics + depth per pixel; zeros where index_img == -1.
 */
int drtk_amd_render(
    drtk_dtype_t dtype, const void* v, const int32_t* vi, const int32_t* index_img, int64_t N,
    int64_t V, int64_t F, int64_t vi_sN, int64_t H, int64_t W, void* depth_img, void* bary_img,
    drtk_stream_t stream);

/* render_backward  replaces render_cuda_backward      (src/render/render_kernel.cu:382-436)
 * grad_v [N,V,3] is zero-filled by this call (render_kernel.cu:397) and then accumulated.
 */
int drtk_amd_render_backward(
    drtk_dtype_t dtype, const void* v, const int32_t* vi, const int32_t* index_img,
    const void* grad_depth_img, const void* grad_bary_img, int64_t N, int64_t V, int64_t F,
    int64_t vi_sN, int64_t H, int64_t W, void* grad_v, drtk_stream_t stream);

/* ------------------------------------------------------------------------------------------
 * interpolate      replaces interpolate_cuda          (src/interpolate/interpolate_kernel.cu:454-570)
 * out[n,c,y,x] = sum_k attrs[n,vi[t,k],c] * bary[n,k,y,x]; background pixels get the
 * reference's +-1 coordinate sweep (interpolate_kernel.cu:104-108).
 */
int drtk_amd_interpolate(
    drtk_dtype_t dtype, const void* attrs, const int32_t* vi, const int32_t* index_img,
    const void* bary_img, int64_t N, int64_t V, int64_t C, int64_t F, int64_t vi_sN, int64_t H,
    int64_t W, void* out, drtk_stream_t stream);

/* Extension (no reference counterpart): interpolate with the background written as 0 instead of the
 * +-1 coordinate sweep -- the fused form of `interpolate(...) * (index_img != -1)[:, None]`, the way every
 * DRTK pipeline uses the op (test/two_triangles.py:52-58).  Same gradient as drtk_amd_interpolate: the
 * backward never reads the upstream gradient of a background pixel. */
int drtk_amd_interpolate_masked(
    drtk_dtype_t dtype, const void* attrs, const int32_t* vi, const int32_t* index_img,
    const void* bary_img, int64_t N, int64_t V, int64_t C, int64_t F, int64_t vi_sN, int64_t H,
    int64_t W, void* out, drtk_stream_t stream);

/* interpolate_backward  replaces interpolate_cuda_backward (interpolate_kernel.cu:642-697)
 * attr_grad [N,V,C] (NULL = not wanted) is zero-filled then accumulated; bary_grad [N,3,H,W]
 * (NULL = not wanted) is fully written.  An EMPTY output (N*V*C == 0 / N*H*W == 0) has no storage, so NULL for it
 * carries no information: both NULL is DRTK_ERR_INVALID_ARGUMENT only when both gradients would have had elements,
 * otherwise there is nothing to write and the call returns DRTK_OK (e.g. a batch of zero views).
 */
int drtk_amd_interpolate_backward(
    drtk_dtype_t dtype, const void* grad_out, const void* attrs, const int32_t* vi,
    const int32_t* index_img, const void* bary_img, int64_t N, int64_t V, int64_t C, int64_t F,
    int64_t vi_sN, int64_t H, int64_t W, void* attr_grad, void* bary_grad, drtk_stream_t stream);
/* The same with an OPTIONAL scratch buffer (round 6).  For float attributes of 11 ... 15 channels with both gradients requested
 * (rows of attr_grad that are not whole 64-byte segments, one channel chunk) the vertex gradient is accumulated in rows padded
 * to 64 bytes inside `workspace` and compacted into attr_grad afterwards: 4-10 % faster than the unpadded route's vertex table
 * (C = 12 0.617 -> 0.554 ms on 8 x 2048^2; other shapes measured slower padded and do not pad).  `_workspace_bytes` returns 0
 * where no workspace is used; a NULL or too small workspace is never an error -- the call then takes the unpadded route of
 * drtk_amd_interpolate_backward.  The workspace must be 64-byte aligned; nothing in it survives the call.  Results equal the
 * unpadded route's up to the order of float summation. */
int drtk_amd_interpolate_backward_workspace_bytes(drtk_dtype_t dtype, int64_t N, int64_t V, int64_t C, size_t* bytes);
int drtk_amd_interpolate_backward_ws(
    drtk_dtype_t dtype, const void* grad_out, const void* attrs, const int32_t* vi,
    const int32_t* index_img, const void* bary_img, int64_t N, int64_t V, int64_t C, int64_t F,
    int64_t vi_sN, int64_t H, int64_t W, void* attr_grad, void* bary_grad, void* workspace, size_t workspace_bytes,
    drtk_stream_t stream);

/* ------------------------------------------------------------------------------------------
 * edge_grad_backward  replaces edge_grad_estimator_cuda_backward (src/edge_grad/edge_grad_kernel.cu:475-506)
 * grad_v_pix_img [N,3,H,W] is fully written (the reference zero-fills and scatters with
 * atomics, edge_grad_kernel.cu:430-445,489; this implementation gathers, same values).
 * `workspace` holds the two per-pixel pair terms (2*N*H*W scalars); query its size first.
 */
int drtk_amd_edge_grad_backward_workspace_bytes(
    drtk_dtype_t dtype, int64_t N, int64_t H, int64_t W, size_t* bytes);
int drtk_amd_edge_grad_backward(
    drtk_dtype_t dtype, const void* v_pix, const void* img, const int32_t* index_img,
    const int32_t* vi, const void* grad_output, int64_t N, int64_t V, int64_t C, int64_t F,
    int64_t vi_sN, int64_t H, int64_t W, double max_dp_dr, void* grad_v_pix_img, void* workspace,
    size_t workspace_bytes, drtk_stream_t stream);

/* edge_grad_backward_fused  =  edge_grad_backward followed by the C=3 interpolate backward that
 * drtk.edge_grad_estimator hangs behind it (drtk/edge_grad_estimator.py:168-176 + interpolate_kernel.cu
 * :642-697), without materialising grad_v_pix_img: writes grad_v_pix [N,V,3] (zero-filled here) directly.
 * Same values as the two calls (within float summation order).  Used by drtk_amd.edge_grad_estimator
 * when no v_pix_img hook is registered.
 */
int drtk_amd_edge_grad_backward_fused_workspace_bytes(
    drtk_dtype_t dtype, int64_t N, int64_t H, int64_t W, size_t* bytes);
int drtk_amd_edge_grad_backward_fused(
    drtk_dtype_t dtype, const void* v_pix, const void* img, const int32_t* index_img,
    const int32_t* vi, const void* bary_img, const void* grad_output, int64_t N, int64_t V, int64_t C,
    int64_t F, int64_t vi_sN, int64_t H, int64_t W, double max_dp_dr, void* grad_v_pix,
    void* workspace, size_t workspace_bytes, drtk_stream_t stream);

/* ------------------------------------------------------------------------------------------
 * Sparse interpolation operators -- the remaining ops of the reference's interpolate_ext:
 *
 * interpolation_matrix           replaces interpolation_matrix_cuda (interpolate_kernel.cu:699-770):
 *   one CSR row per foreground pixel (row_pixels = flat [N*H*W] indices of index_img != -1, ascending,
 *   computed by the caller), 3 entries per row: vertex columns sorted ascending with their
 *   barycentric weights.  crow_indices is arange(0, 3R+1, 3) and is left to the caller.
 * interpolation_matrix_backward  replaces interpolation_matrix_cuda_backward (:772-819): scatters
 *   d values back to bary_grad [N,3,H,W] (zero-filled here).
 * interpolation_normal_matrix_values[_backward]  replace ..._values_cuda[_backward] (:821-907):
 *   values[pair_indices[n,tri,3i+j]] += bary_i * bary_j over foreground pixels (values zero-filled
 *   here); pair_indices [N,F,9] int32 with batch stride pair_sN (0 = shared).  The CSR pattern itself
 *   (crow / col / pair_indices) is topology-only host work done by the torch shim.
 * All four judge dtype and sizes first -- an unknown dtype is DRTK_ERR_INVALID_ARGUMENT also where there is nothing to do
 * (R == 0, nnz == 0, no pixel) -- and every pointer before they write: a rejected call has cleared nothing.
 */
int drtk_amd_interpolation_matrix(
    drtk_dtype_t dtype, const int32_t* vi, const int32_t* index_img, const void* bary_img,
    const int64_t* row_pixels, int64_t R, int64_t N, int64_t F, int64_t vi_sN, int64_t H, int64_t W,
    int64_t* col_indices, void* values, drtk_stream_t stream);
int drtk_amd_interpolation_matrix_backward(
    drtk_dtype_t dtype, const void* grad_values, const int32_t* vi, const int32_t* index_img,
    const int64_t* row_pixels, int64_t R, int64_t N, int64_t F, int64_t vi_sN, int64_t H, int64_t W,
    void* bary_grad, drtk_stream_t stream);
int drtk_amd_interpolation_normal_matrix_values(
    drtk_dtype_t dtype, const int32_t* pair_indices, const int32_t* index_img, const void* bary_img,
    int64_t N, int64_t F, int64_t pair_sN, int64_t H, int64_t W, int64_t nnz, void* values,
    drtk_stream_t stream);
int drtk_amd_interpolation_normal_matrix_values_backward(
    drtk_dtype_t dtype, const void* grad_values, const int32_t* pair_indices, const int32_t* index_img,
    const void* bary_img, int64_t N, int64_t F, int64_t pair_sN, int64_t H, int64_t W, void* bary_grad,
    drtk_stream_t stream);

/* ------------------------------------------------------------------------------------------
 * mipmap_grid_sampler_2d -- grid_sample with trilinear mip selection and anisotropic taps; replaces
 * mipmap_aniso_grid_sampler_2d_cuda / _cuda_backward (mipmap_grid_sampler_kernel.cu:899-1249).
 *   levels[l]    device pointer of mip level l, [N,C,level_h[l],level_w[l]] with contiguous views, l < mipmaps <= 11
 *                (the arrays levels / level_h / level_w / level_sN / grad_levels themselves are HOST arrays)
 *   level_sN[l]  elements between consecutive views of level l: C*h*w for a contiguous tensor, 0 for ONE texture
 *                shared by all views (a [1,C,h,w] tensor expanded to N: the reference indexes through the tensor's
 *                strides, mipmap_grid_sampler_kernel.cu:40,65 (`input.data + n * inp_sN`), so an expanded pyramid is never copied);
 *                NULL = every level contiguous
 *   grid         [N,H,W,2] uv in [-1,1];  vt_dxdy_img [N,H,W,2,2] = [[du/dx, dv/dx],[du/dy, dv/dy]], contiguous
 *   grid_layout  HOST array {sN, sP, sC}: element (n, pixel y*W+x, c) of grid lies n*sN + pixel*sP + c*sC elements from
 *                `grid` (the reference reads grid through its strides, :430-445).  NULL = contiguous {2HW, 2, 1}; the
 *                channel-first uv image of `interpolate` seen through permute(0,2,3,1) is {2HW, 1, HW} -- no copy.
 *                grad_grid_layout: the same for grad_grid (every element is written)
 *   out          [N,C,H,W]
 *   padding_mode 0 zeros | 1 border | 2 reflection;  interpolation_mode 0 bilinear | 2 bicubic
 *   align_corners is ignored by the forward pass and honoured by the backward pass -- as in the
 *   reference (:423 vs :641-897).
 * Backward: grad_levels[l] (contiguous [N,C,h,w] whatever level_sN is, zero-filled here) and grad_grid [N,H,W,2]
 * (fully written); no gradient is defined for vt_dxdy_img.
 * NO ALIASING: grad_grid and grad_levels[] must not overlap any input (grad_out, levels, grid, vt_dxdy_img) nor each other --
 * textures of more than four channels are processed in several launches of one stream, each adding its part of the grid
 * gradient to what the previous launch stored (the torch operator allocates fresh outputs; tests/test_gpu_mipmap.py covers
 * C = 5 ... 16 in both grid layouts).
 * FINITE TEXELS ASSUMED where a weight is exactly zero: the forward pass skips a mip level whose blend weight is
 * exactly 0, the backward pass skips (pixel, level) pairs whose weighted upstream gradient is 0 in every channel and
 * whole tiles without upstream gradient.  The reference evaluates 0 * texel there, so an Inf / NaN texel in a level
 * that does not contribute (or under a zero upstream gradient) turns its output / gradient into NaN; here the
 * result stays finite.  For finite textures the two agree exactly (tests/test_gpu_mipmap.py pins the difference).
 */
int drtk_amd_mipmap_grid_sampler_2d(
    drtk_dtype_t dtype, const void* const* levels, const int64_t* level_h, const int64_t* level_w,
    const int64_t* level_sN, int mipmaps, const void* grid, const int64_t* grid_layout, const void* vt_dxdy_img, int64_t N,
    int64_t C, int64_t H, int64_t W, int max_aniso, int padding_mode, int interpolation_mode, int align_corners,
    int force_max_aniso, int clip_grad, void* out, drtk_stream_t stream);
int drtk_amd_mipmap_grid_sampler_2d_backward(
    drtk_dtype_t dtype, const void* grad_out, const void* const* levels, const int64_t* level_h,
    const int64_t* level_w, const int64_t* level_sN, int mipmaps, const void* grid, const int64_t* grid_layout,
    const void* vt_dxdy_img, int64_t N, int64_t C, int64_t H, int64_t W, int max_aniso, int padding_mode,
    int interpolation_mode, int align_corners, int force_max_aniso, int clip_grad, void* const* grad_levels,
    void* grad_grid, const int64_t* grad_grid_layout, drtk_stream_t stream);

/* ------------------------------------------------------------------------------------------
 * grid_scatter_2d -- the splatting counterpart of grid_sample: every input pixel ADDS weight * input to the texels
 * grid_sample would have read at its grid location; replaces grid_scatter_2d_cuda / _cuda_backward
 * (grid_scatter_kernel.cu:624-788).  Coordinates are grid_sample's: normalised [-1,1], align_corners, padding.
 *   input        [N,C,H,W] contiguous;  grid [N,H,W,2], read through grid_layout (see mipmap_grid_sampler_2d: NULL =
 *                contiguous, {2HW, 1, HW} = the channel-first uv image of `interpolate` seen through permute(0,2,3,1))
 *   out          [N,C,output_height,output_width]; zero-filled here (a fill kernel on `stream`), then accumulated into
 *   padding_mode 0 zeros | 1 border | 2 reflection;  interpolation_mode 0 bilinear | 2 bicubic
 *   route_counts NULL, or two device counters the caller has zeroed: the call adds the number of workgroups (tiles of
 *                16 x 16 input pixels that reach the output at all) that took the windowed route -- the texels of the tile
 *                fit an LDS window, one global atomic per touched texel, channel and workgroup, in row segments -- to
 *                [0], and of those that fell back to one global atomic per tap and channel to [1].  The route is chosen
 *                on the device from the tile's own grid values; the host never reads the grid.  Diagnostics only.
 * H * W < 2^31 and output_height * output_width < 2^31, both output sizes > 0.  Non-finite grid coordinates add nothing
 * (zeros padding) or land on a border texel; they never write out of range.
 * BICUBIC CENTRE RULE: as in the reference, the centre coordinate goes through the whole padding transform (clip, or reflect
 * and clip) before floor and the fractional part are taken, and each of the sixteen tap indices goes through it again;
 * torch's grid_sample only unnormalises the centre.  The two differ for border / reflection padding where the unnormalised
 * coordinate lies outside [0, size - 1]; everywhere else (all bilinear modes, bicubic zeros) out is exactly the adjoint of
 * grid_sample ("Texture-space scatter").
 * REPRODUCIBILITY: out is accumulated with float atomics in varying order: equal up to rounding from run to run, not
 * bitwise (the reference's is atomic-ordered too).  The backward pass is a gather and bit-reproducible.
 * Backward: grad_input [N,C,H,W] = grid_sample(grad_out, grid) and grad_grid (laid out by grad_grid_layout) =
 * d/dgrid <grid_sample(grad_out, grid), input>; either may be NULL (not computed), what is given is written fully.
 * `input` is only read for grad_grid.
 */
int drtk_amd_grid_scatter_2d(
    drtk_dtype_t dtype, const void* input, const void* grid, const int64_t* grid_layout, int64_t N, int64_t C, int64_t H,
    int64_t W, int64_t output_height, int64_t output_width, int padding_mode, int interpolation_mode, int align_corners,
    void* out, uint32_t* route_counts, drtk_stream_t stream);
int drtk_amd_grid_scatter_2d_backward(
    drtk_dtype_t dtype, const void* grad_out, const void* input, const void* grid, const int64_t* grid_layout, int64_t N,
    int64_t C, int64_t H, int64_t W, int64_t output_height, int64_t output_width, int padding_mode, int interpolation_mode,
    int align_corners, void* grad_input, void* grad_grid, const int64_t* grad_grid_layout, drtk_stream_t stream);

/* ------------------------------------------------------------------------------------------
 * msi -- multi-sphere-image background rendering (NeRF++ style): a stack of L equirectangular RGB-sigma layers on
 * concentric spheres, one ray per pixel marched through them from the inside out; replaces msi_forward_cuda /
 * msi_backward_cuda (msi_kernel.cu:411-628).
 *   ray_o, ray_d [N,3] float32 (whatever the texture's type; ray_d need not be normalised);  texture [L,4,H,W] (r, g, b,
 *   sigma), contiguous;  out [N,4] = (r, g, b, log_transmit), written fully.
 *   n = L * sub_step_count spheres with inverse radii from min_inv_r (innermost) towards max_inv_r, sampled bilinearly
 *   within a layer and by cubic convolution (A = -0.75) across layers, coordinates as grid_sample's align_corners=False
 *   with border padding; a sample with sigma > 0 adds exp(lt) (1 - exp(-sigma / n)) max(rgb, 0) and lowers lt by
 *   sigma / n; a ray whose exp(lt) falls below stop_thresh ends with log_transmit = -1000 (csrc/msi.hip has every step).
 *   sub_step_count >= 1, min_inv_r > max_inv_r, 0 < stop_thresh < 1, N < 2^31, L * 4 * H * W < 2^31.
 * The texture is read in place, as given: a tap is four loads H * W apart.  No workspace.
 * ELEMENT TYPES: DRTK_F32 is the tuned path.  With DRTK_F64 the rays are promoted to double on load and the geometry
 * runs in double too (the reference keeps it in float).
 * Backward: grad_texture [L,4,H,W] only (the rays get no gradient), zero-filled here and accumulated into; `out` is the
 * forward's result; grad_out [N,4], of which column 3 is not read.
 * SIGMA GRADIENT: the reference's expression, sum_ch(max(rgb, 0) g exp(-sigma) T - acc) with T = exp(lt) after the sample
 * and acc the part of g . out_rgb not yet composited -- not the derivative of the forward, which is
 * (ref + sum_ch max(rgb, 0) g T (1 - exp(-sigma))) / n ("Multi-sphere background").
 * REPRODUCIBILITY: the forward is a gather and bit-reproducible; grad_texture is summed with float atomics in varying
 * order: equal up to rounding from run to run, not bitwise (the reference's is atomic-ordered too).
 */
int drtk_amd_msi_forward(
    drtk_dtype_t dtype, const float* ray_o, const float* ray_d, const void* texture, int64_t N, int64_t L, int64_t H, int64_t W,
    int sub_step_count, double min_inv_r, double max_inv_r, double stop_thresh, void* out, drtk_stream_t stream);
int drtk_amd_msi_backward(
    drtk_dtype_t dtype, const void* grad_out, const void* out, const float* ray_o, const float* ray_d, const void* texture,
    int64_t N, int64_t L, int64_t H, int64_t W, int sub_step_count, double min_inv_r, double max_inv_r, double stop_thresh,
    void* grad_texture, drtk_stream_t stream);

/* ------------------------------------------------------------------------------------------
 * composite_layers -- front-to-back compositing of K layers (what rasterize_layers + render + interpolate produce) into
 * one image, forward and backward, one streaming kernel each way; no reference counterpart.  Per pixel, in the tensors'
 * own type and in this order of operations (the forward is this loop bit for bit):
 *   img = 0, T = 1;  for k = 0 .. K-1 (0 is nearest): img[c] = img[c] + (T * a_k) * color[k][c], T = T * (1 - a_k);
 *   with a background: img[c] = img[c] + T * background[c].
 *   color [N,K,C,H,W] and alpha [N,K,H,W]: every H x W plane contiguous, element strides between planes given as
 *     color_strides = {view, layer, channel}, alpha_strides = {view, layer} (all >= 0) -- split tensors, one rgba tensor
 *     [N,K,C+1,H,W] (alpha = color + C * H * W, same view / layer strides) and channel slices are read in place.
 *   index_img [N,K,H,W] int32, contiguous, or NULL: a layer whose index is -1 is SKIPPED (it may sit between two present
 *     layers); neither its colour nor its alpha is read, so a NaN there does not propagate.  NULL: all layers present.
 *   background [N,C,H,W] with view stride background_sN (0: one image for all views) and contiguous views, or NULL.
 *   img [N,C,H,W], transmittance [N,1,H,W]: contiguous, written fully.
 *   Once T is exactly 0 the colours behind are not read (for finite inputs the result is the same bit for bit).
 *   1 <= K <= DRTK_AMD_MAX_RASTER_LAYERS, C >= 1 (any), H * W < 2^31, any N; DRTK_F32 and DRTK_F64; tensors need the
 *   alignment of their element only.  Judged first, before any pointer: dtype, sizes, K.  N * H * W == 0: DRTK_OK, nothing
 *   is looked at.  No workspace, no atomics: bitwise reproducible.  Enqueues only (no sync, no host read).
 * Backward (division-free, exact at alpha == 1): with T_k the transmittance in front of layer k, g = grad_img,
 *   d_k = sum_c color[k][c] g[c] and R_K = grad_transmittance + sum_c background[c] g[c], for k = K-1 .. 0
 *   grad_alpha[k] = T_k (d_k - R_{k+1}), R_k = a_k d_k + (1 - a_k) R_{k+1};  grad_color[k][c] = (T_k a_k) g[c];
 *   grad_background[c] = T_K g[c].  grad_img [N,C,H,W] and grad_transmittance [N,1,H,W] are contiguous; either may be NULL
 *   (taken as zeros, never read).  grad_color / grad_alpha are laid out by their own stride triples / pairs, grad_background
 *   is [N,C,H,W] contiguous (also when the background was shared between views); each may be NULL (not wanted, its strides
 *   are then not looked at) and each one given is written fully, zeros at skipped layers.  grad_background needs background.
 */
int drtk_amd_composite_layers(
    drtk_dtype_t dtype, const void* color, const int64_t* color_strides, const void* alpha, const int64_t* alpha_strides,
    const int32_t* index_img, const void* background, int64_t background_sN, int64_t N, int64_t K, int64_t C, int64_t H, int64_t W,
    void* img, void* transmittance, drtk_stream_t stream);
int drtk_amd_composite_layers_backward(
    drtk_dtype_t dtype, const void* grad_img, const void* grad_transmittance, const void* color, const int64_t* color_strides,
    const void* alpha, const int64_t* alpha_strides, const int32_t* index_img, const void* background, int64_t background_sN,
    int64_t N, int64_t K, int64_t C, int64_t H, int64_t W, void* grad_color, const int64_t* grad_color_strides, void* grad_alpha,
    const int64_t* grad_alpha_strides, void* grad_background, drtk_stream_t stream);

/* ------------------------------------------------------------------------------------------
 * mipmap_pyramid -- the mip chain that mipmap_grid_sampler_2d reads, made from one texture in one pass (two launches
 * beyond seven levels), and its backward: the sampler's per-level gradients folded back into the texture in one launch.
 * No reference counterpart (its callers loop over avg_pool2d).  In the tensor's own type, every level from the previous
 * level as stored, in this order of operations (avg_pool2d's chain bit for bit):
 *   h_{l+1} = h_l / 2, w_{l+1} = w_l / 2 (floor: a trailing odd row / column is dropped);
 *   x_{l+1}[i][j] = (((x_l[2i][2j] + x_l[2i][2j+1]) + x_l[2i+1][2j]) + x_l[2i+1][2j+1]) * 0.25.
 *   input [N,C,H,W]: every H x W plane contiguous, element strides input_sN (view) and input_sC (channel), both >= 0 --
 *     channel slices and a view-shared texture are read in place.  It is level 0 and is not written.
 *   out, out_sN: `levels` entries; out[l] is level l, [N,C,H >> l,W >> l] with contiguous views out_sN[l] >= 0 elements
 *     apart, written fully, each element once.  Entry 0 is not looked at.
 *   1 <= levels <= min(11, 1 + floor(log2(min(H, W)))), C >= 1 (any), H * W < 2^31, any N; DRTK_F32 and DRTK_F64; tensors
 *   need the alignment of their element only (rows move as 16-byte vectors where the address allows).  Judged first,
 *   before any pointer: dtype, sizes, levels.  N * H * W == 0 or levels == 1: DRTK_OK, nothing is looked at or launched.
 *   No workspace, no atomics: bitwise reproducible.  Enqueues only (no sync, no host read).
 * Backward: with g_l = grad_levels[l], [N,C,H >> l,W >> l] with contiguous views grad_sN[l] elements apart, or NULL (taken
 *   as zeros, never read; its stride is then not looked at):
 *   G_{levels-1} = g_{levels-1};  G_l[i][j] = g_l[i][j] + 0.25 * G_{l+1}[i/2][j/2];  grad_input = G_0, [N,C,H,W] contiguous,
 *   written fully, each element once.  A texel of a dropped row / column has no parent and keeps g_l alone.  One add and
 *   one exact multiply per level: the order of the sum is unique, the result is autograd of the chain bit for bit.
 */
int drtk_amd_mipmap_pyramid(
    drtk_dtype_t dtype, const void* input, int64_t input_sN, int64_t input_sC, int64_t N, int64_t C, int64_t H, int64_t W, int levels,
    void* const* out, const int64_t* out_sN, drtk_stream_t stream);
int drtk_amd_mipmap_pyramid_backward(
    drtk_dtype_t dtype, const void* const* grad_levels, const int64_t* grad_sN, int64_t N, int64_t C, int64_t H, int64_t W, int levels,
    void* grad_input, drtk_stream_t stream);

/* ------------------------------------------------------------------------------------------
 * filter2d -- fused separable up/down-sampling FIR filters: zero-insertion by `up`, a k-tap 1-D filter f (float32,
 * whatever the image's type) along both axes, decimation by `down`, one kernel, no workspace; replaces filter2d_cuda
 * (src/filter2d/filter2d.cpp, filter2d_kernel.cu) without its limits: any (up, down, k) the rule below admits (the
 * reference's table of tuned combinations is compiled with the taps unrolled, everything else takes a generic
 * instantiation, up to the k whose tile of one output row still fits the 160 KiB of LDS: DRTK_ERR_UNSUPPORTED beyond), a
 * double kernel, any number of planes.
 *   x [planes,H,W] -> y [planes,OH,OW], contiguous, written fully; planes = N * C.  Per axis (floor divisions):
 *     pad0 = k / 2 if up == down == 1, (k - down + 1) / 2 if down != 1, else (k + up - 1) / 2
 *     pad1 = (k - 1) / 2           |   (k - down) / 2                |      (k - up) / 2
 *     total = pad0 + pad1,  out = (in * up + total - k + down) / down     (drtk_amd_filter2d_output_size: host only)
 *     backward == 0:  lead = pad0,  F[j] = f[k - 1 - j]
 *     backward != 0:  lead = k - 1 - pad0 of (up = down, down = up),  F[j] = f[j]: the call is the gradient of the
 *                     operator with the factors exchanged, applied to its grad_out
 *     y[o] = sum_j Z[o * down + j - lead] F[j],  Z[u] = X[u / up] where up divides u, else 0;  X outside the image is 0
 *     (reflect == 0) or read at one reflection that does not repeat the edge (reflect != 0).
 *   The horizontal pass runs first and is not rounded to the storage type before the vertical one; sums are float for
 *   DRTK_F16 and DRTK_F32, double for DRTK_F64, taps in ascending order.  Bitwise reproducible.
 * DRTK_ERR_INVALID_ARGUMENT, judged before any pointer is looked at: an unknown dtype, planes < 0, H, W, k, up or down
 * below 1, a filter too short for the sampling factors (lead < 0 or total - lead < 0), an output smaller than 1 x 1,
 * reflection with ceil(lead / up) or ceil((total - lead) / up) not below H and W (torch's rule for reflect padding), sizes
 * past 2^31; then planes == 0 is DRTK_OK without a launch, and a null x, f or y is invalid.
 * UNDER REFLECTION the `backward` call is the reference's expression, NOT the derivative of the forward: within a filter's
 * reach of the border it reflects the incoming gradient instead of folding the border contributions back.  With zeros
 * padding it is the exact adjoint.
 * force_generic != 0 (TESTS ONLY) sends a tuned combination through the generic instantiation.
 */
int drtk_amd_filter2d_output_size(int64_t in, int64_t k, int64_t up, int64_t down, int64_t* out);
int drtk_amd_filter2d(
    drtk_dtype_t dtype, const void* x, const float* f, int64_t planes, int64_t H, int64_t W, int64_t k, int64_t up, int64_t down,
    int reflect, int backward, int force_generic, void* y, drtk_stream_t stream);

/* ------------------------------------------------------------------------------------------
 * image_loss -- SSIM and the L1 / D-SSIM photometric loss of two images under a per-pixel weight (the foreground mask of a
 * render), one fused pass each way.  No reference counterpart.  Evaluated in the images' type, sums of the means in double:
 *   g[i] = exp(-(i - r)^2 / (2 sigma^2)), r = window_size / 2, normalised to sum 1 (host, double); G*z the separable blur
 *   of a channel with g.  valid == 0 ("same"): zeros outside the image, the map domain D is the image, OH = H, OW = W;
 *   valid != 0: only windows inside the image, D is the interior, OH = H - 2r, OW = W - 2r (H, W >= window_size).
 *   C1 = (0.01 data_range)^2, C2 = (0.03 data_range)^2;  mu_x = G*x, mu_y = G*y, s_x = G*(x x) - mu_x^2, s_y = G*(y y) - mu_y^2,
 *   s_xy = G*(x y) - mu_x mu_y;  A1 = 2 mu_x mu_y + C1, A2 = 2 s_xy + C2, B1 = mu_x^2 + mu_y^2 + C1, B2 = s_x + s_y + C2;
 *   S = A1 A2 / (B1 B2), [N,C,OH,OW];  ssim = sum_D(w S) / (C sum_D w) with w cropped to D;  l1 = sum(w |x - y|) / (C sum w)
 *   over the whole image.  A weight sum of 0 makes that mean, and its gradient, 0 (decided on the device).
 *   mode 0: out = S (contiguous [N,C,OH,OW]; weight_kind must be 0; scalars and workspace are not looked at)
 *   mode 1: out[0] = ssim            mode 2: out[0] = l1_weight l1 + ssim_weight (1 - ssim)
 *   img, target [N,C,H,W]: rows contiguous, strides {sN, sC, sH} in elements, all >= 0 (channel and view slices are read
 *     in place).  weight [N,H,W], strides {sN, sH}: weight_kind 0 none (w = 1), 1 bytes (nonzero is 1), 2 the images' type;
 *     assumed non-negative, never validated.
 *   maps: NULL, or [3,N,C,OH,OW] contiguous, which receives dmu, dxx, dxy below (what the backward needs); without it a
 *     call of mode 1 / 2 writes nothing but its partial sums and scalars.
 *   scalars: 4 doubles (ssim, l1, 1 / (C sum_D w), 1 / (C sum w), an inverse being 0 where its sum is 0), read by the backward
 *     from device memory.  workspace: drtk_amd_image_loss_workspace_bytes, 8-byte aligned: one slot of double partial sums
 *     per workgroup, added in a fixed order by a second, one-workgroup launch.  No atomics, no zero-fill: bitwise
 *     reproducible.  Enqueues only (no sync, no host read, no copy: the window travels in the kernel arguments).
 * Backward, with h the upstream gradient on D, zero outside it -- grad_out is [N,C,OH,OW] (mode 0) or ONE element g, in
 *   which case h = g w / (C sum_D w) (times -ssim_weight in mode 2), formed from `scalars`:
 *   dmu = 2 mu_y (A2 - A1) / (B1 B2) - 2 mu_x S (1 / B1 - 1 / B2),  dxx = -S / B2,  dxy = 2 A1 / (B1 B2)
 *   grad_img = G*(h dmu) + 2 x G*(h dxx) + y G*(h dxy)  [+ g l1_weight w sign(x - y) / (C sum w) in mode 2, sign(0) = 0],
 *   the blurs over the maps zero-extended to the image; [N,C,H,W] contiguous, written fully.  target and weight get none.
 * Judged first, before any pointer: dtype (DRTK_F32, DRTK_F64), mode, weight_kind, window_size odd in 3 ... 15, sigma and
 * data_range positive and finite, N, C, H, W >= 1, H W < 2^31, the "valid" rule, the number of tiles below 2^31.
 */
int drtk_amd_image_loss_workspace_bytes(int64_t N, int64_t H, int64_t W, int window_size, int valid, size_t* bytes);
int drtk_amd_image_loss_forward(
    drtk_dtype_t dtype, const void* img, const int64_t* img_strides, const void* target, const int64_t* target_strides,
    const void* weight, int weight_kind, const int64_t* weight_strides, int64_t N, int64_t C, int64_t H, int64_t W, int window_size,
    double sigma, double data_range, int valid, int mode, double l1_weight, double ssim_weight, void* out, void* maps, void* scalars,
    void* workspace, size_t workspace_bytes, drtk_stream_t stream);
int drtk_amd_image_loss_backward(
    drtk_dtype_t dtype, const void* img, const int64_t* img_strides, const void* target, const int64_t* target_strides,
    const void* weight, int weight_kind, const int64_t* weight_strides, int64_t N, int64_t C, int64_t H, int64_t W, int window_size,
    double sigma, double data_range, int valid, int mode, double l1_weight, double ssim_weight, const void* maps, const void* grad_out,
    const void* scalars, void* grad_img, drtk_stream_t stream);

/* ------------------------------------------------------------------------------------------
 * shade -- Blinn-Phong deferred shading of an interpolated G-buffer, one fused pass each way.  No reference counterpart (the
 * reference's tutorial writes it in PyTorch).  Per pixel of view n, in the tensors' type, unit(x) = x / max(||x||, 1e-12):
 *   L = unit(light_dir);  nv = unit(normal);  d = max(-(nv . L), 0);  col[c] = albedo[c] (d + ambient[c])
 *   with specular != NULL:  w = unit(pos);  h = unit(L - w);  b = max(-(h . nv), 1e-8);  col[c] += b^shininess specular[c]
 *   out[c] = col[c] where index_img is NULL or != -1, else background[c] (0 without one)
 *   with gamma > 0:  out[c] = max(out[c], 0)^(1 / gamma), background pixels included.  gamma == 0: no such step.
 *   normal_img, pos_img [N,3,H,W], albedo_img, background [N,C,H,W]: W stride 1, strides {sN, sC, sH} in elements, all >= 0
 *     (channel slices, view slices, crops and a view-shared background with sN = 0 are read in place); index_img [N,H,W]
 *     int32, strides {sN, sH}.  Element alignment is enough.  Exactly one of albedo (a vector) and albedo_img is given.
 *   light_dir [3], albedo, ambient, specular [C], shininess [1]: one per view (`_sN` = the count) or shared (`_sN` = 0).
 *     1 <= C <= 4.  specular != NULL requires pos_img and shininess.
 *   out [N,C,H,W] contiguous, written fully.  Where index_img == -1 none of normal_img, pos_img, albedo_img is read; where
 *   it is not, background is not.
 * Backward: the derivative of the above; d passes a gradient only where -(nv . L) > 0, b only where -(h . nv) > 1e-8, the
 *   gamma step only where its argument is > 0 (else exactly 0), unit(x) with ||x|| <= 1e-12 is a constant.  Every gradient
 *   pointer may be NULL (not wanted, not computed); the image gradients are contiguous and written fully (0 at background
 *   pixels for the foreground images, 0 at foreground pixels for grad_background); a parameter gradient is one per view
 *   (`_sN` = the count) or the sum over the views (`_sN` = 0), written fully.  The parameter terms are accumulated in
 *   double: one row of 16 doubles per workgroup in `workspace` (drtk_amd_shade_workspace_bytes, 16-byte aligned, looked at
 *   only when a parameter gradient is wanted; alignment is judged before size), added in a fixed order by a second launch,
 *   and by a third for gradients shared by N > 1 views.  No atomics, no zero-fill: bitwise reproducible.  Enqueues only.
 * Judged first, before any pointer: dtype (DRTK_F32, DRTK_F64), N, H, W >= 0, H W < 2^31, 1 <= C <= 4, gamma >= 0 and
 *   finite, the `_sN` values; then N == 0 or H W == 0 is DRTK_OK without a launch.
 */
int drtk_amd_shade_workspace_bytes(drtk_dtype_t dtype, int64_t N, int64_t H, int64_t W, size_t* bytes);
int drtk_amd_shade_forward(
    drtk_dtype_t dtype, const void* normal_img, const int64_t* normal_strides, const void* pos_img, const int64_t* pos_strides,
    const void* albedo_img, const int64_t* albedo_img_strides, const void* background, const int64_t* background_strides,
    const int32_t* index_img, const int64_t* index_strides, const void* light_dir, int64_t light_dir_sN, const void* albedo,
    int64_t albedo_sN, const void* ambient, int64_t ambient_sN, const void* specular, int64_t specular_sN, const void* shininess,
    int64_t shininess_sN, double gamma, int64_t N, int64_t C, int64_t H, int64_t W, void* out, drtk_stream_t stream);
int drtk_amd_shade_backward(
    drtk_dtype_t dtype, const void* grad_out, const void* normal_img, const int64_t* normal_strides, const void* pos_img,
    const int64_t* pos_strides, const void* albedo_img, const int64_t* albedo_img_strides, const void* background,
    const int64_t* background_strides, const int32_t* index_img, const int64_t* index_strides, const void* light_dir,
    int64_t light_dir_sN, const void* albedo, int64_t albedo_sN, const void* ambient, int64_t ambient_sN, const void* specular,
    int64_t specular_sN, const void* shininess, int64_t shininess_sN, double gamma, int64_t N, int64_t C, int64_t H, int64_t W,
    void* grad_normal_img, void* grad_pos_img, void* grad_albedo_img, void* grad_background, void* grad_light_dir,
    int64_t grad_light_dir_sN, void* grad_albedo, int64_t grad_albedo_sN, void* grad_ambient, int64_t grad_ambient_sN,
    void* grad_specular, int64_t grad_specular_sN, void* grad_shininess, int64_t grad_shininess_sN, void* workspace,
    size_t workspace_bytes, drtk_stream_t stream);

/* ------------------------------------------------------------------------------------------
 * screen_space_uv_derivative -- vt_dxdy_img [N,H,W,2,2] = [[du/dx, dv/dx],[du/dy, dv/dy]] per pixel, the
 * Jacobian input of mipmap_grid_sampler_2d; replaces the PyTorch composite
 * drtk/screen_space_uv_derivative.py:15-80 (face_dpdt + 2x interpolate + project_points_grad + inv_ex +
 * mask) with one kernel.  Pinhole cameras only (as project_points_grad, projection.py:650-709).
 *   v [N,V,3] world-space (v_sN = 3V, or 0 for one shared [V,3]);  vt [N,T,2] (vt_sN = 2T or 0)
 *   vi, vti [F,3] int32;  index_img [N,H,W];  bary_img [N,3,H,W];  mask [N,H,W] uint8 or NULL
 *   campos [N,3], camrot [N,3,3], focal [N,2,2].   Pixels with index -1 or mask 0 are written 0.
 * A face with ZERO UV AREA: the reference inverts every face's UV edge matrix up front (face_dpdt,
 * drtk/utils/geometry.py:71-82, th.inverse) and raises for the whole call, visible face or not.  This kernel works
 * per pixel and never inverts that matrix (J^-1 = (A^-1 G)^-1 is evaluated as G^-1 A, A the UV edge matrix, G the
 * projected position edges): pixels of such a face get the finite limit, every other pixel is unaffected.  The one
 * 2x2 inverse left is ill-conditioned for triangles seen edge-on ON SCREEN, where the derivative itself is large; in
 * float32 the result is as near the float64 composite as the reference's float32 composite is, and 10-30x nearer on
 * faces that are slivers in UV space (tests/fuzz_next_ops.py).
 * Forward only.  (The reference composite looks differentiable but is not: it masks the output of linalg.inv_ex in
 * place, drtk/screen_space_uv_derivative.py:79, and backward() through it raises -- recorded from the reference in
 * tests/golden/refpy_uv_derivative_autograd.npz; its consumer, mipmap_grid_sampler_2d, defines no gradient for this
 * input.  The Python wrapper reproduces exactly that: part of the graph, an error only if a gradient arrives.)
 */
int drtk_amd_screen_space_uv_derivative(
    drtk_dtype_t dtype, const void* v, int64_t v_sN, const void* vt, int64_t vt_sN, const int32_t* vi,
    const int32_t* vti, const int32_t* index_img, const void* bary_img, const uint8_t* mask,
    const void* campos, const void* camrot, const void* focal, int64_t N, int64_t V, int64_t T, int64_t F,
    int64_t H, int64_t W, void* out, drtk_stream_t stream);

/* ------------------------------------------------------------------------------------------
 * transform_pinhole  -- the vertex stage in front of the path; replaces the pure-PyTorch pinhole
 * branch of drtk.transform (drtk/transform.py:13-119, drtk/utils/projection.py:33-53,486-540):
 *   v_cam = camrot (v - campos);  v_pix = (focal (v_cam.xy / clamp(v_cam.z)) + princpt, v_cam.z)
 * v: [N,V,3] (v_sN = 3V) or ONE shared [V,3] (v_sN = 0); campos [N,3], camrot [N,3,3] row-major,
 * focal [N,2,2], princpt [N,2]; v_pix [N,V,3]; v_cam [N,V,3] or NULL.
 * The backward gives the gradient wrt v only ([N,V,3], or [V,3] already summed over the views
 * when v is shared); camera parameters are treated as constants.
 */
int drtk_amd_transform_pinhole(
    drtk_dtype_t dtype, const void* v, int64_t v_sN, const void* campos, const void* camrot,
    const void* focal, const void* princpt, int64_t N, int64_t V, void* v_pix, void* v_cam,
    drtk_stream_t stream);
int drtk_amd_transform_pinhole_backward(
    drtk_dtype_t dtype, const void* v, int64_t v_sN, const void* campos, const void* camrot,
    const void* focal, const void* princpt, const void* grad_v_pix, int64_t N, int64_t V,
    void* grad_v, drtk_stream_t stream);

/* ------------------------------------------------------------------------------------------
 * transform_distort  -- transform_pinhole with the distortion camera models of drtk.transform
 * (drtk/utils/projection.py:56-310, 618-644), one kernel each way.  The pinhole arguments as above, plus:
 *   mode_all       0 pinhole, 1 radial-tangential, 2 fisheye, 3 fisheye62 -- the model of every view ...
 *   mode_per_view  ... unless this device int32 [N] is given (NULL: mode_all); an id outside 0..3 projects as pinhole
 *   coeff          [N,ncoef], ncoef 4, 5 or 8: radial-tangential (k1,k2,p1,p2[,k3[,k4,k5,k6]]); fisheye reads the first
 *                  four; fisheye62 (k0..k5,p0,p1) needs ncoef = 8 (coefficients a row does not have read as 0)
 *   fov            [N] the largest normalised radius (+inf allowed); not read by pinhole views
 *   cull_outside_fov  nonzero: a fisheye62 vertex with |(x/z, y/z)| > fov gets v_pix.z = -1 (the rasterizer culls it)
 *   lut, lut_spacing  [N,2,Hl,Wl] pixel offsets and [N,2] spacing, or NULL: added to the pixel position of fisheye62
 *                  views, bilinear with align_corners; x is normalised by Hl - 1 and y by Wl - 1 as the reference does,
 *                  and the offset is zero where the normalised position leaves [-1, 1]
 * v_pix [N,V,3]; v_cam [N,V,3] or NULL.  The backward takes grad_v_pix and / or grad_v_cam ([N,V,3], either may be NULL)
 * and gives the gradient wrt v only, as transform_pinhole_backward does; every clamp of the models has zero gradient
 * where it is active, and on the optical axis of the fisheye models (r < 1e-8) the gradient is finite.
 */
int drtk_amd_transform_distort(
    drtk_dtype_t dtype, const void* v, int64_t v_sN, const void* campos, const void* camrot, const void* focal,
    const void* princpt, int mode_all, const int32_t* mode_per_view, const void* coeff, int ncoef, const void* fov,
    int cull_outside_fov, const void* lut, const void* lut_spacing, int64_t Hl, int64_t Wl, int64_t N, int64_t V,
    void* v_pix, void* v_cam, drtk_stream_t stream);
int drtk_amd_transform_distort_backward(
    drtk_dtype_t dtype, const void* v, int64_t v_sN, const void* campos, const void* camrot, const void* focal,
    const void* princpt, int mode_all, const int32_t* mode_per_view, const void* coeff, int ncoef, const void* fov,
    int cull_outside_fov, const void* lut, const void* lut_spacing, int64_t Hl, int64_t Wl, const void* grad_v_pix,
    const void* grad_v_cam, int64_t N, int64_t V, void* grad_v, drtk_stream_t stream);

/* ------------------------------------------------------------------------------------------
 * Mesh geometry -- drtk.utils.geometry (face_info, vert_normals, face_attribute_to_vert, face_dpdt, vert_binormals;
 * pure PyTorch in the reference: drtk/utils/geometry.py) in two passes without float atomics.
 *
 * Shapes: v [N,V,3] (v_sN = 3V, or 0: one [V,3] shared by the views); vi int32 [N,F,3] (vi_sN = 3F) or [F,3]
 * (vi_sN = 0); vt [N,T,2] (vt_sN = 2T or 0); vti int32 [F,3].  Every launch is a 1-D grid over N*F or N*V lanes with
 * 64-bit offsets (any N).
 *
 * Vertex incidence (CSR), built by the caller once per index tensor (drtk_amd_ext::vertex_incidence builds and caches
 * it; drtk_amd/capi.py has a numpy builder):
 *   B        topology batches: 1 (vi shared by all views) or N
 *   crow     int32 [B*V+1]   row r = b*V + vertex; crow[0] = 0, crow[B*V] = 3*B*F
 *   entries  int32 [3*B*F]   the (face, corner) pairs f*3+k of row r, local to its batch, ASCENDING within the row
 * Rows longer than DRTK_GEOMETRY_CHUNK entries are summed in chunks of that length (an empty chunk list is allowed
 * when no row is longer):
 *   chunk_ptr   int32 [B*V+1]  row r's chunks are chunk_ptr[r] .. chunk_ptr[r+1]-1 (none: the row is short)
 *   chunk_begin int32 [C]      first entry of the chunk (crow[row] + j*DRTK_GEOMETRY_CHUNK for its j-th chunk)
 *   chunk_row   int32 [C]      its row
 * The kernels trust the incidence (it is not validated on the device): every crow / entries / chunk value must lie in
 * range, and every index of vi / vti in [0, V) / [0, T).
 *
 * face_forward: per (view, face) with c = (p0 - p2) x (p1 - p0): normals [N,F,3] = c / max(|c|, 1e-8),
 *   areas [N,F,1] = |c| / 2, edges [N,F,3,3] = (p1-p0, p0-p2, p2-p1), and with vt/vti: dpdt [N,F,2,3] =
 *   inv([t1-t0; t2-t0]) [p1-p0; p2-p0] (closed-form 2x2 inverse, formed in double for either dtype, as are the
 *   gradients through it: a singular UV matrix gives inf / nan where the reference raises), dpdt_u [N,F,3] = its first row, v012 [N,F,3,3] = (p0, p1, p2).  NULL outputs are skipped;
 *   at least one must be given.
 * face_backward: per-corner gradient rows pos_rows [N,F,3,3] (and, with vt given, uv_rows [N,F,3,2]) of the face
 *   pass from the optional upstream gradients grad_normals / grad_areas / grad_edges (vt NULL) or grad_dpdt /
 *   grad_v012 (vt given), plus an optional per-VERTEX gradient grad_vert [N,V,3] gathered at the three corners -- of
 *   the normals (vt NULL: vert_normals) or of dpdt's first row (vt given: vert_binormals) -- through F.normalize's
 *   backward (eps 1e-12) from vert_sums [N,V,3], the unnormalised sums, when those are given.  Reduce the rows to
 *   grad_v (grad_vt) with vertex_gather (per_corner = 1) over the vi (vti) incidence.
 * face_gather: out [N,F,A] = sum over the three corners of grad_vert [N,V,A] (through F.normalize's backward from
 *   vert_sums when given; A = 3 then): the backward of face_attribute_to_vert.
 * vertex_gather: out [N,V,A] = per row, the sum of src rows (src [N,F,A] with per_corner = 0: row f = entry / 3;
 *   [N,F,3,A] with per_corner = 1: row = entry; src_sN = F*A*(per_corner ? 3 : 1)) in entry order; a chunked row adds
 *   its chunk sums in chunk order.  normalize = 1 (A = 3): out = sum / max(|sum|, 1e-12) and vert_sums (optional)
 *   receives the sums.  With chunks the call needs a workspace of _workspace_bytes (any alignment of the element type).
 * Results are bitwise reproducible: every sum has one fixed order, independent of the launch shape.
 */
#define DRTK_GEOMETRY_CHUNK 256
int drtk_amd_geometry_face_forward(
    drtk_dtype_t dtype, const void* v, int64_t v_sN, const int32_t* vi, int64_t vi_sN, const void* vt, int64_t vt_sN,
    const int32_t* vti, int64_t N, int64_t V, int64_t T, int64_t F, void* normals, void* areas, void* edges,
    void* dpdt, void* dpdt_u, void* v012, drtk_stream_t stream);
int drtk_amd_geometry_face_backward(
    drtk_dtype_t dtype, const void* v, int64_t v_sN, const int32_t* vi, int64_t vi_sN, const void* vt, int64_t vt_sN,
    const int32_t* vti, int64_t N, int64_t V, int64_t T, int64_t F, const void* grad_vert, const void* vert_sums,
    const void* grad_normals, const void* grad_areas, const void* grad_edges, const void* grad_dpdt,
    const void* grad_v012, void* pos_rows, void* uv_rows, drtk_stream_t stream);
int drtk_amd_geometry_face_gather(
    drtk_dtype_t dtype, const void* grad_vert, const void* vert_sums, const int32_t* vi, int64_t vi_sN, int64_t N,
    int64_t V, int64_t F, int64_t A, void* out, drtk_stream_t stream);
int drtk_amd_geometry_vertex_gather_workspace_bytes(
    drtk_dtype_t dtype, int64_t N, int64_t B, int64_t num_chunks, int64_t A, size_t* bytes);
int drtk_amd_geometry_vertex_gather(
    drtk_dtype_t dtype, const void* src, int64_t src_sN, int per_corner, int64_t A, const int32_t* crow,
    const int32_t* entries, const int32_t* chunk_ptr, const int32_t* chunk_begin, const int32_t* chunk_row,
    int64_t num_chunks, int64_t B, int64_t N, int64_t V, int64_t F, int normalize, void* out, void* vert_sums,
    void* workspace, size_t workspace_bytes, drtk_stream_t stream);

/* ------------------------------------------------------------------------------------------
 * Mesh regulariser -- cotangent weights and the weighted graph Laplacian of a triangle mesh (no counterpart in the
 * reference's library; its hand-fitting tutorial builds a padded table on the host), on the passes and the vertex
 * incidence of "Mesh geometry" above; shapes, strides and trust in the incidence as there.
 *
 * Face f has corners a0, a1, a2 = vi[f]; weight [f,k] belongs to the edge OPPOSITE corner k, a_{k+1} -- a_{k+2}
 * (indices mod 3).
 * cot_weights: weights [N,F,3], w[n,f,k] = dot(p_{k+1} - p_k, p_{k+2} - p_k) / (2 |c|) = cot(angle at corner k) / 2 with
 *   c = (p0 - p2) x (p1 - p0); exactly 0 for all three k where |c| > 0 is false (c zero or NaN).
 * cot_weights_backward: per-corner rows pos_rows [N,F,3,3] of grad_v from grad_weights [N,F,3] (zero rows for a face
 *   with the degenerate zeros); reduce them with vertex_gather (per_corner = 1, A = 3).
 * laplacian: out [N,V,C] from x [N,V,C] (contiguous, C >= 1):
 *     out[n,i,:] = sum over the entries (f,k) of vertex i's incidence row, in entry order, of
 *                  w[f,k+1] * (x[a_{k+2}] - x[i]) + w[f,k+2] * (x[a_{k+1}] - x[i])
 *   = sum_j w_ij (x_j - x_i); each bracket is evaluated as written and then added; a chunked row adds its chunk sums in
 *   chunk order.  weights [N,F,3] (w_sN = 3F) or one [F,3] for all views (w_sN = 0), independent of the topology's
 *   batch; weights NULL (w_sN = 0): every w is 1/2 (the uniform Laplacian: an interior manifold edge totals 1) and no
 *   weight is read.  vi / vi_sN must be the topology the incidence was built from: vi_sN = 0 with B = 1, 3F with
 *   B = N.  The operator is symmetric: its backward with respect to x is the same call on the gradient.  With chunks
 *   the call needs a workspace of _workspace_bytes.
 * laplacian_grad_weights: grad_weights [weights_B,F,3], weights_B = N or 1,
 *     [n,f,k] = -dot(grad_out[a_{k+1}] - grad_out[a_{k+2}], x[a_{k+1}] - x[a_{k+2}]) over the C channels, ascending;
 *   weights_B = 1 (shared weights): the views' dots subtracted from 0 in ascending n.
 * Results are bitwise reproducible: every sum has one fixed order, independent of the launch shape.
 */
int drtk_amd_geometry_cot_weights(
    drtk_dtype_t dtype, const void* v, int64_t v_sN, const int32_t* vi, int64_t vi_sN, int64_t N, int64_t V, int64_t F,
    void* weights, drtk_stream_t stream);
int drtk_amd_geometry_cot_weights_backward(
    drtk_dtype_t dtype, const void* v, int64_t v_sN, const int32_t* vi, int64_t vi_sN, int64_t N, int64_t V, int64_t F,
    const void* grad_weights, void* pos_rows, drtk_stream_t stream);
int drtk_amd_geometry_laplacian_workspace_bytes(
    drtk_dtype_t dtype, int64_t N, int64_t B, int64_t num_chunks, int64_t C, size_t* bytes);
int drtk_amd_geometry_laplacian(
    drtk_dtype_t dtype, const void* x, int64_t C, const int32_t* vi, int64_t vi_sN, const void* weights, int64_t w_sN,
    const int32_t* crow, const int32_t* entries, const int32_t* chunk_ptr, const int32_t* chunk_begin,
    const int32_t* chunk_row, int64_t num_chunks, int64_t B, int64_t N, int64_t V, int64_t F, void* out, void* workspace,
    size_t workspace_bytes, drtk_stream_t stream);
int drtk_amd_geometry_laplacian_grad_weights(
    drtk_dtype_t dtype, const void* grad_out, const void* x, int64_t C, const int32_t* vi, int64_t vi_sN, int64_t N,
    int64_t V, int64_t F, int64_t weights_B, void* grad_weights, drtk_stream_t stream);

/* ------------------------------------------------------------------------------------------
 * Linear blend skinning (no counterpart in the reference's library): the posed vertices
 *     out[n,i] = sum over the slots k ascending with joint_idx[i,k] >= 0 of w[i,k] * (R[n,j] v[n,i] + t[n,j]),  j = joint_idx[i,k]
 * and the three gradients, without float atomics.
 *
 * Shapes: v [N,V,3] (v_sN = 3V, or 0: one [V,3] shared by the views); joint_idx int32 [V,K], 1 <= K <=
 * DRTK_SKIN_MAX_SLOTS, entries in [-1, J): -1 is an empty slot (nothing added, its weight is not read, gradient 0);
 * joint_weights [V,K], used as given; transforms: rows 0..2 of joint j of view n are the 12 consecutive elements at
 * n*t_sN + j*t_sJ ([N,J,3,4]: t_sJ = 12; [N,J,4,4], whose fourth row is not read: t_sJ = 16; t_sN = J*t_sJ, more for a
 * view of a larger tensor, or 0: one set for all views); out [N,V,3].  The kernels trust joint_idx (it is not validated
 * on the device).
 *
 * Evaluation order (every product and sum as written, no contraction): M = 0; M += w[i,k] * T[n,j] over the slots in
 * ascending k (the 3x4 is blended first); out_a = M[a][0]*x + M[a][1]*y + M[a][2]*z + M[a][3].  A vertex whose slots
 * are all empty gives exactly 0.
 *
 * skin_backward: grad_out [N,V,3]; NULL outputs are skipped, at least one must be given.
 *   grad_v [grad_v_B,V,3], grad_v_B = N or 1: M^T grad_out[n,i] (M's 3x3 part, blended as in the forward);
 *     grad_v_B = 1: the views' rows added in ascending n.
 *   grad_weights [V,K]: sum over n ascending of dot(grad_out[n,i], R[n,j] v[n,i] + t[n,j]); 0 for an empty slot.
 *   grad_transforms [N,J,grad_t_rows,4], grad_t_rows = 3 or 4 (the fourth row receives exactly 0):
 *     [n,j,a,b] = sum over the entries (i,k) with joint_idx[i,k] = j of w[i,k] * grad_out[n,i,a] * [v[n,i]; 1]_b,
 *     accumulated in double for either dtype and rounded once.  It needs the JOINT INCIDENCE of joint_idx, built by the
 *     caller once per index tensor (drtk_amd_ext::joint_incidence builds and caches it; drtk_amd/capi.py has a numpy
 *     builder), and a workspace of _workspace_bytes (8-byte aligned):
 *       crow        int32 [J+1]   joint j's entries are entries[crow[j] .. crow[j+1]-1]
 *       entries     int32 [>= crow[J]]  the slots i*K+k that name the joint, ASCENDING within the joint
 *       chunk_ptr   int32 [J+1]   joint j's chunks are chunk_ptr[j] .. chunk_ptr[j+1]-1; EVERY row is cut into
 *                                 ceil(length / DRTK_SKIN_CHUNK) chunks (none for a joint nobody names, which gets 0)
 *       chunk_begin int32 [C]     first entry of the chunk (crow[j] + c*DRTK_SKIN_CHUNK for the joint's c-th chunk)
 *       chunk_joint int32 [C]     its joint
 *     Order of the sum: within a chunk, lane l of a 64-lane wave adds the chunk's entries l, l+64, ... in that order,
 *     the 64 lane sums are added in a butterfly (partner lane xor 32, 16, 8, 4, 2, 1), and a joint's chunk sums are added
 *     in chunk order.
 * Results are bitwise reproducible: every sum has one fixed order, independent of the launch shape.
 */
#define DRTK_SKIN_MAX_SLOTS 8
#define DRTK_SKIN_CHUNK 512
int drtk_amd_skin_forward(
    drtk_dtype_t dtype, const void* v, int64_t v_sN, const int32_t* joint_idx, const void* joint_weights,
    const void* transforms, int64_t t_sN, int64_t t_sJ, int64_t N, int64_t V, int64_t J, int64_t K, void* out,
    drtk_stream_t stream);
int drtk_amd_skin_backward_workspace_bytes(drtk_dtype_t dtype, int64_t N, int64_t num_chunks, size_t* bytes);
int drtk_amd_skin_backward(
    drtk_dtype_t dtype, const void* grad_out, const void* v, int64_t v_sN, const int32_t* joint_idx,
    const void* joint_weights, const void* transforms, int64_t t_sN, int64_t t_sJ, const int32_t* crow,
    const int32_t* entries, const int32_t* chunk_ptr, const int32_t* chunk_begin, const int32_t* chunk_joint,
    int64_t num_chunks, int64_t N, int64_t V, int64_t J, int64_t K, int64_t grad_v_B, void* grad_v, void* grad_weights,
    int64_t grad_t_rows, void* grad_transforms, void* workspace, size_t workspace_bytes, drtk_stream_t stream);

/* ------------------------------------------------------------------------------------------
 * Forward kinematics along a joint tree (no counterpart in the reference's library): from the pose to the skinning
 * matrices drtk_amd_skin_forward reads and the posed joints, and the gradients, without atomics.  With p = parents[j]
 * (-1: a root; else 0 <= p < j), R_j the local rotation and c_j the rest joint:
 *     root:   G_j.R = R_j              G_j.t = c_j + translation[n]
 *     child:  G_j.R = G_p.R R_j        G_j.t = G_p.R (c_j - c_p) + G_p.t
 *     posed_joints[n,j] = G_j.t        transforms[n,j] = [ G_j.R | G_j.t - G_j.R c_j ]      ([N,J,3,4], [N,J,3], contiguous)
 *
 * rotations: rot_is_matrix = 0: axis-angle vectors, component a of joint j of view n at n*rot_strides[0] + j*rot_strides[1] +
 * a*rot_strides[2] (rot_strides[3] is not read); R = I + a K + b K^2 with K the skew matrix of r, t2 = r.r, a = sin(t)/t,
 * b = (1/2) (sin(t/2) / (t/2))^2; for t2 below 1/16 (float32) or 1/256 (float64) a, b and their derivatives are five-term
 * Taylor series in t2, so r = 0 gives I and the finite gradient of the exponential map.  No wrapping of angles.
 * rot_is_matrix = 1: 3x3 matrices used as given, element (a,b) at ... + a*rot_strides[2] + b*rot_strides[3].  Strides in
 * elements, any values.  joints: [J,3] shared by the views (c_sN = 0) or [N,J,3] (c_sN = 3J), rows contiguous.
 * translation: [N,3] or NULL.
 *
 * The SCHEDULE of `parents`, built by the caller once per tree (drtk_amd_ext::kinematic_schedule builds and caches it;
 * drtk_amd/capi.py has a numpy builder); the kernels trust it and `parents`:
 *     order         int32 [J]     the joints sorted by (depth, index)
 *     level_start   int32 [D+1]   level l is order[level_start[l] .. level_start[l+1]-1]; num_levels = D (level 0: the roots)
 *     child_crow    int32 [J+1]   joint j's children are child_entries[child_crow[j] .. child_crow[j+1]-1], ASCENDING
 *     child_entries int32 [J - number of roots]
 *
 * One workgroup of 64 lanes per view holds every joint's 3x4 in LDS: J <= DRTK_FK_MAX_JOINTS, above which the entry points
 * return DRTK_ERR_INVALID_ARGUMENT.  320: the backward keeps two arrays of 12 values per joint, 2 * 12 * 8 bytes * 320 =
 * 61440 bytes of double, inside the 65536 bytes a workgroup may declare statically.
 *
 * kinematics_backward: grad_transforms [N,J,3,4] and grad_posed [N,J,3], either may be NULL (zero).  NULL outputs are
 * skipped, at least one must be given.  grad_rotations [N,J,3] or [N,J,3,3] (the plain matrix gradient), contiguous;
 * grad_joints [grad_joints_B,J,3], grad_joints_B = N, or 1: the views' rows, written to the workspace of _workspace_bytes
 * (8-byte aligned; 0 bytes when N = 1), are added in ascending n in double by a second launch; grad_translation [N,3]: the
 * roots' gradients added in ascending index.  A joint adds its children's terms in child_entries order.  Results are
 * bitwise reproducible, and each gradient requested alone has the bits it has when all are requested.
 */
#define DRTK_FK_MAX_JOINTS 320
int drtk_amd_kinematics_forward(
    drtk_dtype_t dtype, const void* rotations, int rot_is_matrix, const int64_t* rot_strides, const void* joints,
    int64_t c_sN, const void* translation, const int32_t* parents, const int32_t* order, const int32_t* level_start,
    int64_t num_levels, int64_t N, int64_t J, void* transforms, void* posed_joints, drtk_stream_t stream);
int drtk_amd_kinematics_backward_workspace_bytes(drtk_dtype_t dtype, int64_t N, int64_t J, int64_t grad_joints_B,
                                                 size_t* bytes);
int drtk_amd_kinematics_backward(
    drtk_dtype_t dtype, const void* grad_transforms, const void* grad_posed, const void* rotations, int rot_is_matrix,
    const int64_t* rot_strides, const void* joints, int64_t c_sN, const void* translation, const int32_t* parents,
    const int32_t* order, const int32_t* level_start, int64_t num_levels, const int32_t* child_crow,
    const int32_t* child_entries, int64_t N, int64_t J, void* grad_rotations, int64_t grad_joints_B, void* grad_joints,
    void* grad_translation, void* workspace, size_t workspace_bytes, drtk_stream_t stream);

/* ------------------------------------------------------------------------------------------
 * Closest-point queries (no counterpart in the reference's library): for every query point p[n,i] the nearest of the
 * view's targets q[n,0..M-1] by brute force, and the gradients of the squared distance, without atomics.
 *
 * Definition, which the kernels produce bit for bit (every operation rounded in `dtype`, in this association, no
 * contraction):
 *     d2(i,j) = ((px-qx)*(px-qx) + (py-qy)*(py-qy)) + (pz-qz)*(pz-qz)
 *     idx[n,i] = the LOWEST j whose d2 is minimal among the candidates with d2 < +inf;  dist2[n,i] = that d2.
 * A candidate whose d2 is NaN or +inf (a NaN coordinate, an overflowing square) is never chosen; with no candidate left
 * (M = 0, a NaN query, every candidate rejected) idx = -1 and dist2 = +inf.
 *
 * Shapes: point i of view n of p is the 3 consecutive elements at n*p_sN + i*p_sP (p_sP >= 3: 3 for [N,P,3], 4 or 6 for the
 * leading three columns of an [N,P,4] / [N,P,6] tensor read in place; p_sN = 0: one set of points shared by the views,
 * else >= (P-1)*p_sP + 3); q likewise with q_sN, q_sM.  dist2 [N,P] in `dtype`, idx [N,P] int32, contiguous.
 * N >= 0, 0 <= P, M < 2^31.
 *
 * Launch rule.  A workgroup of 256 lanes holds DRTK_NEAREST_QUERIES = 256 * DRTK_NEAREST_R queries of one view in
 * registers (DRTK_NEAREST_R per lane) and walks the targets in LDS tiles of DRTK_NEAREST_TILE, j ascending, keeping the
 * minimum with a strict `<`.  B = N * ceil(P / DRTK_NEAREST_QUERIES) workgroups cover the queries.  When
 * B < DRTK_NEAREST_SPLIT_BLOCKS (twice the 256 compute units of the card) and M > DRTK_NEAREST_TILE, the targets are split
 * into S contiguous ranges, one workgroup per (queries, range):
 *     S0 = min(ceil(DRTK_NEAREST_SPLIT_BLOCKS / B), ceil(M / DRTK_NEAREST_TILE))
 *     L  = ceil(ceil(M / S0) / DRTK_NEAREST_TILE) * DRTK_NEAREST_TILE        (targets per range, whole tiles)
 *     S  = ceil(M / L)                                                       (the last range may be short)
 * otherwise S = 1.  With S > 1 every range writes its (d2, idx) to the workspace ([N,S,P] of `dtype`, then [N,S,P] int32)
 * and a merge launch takes them in ascending range order with a strict `<`; with S = 1 the outputs are written directly
 * and the workspace is not touched: _forward_workspace_bytes is N*S*P*(sizeof(dtype) + 4) for S > 1 and 0 for S = 1.  The
 * rule depends on the sizes alone and the results do not depend on it.  Workspaces are 8-byte aligned.
 *
 * nearest_backward: grad_dist2 [N,P], idx as the forward wrote it.  NULL outputs are skipped, at least one must be given.
 *   grad_p [grad_p_B,P,3], grad_p_B = N or 1:  2 g[n,i] (p_i - q_idx), exactly 0 where idx = -1; grad_p_B = 1: the views'
 *     rows added in ascending n in double.
 *   grad_q [grad_q_B,M,3], grad_q_B = N or 1:  - sum over the i with idx[n,i] = j of 2 g[n,i] (p_i - q_j), every term and
 *     the sum in double, rounded once; exactly 0 for a target nobody chose; grad_q_B = 1: the views added in ascending n.
 *     It needs `order` int32 [N,P]: per view the STABLE ascending argsort of idx[n,:] (equal indices keep ascending i; the
 *     -1 rows come first and are skipped), built by the caller (drtk_amd_ext::nearest_points sorts on the device), and
 *     the workspace of _backward_workspace_bytes (0 without grad_q; else N*P*(3*8 + 4) bytes rounded up to 8).
 *     Order of the sum: the sorted list of a view is cut into chunks of DRTK_NEAREST_CHUNK positions; within a chunk the
 *     terms of one target are added in ascending sorted position; a target's chunk sums are added in ascending chunk
 *     order; shared targets then add the views in ascending n.  A second launch, one lane per target, finds the target's
 *     run by bisection, adds its chunk sums and is the only writer of grad_q (zeros included).
 * Results are bitwise reproducible; each gradient requested alone has the bits it has when both are requested.
 */
#define DRTK_NEAREST_R 4
#define DRTK_NEAREST_QUERIES 1024
#define DRTK_NEAREST_TILE 1024
#define DRTK_NEAREST_SPLIT_BLOCKS 512
#define DRTK_NEAREST_CHUNK 256
int drtk_amd_nearest_forward_workspace_bytes(drtk_dtype_t dtype, int64_t N, int64_t P, int64_t M, size_t* bytes);
int drtk_amd_nearest_forward(
    drtk_dtype_t dtype, const void* p, int64_t p_sN, int64_t p_sP, const void* q, int64_t q_sN, int64_t q_sM, int64_t N,
    int64_t P, int64_t M, void* dist2, int32_t* idx, void* workspace, size_t workspace_bytes, drtk_stream_t stream);
int drtk_amd_nearest_backward_workspace_bytes(drtk_dtype_t dtype, int64_t N, int64_t P, int64_t M, int need_grad_q,
                                              size_t* bytes);
int drtk_amd_nearest_backward(
    drtk_dtype_t dtype, const void* grad_dist2, const void* p, int64_t p_sN, int64_t p_sP, const void* q, int64_t q_sN,
    int64_t q_sM, const int32_t* idx, const int32_t* order, int64_t N, int64_t P, int64_t M, int64_t grad_p_B, void* grad_p,
    int64_t grad_q_B, void* grad_q, void* workspace, size_t workspace_bytes, drtk_stream_t stream);

/* Diagnostics: compares the rasterizer's reciprocal-based exact division with the IEEE `/` on `count`
 * pseudo-random operand pairs on the device; *d_mismatches (device memory) receives the number of
 * differing results (must be 0). */
int drtk_amd_selftest_exact_div(
    drtk_dtype_t dtype, uint64_t seed, int64_t count, uint64_t* d_mismatches, drtk_stream_t stream);

/* Per-kernel timing for benchmarks (bench.py's `roofline`): between _begin and _report every kernel the library
 * launches -- from any entry point above, on any stream -- is bracketed by a pair of HIP events recorded on the
 * stream it is launched on.  Results are unaffected; outside a collection a launch pays one atomic load.  Do not
 * open a collection while a stream is being captured into a graph (event records would become graph nodes).
 * _report closes the collection, waits for the recorded events and writes one line per launch site in order of
 * first launch, "<kernel as spelled at the launch site>\t<launches>\t<total milliseconds>\n", NUL-terminated, into
 * buf[0..capacity); *needed (optional) receives the size the whole report takes, and a report that did not fit
 * returns DRTK_ERR_WORKSPACE_TOO_SMALL.  Process-global, serialised by a mutex. */
int drtk_amd_kernel_timing_begin(void);
int drtk_amd_kernel_timing_report(char* buf, size_t capacity, size_t* needed);

#if defined(__GNUC__) || defined(__clang__)
#pragma GCC visibility pop
#endif

#ifdef __cplusplus
}
#endif
#endif /* DRTK_AMD_H */
