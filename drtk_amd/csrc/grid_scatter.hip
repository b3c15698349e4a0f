// grid_scatter_2d -- the splatting counterpart of grid_sample: every input pixel ADDS weight * input to the texels that
// grid_sample would have read at its grid location (the adjoint of grid_sample with respect to the texture), forward and
// backward.
//
// Reference: src/grid_scatter/grid_scatter_kernel.cu:18-788 -- one thread per input pixel, four (bilinear) or sixteen
// (bicubic) global atomic adds per pixel and channel, each lane of a wave in a row of its own: the slow regime of the
// float-atomic unit (one lane per row is ~17x below the rate of contiguous row segments).
//
// Forward here: a workgroup owns a tile of 16 x 16 input pixels.
//   * The tap geometry of a pixel (texel columns / rows after padding, and the weights) is computed once and reused by all
//     channels.
//   * The workgroup finds the bounding box of the texels its tile touches (wave min / max, joined through LDS) and decides
//     its ROUTE from it -- wave-uniform, from the data, without the host ever looking at the grid:
//       windowed  the box has at most kGsWinCells texels: the tile accumulates a block of channels in an LDS window shaped
//                 like the box (double accumulators, ds_add_f64), then flushes the cells that are not zero row by row, consecutive lanes on
//                 consecutive texels -- ONE global atomic per touched texel, channel and workgroup, in contiguous row
//                 segments.  Coherent grids (a UV image, a smooth warp, minification, everything aimed at one texel).
//       direct    otherwise (an incoherent grid, heavy magnification): the reference's scheme, one global atomic per tap
//                 and channel.
//   * `route_counts` (optional, two device counters) receives the number of workgroups per route: what the tests and
//     profiles/grid_scatter_bench.py read; NULL in the product path.
// The output is zeroed by a fill kernel on the same stream; a call only enqueues work and captures into a HIP graph.
// Float sums arrive in atomic order: results are not bitwise reproducible from run to run (neither are the reference's).
//
// Coordinate rule: the reference's.  The centre goes through the whole padding transform (grid_sampler_compute_source_index:
// unnormalise, then clip / reflect-and-clip) BEFORE floor and the fractional part are taken -- for bicubic too, where
// torch's grid_sample only unnormalises -- and each bicubic tap index goes through it again (compute_coordinates).  The two
// rules differ only for bicubic under border / reflection padding with the unnormalised coordinate outside [0, size - 1].
//
// Backward: grad_input = grid_sample(grad_out, grid) and grad_grid = d/dgrid <grid_sample(grad_out, grid), input>: a gather
// per input pixel, one thread per pixel walking the channels, no atomics; both outputs are written fully, either may be
// left out (NULL).
#include <type_traits>

#include "common.hpp"
#include "grid_coords.hpp"

namespace drtk_amd {
namespace {

constexpr int kGsTileW = 16, kGsTileH = 16; // input pixels per workgroup: a wave covers 16 x 4
static_assert(kGsTileW * kGsTileH == kBlock && kGsTileW * 4 == kWave, "one thread per pixel of the tile");
// The LDS window: 32 KB of DOUBLE accumulators whatever the element type (five workgroups per CU) -- ds_add_f32 retires a third
// of a lane per clock on this part, ds_add_f64 twenty times that (profiles/NOTES.md, LDS atomics), and the float sums gain
// the precision for free.  A tile whose texels fit kGsWinCells is windowed; its channels go through the window in blocks of
// as many as fit the slots (four up to 1 024 texels, two up to 2 048).  2 048 texels hold the footprint of a 16 x 16 tile up
// to a magnification of ~2.7 per axis.
constexpr int kGsWinCells = 2048;
constexpr int kGsSlots = 4096;
constexpr int kGsMaxChannelBlock = 4;
static_assert(kGsSlots / kGsWinCells >= 1, "a window that is accepted holds at least one channel");
// the interior shortcut of the bicubic taps needs k + 1/2 to be exact in T (see gs_axis)
constexpr int kGsExactHalf = 1 << 22;

// One axis of a pixel's footprint: K texel indices after padding (-1: the tap falls outside and adds nothing) and their
// weights; `mult` = d(source index) / d(grid coordinate), `t` the fractional part (bicubic).
//   bilinear (K = 2): grid_scatter_kernel.cu:43-60      bicubic (K = 4): :140-153 and grid_utils.h:144-164
template <typename T, int MODE, int PAD>
__device__ __forceinline__ void gs_axis(T coord, int size, bool align_corners, int (&idx)[MODE == 2 ? 4 : 2], T (&w)[MODE == 2 ? 4 : 2], T& mult, T& t) {
  const T ic = source_index(coord, size, PAD, align_corners, &mult);
  const T fl = floor(ic);
  if constexpr (MODE == 0) {
    const int nw = static_cast<int>(fl);
    const int se = static_cast<int>(static_cast<unsigned>(nw) + 1u);
    w[0] = se - ic, w[1] = ic - nw;
    idx[0] = (nw >= 0 && nw < size) ? nw : -1;
    idx[1] = (se >= 0 && se < size) ? se : -1;
    t = w[1];
  } else {
    t = ic - fl;
    cubic_coeffs(w, t);
    // Taps nw - 1 ... nw + 2 that all lie inside the texture are their own image under clip, reflect and the integer-range
    // guard (reflection: (k + 1/2) - 1/2 with fmod(k + 1/2, size) == k + 1/2 and no flip), so the four transforms -- an fmod,
    // a division and a floor each under reflection -- are only evaluated at the border.
    if (size < kGsExactHalf && fabs(ic) < T(1e9)) { // (false for NaN)
      const int k = static_cast<int>(fl);
      if (k >= 1 && k + 2 < size) {
#pragma unroll
        for (int i = 0; i < 4; ++i) idx[i] = k - 1 + i;
        return;
      }
    }
#pragma unroll
    for (int i = 0; i < 4; ++i) {
      const int k = static_cast<int>(compute_coordinates<T>(fl - 1 + i, size, PAD, align_corners));
      idx[i] = (k >= 0 && k < size) ? k : -1;
    }
  }
}

template <typename T>
__device__ __forceinline__ void gs_load_uv(const T* __restrict__ grid, const GridLayout& gl, int64_t n, int64_t pix, T& u, T& v) {
  const T* g = grid + n * gl.sN + pix * gl.sP;
  if (gl.pair) {
    using V2 = typename std::conditional<sizeof(T) == 4, float2, double2>::type;
    const V2 q = *reinterpret_cast<const V2*>(g);
    u = q.x, v = q.y;
  } else {
    u = g[0], v = g[gl.sC];
  }
}

// what a tap adds: (wx * wy) * value bilinear (:57-60, :76), (value * wx) * wy bicubic (:173)
template <typename T, int MODE>
__device__ __forceinline__ T gs_term(T value, T wx, T wy) {
  return MODE == 0 ? (wx * wy) * value : (value * wx) * wy;
}

template <typename T, int MODE, int PAD>
__global__ __launch_bounds__(kBlock) void grid_scatter_forward_kernel(
    const T* __restrict__ input, const T* __restrict__ grid, GridLayout gl, int C, int H, int W, int OH, int OW, int tiles_x,
    bool align_corners, T* __restrict__ out, unsigned int* __restrict__ route_counts, int strip) {
  constexpr int K = MODE == 2 ? 4 : 2;
  constexpr int CB = kGsMaxChannelBlock;
  __shared__ double s_win[kGsSlots];
  __shared__ int s_box[kBlock / kWave][4];
  const int tid = threadIdx.x;
  const int wave = tid / kWave, lane = tid & (kWave - 1);
  const int n = blockIdx.y;
  const int tile = tile_index(strip);
  const int ty = tile / tiles_x, tx = tile - ty * tiles_x;
  const int px = tx * kGsTileW + (lane & (kGsTileW - 1)), py = ty * kGsTileH + wave * (kWave / kGsTileW) + lane / kGsTileW;
  const bool valid = px < W && py < H;
  const int64_t HW = int64_t(H) * W, OHW = int64_t(OH) * OW;
  const int64_t pix = int64_t(py) * W + px;

  int xi[K], yi[K];
  T wx[K], wy[K];
#pragma unroll
  for (int i = 0; i < K; ++i) xi[i] = yi[i] = -1, wx[i] = wy[i] = T(0);
  if (valid) {
    T u, v, unused_m, unused_t;
    gs_load_uv<T>(grid, gl, n, pix, u, v);
    gs_axis<T, MODE, PAD>(u, OW, align_corners, xi, wx, unused_m, unused_t);
    gs_axis<T, MODE, PAD>(v, OH, align_corners, yi, wy, unused_m, unused_t);
  }
  // the texels this pixel adds to: columns x rows; a pixel without a column or without a row adds nothing
  int lx0 = INT32_MAX, ly0 = INT32_MAX, lx1 = INT32_MIN, ly1 = INT32_MIN;
#pragma unroll
  for (int i = 0; i < K; ++i) {
    if (xi[i] >= 0) lx0 = min(lx0, xi[i]), lx1 = max(lx1, xi[i]);
    if (yi[i] >= 0) ly0 = min(ly0, yi[i]), ly1 = max(ly1, yi[i]);
  }
  const bool live = lx1 >= 0 && ly1 >= 0;
  {
    const int x0 = wave_min_i32(live ? lx0 : INT32_MAX), y0 = wave_min_i32(live ? ly0 : INT32_MAX);
    const int x1 = wave_max_i32(live ? lx1 : INT32_MIN), y1 = wave_max_i32(live ? ly1 : INT32_MIN);
    if (lane == 0) s_box[wave][0] = x0, s_box[wave][1] = y0, s_box[wave][2] = x1, s_box[wave][3] = y1;
  }
  __syncthreads();
  int bx0 = s_box[0][0], by0 = s_box[0][1], bx1 = s_box[0][2], by1 = s_box[0][3];
#pragma unroll
  for (int w = 1; w < kBlock / kWave; ++w) {
    bx0 = min(bx0, s_box[w][0]), by0 = min(by0, s_box[w][1]), bx1 = max(bx1, s_box[w][2]), by1 = max(by1, s_box[w][3]);
  }
  if (bx1 < bx0) return; // nothing of this tile lands in the output (the whole workgroup leaves)
  // 0 <= bx0 <= bx1 < OW and 0 <= by0 <= by1 < OH from here on: every index that entered the box passed the bounds test
  const int ww = bx1 - bx0 + 1, wh = by1 - by0 + 1;
  const bool windowed = int64_t(ww) * wh <= kGsWinCells;
  if (route_counts != nullptr && tid == 0) atomicAdd(route_counts + (windowed ? 0 : 1), 1u);

  const T* in_px = input + int64_t(n) * C * HW + pix;
  T* const out_n = out + int64_t(n) * C * OHW;
  if (!windowed) {
    if (!live) return;
    for (int c = 0; c < C; ++c) {
      const T value = in_px[int64_t(c) * HW];
      const GlobalPtr<T> plane = (GlobalPtr<T>)(out_n + int64_t(c) * OHW);
#pragma unroll
      for (int i = 0; i < K; ++i) {
#pragma unroll
        for (int j = 0; j < K; ++j) {
          if (xi[i] >= 0 && yi[j] >= 0) atomic_add_g1(plane + (yi[j] * OW + xi[i]), gs_term<T, MODE>(value, wx[i], wy[j]));
        }
      }
    }
    return;
  }

  const int cells = ww * wh;
  const int cb = min(CB, kGsSlots / cells); // channels per pass: what fits the slots
  for (int i = tid; i < cb * cells; i += kBlock) s_win[i] = 0.0; // every flush leaves the window zeroed again
  __syncthreads();
  for (int c0 = 0; c0 < C; c0 += cb) {
    const int cc = min(cb, C - c0);
    if (live) {
      T value[CB];
#pragma unroll
      for (int c = 0; c < CB; ++c) value[c] = c < cc ? in_px[int64_t(c0 + c) * HW] : T(0);
#pragma unroll
      for (int j = 0; j < K; ++j) {
        if (yi[j] < 0) continue;
        const int row = (yi[j] - by0) * ww - bx0;
#pragma unroll
        for (int i = 0; i < K; ++i) {
          if (xi[i] < 0) continue;
          double* cell = s_win + row + xi[i];
#pragma unroll
          for (int c = 0; c < CB; ++c) {
            if (c < cc) lds_add(cell + c * cells, static_cast<double>(gs_term<T, MODE>(value[c], wx[i], wy[j])));
          }
        }
      }
    }
    __syncthreads();
    // flush: the window row by row, consecutive lanes on consecutive texels of a row; untouched (zero) cells are skipped
    for (int c = 0; c < cc; ++c) {
      const GlobalPtr<T> plane = (GlobalPtr<T>)(out_n + int64_t(c0 + c) * OHW + (int64_t(by0) * OW + bx0));
      double* const win = s_win + c * cells;
      for (int r = tid; r < cells; r += kBlock) {
        const double sum = win[r];
        if (sum != 0.0) {
          const int y = r / ww, x = r - y * ww;
          win[r] = 0.0;
          atomic_add_g1(plane + (y * OW + x), static_cast<T>(sum));
        }
      }
    }
    __syncthreads();
  }
}

// ---- backward ---------------------------------------------------------------------------------------------------------
// grid_scatter_kernel.cu:183-285 (bilinear) and :287-422 (bicubic).  grad_input / grad_grid: either may be NULL.
template <typename T, int MODE, int PAD>
__global__ __launch_bounds__(kBlock) void grid_scatter_backward_kernel(
    const T* __restrict__ grad_out, const T* __restrict__ input, const T* __restrict__ grid, GridLayout gl, int C, int64_t HW,
    int OH, int OW, bool align_corners, T* __restrict__ grad_input, T* __restrict__ grad_grid, GridLayout ggl, int strip) {
  constexpr int K = MODE == 2 ? 4 : 2;
  const int n = blockIdx.y;
  const int64_t pix = int64_t(tile_index(strip)) * kBlock + threadIdx.x;
  if (pix >= HW) return;
  const int64_t OHW = int64_t(OH) * OW;
  T u, v, mx, my, tx, ty;
  int xi[K], yi[K];
  T wx[K], wy[K];
  gs_load_uv<T>(grid, gl, n, pix, u, v);
  gs_axis<T, MODE, PAD>(u, OW, align_corners, xi, wx, mx, tx);
  gs_axis<T, MODE, PAD>(v, OH, align_corners, yi, wy, my, ty);
  const T* go_n = grad_out + int64_t(n) * C * OHW;
  const T* in_px = input + int64_t(n) * C * HW + pix;
  T* gi_px = grad_input + int64_t(n) * C * HW + pix;
  T gx = T(0), gy = T(0);
  if constexpr (MODE == 0) {
    // corners nw, ne, sw, se: offsets (-1: outside) and weights
    const int o_nw = (xi[0] >= 0 && yi[0] >= 0) ? yi[0] * OW + xi[0] : -1, o_ne = (xi[1] >= 0 && yi[0] >= 0) ? yi[0] * OW + xi[1] : -1;
    const int o_sw = (xi[0] >= 0 && yi[1] >= 0) ? yi[1] * OW + xi[0] : -1, o_se = (xi[1] >= 0 && yi[1] >= 0) ? yi[1] * OW + xi[1] : -1;
    const T nw = wx[0] * wy[0], ne = wx[1] * wy[0], sw = wx[0] * wy[1], se = wx[1] * wy[1];
    for (int c = 0; c < C; ++c) {
      const T* go = go_n + int64_t(c) * OHW;
      const T g_nw = o_nw >= 0 ? go[o_nw] : T(0), g_ne = o_ne >= 0 ? go[o_ne] : T(0);
      const T g_sw = o_sw >= 0 ? go[o_sw] : T(0), g_se = o_se >= 0 ? go[o_se] : T(0);
      if (grad_input != nullptr) {
        T g = T(0);
        if (o_nw >= 0) g += g_nw * nw;
        if (o_ne >= 0) g += g_ne * ne;
        if (o_sw >= 0) g += g_sw * sw;
        if (o_se >= 0) g += g_se * se;
        gi_px[int64_t(c) * HW] = g;
      }
      if (grad_grid != nullptr) {
        const T value = in_px[int64_t(c) * HW];
        if (o_nw >= 0) gx -= value * wy[0] * g_nw, gy -= value * wx[0] * g_nw;
        if (o_ne >= 0) gx += value * wy[0] * g_ne, gy -= value * wx[1] * g_ne;
        if (o_sw >= 0) gx -= value * wy[1] * g_sw, gy += value * wx[0] * g_sw;
        if (o_se >= 0) gx += value * wy[1] * g_se, gy += value * wx[1] * g_se;
      }
    }
  } else {
    T dx[4], dy[4];
    cubic_coeffs_grad(dx, tx);
    cubic_coeffs_grad(dy, ty);
    for (int c = 0; c < C; ++c) {
      const T* go = go_n + int64_t(c) * OHW;
      T g[4][4]; // [row j][column i]
#pragma unroll
      for (int j = 0; j < 4; ++j) {
#pragma unroll
        for (int i = 0; i < 4; ++i) g[j][i] = (xi[i] >= 0 && yi[j] >= 0) ? go[yi[j] * OW + xi[i]] : T(0);
      }
      if (grad_input != nullptr) { // cubic_interp1d of the four rows, then of the column of results (:352-398)
        T rows[4];
#pragma unroll
        for (int j = 0; j < 4; ++j) rows[j] = g[j][0] * wx[0] + g[j][1] * wx[1] + g[j][2] * wx[2] + g[j][3] * wx[3];
        gi_px[int64_t(c) * HW] = rows[0] * wy[0] + rows[1] * wy[1] + rows[2] * wy[2] + rows[3] * wy[3];
      }
      if (grad_grid != nullptr) {
        const T value = in_px[int64_t(c) * HW];
#pragma unroll
        for (int i = 0; i < 4; ++i) {
#pragma unroll
          for (int j = 0; j < 4; ++j) {
            const T gv = g[j][i] * value;
            gx -= gv * (dx[i] * wy[j]);
            gy -= gv * (dy[j] * wx[i]);
          }
        }
      }
    }
  }
  if (grad_grid != nullptr) store_grid_grad<T>(grad_grid, ggl, n, pix, mx * gx, my * gy);
}

int gs_validate(drtk_dtype_t dtype, int64_t N, int64_t C, int64_t H, int64_t W, int64_t OH, int64_t OW, int padding_mode, int interpolation_mode) {
  constexpr int64_t kLimit = int64_t(1) << 31;
  // (not bad_image() alone: H and W are bounded one by one, too -- an empty input of 2^31 rows is invalid here)
  if (H >= kLimit || W >= kLimit || bad_image(N, H, W) || C < 0 || C >= (1 << 20)) return DRTK_ERR_INVALID_ARGUMENT;
  if (OH <= 0 || OW <= 0 || OH >= kLimit || OW >= kLimit || OH * OW >= kLimit) return DRTK_ERR_INVALID_ARGUMENT;
  if (padding_mode < 0 || padding_mode > 2 || (interpolation_mode != 0 && interpolation_mode != 2)) return DRTK_ERR_INVALID_ARGUMENT;
  if (!valid_dtype(dtype)) return DRTK_ERR_INVALID_ARGUMENT;
  return DRTK_OK;
}

} // namespace
} // namespace drtk_amd

using namespace drtk_amd;

extern "C" int drtk_amd_grid_scatter_2d(
    drtk_dtype_t dtype, const void* input, const void* grid, const int64_t* grid_layout, int64_t N, int64_t C, int64_t H,
    int64_t W, int64_t output_height, int64_t output_width, int padding_mode, int interpolation_mode, int align_corners,
    void* out, uint32_t* route_counts, drtk_stream_t stream) {
  const int64_t OH = output_height, OW = output_width;
  const int st = gs_validate(dtype, N, C, H, W, OH, OW, padding_mode, interpolation_mode);
  if (st != DRTK_OK) return st;
  const size_t es = dtype_size(dtype);
  const int64_t out_elems = N * C * OH * OW, count = N * H * W;
  if (out_elems > 0 && !out) return DRTK_ERR_INVALID_ARGUMENT;
  if (count > 0 && C > 0 && (!input || !grid)) return DRTK_ERR_INVALID_ARGUMENT;
  GridLayout gl;
  if (make_grid_layout(gl, grid_layout, grid, H, W, es) != DRTK_OK) return DRTK_ERR_INVALID_ARGUMENT;
  if (N > kMaxViewsPerLaunch) return for_view_slices(N, [&](int64_t n0, int64_t n) {
    const int64_t layout[3] = {gl.sN, gl.sP, gl.sC};
    return drtk_amd_grid_scatter_2d(
        dtype, advance(input, n0 * C * H * W, es), advance(grid, n0 * gl.sN, es), layout, n, C, H, W, OH, OW, padding_mode,
        interpolation_mode, align_corners, advance(out, n0 * C * OH * OW, es), route_counts, stream);
  });
  hipStream_t s = static_cast<hipStream_t>(stream);
  if (out_elems > 0 && fill_bytes_async(out, 0, es * size_t(out_elems), s) != DRTK_OK) return DRTK_ERR_LAUNCH;
  if (count == 0 || C == 0) return DRTK_OK;
  const int tiles_x = static_cast<int>(ceil_div(W, kGsTileW)), tiles_y = static_cast<int>(ceil_div(H, kGsTileH));
  const dim3 grid_dim(static_cast<unsigned>(int64_t(tiles_x) * tiles_y), static_cast<unsigned>(N));
  return dispatch_dtype(dtype, [&](auto tag) {
    using T = decltype(tag);
    with_constant<0, 1>(interpolation_mode / 2, [&](auto bicubic) {
      with_constant<0, 2>(padding_mode, [&](auto pad) {
        constexpr int MODE = 2 * decltype(bicubic)::value, PAD = decltype(pad)::value;
        static const std::string name = instance_name<MODE, PAD>("grid_scatter_forward_kernel");
        launch_as(
            name, grid_scatter_forward_kernel<T, MODE, PAD>, grid_dim, kBlock, 0, s, static_cast<const T*>(input),
            static_cast<const T*>(grid), gl, (int)C, (int)H, (int)W, (int)OH, (int)OW, tiles_x, align_corners != 0,
            static_cast<T*>(out), route_counts, xcd_strip(tiles_x));
      });
    });
    DRTK_RETURN_IF_LAUNCH_FAILED();
    return DRTK_OK;
  });
}

extern "C" int drtk_amd_grid_scatter_2d_backward(
    drtk_dtype_t dtype, const void* grad_out, const void* input, const void* grid, const int64_t* grid_layout, int64_t N,
    int64_t C, int64_t H, int64_t W, int64_t output_height, int64_t output_width, int padding_mode, int interpolation_mode,
    int align_corners, void* grad_input, void* grad_grid, const int64_t* grad_grid_layout, drtk_stream_t stream) {
  const int64_t OH = output_height, OW = output_width;
  const int st = gs_validate(dtype, N, C, H, W, OH, OW, padding_mode, interpolation_mode);
  if (st != DRTK_OK) return st;
  const size_t es = dtype_size(dtype);
  const int64_t count = N * H * W;
  if (count == 0 || (!grad_input && !grad_grid)) return DRTK_OK;
  if (C == 0 && !grad_grid) return DRTK_OK;
  if (!grid || (C > 0 && !grad_out) || (C > 0 && grad_grid && !input)) return DRTK_ERR_INVALID_ARGUMENT;
  GridLayout gl, ggl;
  if (make_grid_layout(gl, grid_layout, grid, H, W, es) != DRTK_OK || make_grid_layout(ggl, grad_grid_layout, grad_grid, H, W, es) != DRTK_OK)
    return DRTK_ERR_INVALID_ARGUMENT;
  if (N > kMaxViewsPerLaunch) return for_view_slices(N, [&](int64_t n0, int64_t n) {
    const int64_t layout[3] = {gl.sN, gl.sP, gl.sC}, glayout[3] = {ggl.sN, ggl.sP, ggl.sC};
    return drtk_amd_grid_scatter_2d_backward(
        dtype, advance(grad_out, n0 * C * OH * OW, es), advance(input, n0 * C * H * W, es), advance(grid, n0 * gl.sN, es), layout, n,
        C, H, W, OH, OW, padding_mode, interpolation_mode, align_corners, advance(grad_input, n0 * C * H * W, es),
        advance(grad_grid, n0 * ggl.sN, es), glayout, stream);
  });
  hipStream_t s = static_cast<hipStream_t>(stream);
  const int64_t HW = H * W;
  const dim3 grid_dim(static_cast<unsigned>(ceil_div(HW, kBlock)), static_cast<unsigned>(N));
  return dispatch_dtype(dtype, [&](auto tag) {
    using T = decltype(tag);
    with_constant<0, 1>(interpolation_mode / 2, [&](auto bicubic) {
      with_constant<0, 2>(padding_mode, [&](auto pad) {
        constexpr int MODE = 2 * decltype(bicubic)::value, PAD = decltype(pad)::value;
        static const std::string name = instance_name<MODE, PAD>("grid_scatter_backward_kernel");
        launch_as(
            name, grid_scatter_backward_kernel<T, MODE, PAD>, grid_dim, kBlock, 0, s, static_cast<const T*>(grad_out),
            static_cast<const T*>(input), static_cast<const T*>(grid), gl, (int)C, HW, (int)OH, (int)OW, align_corners != 0,
            static_cast<T*>(grad_input), static_cast<T*>(grad_grid), ggl, xcd_strip(ceil_div(16 * W, kBlock)));
      });
    });
    DRTK_RETURN_IF_LAUNCH_FAILED();
    return DRTK_OK;
  });
}
