// mipmap_pyramid -- the mip chain mipmap_grid_sampler_2d reads, made from one texture, and its backward pass: the per-level
// gradients of the sampler folded back into the texture (no reference counterpart: its callers loop over avg_pool2d).
//
// Definition, in the tensor's own type, every level from the previous level AS STORED (the library is built with
// -ffp-contract=off, so this is avg_pool2d's chain bit for bit):
//   h_{l+1} = h_l / 2, w_{l+1} = w_l / 2 (floor: a trailing odd row / column is dropped)
//   x_{l+1}[i][j] = (((x_l[2i][2j] + x_l[2i][2j+1]) + x_l[2i+1][2j]) + x_l[2i+1][2j+1]) * 0.25
// Backward, with g_l the incoming gradient of level l (absent: zero, never read):
//   G_{L-1} = g_{L-1};  G_l[i][j] = g_l[i][j] + 0.25 * G_{l+1}[i/2][j/2];  grad_input = G_0
//   A texel of a dropped row / column has no parent and keeps g_l alone.  One add and one exact multiply per level.
//
// Both kernels work on 64 x 64 tiles of the level a launch starts from, one workgroup of 256 lanes per (tile, plane); lane
// t owns the 4 x 4 block (t / 16, t % 16) of the tile, hence the 2 x 2 of the next level and ONE texel of the one after.
// Sizes are floored, so a texel that exists has all four children: a partial tile predicates on i < h_k, j < w_k only, and
// whatever was formed from texels outside the level is never stored.
//
// Forward: the lane forms levels 1 and 2 of its block in registers.  The 16 lanes of a level-2 row are consecutive and a
// wave holds four such rows, so levels 3 and 4 are cross-lane moves inside the wave (every lane of a 2 x 2 / 4 x 4 group
// evaluates the same sum in the same order, one of them stores); the 4 x 4 texels of level 4 meet in LDS, and one lane
// forms levels 5 and 6 from them.  Level 0 is read once, every level is written once.  Levels beyond the sixth come from a
// second launch of the same kernel on level 6 (at most 1 / 4096 of the base): no communication between workgroups.
//
// Backward: one launch, no workspace, no LDS.  All ancestors of a lane's block above level 1 are single texels, one per
// level, so the lane evaluates G_{L-1} .. G_2 along that chain -- coarse to fine, the chain starting anew below an ancestor
// that does not exist --, then its 2 x 2 of G_1 and its 4 x 4 of G_0.  Lanes (and workgroups) that share an ancestor
// evaluate the same expression on the same values: the result is the recurrence bit for bit, and the shared loads are
// same-address loads within a wave.  The launch reads every gradient texel that exists and writes grad_input once.
//
// Rows move as 16-byte vectors (8-byte pairs at level 1) where the address allows and the block lies inside the level,
// element by element otherwise (odd widths, odd base offsets, the last block of a row).  No atomics: bitwise reproducible.
#include "common.hpp"

namespace drtk_amd {
namespace {

constexpr int kPyramidMaxLevels = 11; // what mipmap_grid_sampler_2d takes
constexpr int kTile = 64;             // texels per tile side: six levels below it end in one texel
constexpr int kTileLevels = 6;

template <typename T>
struct PyramidForwardArgs {
  const T* in; // the level this launch starts from: planes of h0 x w0, contiguous
  int64_t in_sN, in_sC;
  int h0, w0;
  T* out[kTileLevels]; // out[k - 1]: level k below the input, [N,C,h0 >> k,w0 >> k], views contiguous
  int64_t out_sN[kTileLevels];
  int nout; // how many of them are wanted: 1 .. 6
  int tiles_x, tiles;
  int strip;
};

template <typename T>
struct PyramidBackwardArgs {
  const T* g[kPyramidMaxLevels]; // g[l]: [N,C,h[l],w[l]], views contiguous, or NULL
  int64_t g_sN[kPyramidMaxLevels];
  int h[kPyramidMaxLevels], w[kPyramidMaxLevels];
  int levels;
  T* out; // [N,C,h[0],w[0]] contiguous
  int C;
  int tiles_x, tiles;
  int strip;
};

template <typename E, int P>
struct PyramidVec {
  typedef E type __attribute__((ext_vector_type(P), aligned(P * sizeof(E) < 16 ? P * sizeof(E) : 16)));
};

template <typename E, int P>
__device__ __forceinline__ bool vector_aligned(const E* p) {
  constexpr uintptr_t kMask = (P * sizeof(E) < 16 ? P * sizeof(E) : 16) - 1;
  return (reinterpret_cast<uintptr_t>(p) & kMask) == 0;
}

// v[j] = row[x + j] for the j with x + j < w (0 elsewhere); `row` is the start of an existing row
template <typename E, int P>
__device__ __forceinline__ void load_row(const E* __restrict__ row, int x, int w, E (&v)[P]) {
  const E* p = row + x;
  if (x + P <= w && vector_aligned<E, P>(p)) {
    const typename PyramidVec<E, P>::type q = *reinterpret_cast<const typename PyramidVec<E, P>::type*>(p);
#pragma unroll
    for (int j = 0; j < P; ++j) v[j] = q[j];
  } else {
#pragma unroll
    for (int j = 0; j < P; ++j) v[j] = x + j < w ? p[j] : E(0);
  }
}
template <typename E, int P>
__device__ __forceinline__ void store_row(E* __restrict__ row, int x, int w, const E (&v)[P]) {
  E* p = row + x;
  if (x + P <= w && vector_aligned<E, P>(p)) {
    typename PyramidVec<E, P>::type q;
#pragma unroll
    for (int j = 0; j < P; ++j) q[j] = v[j];
    *reinterpret_cast<typename PyramidVec<E, P>::type*>(p) = q;
  } else {
#pragma unroll
    for (int j = 0; j < P; ++j) {
      if (x + j < w) p[j] = v[j];
    }
  }
}

template <typename T>
__device__ __forceinline__ T box(T a, T b, T c, T d) {
  return (((a + b) + c) + d) * T(0.25);
}

// blockIdx.x (through tile_index) -> channel and tile of the launch; blockIdx.y is the view
struct TileOf {
  int c, ty, tx;
};
__device__ __forceinline__ TileOf tile_of(int strip, int tiles, int tiles_x) {
  const int b = tile_index(strip);
  const int tile = b % tiles;
  return {b / tiles, tile / tiles_x, tile % tiles_x};
}

template <typename T>
__global__ __launch_bounds__(kBlock) void mipmap_pyramid_forward_kernel(const PyramidForwardArgs<T> a) {
  __shared__ T level4[4][4];
  const TileOf t = tile_of(a.strip, a.tiles, a.tiles_x);
  const int n = blockIdx.y;
  const int br = threadIdx.x >> 4, bc = threadIdx.x & 15;
  const int h0 = a.h0, w0 = a.w0;
  // element offset of this (view, channel) plane at level k
  auto plane = [&](int k) { return int64_t(n) * a.out_sN[k - 1] + int64_t(t.c) * ((h0 >> k) * int64_t(w0 >> k)); };

  // level 0: the lane's 4 x 4 block, rows outside the level as zeros (nothing made of them is stored)
  const int y0 = t.ty * kTile + 4 * br, x0 = t.tx * kTile + 4 * bc;
  const T* ip = a.in + int64_t(n) * a.in_sN + int64_t(t.c) * a.in_sC;
  T v[4][4];
#pragma unroll
  for (int r = 0; r < 4; ++r) {
#pragma unroll
    for (int j = 0; j < 4; ++j) v[r][j] = T(0);
    if (y0 + r < h0 && x0 < w0) load_row<T, 4>(ip + int64_t(y0 + r) * w0, x0, w0, v[r]);
  }

  // level 1: 2 x 2 per lane
  T v1[2][2];
#pragma unroll
  for (int i = 0; i < 2; ++i) {
#pragma unroll
    for (int j = 0; j < 2; ++j) v1[i][j] = box(v[2 * i][2 * j], v[2 * i][2 * j + 1], v[2 * i + 1][2 * j], v[2 * i + 1][2 * j + 1]);
  }
  {
    const int h = h0 >> 1, w = w0 >> 1, y = y0 >> 1, x = x0 >> 1;
    T* op = a.out[0] + plane(1);
#pragma unroll
    for (int i = 0; i < 2; ++i) {
      if (y + i < h && x < w) store_row<T, 2>(op + int64_t(y + i) * w, x, w, v1[i]);
    }
  }
  if (a.nout < 2) return;

  // level 2: one texel per lane, 16 consecutive lanes per row
  const T v2 = box(v1[0][0], v1[0][1], v1[1][0], v1[1][1]);
  {
    const int h = h0 >> 2, w = w0 >> 2, y = y0 >> 2, x = x0 >> 2;
    if (y < h && x < w) a.out[1][plane(2) + int64_t(y) * w + x] = v2;
  }
  if (a.nout < 3) return;

  // level 3: the lanes {l, l ^ 1, l ^ 16, l ^ 17} of a wave hold one 2 x 2 group (every lane of the wave takes part)
  const int lane = threadIdx.x & (kWave - 1);
  const int q3 = lane & ~17;
  const T v3 = box(__shfl(v2, q3), __shfl(v2, q3 | 1), __shfl(v2, q3 | 16), __shfl(v2, q3 | 17));
  {
    const int h = h0 >> 3, w = w0 >> 3, y = y0 >> 3, x = x0 >> 3;
    if ((lane & 17) == 0 && y < h && x < w) a.out[2][plane(3) + int64_t(y) * w + x] = v3;
  }
  if (a.nout < 4) return;

  // level 4: a wave's four level-2 rows are two level-3 rows, one level-4 row of four texels
  const int q4 = lane & 12;
  const T v4 = box(__shfl(v3, q4), __shfl(v3, q4 + 2), __shfl(v3, q4 + 32), __shfl(v3, q4 + 34));
  const bool first4 = (lane & ~12) == 0; // lanes 0, 4, 8, 12
  {
    const int h = h0 >> 4, w = w0 >> 4, y = y0 >> 4, x = x0 >> 4;
    if (first4 && y < h && x < w) a.out[3][plane(4) + int64_t(y) * w + x] = v4;
  }
  if (a.nout < 5) return;

  // levels 5 and 6: the 4 x 4 texels of level 4 meet in LDS, one lane finishes
  if (first4) level4[threadIdx.x >> 6][lane >> 2] = v4;
  __syncthreads();
  if (threadIdx.x != 0) return;
  T v5[2][2];
#pragma unroll
  for (int i = 0; i < 2; ++i) {
#pragma unroll
    for (int j = 0; j < 2; ++j)
      v5[i][j] = box(level4[2 * i][2 * j], level4[2 * i][2 * j + 1], level4[2 * i + 1][2 * j], level4[2 * i + 1][2 * j + 1]);
  }
  {
    const int h = h0 >> 5, w = w0 >> 5, y = t.ty * 2, x = t.tx * 2;
    T* op = a.out[4] + plane(5);
#pragma unroll
    for (int i = 0; i < 2; ++i) {
#pragma unroll
      for (int j = 0; j < 2; ++j) {
        if (y + i < h && x + j < w) op[int64_t(y + i) * w + (x + j)] = v5[i][j];
      }
    }
  }
  if (a.nout < 6) return;
  if (t.ty < (h0 >> 6) && t.tx < (w0 >> 6))
    a.out[5][plane(6) + int64_t(t.ty) * (w0 >> 6) + t.tx] = box(v5[0][0], v5[0][1], v5[1][0], v5[1][1]);
}

template <typename T>
__global__ __launch_bounds__(kBlock) void mipmap_pyramid_backward_kernel(const PyramidBackwardArgs<T> a) {
  const TileOf t = tile_of(a.strip, a.tiles, a.tiles_x);
  const int n = blockIdx.y;
  const int br = threadIdx.x >> 4, bc = threadIdx.x & 15;
  const int y0 = t.ty * kTile + 4 * br, x0 = t.tx * kTile + 4 * bc;
  const int H = a.h[0], W = a.w[0];
  if (y0 >= H || x0 >= W) return; // nothing of level 0 here, hence nothing of any level
  auto plane = [&](int l) { return int64_t(n) * a.g_sN[l] + int64_t(t.c) * (a.h[l] * int64_t(a.w[l])); };

  // the loads: the lane's one ancestor per level above 1, its 2 x 2 of level 1, its 4 x 4 of level 0
  T gk[kPyramidMaxLevels];
  bool ex[kPyramidMaxLevels];
#pragma unroll
  for (int l = 2; l < kPyramidMaxLevels; ++l) {
    gk[l] = T(0);
    ex[l] = false;
    if (l < a.levels) {
      const int i = y0 >> l, j = x0 >> l;
      ex[l] = i < a.h[l] && j < a.w[l];
      if (ex[l] && a.g[l]) gk[l] = a.g[l][plane(l) + int64_t(i) * a.w[l] + j];
    }
  }
  T g1[2][2], g0[4][4];
#pragma unroll
  for (int i = 0; i < 2; ++i) {
#pragma unroll
    for (int j = 0; j < 2; ++j) g1[i][j] = T(0);
  }
  const int y1 = y0 >> 1, x1 = x0 >> 1;
  const int h1 = a.levels > 1 ? a.h[1] : 0, w1 = a.levels > 1 ? a.w[1] : 0;
  if (a.levels > 1 && a.g[1]) {
    const T* gp = a.g[1] + plane(1);
#pragma unroll
    for (int i = 0; i < 2; ++i) {
      if (y1 + i < h1 && x1 < w1) load_row<T, 2>(gp + int64_t(y1 + i) * w1, x1, w1, g1[i]);
    }
  }
#pragma unroll
  for (int r = 0; r < 4; ++r) {
#pragma unroll
    for (int j = 0; j < 4; ++j) g0[r][j] = T(0);
  }
  if (a.g[0]) {
    const T* gp = a.g[0] + plane(0);
#pragma unroll
    for (int r = 0; r < 4; ++r) {
      if (y0 + r < H) load_row<T, 4>(gp + int64_t(y0 + r) * W, x0, W, g0[r]);
    }
  }

  // G_{L-1} .. G_2 at the lane's ancestors, coarse to fine; below an ancestor that does not exist the chain starts anew
  T up = T(0);
  bool has = false;
#pragma unroll
  for (int l = kPyramidMaxLevels - 1; l >= 2; --l) {
    if (l < a.levels) {
      up = has ? gk[l] + T(0.25) * up : gk[l];
      has = ex[l];
    }
  }
  // G_1, then G_0
  T* op = a.out + (int64_t(n) * a.C + t.c) * (int64_t(H) * W);
  T G1[2][2];
  bool has1[2][2];
#pragma unroll
  for (int i = 0; i < 2; ++i) {
#pragma unroll
    for (int j = 0; j < 2; ++j) {
      G1[i][j] = has ? g1[i][j] + T(0.25) * up : g1[i][j];
      has1[i][j] = y1 + i < h1 && x1 + j < w1;
    }
  }
#pragma unroll
  for (int r = 0; r < 4; ++r) {
    T o[4];
#pragma unroll
    for (int j = 0; j < 4; ++j) o[j] = has1[r >> 1][j >> 1] ? g0[r][j] + T(0.25) * G1[r >> 1][j >> 1] : g0[r][j];
    if (y0 + r < H) store_row<T, 4>(op + int64_t(y0 + r) * W, x0, W, o);
  }
}

int pyramid_max_levels(int64_t H, int64_t W) {
  int64_t m = H < W ? H : W;
  int levels = 0;
  while (m >= 1 && levels < kPyramidMaxLevels) m >>= 1, ++levels;
  return levels;
}

// what is judged before any pointer: dtype, sizes, levels
int pyramid_validate(drtk_dtype_t dtype, int64_t N, int64_t C, int64_t H, int64_t W, int levels) {
  constexpr int64_t kLimit = int64_t(1) << 31;
  if (!valid_dtype(dtype)) return DRTK_ERR_INVALID_ARGUMENT;
  // (H and W also one by one: an empty image of 2^31 rows is invalid here)
  if (C < 0 || C >= kLimit || H >= kLimit || W >= kLimit || bad_image(N, H, W)) return DRTK_ERR_INVALID_ARGUMENT;
  if (levels < 1 || levels > kPyramidMaxLevels) return DRTK_ERR_INVALID_ARGUMENT;
  if (H * W > 0 && levels > pyramid_max_levels(H, W)) return DRTK_ERR_INVALID_ARGUMENT;
  if (N > 0 && H * W > 0 && C < 1) return DRTK_ERR_INVALID_ARGUMENT;
  return DRTK_OK;
}

// The grid of one launch: x = channels * tiles (through tile_index, strips of a quarter tile row: 16 image rows), y = views.
// Channels are taken in slices whose grid fits 31 bits.
struct PyramidGrid {
  int tiles_x, tiles, strip;
  int64_t channels_per_launch;
};
PyramidGrid pyramid_grid(int64_t h, int64_t w) {
  PyramidGrid g;
  g.tiles_x = static_cast<int>(ceil_div(w, kTile));
  g.tiles = g.tiles_x * static_cast<int>(ceil_div(h, kTile));
  g.strip = xcd_strip(ceil_div(g.tiles_x, 4));
  g.channels_per_launch = ((int64_t(1) << 30) / g.tiles);
  return g;
}

// levels h0 x w0 -> (h0 >> 1) x (w0 >> 1) ... : `nout` levels below `in`, out[k] / out_sN[k] the (k + 1)-th of them
template <typename T>
void pyramid_forward_launch(
    const void* in, int64_t in_sN, int64_t in_sC, int64_t N, int64_t C, int64_t h0, int64_t w0, void* const* out, const int64_t* out_sN,
    int nout, hipStream_t s) {
  const PyramidGrid g = pyramid_grid(h0, w0);
  for (int64_t c0 = 0; c0 < C; c0 += g.channels_per_launch) {
    const int64_t c = C - c0 < g.channels_per_launch ? C - c0 : g.channels_per_launch;
    PyramidForwardArgs<T> a = {};
    a.in = static_cast<const T*>(in) + c0 * in_sC, a.in_sN = in_sN, a.in_sC = in_sC;
    a.h0 = static_cast<int>(h0), a.w0 = static_cast<int>(w0);
    for (int k = 0; k < nout; ++k) {
      a.out[k] = static_cast<T*>(out[k]) + c0 * ((h0 >> (k + 1)) * (w0 >> (k + 1)));
      a.out_sN[k] = out_sN[k];
    }
    a.nout = nout, a.tiles_x = g.tiles_x, a.tiles = g.tiles, a.strip = g.strip;
    const dim3 grid(static_cast<unsigned>(c * g.tiles), static_cast<unsigned>(N));
    DRTK_LAUNCH((mipmap_pyramid_forward_kernel<T>), grid, dim3(kBlock), 0, s, a);
  }
}

template <typename T>
void pyramid_backward_launch(
    const void* const* grad_levels, const int64_t* grad_sN, int64_t N, int64_t C, int64_t H, int64_t W, int levels, void* grad_input,
    hipStream_t s) {
  const PyramidGrid g = pyramid_grid(H, W);
  for (int64_t c0 = 0; c0 < C; c0 += g.channels_per_launch) {
    const int64_t c = C - c0 < g.channels_per_launch ? C - c0 : g.channels_per_launch;
    PyramidBackwardArgs<T> a = {};
    for (int l = 0; l < levels; ++l) {
      a.h[l] = static_cast<int>(H >> l), a.w[l] = static_cast<int>(W >> l);
      a.g[l] = grad_levels[l] ? static_cast<const T*>(grad_levels[l]) + c0 * ((H >> l) * (W >> l)) : nullptr;
      a.g_sN[l] = grad_sN[l];
    }
    a.levels = levels;
    a.out = static_cast<T*>(grad_input) + c0 * (H * W);
    a.C = static_cast<int>(C);
    a.tiles_x = g.tiles_x, a.tiles = g.tiles, a.strip = g.strip;
    const dim3 grid(static_cast<unsigned>(c * g.tiles), static_cast<unsigned>(N));
    DRTK_LAUNCH((mipmap_pyramid_backward_kernel<T>), grid, dim3(kBlock), 0, s, a);
  }
}

} // namespace
} // namespace drtk_amd

using namespace drtk_amd;

extern "C" int drtk_amd_mipmap_pyramid(
    drtk_dtype_t dtype, const void* input, int64_t input_sN, int64_t input_sC, int64_t N, int64_t C, int64_t H, int64_t W, int levels,
    void* const* out, const int64_t* out_sN, drtk_stream_t stream) {
  const int st = pyramid_validate(dtype, N, C, H, W, levels);
  if (st != DRTK_OK) return st;
  if (N == 0 || H * W == 0 || levels == 1) return DRTK_OK; // level 0 is the input itself
  if (!input || input_sN < 0 || input_sC < 0 || !out || !out_sN) return DRTK_ERR_INVALID_ARGUMENT;
  for (int l = 1; l < levels; ++l) {
    if (!out[l] || out_sN[l] < 0) return DRTK_ERR_INVALID_ARGUMENT;
  }
  const size_t es = dtype_size(dtype);
  if (N > kMaxViewsPerLaunch) return for_view_slices(N, [&](int64_t n0, int64_t n) {
    void* slice[kPyramidMaxLevels] = {};
    for (int l = 1; l < levels; ++l) slice[l] = advance(out[l], n0 * out_sN[l], es);
    return drtk_amd_mipmap_pyramid(dtype, advance(input, n0 * input_sN, es), input_sN, input_sC, n, C, H, W, levels, slice, out_sN, stream);
  });
  hipStream_t s = static_cast<hipStream_t>(stream);
  const int first = levels - 1 < kTileLevels ? levels - 1 : kTileLevels; // levels 1 .. first from the input
  const int second = levels - 1 - first;                                 // levels 7 .. from level 6 as stored
  const int64_t h6 = H >> kTileLevels, w6 = W >> kTileLevels;
  return dispatch_dtype(dtype, [&](auto tag) {
    using T = decltype(tag);
    pyramid_forward_launch<T>(input, input_sN, input_sC, N, C, H, W, out + 1, out_sN + 1, first, s);
    if (second > 0)
      pyramid_forward_launch<T>(out[kTileLevels], out_sN[kTileLevels], h6 * w6, N, C, h6, w6, out + 1 + kTileLevels, out_sN + 1 + kTileLevels, second, s);
    DRTK_RETURN_IF_LAUNCH_FAILED();
    return DRTK_OK;
  });
}

extern "C" int drtk_amd_mipmap_pyramid_backward(
    drtk_dtype_t dtype, const void* const* grad_levels, const int64_t* grad_sN, int64_t N, int64_t C, int64_t H, int64_t W, int levels,
    void* grad_input, drtk_stream_t stream) {
  const int st = pyramid_validate(dtype, N, C, H, W, levels);
  if (st != DRTK_OK) return st;
  if (N == 0 || H * W == 0) return DRTK_OK;
  if (!grad_levels || !grad_sN || !grad_input) return DRTK_ERR_INVALID_ARGUMENT;
  for (int l = 0; l < levels; ++l) {
    if (grad_levels[l] && grad_sN[l] < 0) return DRTK_ERR_INVALID_ARGUMENT;
  }
  const size_t es = dtype_size(dtype);
  if (N > kMaxViewsPerLaunch) return for_view_slices(N, [&](int64_t n0, int64_t n) {
    const void* slice[kPyramidMaxLevels] = {};
    for (int l = 0; l < levels; ++l) slice[l] = advance(grad_levels[l], n0 * grad_sN[l], es);
    return drtk_amd_mipmap_pyramid_backward(dtype, slice, grad_sN, n, C, H, W, levels, advance(grad_input, n0 * C * H * W, es), stream);
  });
  return dispatch_dtype(dtype, [&](auto tag) {
    using T = decltype(tag);
    pyramid_backward_launch<T>(grad_levels, grad_sN, N, C, H, W, levels, grad_input, static_cast<hipStream_t>(stream));
    DRTK_RETURN_IF_LAUNCH_FAILED();
    return DRTK_OK;
  });
}
