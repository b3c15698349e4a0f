// Grid-sampler coordinate helpers and the small device utilities shared by the sampler (mipmap.hip) and the scatter
// (grid_scatter.hip) kernels: PyTorch's grid-sampler primitives (ATen/native/cuda/GridSampler.cuh, UpSample.cuh --
// unnormalize, clip / reflect, safe_downgrade_to_int_range, cubic convolution with A = -0.75), the uv-field layout,
// wave-wide integer min / max and the typed global / LDS float adds.  Moved here verbatim from mipmap.hip: every
// translation unit gets its own copy (anonymous namespace), as before.
#pragma once

#include <type_traits>

#include "common.hpp"

namespace drtk_amd {
namespace {

// GridSampler.cuh primitives -------------------------------------------------------------------
template <typename T>
__device__ __forceinline__ T unnormalize(T coord, int size, bool align_corners, T* grad_in) {
  if (align_corners) {
    *grad_in = static_cast<T>(size - 1) / 2;
    return ((coord + 1.f) / 2) * (size - 1);
  }
  *grad_in = static_cast<T>(size) / 2;
  return ((coord + 1.f) * size - 1) / 2;
}
template <typename T>
__device__ __forceinline__ T clip_coord(T in, int limit, T* grad_in) {
  if (in <= T(0)) {
    *grad_in = T(0);
    return T(0);
  }
  const T mx = static_cast<T>(limit - 1);
  if (in >= mx) {
    *grad_in = T(0);
    return mx;
  }
  *grad_in = T(1);
  return in;
}
template <typename T>
__device__ __forceinline__ T clip_plain(T in, int limit) { // ::min(limit-1, ::max(in, 0))
  const T hi = static_cast<T>(limit - 1);
  const T lo = in > T(0) ? in : T(0);
  return hi < lo ? hi : lo;
}
template <typename T>
__device__ __forceinline__ T reflect_coord(T in, int twice_low, int twice_high, T* grad_in) {
  if (twice_low == twice_high) {
    *grad_in = T(0);
    return T(0);
  }
  int mult = 1;
  const T mn = static_cast<T>(twice_low) / 2;
  const T span = static_cast<T>(twice_high - twice_low) / 2;
  in = in - mn;
  if (in < T(0)) {
    mult = -1;
    in = -in;
  }
  const T extra = fmod(in, span);
  const int flips = static_cast<int>(floor(in / span));
  if (flips % 2 == 0) {
    *grad_in = static_cast<T>(mult);
    return extra + mn;
  }
  *grad_in = static_cast<T>(-mult);
  return span - extra + mn;
}

template <typename T>
__device__ __forceinline__ T safe_int_range(T x) {
  if (x > static_cast<T>(INT32_MAX - 1) || x < static_cast<T>(INT32_MIN) || !isfinite(static_cast<double>(x)))
    return T(-100.0);
  return x;
}
template <typename T>
__device__ __forceinline__ T compute_coordinates(T coord, int size, int padding, bool align_corners) {
  T unused;
  if (padding == 1) {
    coord = clip_plain(coord, size);
  } else if (padding == 2) {
    coord = align_corners ? reflect_coord(coord, 0, 2 * (size - 1), &unused) : reflect_coord(coord, -1, 2 * size - 1, &unused);
    coord = clip_plain(coord, size);
  }
  return safe_int_range(coord);
}
template <typename T>
__device__ __forceinline__ T source_index(T coord, int size, int padding, bool align_corners, T* grad_in) {
  T g_un, g_clip = T(1), g_refl = T(1);
  coord = unnormalize(coord, size, align_corners, &g_un);
  if (padding == 1) {
    coord = clip_coord(coord, size, &g_clip);
    g_un = g_un * g_clip;
  } else if (padding == 2) {
    coord = align_corners ? reflect_coord(coord, 0, 2 * (size - 1), &g_refl) : reflect_coord(coord, -1, 2 * size - 1, &g_refl);
    coord = clip_coord(coord, size, &g_clip);
    g_un = g_un * g_refl * g_clip;
  }
  *grad_in = g_un;
  return safe_int_range(coord);
}
template <typename T>
__device__ __forceinline__ void cubic_coeffs(T co[4], T t) { // UpSample.cuh get_cubic_upsampling_coefficients
  const T A = T(-0.75);
  T x = t + T(1.0);
  co[0] = ((A * x - 5 * A) * x + 8 * A) * x - 4 * A;
  x = t;
  co[1] = ((A + 2) * x - (A + 3)) * x * x + 1;
  x = T(1.0) - t;
  co[2] = ((A + 2) * x - (A + 3)) * x * x + 1;
  x = x + T(1.0);
  co[3] = ((A * x - 5 * A) * x + 8 * A) * x - 4 * A;
}
template <typename T>
__device__ __forceinline__ void cubic_coeffs_grad(T co[4], T t) { // grid_utils.h:130-144
  const T A = T(-0.75);
  T x = -1 - t;
  co[0] = (-3 * A * x - 10 * A) * x - 8 * A;
  x = -t;
  co[1] = (-3 * (A + 2) * x - 2 * (A + 3)) * x;
  x = 1 - t;
  co[2] = (3 * (A + 2) * x - 2 * (A + 3)) * x;
  x = 2 - t;
  co[3] = (3 * A * x - 10 * A) * x + 8 * A;
}

// Where element (n, pixel, c) of a uv field [N,H,W,2] lives: n * sN + pixel * sP + c * sC elements from the base (pixel =
// y * W + x).  Contiguous: (2HW, 2, 1), read and written as one 8- / 16-byte pair per pixel (`pair`); the channel-first
// image `interpolate` produces, seen through permute(0, 2, 3, 1): (2HW, 1, HW) -- two coalesced loads, no copy.
struct GridLayout {
  long long sN, sP, sC;
  bool pair;
};
template <typename T>
__device__ __forceinline__ void store_grid_grad(T* __restrict__ gg, const GridLayout& gl, int64_t n, int64_t pix, T gx, T gy) {
  T* g = gg + n * gl.sN + pix * gl.sP;
  if (gl.pair) {
    using V2 = typename std::conditional<sizeof(T) == 4, float2, double2>::type;
    *reinterpret_cast<V2*>(g) = V2{gx, gy};
  } else {
    g[0] = gx, g[gl.sC] = gy;
  }
}

template <typename T>
using GlobalPtr = __attribute__((address_space(1))) T*;

// float/double atomic add through an explicitly global pointer (global_atomic_add_f32 / _f64)
template <typename T>
__device__ __forceinline__ void atomic_add_g1(GlobalPtr<T> p, T v) {
  __hip_atomic_fetch_add(p, v, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
}

// float/double add on an explicitly LDS-typed pointer (ds_add_f32 / ds_add_f64, no return)
template <typename T>
__device__ __forceinline__ void lds_add(T* p, T v) {
  using LdsPtr = __attribute__((address_space(3))) T*;
  __hip_atomic_fetch_add((LdsPtr)p, v, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_WORKGROUP);
}

// Wave-wide min / max of an int, every lane active: four DPP steps leave each 16-lane row's result in all of its lanes,
// four v_readlane + scalar min / max join the rows (a __shfl_xor ladder is six dependent ds_bpermute round trips).
template <int CTRL>
__device__ __forceinline__ int dpp_i32(int v) {
  return __builtin_amdgcn_update_dpp(v, v, CTRL, 0xF, 0xF, false);
}
__device__ __forceinline__ int wave_min_i32(int v) {
  v = min(v, dpp_i32<0xB1>(v));  // quad_perm [1,0,3,2]
  v = min(v, dpp_i32<0x4E>(v));  // quad_perm [2,3,0,1]
  v = min(v, dpp_i32<0x141>(v)); // row_half_mirror
  v = min(v, dpp_i32<0x140>(v)); // row_mirror
  return min(min(__builtin_amdgcn_readlane(v, 0), __builtin_amdgcn_readlane(v, 16)),
             min(__builtin_amdgcn_readlane(v, 32), __builtin_amdgcn_readlane(v, 48)));
}
__device__ __forceinline__ int wave_max_i32(int v) {
  v = max(v, dpp_i32<0xB1>(v));
  v = max(v, dpp_i32<0x4E>(v));
  v = max(v, dpp_i32<0x141>(v));
  v = max(v, dpp_i32<0x140>(v));
  return max(max(__builtin_amdgcn_readlane(v, 0), __builtin_amdgcn_readlane(v, 16)),
             max(__builtin_amdgcn_readlane(v, 32), __builtin_amdgcn_readlane(v, 48)));
}

__device__ __forceinline__ void wave_minmax2(int x, int y, bool on, int& x0, int& y0, int& x1, int& y1) {
  x0 = wave_min_i32(on ? x : INT32_MAX), y0 = wave_min_i32(on ? y : INT32_MAX);
  x1 = wave_max_i32(on ? x : INT32_MIN), y1 = wave_max_i32(on ? y : INT32_MIN);
}

// grid_layout = {sN, sP, sC} in elements (NULL: contiguous [N,H,W,2]); the pair access needs sC = 1, even strides and a
// base aligned to two elements
int make_grid_layout(GridLayout& gl, const int64_t* layout, const void* base, int64_t H, int64_t W, size_t elem) {
  gl.sN = layout ? layout[0] : 2 * H * W;
  gl.sP = layout ? layout[1] : 2;
  gl.sC = layout ? layout[2] : 1;
  if (gl.sN < 0 || gl.sP <= 0 || gl.sC <= 0) return DRTK_ERR_INVALID_ARGUMENT;
  gl.pair = gl.sC == 1 && gl.sP % 2 == 0 && gl.sN % 2 == 0 && reinterpret_cast<uintptr_t>(base) % (2 * elem) == 0;
  return DRTK_OK;
}

} // namespace
} // namespace drtk_amd
