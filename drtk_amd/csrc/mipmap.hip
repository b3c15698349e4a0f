// mipmap_grid_sampler_2d -- grid_sample with trilinear mip selection and anisotropic taps, forward
// and backward.
//
// Reference: src/mipmap_grid_sampler/mipmap_grid_sampler_kernel.cu:20-897 (device code), built on
// PyTorch's grid-sampler primitives (ATen/native/cuda/GridSampler.cuh, UpSample.cuh -- unnormalize,
// clip / reflect, safe_downgrade_to_int_range, cubic convolution with A = -0.75).
//
// Reference shape: one thread per output pixel; for every tap and mip level it walks the channels
// and read-modify-writes the *global* output once per corner (4 RMW per tap, level and channel).
// Here: lane = output pixel as well (the uv field is pixel-ordered, so grid / Jacobian loads are one
// 8- and one 16-byte vector per lane and the channel planes of the output are written coalesced),
// but
//   * the tap geometry (source index, padding, corner offsets and weights -- or the 4+4 bicubic
//     coordinates) is computed once per (tap, level) and reused by all channels,
//   * channels accumulate in registers in blocks of four and every output element is stored once,
//   * the level table lives in LDS (levels are selected per lane, so a kernel-argument array would
//     be indexed through scratch memory).
// Accumulation order per output element is the reference's (taps, then level d1 / d1+1, then
// corners), so results match the CPU restatement to rounding of the transcendental log2 only.
// The forward pass ignores align_corners exactly like the reference (:423 forces it to false);
// the backward pass honours it (:641 ff).
#include <type_traits>

#include "common.hpp"
#include "grid_coords.hpp" // coordinate transforms, GridLayout, wave min / max, typed atomic adds
#include "segscatter.hpp" // wave_lds_sync

#ifdef DRTK_AMD_ABLATION
// Profiling build only: what the tiled backward's rounds are made of (profiles/mipmap_bench.py --rounds-stats).
// [0] tiles with upstream gradient, [r] tiles that enter round r (1..7), [8] (tap, level) pairs walked in the first pass,
// [9] pairs left pending by it, [10] pairs that end in global memory after the last round
namespace drtk_amd {
__device__ unsigned long long g_mip_stats[16];
}
extern "C" __attribute__((visibility("default"))) int drtk_amd_debug_read_mip_stats(unsigned long long* out) {
  if (hipMemcpyFromSymbol(out, HIP_SYMBOL(drtk_amd::g_mip_stats), sizeof(unsigned long long) * 16) != hipSuccess) return -3;
  unsigned long long z[16] = {};
  if (hipMemcpyToSymbol(HIP_SYMBOL(drtk_amd::g_mip_stats), z, sizeof(z)) != hipSuccess) return -3;
  return 0;
}
#define DRTK_MIP_STAT(i, v) do { if (DRTK_DBG(dbg, 64)) atomicAdd(&::drtk_amd::g_mip_stats[i], static_cast<unsigned long long>(v)); } while (0)
// ... and WHERE the pairs are that end in global memory (flag 64 as well): {view << 24 | tile, thread << 16 | level, x, y} of
// the pair's north-west texel, the first 2^20 of them (profiles/mipmap_bench.py --leftover-dump)
namespace drtk_amd {
constexpr unsigned kMipDumpMax = 1u << 20;
__device__ unsigned int g_mip_dump_n;
__device__ uint4 g_mip_dump[kMipDumpMax];
}
extern "C" __attribute__((visibility("default"))) int drtk_amd_debug_read_mip_dump(unsigned int* out, unsigned int* n) {
  if (hipMemcpyFromSymbol(n, HIP_SYMBOL(drtk_amd::g_mip_dump_n), sizeof(unsigned int)) != hipSuccess) return -3;
  if (*n > drtk_amd::kMipDumpMax) *n = drtk_amd::kMipDumpMax;
  if (*n && hipMemcpyFromSymbol(out, HIP_SYMBOL(drtk_amd::g_mip_dump), sizeof(uint4) * *n) != hipSuccess) return -3;
  const unsigned int z = 0;
  if (hipMemcpyToSymbol(HIP_SYMBOL(drtk_amd::g_mip_dump_n), &z, sizeof(z)) != hipSuccess) return -3;
  return 0;
}
#define DRTK_MIP_DUMP_IF(flag, a, b, c, d) do { if (DRTK_DBG(dbg, flag)) { const unsigned int k_ = atomicAdd(&::drtk_amd::g_mip_dump_n, 1u); \
  if (k_ < ::drtk_amd::kMipDumpMax) ::drtk_amd::g_mip_dump[k_] = make_uint4(a, b, c, d); } } while (0)
#define DRTK_MIP_DUMP(a, b, c, d) DRTK_MIP_DUMP_IF(64, a, b, c, d)
// flag 1 << 20: a tile's timeline instead -- {view << 24 | tile, further rounds, start, end} in 10 ns ticks (--tile-times)
#define DRTK_MIP_TILE_T0() const unsigned int tile_t0_ = static_cast<unsigned int>(wall_clock64()); unsigned int tile_ph_[3] = {0u, 0u, 0u}
#define DRTK_MIP_TILE_PHASE(k) tile_ph_[k] = static_cast<unsigned int>(wall_clock64()) - tile_t0_
// flag 1 << 21: the phases of a tile instead -- {.., rounds | inputs there << 16, windows placed | taps done << 16, end}, ticks since the start
#define DRTK_MIP_TILE_DONE(rounds) do { if (tid == 0) { \
  DRTK_MIP_DUMP_IF(1 << 20, static_cast<unsigned>(n) << 24 | static_cast<unsigned>(tile), rounds, tile_t0_, static_cast<unsigned int>(wall_clock64())); \
  DRTK_MIP_DUMP_IF(1 << 21, static_cast<unsigned>(n) << 24 | static_cast<unsigned>(tile), static_cast<unsigned>(rounds) | tile_ph_[0] << 16, tile_ph_[1] | tile_ph_[2] << 16, static_cast<unsigned int>(wall_clock64()) - tile_t0_); } } while (0)
#else
#define DRTK_MIP_STAT(i, v) do { } while (0)
#define DRTK_MIP_DUMP(a, b, c, d) do { } while (0)
#define DRTK_MIP_TILE_T0() do { } while (0)
#define DRTK_MIP_TILE_PHASE(k) do { } while (0)
#define DRTK_MIP_TILE_DONE(rounds) do { } while (0)
#endif

namespace drtk_amd {
namespace {

constexpr int kMaxLevels = 11; // mipmap_grid_sampler_kernel.cu:16

struct LevelTable {
  const void* ptr[kMaxLevels];
  void* grad[kMaxLevels];
  long long sn[kMaxLevels]; // elements between the views of a level (0: one texture shared by all views)
  int h[kMaxLevels];
  int w[kMaxLevels];
};

// Correctly rounded (the footprint lengths feed a floor() that picks the mip level).  Not `__fsqrt_rn`, which this
// toolchain defines as the native 1-ulp square root -- see edge_grad.hip: sqrt_t.
__device__ __forceinline__ float sqrt_rn(float x) {
  return __builtin_sqrtf(x);
}
__device__ __forceinline__ double sqrt_rn(double x) {
  return __builtin_sqrt(x);
}

__device__ __forceinline__ float tmin(float a, float b) { return fminf(a, b); }
__device__ __forceinline__ double tmin(double a, double b) { return fmin(a, b); }
__device__ __forceinline__ float tmax(float a, float b) { return fmaxf(a, b); }
__device__ __forceinline__ double tmax(double a, double b) { return fmax(a, b); }
__device__ __forceinline__ float tfma(float a, float b, float c) { return __builtin_fmaf(a, b, c); }
__device__ __forceinline__ double tfma(double a, double b, double c) { return __builtin_fma(a, b, c); }
__device__ __forceinline__ float tabs(float a) { return fabsf(a); }
__device__ __forceinline__ double tabs(double a) { return fabs(a); }
// reflect_coord for the lean kernels: the same value and multiplier, the long form only when a lane of the wave needs it.
// With a = |in - low| < span no flip occurs: fmod(a, span) == a exactly and floor(a / span) == 0, so the reference's
// `extra + low` is `a + low` -- two additions instead of an fmod, a division and a floor.  (Taps further than one texture
// width beyond the border, or non-finite: the wave takes reflect_coord itself.)
template <typename T>
__device__ __forceinline__ T reflect_coord_lean(T in, int twice_low, int twice_high, T* grad_in) {
  if (twice_low == twice_high) {
    *grad_in = T(0);
    return T(0);
  }
  const T mn = static_cast<T>(twice_low) / 2;
  const T span = static_cast<T>(twice_high - twice_low) / 2;
  T a = in - mn;
  T m = T(1);
  if (a < T(0)) m = T(-1), a = -a;
  if (__ballot(!(a < span)) != 0) return reflect_coord(in, twice_low, twice_high, grad_in);
  *grad_in = m;
  return a + mn;
}
// ... followed by the clamp to the level (clip_coord: a clamped coordinate has a zero gradient), both axes of a tap
template <typename T>
__device__ __forceinline__ void reflect_clip_lean(T ixu, T iyu, int w, int h, bool align_corners, T& ix, T& iy, T& mx, T& my) {
  T gx, gy;
  const T rx = align_corners ? reflect_coord_lean(ixu, 0, 2 * (w - 1), &gx) : reflect_coord_lean(ixu, -1, 2 * w - 1, &gx);
  const T ry = align_corners ? reflect_coord_lean(iyu, 0, 2 * (h - 1), &gy) : reflect_coord_lean(iyu, -1, 2 * h - 1, &gy);
  const T wm1 = static_cast<T>(w - 1), hm1 = static_cast<T>(h - 1);
  mx = ((rx > T(0)) & (rx < wm1)) ? mx * gx : T(0), my = ((ry > T(0)) & (ry < hm1)) ? my * gy : T(0);
  ix = tmin(tmax(rx, T(0)), wm1), iy = tmin(tmax(ry, T(0)), hm1);
}

// Per-pixel tap setup: mipmap_grid_sampler_kernel.cu:441-508 (== :679-746 in the backward kernel).
template <typename T>
struct Taps {
  T u, v, du, dv, a;
  int d1, n;
};
// the pixel's uv and uv Jacobian: one 8- and one 16-byte load (float)
template <typename T>
struct PixelUV {
  T u, v, dudx, dvdx, dudy, dvdy;
};
template <typename T>
__device__ __forceinline__ PixelUV<T> load_pixel_uv(
    const T* __restrict__ grid, const GridLayout& gl, const T* __restrict__ vt, int64_t n, int64_t pix, int64_t index) {
  PixelUV<T> p;
  const T* g = grid + n * gl.sN + pix * gl.sP;
  if (gl.pair) {
    using V2 = typename std::conditional<sizeof(T) == 4, float2, double2>::type;
    const V2 q = *reinterpret_cast<const V2*>(g);
    p.u = q.x, p.v = q.y;
  } else {
    p.u = g[0], p.v = g[gl.sC];
  }
  if constexpr (sizeof(T) == 4) {
    const float4 j = *reinterpret_cast<const float4*>(vt + index * 4);
    p.dudx = j.x, p.dvdx = j.y, p.dudy = j.z, p.dvdy = j.w;
  } else {
    const double2 j0 = *reinterpret_cast<const double2*>(vt + index * 4);
    const double2 j1 = *reinterpret_cast<const double2*>(vt + index * 4 + 2);
    p.dudx = j0.x, p.dvdx = j0.y, p.dudy = j1.x, p.dvdy = j1.y;
  }
  return p;
}
template <typename T>
__device__ __forceinline__ Taps<T> setup_taps(
    const PixelUV<T>& uv, int inp_H, int inp_W, int mipmaps, int max_aniso, bool force_max_aniso, bool clip_grad) {
  Taps<T> t;
  t.u = uv.u, t.v = uv.v;
  T dudx = uv.dudx, dvdx = uv.dvdx, dudy = uv.dudy, dvdy = uv.dvdy;
  // footprint lengths (:455-456, written with pow there): sqrt(a*a + b*b + 1e-12) with IEEE multiply and
  // sqrt -- the tap count below is a discontinuous function of them, so they are evaluated in the one
  // form that is bit-reproducible everywhere (profiles/NOTES.md §3.7)
  const T ax = fabs(dudx * inp_W), bx = fabs(dvdx * inp_H);
  const T ay = fabs(dudy * inp_W), by = fabs(dvdy * inp_H);
  const T px = sqrt_rn(ax * ax + bx * bx + 1e-12f);
  const T py = sqrt_rn(ay * ay + by * by + 1e-12f);
  const T p_max = px > py ? px : py;
  const T p_min = px < py ? px : py;
  T Nf = ceil(p_max / p_min);
  if (static_cast<T>(max_aniso) < Nf) Nf = static_cast<T>(max_aniso);
  if (p_min == 0.0 || Nf == 0) Nf = 1;
  T lambda_ = log2(p_max / Nf);
  if (isnan(lambda_) || isinf(lambda_)) lambda_ = 0.0f;
  const double lim = static_cast<double>(mipmaps - 1) - 1e-6;
  T l = static_cast<T>(static_cast<double>(lambda_) < lim ? static_cast<double>(lambda_) : lim);
  if (clip_grad && lambda_ > static_cast<T>(mipmaps - 1)) {
    const T p_max_corrected = exp2(l) * Nf;
    const T scaling = p_max_corrected / p_max;
    dudx *= scaling;
    dvdx *= scaling;
    dudy *= scaling;
    dvdy *= scaling;
  }
  l = static_cast<T>(static_cast<double>(l) > 0.0 ? static_cast<double>(l) : 0.0);
  t.d1 = static_cast<int>(floor(l));
  t.a = l - static_cast<T>(t.d1);
  t.n = force_max_aniso ? max_aniso : static_cast<int>(Nf);
  if (px > py) {
    t.du = dudx, t.dv = dvdx;
  } else {
    t.du = dudy, t.dv = dvdy;
  }
  return t;
}

// Bilinear corner geometry of one (tap, level): offsets (or -1 when out of bounds) and weights.
template <typename T>
struct Quad {
  int o_nw, o_ne, o_sw, o_se;
  T nw, ne, sw, se;
  T ix, iy;
  int ix_nw, iy_nw;
  T mx, my;
};
template <typename T>
__device__ __forceinline__ Quad<T> bilinear_quad(T x, T y, int H, int W, int padding, bool align_corners) {
  Quad<T> q;
  q.ix = source_index(x, W, padding, align_corners, &q.mx);
  q.iy = source_index(y, H, padding, align_corners, &q.my);
  q.ix_nw = static_cast<int>(floor(q.ix));
  q.iy_nw = static_cast<int>(floor(q.iy));
  const int ix_se = q.ix_nw + 1, iy_se = q.iy_nw + 1;
  q.nw = (ix_se - q.ix) * (iy_se - q.iy);
  q.ne = (q.ix - q.ix_nw) * (iy_se - q.iy);
  q.sw = (ix_se - q.ix) * (q.iy - q.iy_nw);
  q.se = (q.ix - q.ix_nw) * (q.iy - q.iy_nw);
  const bool x0 = q.ix_nw >= 0 && q.ix_nw < W, x1 = ix_se >= 0 && ix_se < W;
  const bool y0 = q.iy_nw >= 0 && q.iy_nw < H, y1 = iy_se >= 0 && iy_se < H;
  q.o_nw = (x0 && y0) ? q.iy_nw * W + q.ix_nw : -1;
  q.o_ne = (x1 && y0) ? q.iy_nw * W + ix_se : -1;
  q.o_sw = (x0 && y1) ? iy_se * W + q.ix_nw : -1;
  q.o_se = (x1 && y1) ? iy_se * W + ix_se : -1;
  return q;
}

// Bicubic footprint of one (tap, level): 4 column and 4 row indices after padding (-1: zero tap).
template <typename T>
struct Cubic {
  int xi[4], yi[4];
  T tx, ty, mx, my;
};
template <typename T>
__device__ __forceinline__ Cubic<T> bicubic_footprint(T x, T y, int H, int W, int padding, bool align_corners) {
  Cubic<T> c;
  const T ix = unnormalize(x, W, align_corners, &c.mx);
  const T iy = unnormalize(y, H, align_corners, &c.my);
  const T ix_nw = floor(ix), iy_nw = floor(iy);
  c.tx = ix - ix_nw;
  c.ty = iy - iy_nw;
  // A footprint whose sixteen texels lie inside the level -- nearly all -- needs none of the eight padding transforms
  // below: clip, reflect and the integer-range guard map an in-range INTEGER coordinate to itself exactly (reflection:
  // (k + 1/2) - 1/2 with fmod(k + 1/2, size) == k + 1/2 and no flip), so the indices are nw - 1 ... nw + 2.
  // Each transform is ~20 instructions (branches on the padding mode, an isfinite through double): 160 per (tap, level).
  if (W >= 4 && H >= 4 && fabs(ix) < T(1e9) && fabs(iy) < T(1e9)) { // (the comparisons are false for NaN)
    const int kx = static_cast<int>(ix_nw), ky = static_cast<int>(iy_nw);
    if (static_cast<unsigned>(kx - 1) < static_cast<unsigned>(W - 3) && static_cast<unsigned>(ky - 1) < static_cast<unsigned>(H - 3)) {
#pragma unroll
      for (int i = 0; i < 4; ++i) c.xi[i] = kx - 1 + i, c.yi[i] = ky - 1 + i;
      return c;
    }
  }
#pragma unroll
  for (int i = 0; i < 4; ++i) {
    const int xv = static_cast<int>(compute_coordinates<T>(ix_nw - 1 + i, W, padding, align_corners));
    const int yv = static_cast<int>(compute_coordinates<T>(iy_nw - 1 + i, H, padding, align_corners));
    c.xi[i] = (xv >= 0 && xv < W) ? xv : -1;
    c.yi[i] = (yv >= 0 && yv < H) ? yv : -1;
  }
  return c;
}

__device__ __forceinline__ void stage_levels(
    const LevelTable& lv, int mipmaps, const void** s_ptr, void** s_grad, int* s_h, int* s_w, long long* s_sn) {
  if (threadIdx.x < kMaxLevels) {
    const int i = threadIdx.x < mipmaps ? threadIdx.x : 0;
    s_ptr[threadIdx.x] = lv.ptr[i];
    s_grad[threadIdx.x] = lv.grad[i];
    s_sn[threadIdx.x] = lv.sn[i];
    s_h[threadIdx.x] = lv.h[i];
    s_w[threadIdx.x] = lv.w[i];
  }
  __syncthreads();
}

// Tap i of n sits at u + du * f, f = (i + 1.0) / (n + 1.0) * 2.0 - 1.0 in double (mipmap_grid_sampler_kernel.cu:497-499):
// a double division per tap and pixel.  The workgroup computes the table of f for n <= 8 once -- with the same device
// arithmetic, so the values are the same -- and the taps read it from LDS; larger n (max_aniso > 8) divide as before.
constexpr int kTapTab = 8; // tap counts 1 ... kTapTab have a row of the table
static_assert(kTapTab * kTapTab <= kBlock, "one table entry per thread");
__device__ __forceinline__ void stage_tap_table(double* s_f) { // call before a __syncthreads()
  if (threadIdx.x < kTapTab * kTapTab) {
    const int i = threadIdx.x % kTapTab, n = threadIdx.x / kTapTab + 1;
    s_f[threadIdx.x] = (i + 1.0) / (n + 1.0) * 2.0 - 1.0;
  }
}
__device__ __forceinline__ double tap_f(const double* s_f, int i, int n) {
  return n <= kTapTab ? s_f[(n - 1) * kTapTab + i] : (i + 1.0) / (n + 1.0) * 2.0 - 1.0;
}

// two horizontally adjacent texels, loaded with one element-aligned 8/16-byte access
template <typename T>
struct PairOf;
template <>
struct PairOf<float> {
  typedef float type __attribute__((ext_vector_type(2), aligned(4)));
};
template <>
struct PairOf<double> {
  typedef double type __attribute__((ext_vector_type(2), aligned(8)));
};
template <typename T>
using Pair = typename PairOf<T>::type;

constexpr int kChBlock = 4; // channels accumulated in registers per sweep over the taps

// ---- Forward, general: bicubic, and bilinear calls the lean kernel below does not take (sampler_route) ---------------------
// PAD: the padding mode as a compile-time constant (see the tile kernels of the backward pass).
// waves per SIMD the kernel is compiled for: float bicubic fits six (76-78 registers; asked for seven it spills 2-3)
template <typename T, int MODE>
constexpr int forward_waves_per_simd() { return (MODE == 2 && sizeof(T) == 4) ? 6 : 1; }
template <typename T, int MODE, int PAD>
__global__ __launch_bounds__(kBlock, (forward_waves_per_simd<T, MODE>())) void mipmap_forward_kernel(
    LevelTable lv, int mipmaps, const T* __restrict__ grid, GridLayout gl, const T* __restrict__ vt, int64_t count, int C,
    int64_t HW, int max_aniso, bool force_max_aniso, bool clip_grad, T* __restrict__ out, int strip) {
  constexpr int padding = PAD;
  __shared__ const void* s_ptr[kMaxLevels];
  __shared__ void* s_grad[kMaxLevels];
  __shared__ int s_h[kMaxLevels], s_w[kMaxLevels];
  __shared__ long long s_sn[kMaxLevels];
  __shared__ double s_f[kTapTab * kTapTab];
  stage_tap_table(s_f);
  stage_levels(lv, mipmaps, s_ptr, s_grad, s_h, s_w, s_sn);
  const int64_t index = int64_t(tile_index(strip)) * kBlock + threadIdx.x;
  if (index >= count) return;
  const int64_t n = index / HW;
  const bool align_corners = false; // mipmap_grid_sampler_kernel.cu:423
  const Taps<T> t = setup_taps<T>(load_pixel_uv<T>(grid, gl, vt, n, index - n * HW, index), s_h[0], s_w[0], mipmaps, max_aniso, force_max_aniso, clip_grad);
  const int n_lv = mipmaps > 1 ? 2 : 1;
  T* out_px = out + n * C * HW + (index - n * HW);
  const T alpha_1 = t.a / t.n;
  const T alpha_2 = static_cast<T>((1.0 - t.a) / t.n);
  // the pixel's two levels: sizes and base pointers once, not per tap (the level pointers come back from LDS as generic
  // pointers: pin them to the global address space, otherwise every texel access is a flat_load)
  int lv_h[2], lv_w[2];
  GlobalPtr<const T> lv_base[2];
#pragma unroll
  for (int s = 0; s < 2; ++s) {
    const int d = s < n_lv ? t.d1 + s : 0;
    lv_h[s] = s_h[d], lv_w[s] = s_w[d];
    lv_base[s] = (GlobalPtr<const T>)(static_cast<const T*>(s_ptr[d]) + n * s_sn[d]);
  }

  for (int c0 = 0; c0 < C; c0 += kChBlock) {
    T acc[kChBlock];
#pragma unroll
    for (int cc = 0; cc < kChBlock; ++cc) acc[cc] = T(0);
    for (int i = 0; i < t.n; ++i) {
      const double f = tap_f(s_f, i, t.n);
      const T x = t.u + static_cast<T>(t.du * f), y = t.v + static_cast<T>(t.dv * f);
#pragma unroll
      for (int s = 0; s < 2; ++s) {
        if (s >= n_lv) break;
        const T alpha = s == 0 ? alpha_2 : alpha_1;
        // A level whose weight is exactly zero -- the second level of every magnified pixel (a == 0) -- contributes
        // +-0 * texel to every channel: skipped, texels are taken to be finite (as in the backward pass).
        if (alpha == T(0)) continue;
        // (bicubic: the level's size and the view's base pointer are re-read from the LDS table per (tap, level) instead of
        // living in registers across the tap loop, as in the lean forward: that is what fits six waves per SIMD)
        const bool reread = MODE == 2;
        const int d_s = t.d1 + s;
        const int h = reread ? s_h[d_s] : lv_h[s], w = reread ? s_w[d_s] : lv_w[s];
        const int64_t plane = int64_t(h) * w;
        const GlobalPtr<const T> base =
            (reread ? (GlobalPtr<const T>)(static_cast<const T*>(s_ptr[d_s]) + n * s_sn[d_s]) : lv_base[s]) + c0 * plane;
        if constexpr (MODE == 0) {
          const Quad<T> q = bilinear_quad<T>(x, y, h, w, padding, align_corners);
          if ((q.o_nw | q.o_ne | q.o_sw | q.o_se) >= 0) {
            // interior tap: two 8-byte loads and four products per channel, no per-corner branch
            Pair<T> top[kChBlock], bot[kChBlock];
#pragma unroll
            for (int cc = 0; cc < kChBlock; ++cc) {
              if (c0 + cc < C) {
                top[cc] = *(GlobalPtr<const Pair<T>>)(base + cc * plane + q.o_nw);
                bot[cc] = *(GlobalPtr<const Pair<T>>)(base + cc * plane + q.o_sw);
              }
            }
#pragma unroll
            for (int cc = 0; cc < kChBlock; ++cc) {
              if (c0 + cc < C) {
                acc[cc] += top[cc].x * q.nw * alpha;
                acc[cc] += top[cc].y * q.ne * alpha;
                acc[cc] += bot[cc].x * q.sw * alpha;
                acc[cc] += bot[cc].y * q.se * alpha;
              }
            }
            continue;
          }
#pragma unroll
          for (int cc = 0; cc < kChBlock; ++cc) {
            if (c0 + cc < C) {
              const GlobalPtr<const T> p = base + cc * plane;
              // the two texels of a row are adjacent in memory: one 8-byte (4-byte aligned) load per row
              T v_nw = T(0), v_ne = T(0), v_sw = T(0), v_se = T(0);
              if (q.o_nw >= 0 && q.o_ne >= 0) {
                const Pair<T> t2 = *(GlobalPtr<const Pair<T>>)(p + q.o_nw);
                v_nw = t2.x, v_ne = t2.y;
              } else {
                if (q.o_nw >= 0) v_nw = p[q.o_nw];
                if (q.o_ne >= 0) v_ne = p[q.o_ne];
              }
              if (q.o_sw >= 0 && q.o_se >= 0) {
                const Pair<T> t2 = *(GlobalPtr<const Pair<T>>)(p + q.o_sw);
                v_sw = t2.x, v_se = t2.y;
              } else {
                if (q.o_sw >= 0) v_sw = p[q.o_sw];
                if (q.o_se >= 0) v_se = p[q.o_se];
              }
              if (q.o_nw >= 0) acc[cc] += v_nw * q.nw * alpha;
              if (q.o_ne >= 0) acc[cc] += v_ne * q.ne * alpha;
              if (q.o_sw >= 0) acc[cc] += v_sw * q.sw * alpha;
              if (q.o_se >= 0) acc[cc] += v_se * q.se * alpha;
            }
          }
        } else {
          const Cubic<T> cb = bicubic_footprint<T>(x, y, h, w, padding, align_corners);
          T cx[4], cy[4];
          cubic_coeffs(cx, cb.tx);
          cubic_coeffs(cy, cb.ty);
          // interior footprint (sixteen consecutive texels inside the level, nearly all): a row is ONE 16-byte load
          // (element-aligned) instead of four predicated 4-byte ones; same products, same order
          const int bx = cb.xi[0];
          const bool interior = bx >= 0 && cb.xi[1] == bx + 1 && cb.xi[2] == bx + 2 && cb.xi[3] == bx + 3 &&
              (cb.yi[0] | cb.yi[1] | cb.yi[2] | cb.yi[3]) >= 0;
#pragma unroll
          for (int cc = 0; cc < kChBlock; ++cc) {
            if (c0 + cc < C) {
              const GlobalPtr<const T> p = base + cc * plane;
              T co[4];
              if (interior) {
                typedef T Quad4 __attribute__((ext_vector_type(4), aligned(sizeof(T))));
                Quad4 row[4];
#pragma unroll
                for (int r = 0; r < 4; ++r) row[r] = *(GlobalPtr<const Quad4>)(p + cb.yi[r] * w + bx);
#pragma unroll
                for (int r = 0; r < 4; ++r) co[r] = row[r].x * cx[0] + row[r].y * cx[1] + row[r].z * cx[2] + row[r].w * cx[3];
              } else {
                // (a footprint on the border of its level, rare: row by row in a loop that is NOT unrolled -- the four rows'
                // sixteen predicated loads in flight at once were part of what this kernel's registers were for; same sums)
                T sum = T(0);
#pragma unroll 1
                for (int r = 0; r < 4; ++r) {
                  const int yr = r == 0 ? cb.yi[0] : r == 1 ? cb.yi[1] : r == 2 ? cb.yi[2] : cb.yi[3];
                  const T cyr = r == 0 ? cy[0] : r == 1 ? cy[1] : r == 2 ? cy[2] : cy[3];
                  T xv[4];
#pragma unroll
                  for (int k = 0; k < 4; ++k) xv[k] = (yr >= 0 && cb.xi[k] >= 0) ? p[yr * w + cb.xi[k]] : T(0);
                  const T cor = xv[0] * cx[0] + xv[1] * cx[1] + xv[2] * cx[2] + xv[3] * cx[3];
                  sum = r == 0 ? cor * cyr : sum + cor * cyr;
                }
                acc[cc] += sum * alpha;
                continue;
              }
              acc[cc] += (co[0] * cy[0] + co[1] * cy[1] + co[2] * cy[2] + co[3] * cy[3]) * alpha;
            }
          }
        }
      }
    }
#pragma unroll
    for (int cc = 0; cc < kChBlock; ++cc) {
      if (c0 + cc < C) out_px[int64_t(c0 + cc) * HW] = acc[cc];
    }
  }
}

// ---- Forward, bilinear, any padding, float and double: the LEAN kernel -----------------------------------------------------
// The general kernel above is INSTRUCTION-bound, not latency-bound (profiles/NOTES.md R5, R13): per (tap, level) it issues ~170
// vector and ~60 scalar instructions -- per-corner validity logic in 87 exec-mask regions, 64-bit address arithmetic per texel
// load, three dependent operations per product, the backward pass's gradient multipliers.  Here the common case -- every corner
// of the tap inside its level -- is ONE straight line for the whole wave:
//   * cell decisions are the reference's operations in the reference's order (tap position through the double product,
//     unnormalise, clip, floor: a tap must land in the same texel cell as in the oracle, the grid gradient's terms are
//     discontinuous there); what is CONTINUOUS is computed the cheap way: corner weights times the level's weight once per
//     tap, then one fma per texel and channel (12 instead of 36 operations for RGB; differs from the reference's
//     (texel * weight) * alpha by an ulp of each term);
//   * lanes whose tap is not interior (or that have no tap i) get offset 0 and weight 0 and run the same loads and fmas -- no
//     exec-mask regions in the loop; the border taps themselves (rare) are added by a branch the wave only takes if it has one;
//   * 32-bit texel offsets from per-pixel level bases.
// Bicubic stays with the kernel above.  Double: the same kernel on `T`.
// Waves per SIMD the kernel is compiled for.  It is a chain of gathers per tap and lives on waves in flight: float with up to
// three channels per sweep fits eight (62-64 registers), four channels seven (70-72), double four (62-102).
template <typename T, int CB>
constexpr int lean_forward_waves_per_simd() { return sizeof(T) == 8 ? 4 : (CB <= 3 ? 8 : 7); }
template <typename T, int PAD, int CB>
__global__ __launch_bounds__(kBlock, (lean_forward_waves_per_simd<T, CB>())) void mipmap_forward_lean_kernel(
    LevelTable lv, int mipmaps, const T* __restrict__ grid, GridLayout gl, const T* __restrict__ vt, int C,
    int64_t HW, int max_aniso, bool force_max_aniso, bool clip_grad, T* __restrict__ out, int strip) {
  static_assert(PAD >= 0 && PAD <= 2, "zeros, border or reflection padding");
  static_assert(CB >= 1 && CB <= 4, "channels per sweep over the taps (C is a multiple of CB)");
  constexpr int padding = PAD;
  constexpr bool align_corners = false; // mipmap_grid_sampler_kernel.cu:423
  __shared__ const void* s_ptr[kMaxLevels];
  __shared__ void* s_grad[kMaxLevels];
  __shared__ int s_h[kMaxLevels], s_w[kMaxLevels];
  __shared__ long long s_sn[kMaxLevels];
  __shared__ double s_f[kTapTab * kTapTab];
  stage_tap_table(s_f);
  stage_levels(lv, mipmaps, s_ptr, s_grad, s_h, s_w, s_sn);
  // (view = blockIdx.y: `index / HW` on a flat grid is a 64-bit division per pixel, ~80 instructions)
  const int64_t n = blockIdx.y;
  const int64_t pix_raw = int64_t(tile_index(strip)) * kBlock + threadIdx.x;
  const bool valid = pix_raw < HW;
  const int64_t pix = valid ? pix_raw : 0;
  const int64_t index = n * HW + pix;
  Taps<T> t = {};
  if (valid) t = setup_taps<T>(load_pixel_uv<T>(grid, gl, vt, n, pix, index), s_h[0], s_w[0], mipmaps, max_aniso, force_max_aniso, clip_grad);
  const int n_lv = mipmaps > 1 ? 2 : 1;
  // the levels' weights a / n and (1 - a) / n: continuous quantities, computed in float from one reciprocal (the reference
  // divides the second one in double, :486: a 16-instruction sequence at a quarter of the float rate, for the last ulp)
  // (double: the reference's two divisions, :485-486 -- the once-per-pixel cost is nothing beside the taps)
  const T rn = T(1) / static_cast<T>(max(t.n, 1));
  const T alpha_1 = !valid ? T(0) : sizeof(T) == 8 ? t.a / static_cast<T>(max(t.n, 1)) : t.a * rn;
  const T alpha_2 = !valid ? T(0) : sizeof(T) == 8 ? (T(1) - t.a) / static_cast<T>(max(t.n, 1)) : (T(1) - t.a) * rn;
  // level slot s = 0: level d1 with weight alpha_2; s = 1: level d1 + 1 with alpha_1.  A slot whose weight is exactly
  // zero -- the coarser level of every magnified pixel -- is dead (as in the kernels above).
  const bool live[2] = {bool(valid & (alpha_2 != T(0))), bool(valid & (n_lv == 2) & (alpha_1 != T(0)))};
  // (per-level sizes and the view's base pointer are re-read from the LDS table inside the tap loop instead of living in
  // twelve registers per lane)
  if (threadIdx.x < kMaxLevels) s_ptr[threadIdx.x] = static_cast<const T*>(s_ptr[threadIdx.x]) + n * s_sn[threadIdx.x];
  __syncthreads();
  const int ld[2] = {live[0] ? t.d1 : 0, live[1] ? t.d1 + 1 : 0};
  const double du_d = t.du, dv_d = t.dv;
  const int n_max = wave_max_i32(valid ? t.n : 0);
  const bool table = max_aniso <= kTapTab; // kernel-uniform: the taps' positions come from the LDS table
  const int tab_row = (max(t.n, 1) - 1) * kTapTab;
  T* out_px = out + n * C * HW + pix;

  for (int c0 = 0; c0 < C; c0 += CB) {
    T acc[CB];
#pragma unroll
    for (int cc = 0; cc < CB; ++cc) acc[cc] = T(0);
    for (int i = 0; i < n_max; ++i) {
      const bool has_tap = i < t.n;
      // tap i of t.n: f = (i + 1.0) / (n + 1.0) * 2.0 - 1.0 (:497-499); a lane that has no tap i reads its last one
      // (its weights are zeroed below)
      const int ic = min(i, max(t.n, 1) - 1);
      const double f = table ? s_f[tab_row + ic] : (ic + 1.0) / (t.n + 1.0) * 2.0 - 1.0;
      const T x = t.u + static_cast<T>(du_d * f), y = t.v + static_cast<T>(dv_d * f);
      const bool ordered = (x == x) & (y == y); // a NaN coordinate samples nothing (safe_downgrade_to_int_range: -100)
#pragma unroll
      for (int s = 0; s < 2; ++s) {
        const bool on = has_tap & live[s];
        if (__ballot(on) == 0) continue; // wave-uniform
        int lw[2], lh[2];
        T lwf[2], lhf[2];
        GlobalPtr<const T> lbase[2];
        lw[s] = s_w[ld[s]], lh[s] = s_h[ld[s]];
        lwf[s] = static_cast<T>(lw[s]), lhf[s] = static_cast<T>(lh[s]);
        lbase[s] = (GlobalPtr<const T>)static_cast<const T*>(s_ptr[ld[s]]);
        // the reference's coordinate pipeline for an INTERIOR tap: unnormalize, clip (border padding), floor.  Values are
        // made finite first (a clamp that cannot move a tap whose cell lies inside the level), so that the weights of the
        // lanes that do not count -- no tap, a tap on or beyond the border, a NaN -- are finite and their products with
        // alpha = 0 vanish; those lanes' real contribution, if any, comes from the branch below.
        T ix = ((x + T(1)) * lwf[s] - 1) / 2, iy = ((y + T(1)) * lhf[s] - 1) / 2;
        bool sane = true; // (reflection: a coordinate the short pipeline must not touch goes to the corner-by-corner branch)
        if (padding == 1) {
          ix = tmin(tmax(ix, T(0)), lwf[s] - T(1)), iy = tmin(tmax(iy, T(0)), lhf[s] - T(1)); // == clip_coord but NaN -> 0
        } else if (padding == 2) {
          sane = (tabs(ix) < T(1e9f)) & (tabs(iy) < T(1e9f)); // (false for NaN)
          T unused_x = T(1), unused_y = T(1);
          reflect_clip_lean<T>(sane ? ix : T(0), sane ? iy : T(0), lw[s], lh[s], align_corners, ix, iy, unused_x, unused_y);
        } else {
          ix = tmin(tmax(ix, T(-4)), T(2e9f)), iy = tmin(tmax(iy, T(-4)), T(2e9f));
        }
        const T fx_floor = floor(ix), fy_floor = floor(iy);
        const int ix_nw = static_cast<int>(fx_floor), iy_nw = static_cast<int>(fy_floor);
        const bool interior = on & ordered & sane & (static_cast<unsigned>(ix_nw) < static_cast<unsigned>(lw[s] - 1)) &
            (static_cast<unsigned>(iy_nw) < static_cast<unsigned>(lh[s] - 1));
        // corner weights (bilinear_quad: (ix_se - ix) with ix_se = ix_nw + 1, an exact float) times the level's weight
        const T wx1 = (fx_floor + T(1)) - ix, wx0 = ix - fx_floor;
        const int plane = lw[s] * lh[s]; // <= kMaxPlane32 (the dispatch): cc * plane + offset fits 32 bits
        const GlobalPtr<const T> b = lbase[s] + int64_t(c0) * plane;
        // Round 6: the tap's loads and fmas run under `interior` -- ONE exec-mask region per (tap, level).  Round 5 let the
        // other lanes (no tap i, a border tap, a NaN coordinate, a dead level) run the same loads at offset 0 with weight 0:
        // that read texels (0,0) / (1,0) of the level for pixels that never sample them -- a NaN or Inf there turned
        // `texel * 0` into NaN where the reference stays finite -- and on a 1 x 1 level the pair at offset 0 of the last
        // channel of the last view ended one element beyond the tensor.  The lanes that are switched off touch nothing now.
        if (interior) {
          const T al = s == 0 ? alpha_2 : alpha_1;
          const T wy1 = ((fy_floor + T(1)) - iy) * al, wy0 = (iy - fy_floor) * al;
          const T w_nw = wx1 * wy1, w_ne = wx0 * wy1, w_sw = wx1 * wy0, w_se = wx0 * wy0;
          const int o_top = iy_nw * lw[s] + ix_nw;
          const int o_bot = o_top + lw[s];
          Pair<T> top[CB], bot[CB];
#pragma unroll
          for (int cc = 0; cc < CB; ++cc) {
            top[cc] = *(GlobalPtr<const Pair<T>>)(b + (cc * plane + o_top));
            bot[cc] = *(GlobalPtr<const Pair<T>>)(b + (cc * plane + o_bot));
          }
#pragma unroll
          for (int cc = 0; cc < CB; ++cc) {
            acc[cc] = tfma(top[cc].x, w_nw, acc[cc]);
            acc[cc] = tfma(top[cc].y, w_ne, acc[cc]);
            acc[cc] = tfma(bot[cc].x, w_sw, acc[cc]);
            acc[cc] = tfma(bot[cc].y, w_se, acc[cc]);
          }
        }
        if (__ballot(on & !interior) != 0) {
          // a tap on the border of its level (or a non-finite coordinate) somewhere in the wave: those lanes alone, corner by
          // corner (the reference's form)
          if (on & !interior) {
            const Quad<T> q = bilinear_quad<T>(x, y, lh[s], lw[s], padding, align_corners);
            const T aq = s == 0 ? alpha_2 : alpha_1;
#pragma unroll
            for (int cc = 0; cc < CB; ++cc) {
              const GlobalPtr<const T> pch = b + cc * plane; // (cc <= 3, plane <= kMaxPlane32)
              if (q.o_nw >= 0) acc[cc] += pch[q.o_nw] * q.nw * aq;
              if (q.o_ne >= 0) acc[cc] += pch[q.o_ne] * q.ne * aq;
              if (q.o_sw >= 0) acc[cc] += pch[q.o_sw] * q.sw * aq;
              if (q.o_se >= 0) acc[cc] += pch[q.o_se] * q.se * aq;
            }
          }
        }
      }
    }
    if (valid) {
#pragma unroll
      for (int cc = 0; cc < CB; ++cc) out_px[int64_t(c0 + cc) * HW] = acc[cc];
    }
  }
}

// ---- Backward, direct: one thread per pixel, every corner a global atomic; any size, any number of views (sampler_route) ----
template <typename T, int MODE>
__global__ __launch_bounds__(kBlock) void mipmap_backward_kernel(
    LevelTable lv, int mipmaps, const T* __restrict__ grad_out, const T* __restrict__ grid, GridLayout gl,
    const T* __restrict__ vt, int64_t count, int C, int64_t HW, int max_aniso, int padding, bool align_corners,
    bool force_max_aniso, bool clip_grad, T* __restrict__ grad_grid, GridLayout ggl, int strip) {
  __shared__ const void* s_ptr[kMaxLevels];
  __shared__ void* s_grad[kMaxLevels];
  __shared__ int s_h[kMaxLevels], s_w[kMaxLevels];
  __shared__ long long s_sn[kMaxLevels];
  stage_levels(lv, mipmaps, s_ptr, s_grad, s_h, s_w, s_sn);
  const int64_t index = int64_t(tile_index(strip)) * kBlock + threadIdx.x;
  if (index >= count) return;
  const int64_t n = index / HW;
  const Taps<T> t = setup_taps<T>(load_pixel_uv<T>(grid, gl, vt, n, index - n * HW, index), s_h[0], s_w[0], mipmaps, max_aniso, force_max_aniso, clip_grad);
  const int n_lv = mipmaps > 1 ? 2 : 1;
  const T* gout_px = grad_out + n * C * HW + (index - n * HW);
  const T alpha_1 = t.a / t.n;
  const T alpha_2 = static_cast<T>((1.0 - t.a) / t.n);
  T acc_x = T(0), acc_y = T(0);
  for (int i = 0; i < t.n; ++i) {
    const double f = (i + 1.0) / (t.n + 1.0) * 2.0 - 1.0;
    const T x = t.u + static_cast<T>(t.du * f), y = t.v + static_cast<T>(t.dv * f);
    for (int s = 0; s < n_lv; ++s) {
      const int d = t.d1 + s;
      const int h = s_h[d], w = s_w[d];
      const int64_t plane = int64_t(h) * w;
      const GlobalPtr<const T> inp = (GlobalPtr<const T>)(static_cast<const T*>(s_ptr[d]) + n * s_sn[d]);
      const GlobalPtr<T> ginp = (GlobalPtr<T>)(static_cast<T*>(s_grad[d]) + n * C * plane);
      const T alpha = s == 0 ? alpha_2 : alpha_1;
      T gix = T(0), giy = T(0);
      if constexpr (MODE == 0) {
        const Quad<T> q = bilinear_quad<T>(x, y, h, w, padding, align_corners);
        const int ix_se = q.ix_nw + 1, iy_se = q.iy_nw + 1;
        for (int c = 0; c < C; ++c) {
          const GlobalPtr<const T> p = inp + c * plane;
          const GlobalPtr<T> gp = ginp + c * plane;
          const T gOut = gout_px[int64_t(c) * HW] * alpha;
          // a zero upstream gradient (masked background) adds nothing: skip its four atomics
          if (gOut != T(0)) {
            if (q.o_nw >= 0) atomic_add_g1(gp + q.o_nw, q.nw * gOut);
            if (q.o_ne >= 0) atomic_add_g1(gp + q.o_ne, q.ne * gOut);
            if (q.o_sw >= 0) atomic_add_g1(gp + q.o_sw, q.sw * gOut);
            if (q.o_se >= 0) atomic_add_g1(gp + q.o_se, q.se * gOut);
          }
          // texel values for the grid gradient: the two texels of a row in one 8-byte load when both exist
          T v_nw = T(0), v_ne = T(0), v_sw = T(0), v_se = T(0);
          if (gOut != T(0)) { // with a zero upstream gradient every term below is +-0 * finite
            if (q.o_nw >= 0 && q.o_ne >= 0) {
              const Pair<T> t2 = *(GlobalPtr<const Pair<T>>)(p + q.o_nw);
              v_nw = t2.x, v_ne = t2.y;
            } else {
              if (q.o_nw >= 0) v_nw = p[q.o_nw];
              if (q.o_ne >= 0) v_ne = p[q.o_ne];
            }
            if (q.o_sw >= 0 && q.o_se >= 0) {
              const Pair<T> t2 = *(GlobalPtr<const Pair<T>>)(p + q.o_sw);
              v_sw = t2.x, v_se = t2.y;
            } else {
              if (q.o_sw >= 0) v_sw = p[q.o_sw];
              if (q.o_se >= 0) v_se = p[q.o_se];
            }
          }
          if (q.o_nw >= 0) {
            gix -= v_nw * (iy_se - q.iy) * gOut;
            giy -= v_nw * (ix_se - q.ix) * gOut;
          }
          if (q.o_ne >= 0) {
            gix += v_ne * (iy_se - q.iy) * gOut;
            giy -= v_ne * (q.ix - q.ix_nw) * gOut;
          }
          if (q.o_sw >= 0) {
            gix -= v_sw * (q.iy - q.iy_nw) * gOut;
            giy += v_sw * (ix_se - q.ix) * gOut;
          }
          if (q.o_se >= 0) {
            gix += v_se * (q.iy - q.iy_nw) * gOut;
            giy += v_se * (q.ix - q.ix_nw) * gOut;
          }
        }
        acc_x += q.mx * gix;
        acc_y += q.my * giy;
      } else {
        const Cubic<T> cb = bicubic_footprint<T>(x, y, h, w, padding, align_corners);
        T xc[4], yc[4], xg[4], yg[4];
        cubic_coeffs(xc, cb.tx);
        cubic_coeffs(yc, cb.ty);
        cubic_coeffs_grad(xg, cb.tx);
        cubic_coeffs_grad(yg, cb.ty);
        for (int c = 0; c < C; ++c) {
          const GlobalPtr<const T> p = inp + c * plane;
          const GlobalPtr<T> gp = ginp + c * plane;
          const T gOut = gout_px[int64_t(c) * HW] * alpha;
#pragma unroll
          for (int i2 = 0; i2 < 4; ++i2) {
#pragma unroll
            for (int j2 = 0; j2 < 4; ++j2) {
              const bool ok = cb.xi[i2] >= 0 && cb.yi[j2] >= 0;
              const int o = ok ? cb.yi[j2] * w + cb.xi[i2] : 0;
              if (ok && gOut != T(0)) atomic_add_g1(gp + o, gOut * xc[i2] * yc[j2]);
              const T val = ok ? p[o] : T(0);
              gix -= gOut * val * (xg[i2] * yc[j2]);
              giy -= gOut * val * (yg[j2] * xc[i2]);
            }
          }
        }
        acc_x += cb.mx * gix;
        acc_y += cb.my * giy;
      }
    }
  }
  store_grid_grad<T>(grad_grid, ggl, n, index - n * HW, acc_x, acc_y);
}

// ---- Backward, bilinear, any padding, any C, float and double: the LEAN tile kernel --------------------------------------
// The direct kernel above is bound by the float-atomic REQUEST rate (~20 G/s): every (tap, level, corner, channel) is one
// atomic instruction touching ~5 64-byte segments.  Here a workgroup owns a 16 x 16 PIXEL tile, whose taps land in a compact
// texel window on the two mip levels its pixels select; the windows (kWinLevels shaped slots, double accumulators) are
// accumulated in LDS and flushed once, row-major, so the global atomics are coalesced and each touched texel costs one
// request per tile instead of one per tap.  Taps the windows did not hold stay pending and get the windows in a further round
// (up to kLeanRounds); what is pending after the last one goes to global memory corner by corner, so any uv field
// is handled.
//   * the level tables, the placement cells and the windows' zero-fill are issued UNDER the loads of the upstream gradient /
//     uv / Jacobian, in front of the first barrier;
//   * reference level and window origins come out of ONE phase: every wave reduces the extremes of its taps per ABSOLUTE
//     level into s_lox / s_loy / s_hiy[d]; after one barrier the origins are read into scalar registers;
//   * taps of a pixel that land in the same 2 x 2 cell are merged in registers before they touch LDS;
//   * the flush reads only the window rows a round can have written;
//   * the tap loop is written the way the lean forward is (one straight line per (tap, level) for the whole wave: no Quad, no
//     per-corner logic, regrouped products, texture channels a template parameter) -- for the instructions, and for the
//     registers: at <= 96 a CU holds five tiles.
// Sums regrouped, never dropped: same results to rounding (fixtures, known answers, fuzz_mipmap, fuzz_mipmap_snapped).
// PAD / ALIGN: padding mode and align_corners as compile-time constants (the coordinate pipeline of every tap branches on
// them).  Wider textures (C > 4: neural textures) run the kernel once per block of four channels (`C_total`, `c0`; the grid
// gradient accumulates over the blocks, the tap geometry is recomputed per block).
// Why the sizes below are what they are: profiles/NOTES.md R13, Lore.
constexpr int kTileW = 16;
constexpr int kTileH = 16; // pixel tile: kTileW x kTileH pixels, one thread each
constexpr int kMipBlock = kTileW * kTileH;
constexpr int kWinLevels = 2; // window slots: the tile's finest live level and the next one
constexpr int kLeanRounds = 32; // rounds a tile's windows are placed at most, the first pass included
constexpr int kLeanHopelessPairs = 16; // a further round that catches fewer (tap, level) pairs than this is the tile's last but one
// Window accumulators per channel and slot (two slots; one slot of twice the size where a tile has one live level), by the
// channels of a pass: sized so that the windows of five tiles fit a CU's LDS.
constexpr int kSlotCells12 = 768; // one or two channels: 12-24 KB of windows
constexpr int kSlotCells3 = 512;  // three channels: 24.5 KB
constexpr int kSlotCells4 = 384;  // four channels: 24.6 KB
template <int CN>
constexpr int lean_slot_cells() { return CN == 4 ? kSlotCells4 : CN == 3 ? kSlotCells3 : kSlotCells12; }
static_assert(kSlotCells3 % 128 == 0 && kSlotCells4 % 128 == 0 && kSlotCells12 % 128 == 0, "whole rows at every slot width (16 ... 128 cells), cells in pairs");
// Tiles per CU (= waves per SIMD) the kernel is compiled for: five for float (94-96 registers, at any channel count of a pass);
// four under reflection padding (the reflect + clip of both axes takes it 2-4 registers over the 96; the windows keep the
// five-tile size); three for double (126-152 registers; asked for four it spills 4-17).
template <typename T, int PAD, int CN>
constexpr int lean_backward_tiles_per_cu() { return sizeof(T) == 8 ? 3 : PAD == 2 ? 4 : 5; }
template <typename T, int PAD, bool ALIGN, int CN>
__global__ __launch_bounds__(kMipBlock, (lean_backward_tiles_per_cu<T, PAD, CN>())) void mipmap_backward_lean_kernel(
    LevelTable lv, int mipmaps, const T* __restrict__ grad_out, const T* __restrict__ grid, GridLayout gl,
    const T* __restrict__ vt, int H, int W, int tiles_x, int max_aniso,
    bool force_max_aniso, bool clip_grad, T* __restrict__ grad_grid, GridLayout ggl, int strip, int dbg, int C_total, int c0) {
  static_assert(PAD >= 0 && PAD <= 2, "zeros, border or reflection padding");
  static_assert(CN >= 1 && CN <= 4, "texture channels");
  constexpr int C = CN;
  constexpr int padding = PAD;
  constexpr bool align_corners = ALIGN;
  __shared__ double s_f[kTapTab * kTapTab];
  __shared__ const void* s_ptr[kMaxLevels];
  __shared__ void* s_grad[kMaxLevels];
  __shared__ int s_h[kMaxLevels], s_w[kMaxLevels];
  __shared__ long long s_sn[kMaxLevels];
  __shared__ int s_ref, s_npend, s_ox[kWinLevels], s_oy[kWinLevels], s_hx[kWinLevels], s_hy[kWinLevels];
  // rounds: the lowest pending (tap, level) bit of the tile (two cells, by round parity), and the placement by THAT tap alone
  __shared__ int s_bit[2], s_refb, s_bx[kWinLevels], s_by[kWinLevels], s_bhx[kWinLevels], s_bhy[kWinLevels];
  __shared__ unsigned long long s_seed[kWinLevels];
  // first-round placement per ABSOLUTE level (so that the reference level and the origins come out of ONE phase):
  // bounding box of the north-west texels of the tile's taps on level d
  __shared__ int s_lox[kMaxLevels + 1], s_loy[kMaxLevels + 1], s_hix[kMaxLevels + 1], s_hiy[kMaxLevels + 1];
  extern __shared__ __attribute__((aligned(16))) unsigned char s_win_raw[];
  double* const s_win = reinterpret_cast<double*>(s_win_raw);
  const int tid = threadIdx.x;
  const int n = blockIdx.y;
  // The tile rows of the launch's LAST view are dispatched from the outside in (0, last, 1, last - 1, ...).  A tile's life varies
  // 20x, and tiles that are dispatched last and live longest are a tail every other CU waits for.  Silhouettes and grazing
  // angles, the expensive tiles, lie around an object; background and the magnified interior are cheap: the interior goes last.
  const int tile_disp = tile_index(strip);
  DRTK_MIP_TILE_T0();
  const int ty_disp = tile_disp / tiles_x, tx = tile_disp - ty_disp * tiles_x;
  const int tiles_y = (H + kTileH - 1) / kTileH;
  int ty = ty_disp;
  if (blockIdx.y + 1 == gridDim.y) {
    ty = (ty_disp & 1) ? tiles_y - 1 - (ty_disp >> 1) : (ty_disp >> 1);
  }
  const int tile = ty * tiles_x + tx;
  (void)tile;
  const int px = tx * kTileW + (tid & (kTileW - 1)), py = ty * kTileH + tid / kTileW;
  const bool valid = px < W && py < H;
  const int64_t HW = int64_t(H) * W;
  const int64_t index = int64_t(n) * HW + int64_t(py) * W + px;
  // the pixel's upstream gradient, uv and Jacobian: one batch of loads ...
  T go[CN];
#pragma unroll
  for (int c = 0; c < CN; ++c) go[c] = T(0);
  if (valid) {
    const T* gout_px = grad_out + (int64_t(n) * C_total + c0) * HW + (int64_t(py) * W + px);
#pragma unroll
    for (int c = 0; c < CN; ++c) go[c] = gout_px[int64_t(c) * HW];
  }
  PixelUV<T> uv = {};
  // (the pixel's index is rebuilt where it is needed -- here, at an early exit, after the tap loop -- from a laundered thread id:
  // carried through the kernel its two registers are the ones that spill at five waves per SIMD)
  auto pixel_index = [&]() -> int64_t {
    int tid_l = tid;
    asm volatile("" : "+v"(tid_l));
    return int64_t(ty * kTileH + tid_l / kTileW) * W + (tx * kTileW + (tid_l & (kTileW - 1)));
  };
  if (valid) uv = load_pixel_uv<T>(grid, gl, vt, n, int64_t(py) * W + px, index);
  // ... and under them everything that needs no data: the tables, the placement cells, the windows' zero-fill (a tile
  // that turns out to have no upstream gradient has zeroed its windows for nothing; the stores wait for nobody)
  stage_tap_table(s_f);
  if (tid < kMaxLevels) {
    const int i = tid < mipmaps ? tid : 0;
    s_ptr[tid] = lv.ptr[i], s_grad[tid] = lv.grad[i], s_sn[tid] = lv.sn[i], s_h[tid] = lv.h[i], s_w[tid] = lv.w[i];
  }
  if (tid <= kMaxLevels) s_lox[tid] = s_loy[tid] = INT32_MAX, s_hix[tid] = s_hiy[tid] = INT32_MIN;
  if (tid == 0) s_ref = kMaxLevels, s_bit[0] = s_bit[1] = 32;
  {
    double2* w2 = reinterpret_cast<double2*>(s_win);
    const double2 z = {0.0, 0.0};
    for (int i = tid; i < C * (kWinLevels * lean_slot_cells<CN>()) / 2; i += kMipBlock) w2[i] = z;
  }
  bool has_go = false;
#pragma unroll
  for (int c = 0; c < CN; ++c) has_go = has_go | (go[c] != T(0));
  if (!__syncthreads_or(has_go)) { // (also publishes the tables and the zero-fill)
    if (valid && c0 == 0) store_grid_grad<T>(grad_grid, ggl, n, pixel_index(), T(0), T(0)); // (a later channel block adds nothing)
    return;
  }
  DRTK_MIP_TILE_PHASE(0);

  Taps<T> t = {};
  if (has_go) t = setup_taps<T>(uv, lv.h[0], lv.w[0], mipmaps, max_aniso, force_max_aniso, clip_grad);
  const int n_lv = mipmaps > 1 ? 2 : 1;
  // the levels' weights a / n and (1 - a) / n: continuous quantities, in float from one reciprocal (as in the lean forward)
  const T rn = T(1) / static_cast<T>(max(t.n, 1));
  const T alpha_1 = has_go ? t.a * rn : T(0);
  const T alpha_2 = has_go ? (T(1) - t.a) * rn : T(0);
  // A (pixel, level) whose weighted upstream gradient is zero in every channel adds nothing anywhere (every term is
  // +-0 * finite): the masked background of a silhouette tile, and the second level of a magnified pixel (a == 0).
  // Such pairs neither place the windows nor run their taps.
  bool live[2];
#pragma unroll
  for (int s = 0; s < 2; ++s) {
    const T alpha = s == 0 ? alpha_2 : alpha_1;
    live[s] = false;
#pragma unroll
    for (int c = 0; c < CN; ++c) live[s] = live[s] || (go[c] * alpha != T(0));
    live[s] = live[s] && s < n_lv;
  }
  auto tap_xy = [&](int i, T& x, T& y) {
    const double f = tap_f(s_f, i, t.n);
    x = t.u + static_cast<T>(t.du * f);
    y = t.v + static_cast<T>(t.dv * f);
  };
  // window origins: the taps of a pixel are collinear, so their extreme texels are those of the first and the last
  // tap.  ANY origin is correct -- a corner is windowed iff its exact cell lies inside, tested below -- so the origin
  // comes from a short form of the coordinate pipeline: unnormalise, clamp to the level, floor (the exact north-west
  // texel for zeros / border padding; under reflection padding taps beyond the border miss the window).
  auto texel_floor = [&](T coord, int size) -> int {
    T unused;
    const T c = unnormalize(coord, size, align_corners, &unused);
    const T lo = padding == 0 ? T(-1) : T(0);
    return static_cast<int>(floor(fmin(fmax(c, lo), static_cast<T>(size - 1)))); // fmax(NaN, lo) = lo
  };
  {
    // ONE phase for the reference level and the origins: the extremes go into cells of their ABSOLUTE level, wave by
    // wave over the (one to three) levels a wave's pixels use
    int lo_x[2] = {INT32_MAX, INT32_MAX}, lo_y[2] = {INT32_MAX, INT32_MAX}, hi_x[2] = {INT32_MIN, INT32_MIN}, hi_y[2] = {INT32_MIN, INT32_MIN};
    if (live[0] || live[1]) {
      for (int e = 0; e < 2; ++e) {
        T x, y;
        tap_xy(e == 0 ? 0 : t.n - 1, x, y);
#pragma unroll
        for (int s = 0; s < 2; ++s) {
          if (s < n_lv && live[s]) {
            const int ox = texel_floor(x, s_w[t.d1 + s]), oy = texel_floor(y, s_h[t.d1 + s]);
            lo_x[s] = min(lo_x[s], ox), lo_y[s] = min(lo_y[s], oy), hi_x[s] = max(hi_x[s], ox), hi_y[s] = max(hi_y[s], oy);
          }
        }
      }
    }
    const int d_lo = wave_min_i32(live[0] ? t.d1 : live[1] ? t.d1 + 1 : kMaxLevels);
    const int d_hi = wave_max_i32(live[1] ? t.d1 + 1 : live[0] ? t.d1 : -1);
    for (int d = d_lo; d <= d_hi; ++d) { // wave-uniform
      const bool m0 = live[0] && t.d1 == d, m1 = live[1] && t.d1 + 1 == d;
      const int a = wave_min_i32(min(m0 ? lo_x[0] : INT32_MAX, m1 ? lo_x[1] : INT32_MAX));
      const int b = wave_min_i32(min(m0 ? lo_y[0] : INT32_MAX, m1 ? lo_y[1] : INT32_MAX));
      const int e = wave_max_i32(max(m0 ? hi_y[0] : INT32_MIN, m1 ? hi_y[1] : INT32_MIN));
      const int g = wave_max_i32(max(m0 ? hi_x[0] : INT32_MIN, m1 ? hi_x[1] : INT32_MIN));
      if ((tid & (kWave - 1)) == 0 && a != INT32_MAX) {
        atomicMin(&s_lox[d], a);
        atomicMin(&s_loy[d], b);
        atomicMax(&s_hix[d], g);
        atomicMax(&s_hiy[d], e);
      }
    }
    if ((tid & (kWave - 1)) == 0 && d_lo < kMaxLevels) atomicMin(&s_ref, d_lo);
  }
  __syncthreads();
  DRTK_MIP_TILE_PHASE(1);
  const int ref = s_ref;
  // ---- the two window SLOTS (round 5: shaped, not square).  Slot l holds level ref + l.  The windows' memory is
  // kWinLevels x kWinSlotCells accumulators per channel; a tile with no live tap on level ref + 1 -- every tile of a magnified
  // texture -- gives it all to slot 0; a slot is 2^sx cells wide, sx chosen by the bounding box of the taps it has to
  // hold (16 ... 128 wide: the elongated footprints of a limb tile fit where a 32 x 32 square needed four rounds).
  // Wave-uniform values: scalar registers.
  constexpr int kWinSlotCells = lean_slot_cells<CN>();
  int wox[kWinLevels], woy[kWinLevels], wsx[kWinLevels], wny[kWinLevels], wcells[kWinLevels], win_rows[kWinLevels];
  auto shape_slots = [&](const int (&lox)[kWinLevels], const int (&loy)[kWinLevels], const int (&hix)[kWinLevels], const int (&hiy)[kWinLevels], bool all_rows) {
    const bool two = lox[1] != INT32_MAX;
#pragma unroll
    for (int l = 0; l < kWinLevels; ++l) {
      wox[l] = lox[l], woy[l] = loy[l];
      wcells[l] = l == 0 ? (two ? kWinSlotCells : kWinLevels * kWinSlotCells) : (two ? kWinSlotCells : 0);
      const long long need_w = static_cast<long long>(hix[l]) - lox[l] + 2, need_h = static_cast<long long>(hiy[l]) - loy[l] + 2;
      int sx = need_w <= 16 ? 4 : need_w <= 32 ? 5 : (need_w <= 64 && need_h <= (wcells[l] >> 6)) ? 6 : (need_w > 64 && need_h <= (wcells[l] >> 7)) ? 7 : 5;
      if (lox[l] == INT32_MAX) sx = 5;
      wsx[l] = sx;
      wny[l] = wcells[l] > 0 ? (wcells[l] >> sx) : 1; // (1: no cell passes the row test of an empty slot)
      win_rows[l] = (all_rows || need_h > wny[l]) ? wny[l] : static_cast<int>(need_h < 0 ? 0 : need_h);
      if (wcells[l] == 0) win_rows[l] = 0;
    }
  };
  {
    int lox[kWinLevels], loy[kWinLevels], hix[kWinLevels], hiy[kWinLevels];
#pragma unroll
    for (int l = 0; l < kWinLevels; ++l) {
      const int d = min(ref + l, kMaxLevels);
      lox[l] = __builtin_amdgcn_readfirstlane(s_lox[d]), loy[l] = __builtin_amdgcn_readfirstlane(s_loy[d]);
      hix[l] = __builtin_amdgcn_readfirstlane(s_hix[d]), hiy[l] = __builtin_amdgcn_readfirstlane(s_hiy[d]);
    }
    // rows the first round can touch: exact for zeros / border padding, where the extremes are the true north-west texels;
    // under reflection padding every row
    shape_slots(lox, loy, hix, hiy, padding == 2);
  }
  // cell of a north-west texel in slot l (the other three corners are +1, +stride, +stride+1), or -1
  auto slot_cell = [&](int l, int ix_nw, int iy_nw) -> int {
    if (l < 0 || l >= kWinLevels) return -1;
    const int wx = ix_nw - (l == 0 ? wox[0] : wox[1]), wy = iy_nw - (l == 0 ? woy[0] : woy[1]);
    // (rows: those the flush walks -- the bounding box the slot was shaped for, where that is less than the slot)
    const int sx = l == 0 ? wsx[0] : wsx[1], ny = l == 0 ? win_rows[0] : win_rows[1];
    return (static_cast<unsigned>(wx) < (1u << sx) - 1u && wy >= 0 && wy < ny - 1) ? (wy << sx) + wx : -1;
  };
  auto slot_stride = [&](int l) -> int { return 1 << (l == 0 ? wsx[0] : wsx[1]); };
  auto slot_chan = [&](int l) -> int { return l == 0 ? wcells[0] : wcells[1]; };  // cells per channel
  auto slot_base = [&](int l) -> int { return l == 0 ? 0 : C * wcells[0]; };        // first cell of the slot's channel 0

  // (tap, level) pairs that find no window cell in this round: not sent to global memory one corner and channel at a
  // time -- scattered float atomics of single lanes, costly although only a few per cent of the taps miss -- but
  // remembered (per level of the pixel: did any tap miss, and where) for a further round with the windows moved onto
  // them (below, up to kLeanRounds rounds).
  // (where they missed is NOT carried through the tap loop -- six registers at its bound: a round recomputes the
  // north-west texels of its pending taps, which it walks anyway)
  uint32_t pending = 0; // bit 2 i + s: tap i on the pixel's level s found no window cell yet (taps >= 16 are never deferred)

  // ---- the tap loop, lean (see mipmap_forward_lean_kernel): ONE straight line per (tap, level) for the whole wave.  Cell
  // decisions are the reference's operations in the reference's order; the continuous quantities are regrouped (corner
  // weights as products of the two axis weights, the grid gradient as differences of texels: 10 operations per channel
  // instead of 24).  A lane whose tap is not interior runs the same loads and products with offset 0 and weight 0; border
  // taps and the (rare) taps beyond the deferral range are added by a branch the wave only takes if it has one.
  T acc_x = T(0), acc_y = T(0);
  {
    const int n_max = wave_max_i32((live[0] || live[1]) ? t.n : 0);
    const bool table = max_aniso <= kTapTab; // kernel-uniform
    const int tn1 = max(t.n, 1);
    const double du_d = t.du, dv_d = t.dv;
    auto grad_base = [&](int d, int64_t plane) -> GlobalPtr<T> { return (GlobalPtr<T>)(static_cast<T*>(s_grad[d]) + (int64_t(n) * C_total + c0) * plane); };
    // (one run slot, for the pixel's FINER level: a magnified pixel has no other live level, and the taps of a minified
    // one are a texel apart on the finer level -- half a texel on the coarser, whose adds go to LDS tap by tap)
    int run_cell = -1;
    T run_w[4] = {T(0), T(0), T(0), T(0)};
    auto emit_run = [&](int l, const T (&g)[CN]) {
      if (run_cell < 0) return;
      double* wp = s_win + slot_base(l) + run_cell;
      const int stride = slot_stride(l), chan = slot_chan(l);
#pragma unroll
      for (int c = 0; c < CN; ++c) {
        lds_add(wp + c * chan, static_cast<double>(run_w[0] * g[c]));
        lds_add(wp + c * chan + 1, static_cast<double>(run_w[1] * g[c]));
        lds_add(wp + c * chan + stride, static_cast<double>(run_w[2] * g[c]));
        lds_add(wp + c * chan + stride + 1, static_cast<double>(run_w[3] * g[c]));
      }
      run_cell = -1;
    };
    for (int i = 0; i < n_max && !DRTK_DBG(dbg, 32); ++i) {
      const bool has_tap = i < t.n;
      const int ic = min(i, tn1 - 1); // a lane that has no tap i recomputes its last one (its weights are zeroed)
      const double f = table ? s_f[(tn1 - 1) * kTapTab + ic] : (ic + 1.0) / (t.n + 1.0) * 2.0 - 1.0;
      const T x = t.u + static_cast<T>(du_d * f), y = t.v + static_cast<T>(dv_d * f);
      const bool ordered = (x == x) & (y == y); // a NaN coordinate samples nothing (safe_downgrade_to_int_range: -100)
#pragma unroll
      for (int s = 0; s < 2; ++s) {
        const bool on = has_tap & live[s];
        if (__ballot(on) == 0) continue; // wave-uniform
        const int d = on ? t.d1 + s : 0;
        const int w = s_w[d], h = s_h[d];
        const T wm1 = static_cast<T>(w - 1), hm1 = static_cast<T>(h - 1);
        // unnormalize (GridSampler.cuh): the position and the gradient multiplier of the coordinate transform
        T ixu, iyu, mx, my;
        if (align_corners) {
          ixu = ((x + 1.f) / 2) * wm1, iyu = ((y + 1.f) / 2) * hm1;
          mx = wm1 / 2, my = hm1 / 2;
        } else {
          ixu = ((x + 1.f) * static_cast<T>(w) - 1) / 2, iyu = ((y + 1.f) * static_cast<T>(h) - 1) / 2;
          mx = static_cast<T>(w) / 2, my = static_cast<T>(h) / 2;
        }
        T ix, iy;
        bool sane = true; // (reflection: a coordinate the short pipeline must not touch goes to the corner-by-corner branch)
        if (padding == 1) { // clip_coord: clamped coordinates have a zero gradient
          mx = ((ixu > T(0)) & (ixu < wm1)) ? mx : T(0), my = ((iyu > T(0)) & (iyu < hm1)) ? my : T(0);
          ix = tmin(tmax(ixu, T(0)), wm1), iy = tmin(tmax(iyu, T(0)), hm1);
        } else if (padding == 2) { // reflect_coord, then clip_coord (source_index's order)
          sane = (tabs(ixu) < T(1e9f)) & (tabs(iyu) < T(1e9f));
          reflect_clip_lean<T>(sane ? ixu : T(0), sane ? iyu : T(0), w, h, align_corners, ix, iy, mx, my);
        } else { // (made finite; a tap whose cell lies inside the level is not moved)
          ix = tmin(tmax(ixu, T(-4)), T(2e9f)), iy = tmin(tmax(iyu, T(-4)), T(2e9f));
        }
        const T fx_floor = floor(ix), fy_floor = floor(iy);
        const int ix_nw = static_cast<int>(fx_floor), iy_nw = static_cast<int>(fy_floor);
        const bool interior = on & ordered & sane & (static_cast<unsigned>(ix_nw) < static_cast<unsigned>(w - 1)) &
            (static_cast<unsigned>(iy_nw) < static_cast<unsigned>(h - 1));
        const T wx1 = (fx_floor + T(1)) - ix, wx0 = ix - fx_floor, wy1 = (fy_floor + T(1)) - iy, wy0 = iy - fy_floor;
        const int l = d - ref;
        const int cell = interior ? slot_cell(l, ix_nw, iy_nw) : -1;
        const T al = interior ? (s == 0 ? alpha_2 : alpha_1) : T(0);
        T g[CN];
#pragma unroll
        for (int c = 0; c < CN; ++c) g[c] = go[c] * al;
        // ---- texture gradient: into the window (merged per cell on the finer level), or pending
        if (!DRTK_DBG(dbg, 1)) {
          if (cell >= 0) {
            const T q_nw = wx1 * wy1, q_ne = wx0 * wy1, q_sw = wx1 * wy0, q_se = wx0 * wy0;
            if (s == 1) {
              double* wp = s_win + slot_base(l) + cell;
              const int stride = slot_stride(l), chan = slot_chan(l);
#pragma unroll
              for (int c = 0; c < CN; ++c) {
                lds_add(wp + c * chan, static_cast<double>(q_nw * g[c]));
                lds_add(wp + c * chan + 1, static_cast<double>(q_ne * g[c]));
                lds_add(wp + c * chan + stride, static_cast<double>(q_sw * g[c]));
                lds_add(wp + c * chan + stride + 1, static_cast<double>(q_se * g[c]));
              }
            } else if (cell != run_cell) {
              emit_run(l, g);
              run_cell = cell;
              run_w[0] = q_nw, run_w[1] = q_ne, run_w[2] = q_sw, run_w[3] = q_se;
            } else {
              run_w[0] += q_nw, run_w[1] += q_ne, run_w[2] += q_sw, run_w[3] += q_se;
            }
          } else if (interior & (i < 16)) {
            pending |= 1u << (2 * i + s);
          }
        }
        // ---- grid gradient: texels of the (interior) tap; d/dx of the bilinear form = differences of texels
        const int plane = w * h; // <= kMaxPlane32 (the dispatch): c * plane + offset fits 32 bits
        const GlobalPtr<const T> inp = (GlobalPtr<const T>)(static_cast<const T*>(s_ptr[d]) + int64_t(n) * s_sn[d]) + int64_t(c0) * plane;
        // (round 6: the loads run under `interior`, one exec-mask region -- the lanes without an interior tap used to load the
        // pair at offset 0 of their level: on a 1 x 1 level, one element beyond the last channel of the last view.  What
        // their registers hold instead is never used: g[c] is zero on those lanes)
        const int o_top = iy_nw * w + ix_nw;
        const int o_bot = o_top + w;
        Pair<T> top[CN], bot[CN];
#pragma unroll
        for (int c = 0; c < CN; ++c) {
          top[c] = __builtin_nondeterministic_value(top[c]);
          bot[c] = __builtin_nondeterministic_value(bot[c]);
        }
        if (interior && !DRTK_DBG(dbg, 2)) {
#pragma unroll
          for (int c = 0; c < CN; ++c) {
            top[c] = *(GlobalPtr<const Pair<T>>)(inp + (c * plane + o_top));
            bot[c] = *(GlobalPtr<const Pair<T>>)(inp + (c * plane + o_bot));
          }
        }
        T gix = T(0), giy = T(0);
#pragma unroll
        for (int c = 0; c < CN; ++c) {
          if (DRTK_DBG(dbg, 16)) break;
          // (with a zero upstream gradient every term is +-0 * finite in the reference: the texels count as 0)
          const T tx = (top[c].y - top[c].x) * wy1 + (bot[c].y - bot[c].x) * wy0;
          const T ty = (bot[c].x - top[c].x) * wx1 + (bot[c].y - top[c].y) * wx0;
          gix += g[c] != T(0) ? g[c] * tx : T(0);
          giy += g[c] != T(0) ? g[c] * ty : T(0);
        }
        acc_x += mx * gix;
        acc_y += my * giy;
        // ---- the lanes the straight line does not serve: a tap on the border of its level (or with a non-finite coordinate),
        // and interior taps beyond the deferral range that found no window (texture gradient straight to global memory)
        const bool slow = on & (!interior | ((cell < 0) & (i >= 16)));
        if (__ballot(slow) != 0) {
          if (slow) {
            const T alpha = s == 0 ? alpha_2 : alpha_1;
            const Quad<T> q = bilinear_quad<T>(x, y, h, w, padding, align_corners);
            const int ix_se = q.ix_nw + 1, iy_se = q.iy_nw + 1;
            const int qcell = slot_cell(l, q.ix_nw, q.iy_nw);
            const int stride = slot_stride(l), chan = slot_chan(l);
            const bool defer = !interior && !DRTK_DBG(dbg, 1) && qcell < 0 && i < 16 && (q.o_nw & q.o_ne & q.o_sw & q.o_se) != -1; // (all four corners outside the level: nothing to add anywhere)
            if (defer) pending |= 1u << (2 * i + s);
            T sgx = T(0), sgy = T(0);
#pragma unroll 1
            for (int c = 0; c < CN; ++c) {
              const T gOut = (c == 0 ? go[0] : c == 1 ? go[CN > 1 ? 1 : 0] : c == 2 ? go[CN > 2 ? 2 : 0] : go[CN > 3 ? 3 : 0]) * alpha;
              if (gOut == T(0)) continue; // a zero upstream gradient (masked channel) adds nothing; its texels count as 0
              if (!DRTK_DBG(dbg, 1)) {
                if (qcell >= 0 && !interior) {
                  double* wp = s_win + slot_base(l) + c * chan + qcell;
                  if (q.o_nw >= 0) lds_add(wp, static_cast<double>(q.nw * gOut));
                  if (q.o_ne >= 0) lds_add(wp + 1, static_cast<double>(q.ne * gOut));
                  if (q.o_sw >= 0) lds_add(wp + stride, static_cast<double>(q.sw * gOut));
                  if (q.o_se >= 0) lds_add(wp + stride + 1, static_cast<double>(q.se * gOut));
                } else if (!defer) {
                  const GlobalPtr<T> gp = grad_base(d, plane) + c * plane;
                  if (q.o_nw >= 0) atomic_add_g1(gp + q.o_nw, q.nw * gOut);
                  if (q.o_ne >= 0) atomic_add_g1(gp + q.o_ne, q.ne * gOut);
                  if (q.o_sw >= 0) atomic_add_g1(gp + q.o_sw, q.sw * gOut);
                  if (q.o_se >= 0) atomic_add_g1(gp + q.o_se, q.se * gOut);
                }
              }
              if (interior) continue; // (its grid gradient is in the straight line above)
              const GlobalPtr<const T> pch = inp + c * plane; // (c <= 3, plane <= kMaxPlane32)
              T v_nw = T(0), v_ne = T(0), v_sw = T(0), v_se = T(0);
              if (!DRTK_DBG(dbg, 2)) {
                if (q.o_nw >= 0) v_nw = pch[q.o_nw];
                if (q.o_ne >= 0) v_ne = pch[q.o_ne];
                if (q.o_sw >= 0) v_sw = pch[q.o_sw];
                if (q.o_se >= 0) v_se = pch[q.o_se];
              }
              if (q.o_nw >= 0) {
                sgx -= v_nw * (iy_se - q.iy) * gOut;
                sgy -= v_nw * (ix_se - q.ix) * gOut;
              }
              if (q.o_ne >= 0) {
                sgx += v_ne * (iy_se - q.iy) * gOut;
                sgy -= v_ne * (q.ix - q.ix_nw) * gOut;
              }
              if (q.o_sw >= 0) {
                sgx -= v_sw * (q.iy - q.iy_nw) * gOut;
                sgy += v_sw * (ix_se - q.ix) * gOut;
              }
              if (q.o_se >= 0) {
                sgx += v_se * (q.iy - q.iy_nw) * gOut;
                sgy += v_se * (q.ix - q.ix_nw) * gOut;
              }
            }
            acc_x += q.mx * sgx;
            acc_y += q.my * sgy;
          }
        }
      }
    }
    // the last run
    if (live[0]) {
      T g[CN];
#pragma unroll
      for (int c = 0; c < CN; ++c) g[c] = go[c] * alpha_2;
      emit_run(t.d1 - ref, g);
    }
  }
  if (valid) {
    const int64_t pix = pixel_index();
    if (c0 != 0) { // a further block of channels of a wide texture: the grid gradient accumulates (one thread per pixel, launches in stream order)
      const T* gq = grad_grid + int64_t(n) * ggl.sN + pix * ggl.sP;
      acc_x += gq[0], acc_y += gq[ggl.sC];
    }
    store_grid_grad<T>(grad_grid, ggl, n, pix, acc_x, acc_y);
    DRTK_MIP_STAT(8, (live[0] ? t.n : 0) + (live[1] ? t.n : 0));
    DRTK_MIP_STAT(9, __popc(pending));
  }
  if (tid == 0) DRTK_MIP_STAT(0, 1);
  __syncthreads();
  DRTK_MIP_TILE_PHASE(2);
  // flush the windows: consecutive threads = consecutive texels of a row; cells that stayed 0 cost nothing,
  // cells outside the level were never written (only in-bounds corners are accumulated).  With `rearm` the cells are
  // zeroed as they are read: the windows serve a second round.
  auto flush = [&](int ref_level, bool rearm) {
#pragma unroll
    for (int l = 0; l < kWinLevels; ++l) {
      const int d = ref_level + l;
      if (d >= mipmaps || wox[l] == INT32_MAX || DRTK_DBG(dbg, 4)) continue;
      const int h = s_h[d], w = s_w[d];
      const int64_t plane = int64_t(h) * w;
      const GlobalPtr<T> ginp = (GlobalPtr<T>)(static_cast<T*>(s_grad[d]) + (int64_t(n) * C_total + c0) * plane);
      for (int c = 0; c < C; ++c) {
        const int stride = 1 << wsx[l], chan = wcells[l];
        // ONE cell per lane: the lanes of an atomic instruction are consecutive texels of a row, so a row's adds travel as
        // one request per 64-byte line -- with two cells per lane (one 16-byte LDS read, round 4) every line was asked for
        // twice, by the even and by the odd texels' instruction: 10.2 M of the kernel's 16.4 M atomic requests on the
        // textured benchmark were this flush (TCP_TCC_ATOMIC_WITHOUT_RET_REQ), at what a request costs at the memory side.
        double* win1 = s_win + (l == 0 ? 0 : C * wcells[0]) + c * chan;
        for (int i = tid; i < win_rows[l] * stride; i += kMipBlock) { // rows beyond win_rows were never written
          const double q = win1[i];
          if (q != 0.0) {
            if (rearm) win1[i] = 0.0;
            const int gx = wox[l] + (i & (stride - 1)), gy = woy[l] + (i >> wsx[l]);
            atomic_add_g1(ginp + c * plane + int64_t(gy) * w + gx, static_cast<T>(q));
          }
        }
      }
    }
  };
  // Does any pixel of the tile have taps the windows did not hold?  (16 % of the tiles of the minified benchmark scenes;
  // on the textured benchmark the atlas seam and the limb of the sphere, where a pixel spreads eight anisotropic taps on
  // two levels over thousands of texels.)  `pending` says which.
  // ---- further rounds: the windows are moved onto taps that are still pending and those taps alone are accumulated
  // (texture gradient only: the grid gradient is complete).  Where the windows go: onto everything pending if that fits
  // (A), else onto ONE tap of the tile's pixels (B) -- see the placement below.  What is still pending after the last
  // round goes to global memory corner by corner, as all misses did before round 3.
  // A round that catches fewer than kLeanHopelessPairs pairs makes the next one the tile's last: its taps are
  // scattered beyond what windows hold (random uv), and a round costs what some tens of pairs' atomics do.
  // the lean form of a tap's cell and axis weights on a level of (h, w) texels -- the operations of the first pass's straight
  // line; returns whether the tap is interior (all four corners inside the level: nearly every pending tap; the others go
  // through bilinear_quad below)
  auto lean_tap = [&](T x, T y, int w, int h, int& ix_nw, int& iy_nw, T& wx0, T& wx1, T& wy0, T& wy1) -> bool {
    const T wm1 = static_cast<T>(w - 1), hm1 = static_cast<T>(h - 1);
    T ixu, iyu;
    if (align_corners) {
      ixu = ((x + 1.f) / 2) * wm1, iyu = ((y + 1.f) / 2) * hm1;
    } else {
      ixu = ((x + 1.f) * static_cast<T>(w) - 1) / 2, iyu = ((y + 1.f) * static_cast<T>(h) - 1) / 2;
    }
    T ix, iy;
    bool sane = true;
    if (padding == 1) {
      ix = tmin(tmax(ixu, T(0)), wm1), iy = tmin(tmax(iyu, T(0)), hm1);
    } else if (padding == 2) {
      sane = (tabs(ixu) < T(1e9f)) & (tabs(iyu) < T(1e9f));
      T unused_x = T(1), unused_y = T(1);
      reflect_clip_lean<T>(sane ? ixu : T(0), sane ? iyu : T(0), w, h, align_corners, ix, iy, unused_x, unused_y);
    } else {
      ix = tmin(tmax(ixu, T(-4)), T(2e9f)), iy = tmin(tmax(iyu, T(-4)), T(2e9f));
    }
    const T fx_floor = floor(ix), fy_floor = floor(iy);
    ix_nw = static_cast<int>(fx_floor), iy_nw = static_cast<int>(fy_floor);
    wx1 = (fx_floor + T(1)) - ix, wx0 = ix - fx_floor, wy1 = (fy_floor + T(1)) - iy, wy0 = iy - fy_floor;
    return sane & ((x == x) & (y == y)) & (static_cast<unsigned>(ix_nw) < static_cast<unsigned>(w - 1)) & (static_cast<unsigned>(iy_nw) < static_cast<unsigned>(h - 1));
  };
  // how many taps away from one of its taps a pixel can have another one inside the same window (<= 128 cells wide and
  // high): the taps are equally spaced, 2 / (n + 1) of (du, dv) apart -- on the coarser of the pixel's levels half as many
  // texels as on the finer.  A filter for the rounds below, not a decision: a tap it wrongly leaves out stays pending.
  // (evaluated where a round needs it: a register less across the tap loop)
  auto tap_span = [&]() -> int {
    const T step = T(2) / static_cast<T>(t.n + 1);
    const T sp = tmax(tabs(static_cast<T>(t.du)) * static_cast<T>(s_w[t.d1]), tabs(static_cast<T>(t.dv)) * static_cast<T>(s_h[t.d1])) * step * T(0.5);
    return static_cast<int>(tmin(T(16), T(258) / tmax(sp, T(1)))) + 1;
  };
  int ref_now = ref, npend_before = 0;
  for (int round = 1;; ++round) {
    {
      const int wb = wave_min_i32(pending ? __builtin_ctz(pending) : 32);
      if ((tid & (kWave - 1)) == 0 && wb < 32) atomicMin(&s_bit[round & 1], wb);
    }
    const bool again = __syncthreads_or(pending != 0) && !DRTK_DBG(dbg, 8);
    flush(ref_now, again);
    if (!again) {
      DRTK_MIP_TILE_DONE(round - 1);
      return;
    }
    if (tid == 0) DRTK_MIP_STAT(round < 7 ? round : 7, 1);
    bool last = round >= kLeanRounds - 1; // (or hopeless, below)
    const int i_star = s_bit[round & 1] >> 1; // the tile's first pending tap
    __syncthreads(); // everybody has finished its flush (it reads the origins)
    if (tid == 0) s_ref = s_refb = kMaxLevels, s_npend = 0, s_bit[(round + 1) & 1] = 32;
    if (tid < kWinLevels) {
      s_ox[tid] = s_oy[tid] = s_bx[tid] = s_by[tid] = INT32_MAX, s_hx[tid] = s_hy[tid] = s_bhx[tid] = s_bhy[tid] = INT32_MIN;
      s_seed[tid] = ~0ull;
    }
    // where this pixel's pending taps are: bounding box of their north-west texels per level (A: all of them), and
    // where its tap i_star is, if pending (B)
    bool miss[2] = {false, false}, star[2] = {false, false};
    int miss_x[2] = {INT32_MAX, INT32_MAX}, miss_y[2] = {INT32_MAX, INT32_MAX}, miss_hx[2] = {INT32_MIN, INT32_MIN}, miss_hy[2] = {INT32_MIN, INT32_MIN};
    int star_x[2] = {0, 0}, star_y[2] = {0, 0};
    // (the taps of a pixel are collinear and ordered: the extremes of its pending taps on a level are the first and the last)
#pragma unroll
    for (int s2 = 0; s2 < 2; ++s2) {
      const uint32_t m = pending & (0x55555555u << s2);
      if (m == 0) continue;
      const int i_lo = __builtin_ctz(m) >> 1, i_hi = (31 - __builtin_clz(m)) >> 1;
      const bool star_pending = ((m >> (2 * i_star + s2)) & 1u) != 0;
      const int d = t.d1 + s2;
      const int w = s_w[d], h = s_h[d];
      miss[s2] = true;
      for (int e = 0; e < 3; ++e) {
        const int i = e == 0 ? i_lo : e == 1 ? i_hi : i_star;
        if ((e == 1 && i_hi == i_lo) || (e == 2 && (!star_pending || i_star == i_lo || i_star == i_hi))) continue;
        T x, y;
        tap_xy(i, x, y);
        int qx, qy; // (of a tap on the border of its level: its clamped position -- any origin is correct)
        T u0, u1, u2, u3;
        lean_tap(x, y, w, h, qx, qy, u0, u1, u2, u3);
        if (e < 2) {
          miss_x[s2] = min(miss_x[s2], qx), miss_y[s2] = min(miss_y[s2], qy);
          miss_hx[s2] = max(miss_hx[s2], qx), miss_hy[s2] = max(miss_hy[s2], qy);
        }
        if (i == i_star) star[s2] = true, star_x[s2] = qx, star_y[s2] = qy;
      }
    }
    __syncthreads();
    {
      const int d_min = wave_min_i32(miss[0] ? t.d1 : miss[1] ? t.d1 + 1 : kMaxLevels);
      const int d_minb = wave_min_i32(star[0] ? t.d1 : star[1] ? t.d1 + 1 : kMaxLevels);
      // the tile's pending (tap, level) pairs: a wave's count from five ballots over the bits of its lanes' counts (<= 32)
      const int pc = __popc(pending);
      int wave_pc = 0;
#pragma unroll
      for (int b = 0; b < 6; ++b) wave_pc += __popcll(__ballot((pc >> b) & 1)) << b;
      if ((tid & (kWave - 1)) == 0) {
        atomicMin(&s_ref, d_min);
        atomicMin(&s_refb, d_minb);
        atomicAdd(&s_npend, wave_pc);
      }
    }
    __syncthreads();
    const int ref_a = s_ref, ref_b = s_refb;
    {
      // HOPELESS: the round before this one caught fewer than kLeanHopelessPairs pairs -- scattered taps; this round is the last
      const int npend = s_npend;
      const bool hopeless = round >= 2 && npend_before - npend < kLeanHopelessPairs;
      if (tid == 0 && hopeless) DRTK_MIP_STAT(11, 1);
      npend_before = npend;
      last = last || hopeless;
    }
    {
      int lo_x[kWinLevels], lo_y[kWinLevels], hi_x[kWinLevels], hi_y[kWinLevels];
      int b_x[kWinLevels], b_y[kWinLevels], b_hx[kWinLevels], b_hy[kWinLevels];
      unsigned long long seed[kWinLevels];
#pragma unroll
      for (int l = 0; l < kWinLevels; ++l) lo_x[l] = lo_y[l] = b_x[l] = b_y[l] = INT32_MAX, hi_x[l] = hi_y[l] = b_hx[l] = b_hy[l] = INT32_MIN, seed[l] = ~0ull;
#pragma unroll
      for (int s2 = 0; s2 < 2; ++s2) {
        const int la = t.d1 + s2 - ref_a, lb = t.d1 + s2 - ref_b;
#pragma unroll
        for (int k = 0; k < kWinLevels; ++k) {
          if (miss[s2] && k == la) {
            lo_x[k] = min(lo_x[k], miss_x[s2]), lo_y[k] = min(lo_y[k], miss_y[s2]);
            hi_x[k] = max(hi_x[k], miss_hx[s2]), hi_y[k] = max(hi_y[k], miss_hy[s2]);
          }
          if (star[s2] && k == lb) {
            b_x[k] = b_hx[k] = star_x[s2], b_y[k] = b_hy[k] = star_y[s2];
            seed[k] = static_cast<unsigned long long>(static_cast<unsigned>(star_y[s2] + 1)) << 32 | static_cast<unsigned>(star_x[s2] + 1);
          }
        }
      }
#pragma unroll
      for (int l = 0; l < kWinLevels; ++l) {
        const int a = wave_min_i32(lo_x[l]), b = wave_min_i32(lo_y[l]);
        const int g = wave_max_i32(hi_x[l]), e = wave_max_i32(hi_y[l]);
        if ((tid & (kWave - 1)) == 0 && a != INT32_MAX) {
          atomicMin(&s_ox[l], a);
          atomicMin(&s_oy[l], b);
          atomicMax(&s_hx[l], g);
          atomicMax(&s_hy[l], e);
        }
        if (__ballot(b_x[l] != INT32_MAX) != 0) { // (wave-uniform)
          const int ba = wave_min_i32(b_x[l]), bb = wave_min_i32(b_y[l]);
          const int bg = wave_max_i32(b_hx[l]), be = wave_max_i32(b_hy[l]);
          if ((tid & (kWave - 1)) == 0) {
            atomicMin(&s_bx[l], ba);
            atomicMin(&s_by[l], bb);
            atomicMax(&s_bhx[l], bg);
            atomicMax(&s_bhy[l], be);
          }
          // the seed: the topmost (then leftmost) of the candidates -- a window that starts on its row and is centred on its
          // column holds at least this tap, whatever the shape of the rest
          if (b_y[l] == bb && b_x[l] != INT32_MAX) atomicMin(&s_seed[l], seed[l]);
        }
      }
    }
    __syncthreads();
    bool fits;
    {
      int lox[kWinLevels], loy[kWinLevels], hix[kWinLevels], hiy[kWinLevels];
#pragma unroll
      for (int l = 0; l < kWinLevels; ++l) {
        lox[l] = __builtin_amdgcn_readfirstlane(s_ox[l]), loy[l] = __builtin_amdgcn_readfirstlane(s_oy[l]);
        hix[l] = __builtin_amdgcn_readfirstlane(s_hx[l]), hiy[l] = __builtin_amdgcn_readfirstlane(s_hy[l]);
      }
      // A: do ALL pending taps of the two finest pending levels fit the slots?  Then the windows take them (the usual case:
      // a tile whose taps overflowed the first windows a little).  Otherwise B: the windows go onto ONE tap of the tile's
      // pixels, the first that is pending anywhere (and its two finest levels).  The pixels of a tile are neighbours, so their
      // taps number i are too, however far the taps of one pixel lie apart -- the limb of the textured benchmark: tiles
      // whose pixels spread eight taps on two levels over thousands of texels; the bounding box of everything pending
      // is then the whole texture, and a window in its corner holds nothing.
      fits = true;
      {
        const bool two = lox[1] != INT32_MAX;
#pragma unroll
        for (int l = 0; l < kWinLevels; ++l) {
          if (lox[l] == INT32_MAX) continue;
          const int cells = two ? kWinSlotCells : kWinLevels * kWinSlotCells;
          const long long need_w = static_cast<long long>(hix[l]) - lox[l] + 2, need_h = static_cast<long long>(hiy[l]) - loy[l] + 2;
          const int sx = need_w <= 16 ? 4 : need_w <= 32 ? 5 : need_w <= 64 ? 6 : 7;
          fits = fits && need_w <= 128 && need_h <= (cells >> sx);
        }
      }
      ref_now = ref_a;
      if (!fits) {
        ref_now = ref_b;
#pragma unroll
        for (int l = 0; l < kWinLevels; ++l) {
          lox[l] = __builtin_amdgcn_readfirstlane(s_bx[l]), loy[l] = __builtin_amdgcn_readfirstlane(s_by[l]);
          hix[l] = __builtin_amdgcn_readfirstlane(s_bhx[l]), hiy[l] = __builtin_amdgcn_readfirstlane(s_bhy[l]);
        }
      }
      // a window whose slot has no pending tap on level ref_now must still exist as slot 0: ref_now IS a level with pending taps
      shape_slots(lox, loy, hix, hiy, false); // (rows: the bounding box's -- slot_cell() admits no others -- so the flush walks no more)
      if (!fits) {
#pragma unroll
        for (int l = 0; l < kWinLevels; ++l) {
          if (lox[l] == INT32_MAX) continue;
          const int width = 1 << wsx[l];
          if (static_cast<long long>(hix[l]) - lox[l] + 2 > width) { // wider than the slot: centred on the seed's column
            const unsigned long long sd = s_seed[l];
            const int seed_x = __builtin_amdgcn_readfirstlane(static_cast<int>(static_cast<unsigned>(sd))) - 1;
            wox[l] = max(lox[l], seed_x - (width / 2 - 1));
          }
        }
      }
    }
    if (pending != 0) {
      uint32_t todo = pending;
      if (!fits && !last) {
        // windows placed by tap i_star: a pixel whose own tap i_star is inside them walks its taps within k_span of it only
        bool star_in = false;
#pragma unroll
        for (int s2 = 0; s2 < 2; ++s2) star_in = star_in || (star[s2] && slot_cell(t.d1 + s2 - ref_now, star_x[s2], star_y[s2]) >= 0);
        if (star_in) {
          const int k_span = tap_span();
          const int b_lo = 2 * max(i_star - k_span, 0), b_hi = 2 * min(i_star + k_span, 15) + 1;
          todo &= (0xFFFFFFFFu << b_lo) & (0xFFFFFFFFu >> (31 - b_hi));
        }
      }
      while (todo) {
        const int bit = __builtin_ctz(todo);
        todo &= todo - 1;
        const int i = bit >> 1, s2 = bit & 1;
        T x, y;
        tap_xy(i, x, y);
        const int d = t.d1 + s2;
        const int h = s_h[d], w = s_w[d];
        const int64_t plane = int64_t(h) * w;
        const T alpha = s2 == 0 ? alpha_2 : alpha_1;
        const int l = d - ref_now;
        {
          int ix_nw, iy_nw;
          T wx0, wx1, wy0, wy1;
          if (lean_tap(x, y, w, h, ix_nw, iy_nw, wx0, wx1, wy0, wy1)) {
            const int cell = slot_cell(l, ix_nw, iy_nw);
            if (cell < 0 && !last) continue; // stays pending: the next round's windows
            pending &= ~(1u << bit);
            if (cell < 0) DRTK_MIP_STAT(10, 1);
            if (cell < 0) DRTK_MIP_STAT(12 + min(max(d - ref, 0), 3), 1);
            if (cell < 0) DRTK_MIP_DUMP(static_cast<unsigned>(n) << 24 | static_cast<unsigned>(tile), static_cast<unsigned>(tid) << 16 | static_cast<unsigned>(d), static_cast<unsigned>(ix_nw), static_cast<unsigned>(iy_nw));
            if (cell < 0 && DRTK_DBG(dbg, 256)) continue; // (ablation: what the left-over global atomics cost)
            const T q_nw = wx1 * wy1, q_ne = wx0 * wy1, q_sw = wx1 * wy0, q_se = wx0 * wy0;
            if (cell >= 0) {
              double* wp = s_win + slot_base(l) + cell;
              const int stride = slot_stride(l), chan = slot_chan(l);
#pragma unroll
              for (int c = 0; c < CN; ++c) {
                const T gc = go[c] * alpha;
                lds_add(wp + c * chan, static_cast<double>(q_nw * gc));
                lds_add(wp + c * chan + 1, static_cast<double>(q_ne * gc));
                lds_add(wp + c * chan + stride, static_cast<double>(q_sw * gc));
                lds_add(wp + c * chan + stride + 1, static_cast<double>(q_se * gc));
              }
            } else {
              const GlobalPtr<T> gp = (GlobalPtr<T>)(static_cast<T*>(s_grad[d]) + (int64_t(n) * C_total + c0) * plane) + (int64_t(iy_nw) * w + ix_nw);
#pragma unroll
              for (int c = 0; c < CN; ++c) {
                const T gc = go[c] * alpha;
                if (gc == T(0)) continue;
                atomic_add_g1(gp + c * plane, q_nw * gc);
                atomic_add_g1(gp + c * plane + 1, q_ne * gc);
                atomic_add_g1(gp + c * plane + w, q_sw * gc);
                atomic_add_g1(gp + c * plane + w + 1, q_se * gc);
              }
            }
            continue;
          }
        }
        const Quad<T> q = bilinear_quad<T>(x, y, h, w, padding, align_corners); // (a deferred tap on the border of its level: rare)
        const int cell = slot_cell(l, q.ix_nw, q.iy_nw);
        const int stride = slot_stride(l), chan = slot_chan(l);
        if (cell < 0 && !last) continue; // stays pending: the next round's windows
        pending &= ~(1u << bit);
        if (cell < 0) DRTK_MIP_STAT(10, 1);
        if (cell < 0) DRTK_MIP_STAT(12 + min(max(d - ref, 0), 3), 1);
        if (cell < 0) DRTK_MIP_DUMP(static_cast<unsigned>(n) << 24 | static_cast<unsigned>(tile), static_cast<unsigned>(tid) << 16 | static_cast<unsigned>(d), static_cast<unsigned>(q.ix_nw), static_cast<unsigned>(q.iy_nw));
        if (cell < 0 && DRTK_DBG(dbg, 256)) continue; // (ablation: what the left-over global atomics cost)
        const GlobalPtr<T> ginp = (GlobalPtr<T>)(static_cast<T*>(s_grad[d]) + (int64_t(n) * C_total + c0) * plane);
#pragma unroll
        for (int c = 0; c < CN; ++c) {
          const T gc = go[c] * alpha;
          if (gc == T(0)) continue;
          if (cell >= 0) {
            double* wp = s_win + slot_base(l) + c * chan + cell;
            if (q.o_nw >= 0) lds_add(wp, static_cast<double>(q.nw * gc));
            if (q.o_ne >= 0) lds_add(wp + 1, static_cast<double>(q.ne * gc));
            if (q.o_sw >= 0) lds_add(wp + stride, static_cast<double>(q.sw * gc));
            if (q.o_se >= 0) lds_add(wp + stride + 1, static_cast<double>(q.se * gc));
          } else {
            const GlobalPtr<T> gp = ginp + c * plane;
            if (q.o_nw >= 0) atomic_add_g1(gp + q.o_nw, q.nw * gc);
            if (q.o_ne >= 0) atomic_add_g1(gp + q.o_ne, q.ne * gc);
            if (q.o_sw >= 0) atomic_add_g1(gp + q.o_sw, q.sw * gc);
            if (q.o_se >= 0) atomic_add_g1(gp + q.o_se, q.se * gc);
          }
        }
      }
    }
  }
}

// ---- Backward, bicubic, any C, float and double: WAVE-PRIVATE 4 x 4 windows ------------------------------------------------
// A WAVE owns its 16 x 4 pixels of the tile and a window of its own (mipmap_grid_sampler_kernel.cu:806-861 is the footprint):
//   * no workgroup barrier after the level table is staged: placement, taps, flush and the further rounds of a wave are
//     ordered by the wave's own LDS counter, so 20+ independent waves per CU overlap each other's round trips;
//   * kWaveCells cells per channel (double accumulators, ds_add_f64) shaped like the bounding box of the wave's taps --
//     2 KB per channel and wave; channels go in blocks of four, so any C runs here (the level pair, tap geometry and grid
//     gradient of a pixel are per block; the reference's sums regrouped);
//   * per-level sizes and pointers are re-read from the LDS table inside the tap loop instead of being carried in
//     registers; a tap spans four cells per axis; interior footprints (sixteen consecutive texels inside the level) are
//     windowed, the others go corner by corner straight to global memory.
// Taps that find no cell stay pending and get the window in a further round (up to kWaveRounds), as in the lean tile kernel.
constexpr int kWaveCells = 256; // window cells per channel and wave, both levels together
constexpr int kWaveWinW = 32;   // widest window row (the flush walks two rows of <= 32 cells per step)
constexpr int kWaveRounds = 6;  // rounds a wave's window is placed at most, the first pass included
// waves per SIMD the kernel is compiled for: float fits three with the compact border path (168 registers)
template <typename T>
constexpr int wave_backward_waves_per_simd() { return sizeof(T) == 8 ? 1 : 3; }
template <typename T, int PAD, bool ALIGN>
__global__ __launch_bounds__(kMipBlock, wave_backward_waves_per_simd<T>()) void mipmap_backward_wave_kernel(
    LevelTable lv, int mipmaps, const T* __restrict__ grad_out, const T* __restrict__ grid, GridLayout gl,
    const T* __restrict__ vt, int H, int W, int C, int tiles_x, int max_aniso,
    bool force_max_aniso, bool clip_grad, T* __restrict__ grad_grid, GridLayout ggl, int strip, int dbg) {
  constexpr int padding = PAD;
  constexpr bool align_corners = ALIGN;
  constexpr int kSpan = 4; // cells per tap and axis
  static_assert(kTileW == 16 && kWave == 64, "a wave covers 16 x 4 pixels");
  __shared__ double s_f[kTapTab * kTapTab];
  __shared__ const void* s_ptr[kMaxLevels];
  __shared__ void* s_grad[kMaxLevels];
  __shared__ int s_h[kMaxLevels], s_w[kMaxLevels];
  __shared__ long long s_sn[kMaxLevels];
  extern __shared__ __attribute__((aligned(16))) unsigned char s_win_raw[]; // [wave][channel of the block][kWaveCells] doubles
  const int tid = threadIdx.x;
  const int wave = tid / kWave, lane = tid & (kWave - 1);
  const int CB = C < kChBlock ? C : kChBlock; // channels per block
  double* const win = reinterpret_cast<double*>(s_win_raw) + wave * CB * kWaveCells;
  stage_tap_table(s_f);
  stage_levels(lv, mipmaps, s_ptr, s_grad, s_h, s_w, s_sn); // the kernel's only workgroup barrier
  for (int i = lane; i < CB * kWaveCells; i += kWave) win[i] = 0.0; // every flush leaves the window zeroed again

  const int n = blockIdx.y;
  const int tile = tile_index(strip);
  const int ty = tile / tiles_x, tx = tile - ty * tiles_x;
  const int px = tx * kTileW + (lane & (kTileW - 1)), py = ty * kTileH + wave * (kWave / kTileW) + lane / kTileW;
  const bool valid = px < W && py < H;
  const int64_t HW = int64_t(H) * W;
  const int64_t pix = int64_t(py) * W + px;
  const int64_t index = int64_t(n) * HW + pix;
  PixelUV<T> uv = {};
  if (valid) uv = load_pixel_uv<T>(grid, gl, vt, n, pix, index);
  const int n_lv = mipmaps > 1 ? 2 : 1;
  Taps<T> t = {};
  bool have_taps = false;
  T acc_x = T(0), acc_y = T(0);
  auto tap_xy = [&](int i, T& x, T& y) {
    const double f = tap_f(s_f, i, t.n);
    x = t.u + static_cast<T>(t.du * f);
    y = t.v + static_cast<T>(t.dv * f);
  };
  auto texel_floor = [&](T coord, int size) -> int { // (any origin is correct)
    T unused;
    const T c = unnormalize(coord, size, align_corners, &unused);
    const T lo = padding == 0 ? T(-1) : T(0);
    return static_cast<int>(floor(fmin(fmax(c, lo), static_cast<T>(size - 1)))) - 1;
  };

  for (int c0 = 0; c0 < C; c0 += kChBlock) {
    const int cc = min(kChBlock, C - c0);
    T go[kChBlock] = {T(0), T(0), T(0), T(0)};
    if (valid) {
      const T* gout_px = grad_out + (int64_t(n) * C + c0) * HW + pix;
#pragma unroll
      for (int c = 0; c < kChBlock; ++c) {
        if (c < cc) go[c] = gout_px[int64_t(c) * HW];
      }
    }
    const bool has_go = go[0] != T(0) || go[1] != T(0) || go[2] != T(0) || go[3] != T(0);
    if (__ballot(has_go) == 0) continue; // masked background: nothing to add anywhere, grid gradient +0
    if (has_go && !have_taps) {
      t = setup_taps<T>(uv, s_h[0], s_w[0], mipmaps, max_aniso, force_max_aniso, clip_grad);
      have_taps = true;
    }
    const T alpha_1 = has_go ? t.a / t.n : T(0);
    const T alpha_2 = has_go ? static_cast<T>((1.0 - t.a) / t.n) : T(0);
    bool live[2];
#pragma unroll
    for (int s = 0; s < 2; ++s) {
      const T alpha = s == 0 ? alpha_2 : alpha_1;
      live[s] = false;
#pragma unroll
      for (int c = 0; c < kChBlock; ++c) live[s] = live[s] || (go[c] * alpha != T(0));
      live[s] = live[s] && s < n_lv;
    }
    // ---- window placement: the finest live level of the wave and the next one, each window the bounding box of the
    // north-west texels of the wave's first and last taps (the taps of a pixel are collinear), clipped to its share of
    // the cells.  Wave-uniform values, no LDS.
    int ref, ox[2], oy[2], ww[2], wh[2], base[2];
    auto place = [&](const bool (&on)[2], const int (&lo_x)[2], const int (&lo_y)[2], const int (&hi_x)[2], const int (&hi_y)[2]) {
      // lane values: per level s of the pixel, the extreme north-west texels it needs (on[s]); d = t.d1 + s
      ref = wave_min_i32(on[0] ? t.d1 : on[1] ? t.d1 + 1 : kMaxLevels);
      int x0[2], y0[2], x1[2], y1[2];
#pragma unroll
      for (int l = 0; l < 2; ++l) {
        const bool m0 = on[0] && t.d1 - ref == l, m1 = on[1] && t.d1 + 1 - ref == l;
        const int lx = min(m0 ? lo_x[0] : INT32_MAX, m1 ? lo_x[1] : INT32_MAX), ly = min(m0 ? lo_y[0] : INT32_MAX, m1 ? lo_y[1] : INT32_MAX);
        const int hx = max(m0 ? hi_x[0] : INT32_MIN, m1 ? hi_x[1] : INT32_MIN), hy = max(m0 ? hi_y[0] : INT32_MIN, m1 ? hi_y[1] : INT32_MIN);
        x0[l] = wave_min_i32(lx), y0[l] = wave_min_i32(ly), x1[l] = wave_max_i32(hx), y1[l] = wave_max_i32(hy);
      }
      const bool both = x0[1] != INT32_MAX;
      const int budget[2] = {both ? kWaveCells - kWaveCells / 4 : kWaveCells, kWaveCells / 4};
#pragma unroll
      for (int l = 0; l < 2; ++l) {
        ox[l] = x0[l], oy[l] = y0[l];
        base[l] = l == 0 ? 0 : budget[0];
        if (x0[l] == INT32_MAX) {
          ww[l] = wh[l] = 0;
          continue;
        }
        // + kSpan: the east / south cells of the extreme taps; at most a flush row
        const long long need_w = static_cast<long long>(x1[l]) - x0[l] + kSpan, need_h = static_cast<long long>(y1[l]) - y0[l] + kSpan;
        ww[l] = static_cast<int>(need_w < kWaveWinW ? need_w : kWaveWinW);
        const int rows = budget[l] / ww[l];
        wh[l] = static_cast<int>(need_h < rows ? need_h : rows);
      }
    };
    {
      bool on[2] = {live[0], live[1]};
      int lo_x[2] = {INT32_MAX, INT32_MAX}, lo_y[2] = {INT32_MAX, INT32_MAX}, hi_x[2] = {INT32_MIN, INT32_MIN}, hi_y[2] = {INT32_MIN, INT32_MIN};
      if (live[0] || live[1]) {
        for (int e = 0; e < 2; ++e) {
          T x, y;
          tap_xy(e == 0 ? 0 : t.n - 1, x, y);
#pragma unroll
          for (int s = 0; s < 2; ++s) {
            if (!live[s]) continue;
            const int fx = texel_floor(x, s_w[t.d1 + s]), fy = texel_floor(y, s_h[t.d1 + s]);
            lo_x[s] = min(lo_x[s], fx), lo_y[s] = min(lo_y[s], fy), hi_x[s] = max(hi_x[s], fx), hi_y[s] = max(hi_y[s], fy);
          }
        }
      }
      place(on, lo_x, lo_y, hi_x, hi_y);
    }
    // window cell of a tap's north-west corner on level d (the other three are +1 in x / y), or -1
    auto cell_of = [&](int d, int ix_nw, int iy_nw, int& stride) -> int {
      const int l = d - ref;
      stride = 0;
      if (l < 0 || l > 1) return -1;
      const int wx = ix_nw - ox[l], wy = iy_nw - oy[l];
      stride = ww[l];
      return (wx >= 0 && wx < ww[l] - (kSpan - 1) && wy >= 0 && wy < wh[l] - (kSpan - 1)) ? base[l] + wy * ww[l] + wx : -1;
    };
    // the wave's windows to global memory; every cell is left zero.  Two rows of <= 32 cells per step: lanes of a half
    // wave = consecutive texels of a row, so the atomics of a row form one or two requests.
    auto flush = [&]() {
      wave_lds_sync();
      if (DRTK_DBG(dbg, 4)) return;
#pragma unroll 1
      for (int l = 0; l < 2; ++l) {
        if (ww[l] == 0) continue;
        const int d = ref + l;
        const int w_tex = s_w[d];
        const int64_t plane = int64_t(s_h[d]) * w_tex;
        const GlobalPtr<T> ginp = (GlobalPtr<T>)(static_cast<T*>(s_grad[d]) + (int64_t(n) * C + c0) * plane);
        const int col = lane & (kWaveWinW - 1), half = lane / kWaveWinW;
        for (int r = half; r < wh[l]; r += kWave / kWaveWinW) {
          if (col < ww[l]) {
            double* wp = win + base[l] + r * ww[l] + col;
            const int64_t o = int64_t(oy[l] + r) * w_tex + ox[l] + col;
            for (int c = 0; c < cc; ++c) {
              const double q = wp[c * kWaveCells];
              if (q != 0.0) {
                wp[c * kWaveCells] = 0.0;
                atomic_add_g1(ginp + c * plane + o, static_cast<T>(q));
              }
            }
          }
        }
      }
      wave_lds_sync();
    };

    bool miss[2] = {false, false};
    int miss_x0[2] = {INT32_MAX, INT32_MAX}, miss_y0[2] = {INT32_MAX, INT32_MAX}, miss_x1[2] = {INT32_MIN, INT32_MIN}, miss_y1[2] = {INT32_MIN, INT32_MIN};
    uint32_t pending = 0; // bit 2 i + s: tap i on the pixel's level s found no window cell yet (taps >= 16 are never deferred)
    auto note_miss = [&](int s, int ix_nw, int iy_nw) {
#pragma unroll
      for (int k = 0; k < 2; ++k) {
        if (k == s) {
          miss[k] = true;
          miss_x0[k] = min(miss_x0[k], ix_nw), miss_y0[k] = min(miss_y0[k], iy_nw);
          miss_x1[k] = max(miss_x1[k], ix_nw), miss_y1[k] = max(miss_y1[k], iy_nw);
        }
      }
    };
    wave_lds_sync(); // (the zero-fill before the first block)
    if (live[0] || live[1]) {
      for (int i = 0; i < t.n; ++i) {
        T x, y;
        tap_xy(i, x, y);
#pragma unroll
        for (int s = 0; s < 2; ++s) {
          if (!live[s]) continue;
          const int d = t.d1 + s;
          const int h = s_h[d], w = s_w[d];
          const int plane = h * w; // <= kMaxPlane32 (the dispatch): c * plane + offset fits 32 bits for c <= 3
          const GlobalPtr<const T> inp = (GlobalPtr<const T>)(static_cast<const T*>(s_ptr[d]) + int64_t(n) * s_sn[d]) + int64_t(c0) * plane;
          const T alpha = s == 0 ? alpha_2 : alpha_1;
          const Cubic<T> cb = bicubic_footprint<T>(x, y, h, w, padding, align_corners);
          T xc[4], yc[4], xg[4], yg[4];
          cubic_coeffs(xc, cb.tx);
          cubic_coeffs(yc, cb.ty);
          cubic_coeffs_grad(xg, cb.tx);
          cubic_coeffs_grad(yg, cb.ty);
          const GlobalPtr<T> gp = (GlobalPtr<T>)(static_cast<T*>(s_grad[d]) + (int64_t(n) * C + c0) * plane);
          T gix = T(0), giy = T(0);
          const int bx = cb.xi[0], by = cb.yi[0];
          const bool interior = bx >= 0 && by >= 0 && cb.xi[1] == bx + 1 && cb.xi[2] == bx + 2 && cb.xi[3] == bx + 3 &&
              cb.yi[1] == by + 1 && cb.yi[2] == by + 2 && cb.yi[3] == by + 3;
          int stride = 0;
          const int cell = interior ? cell_of(d, bx, by, stride) : -1;
          const bool defer = interior && cell < 0 && i < 16 && !DRTK_DBG(dbg, 1);
          if (defer) {
            pending |= 1u << (2 * i + s);
            note_miss(s, bx, by);
          }
#pragma unroll 1
          for (int c = 0; c < cc; ++c) {
            const T gOut = go[c] * alpha;
            if (gOut == T(0)) continue; // every term below would be +-0 * finite
            const GlobalPtr<const T> pc = inp + c * plane;
            if (sizeof(T) == 4 && interior && !DRTK_DBG(dbg, 2)) { // (double: 12 registers spilled with the rows in flight)
              // the sixteen texels of an interior footprint as FOUR 16-byte row loads (element-aligned), like the forward --
              // not sixteen predicated 4-byte loads, each in its own exec-mask region with its own wait.  NOT the per-cell
              // paths' products in their order (below; what double and the ablation build take): the weights are regrouped
              // to (gOut yc[j]) xc[i] and the grid gradient to row dot-products, so the results agree with those paths up to
              // float summation order, in the last bits.
              typedef T Quad4 __attribute__((ext_vector_type(4), aligned(sizeof(T))));
              Quad4 row[4];
#pragma unroll
              for (int r = 0; r < 4; ++r) row[r] = *(GlobalPtr<const Quad4>)(pc + (by + r) * w + bx);
              // ... and ROW BY ROW: the footprint's weights are an outer product xc (x) yc, so a row's four cells share
              // gOut yc[j] and the grid gradient is  -gOut sum_j yc[j] (row_j . xg)  /  -gOut sum_j yg[j] (row_j . xc): 8
              // multiply-adds per row instead of six operations per cell with their 48 hoisted coefficient products
              // (the registers that held the kernel at two waves per SIMD)
#pragma unroll
              for (int j2 = 0; j2 < 4; ++j2) {
                const T gy = gOut * yc[j2];
                if (DRTK_DBG(dbg, 1)) {
                } else if (cell >= 0) {
                  double* wp = win + cell + c * kWaveCells + j2 * stride;
#pragma unroll
                  for (int i2 = 0; i2 < 4; ++i2) lds_add(wp + i2, static_cast<double>(gy * xc[i2]));
                } else if (!defer) {
                  const GlobalPtr<T> gq = gp + c * plane + ((by + j2) * w + bx);
#pragma unroll
                  for (int i2 = 0; i2 < 4; ++i2) atomic_add_g1(gq + i2, gy * xc[i2]);
                }
                const T sx = row[j2].x * xg[0] + row[j2].y * xg[1] + row[j2].z * xg[2] + row[j2].w * xg[3];
                const T sc = row[j2].x * xc[0] + row[j2].y * xc[1] + row[j2].z * xc[2] + row[j2].w * xc[3];
                gix -= gy * sx;
                giy -= (gOut * yg[j2]) * sc;
              }
              continue;
            }
            if constexpr (sizeof(T) == 4) {
              // a footprint that touches the border of its level (rare): the sixteen cells in a loop that is NOT unrolled,
              // coefficients and indices picked by selects -- the unrolled form below (sixteen predicated loads and their
              // products in flight) is what kept this kernel at 225-243 registers = two waves per SIMD
              auto sel4 = [](const auto (&a)[4], int k) { return k == 0 ? a[0] : k == 1 ? a[1] : k == 2 ? a[2] : a[3]; };
#pragma unroll 1
              for (int e = 0; e < 16; ++e) {
                const int i2 = e >> 2, j2 = e & 3;
                const int xi = sel4(cb.xi, i2), yi = sel4(cb.yi, j2);
                const bool ok = xi >= 0 && yi >= 0;
                const int o = ok ? yi * w + xi : 0;
                const T cxw = sel4(xc, i2), cyw = sel4(yc, j2);
                const T wgt = gOut * cxw * cyw;
                if (DRTK_DBG(dbg, 1)) {
                } else if (cell >= 0) { // (an interior footprint whose rows were not taken above: the ablation build only)
                  lds_add(win + cell + c * kWaveCells + j2 * stride + i2, static_cast<double>(wgt));
                } else if (ok && !defer) {
                  atomic_add_g1(gp + c * plane + o, wgt);
                }
                const T val = (ok && !DRTK_DBG(dbg, 2)) ? pc[o] : T(0);
                gix -= gOut * val * (sel4(xg, i2) * cyw);
                giy -= gOut * val * (sel4(yg, j2) * cxw);
              }
              continue;
            }
#pragma unroll
            for (int i2 = 0; i2 < 4; ++i2) {
#pragma unroll
              for (int j2 = 0; j2 < 4; ++j2) {
                const bool ok = cb.xi[i2] >= 0 && cb.yi[j2] >= 0;
                const int o = ok ? cb.yi[j2] * w + cb.xi[i2] : 0;
                const T wgt = gOut * xc[i2] * yc[j2];
                if (DRTK_DBG(dbg, 1)) {
                } else if (cell >= 0) {
                  lds_add(win + cell + c * kWaveCells + j2 * stride + i2, static_cast<double>(wgt));
                } else if (ok && !defer) {
                  atomic_add_g1(gp + c * plane + o, wgt);
                }
                const T val = (ok && !DRTK_DBG(dbg, 2)) ? pc[o] : T(0);
                gix -= gOut * val * (xg[i2] * yc[j2]);
                giy -= gOut * val * (yg[j2] * xc[i2]);
              }
            }
          }
          acc_x += cb.mx * gix;
          acc_y += cb.my * giy;
        }
      }
    }
    flush();
    // ---- further rounds: the window moves onto the taps that are still pending (texture gradient only: the grid
    // gradient of the block is complete); what is pending after the last round goes to global memory
    for (int round = 1; __ballot(pending != 0) != 0 && !DRTK_DBG(dbg, 8); ++round) {
      const bool last = round >= kWaveRounds - 1;
      place(miss, miss_x0, miss_y0, miss_x1, miss_y1);
      miss[0] = miss[1] = false;
#pragma unroll
      for (int k = 0; k < 2; ++k) miss_x0[k] = miss_y0[k] = INT32_MAX, miss_x1[k] = miss_y1[k] = INT32_MIN;
      uint32_t todo = pending;
      while (todo) {
        const int bit = __builtin_ctz(todo);
        todo &= todo - 1;
        const int i = bit >> 1, s2 = bit & 1;
        T x, y;
        tap_xy(i, x, y);
        const int d = t.d1 + s2;
        const int h = s_h[d], w = s_w[d];
        const int plane = h * w;
        const T alpha = s2 == 0 ? alpha_2 : alpha_1;
        const Cubic<T> cb = bicubic_footprint<T>(x, y, h, w, padding, align_corners); // (interior: only those are deferred)
        T xc[4], yc[4];
        cubic_coeffs(xc, cb.tx);
        cubic_coeffs(yc, cb.ty);
        const int bx = cb.xi[0], by = cb.yi[0];
        int stride;
        const int cell = cell_of(d, bx, by, stride);
        if (cell < 0 && !last) {
          note_miss(s2, bx, by);
          continue;
        }
        pending &= ~(1u << bit);
        const GlobalPtr<T> gp = (GlobalPtr<T>)(static_cast<T*>(s_grad[d]) + (int64_t(n) * C + c0) * plane);
#pragma unroll 1
        for (int c = 0; c < cc; ++c) {
          const T gOut = go[c] * alpha;
          if (gOut == T(0)) continue;
#pragma unroll
          for (int i2 = 0; i2 < 4; ++i2) {
#pragma unroll
            for (int j2 = 0; j2 < 4; ++j2) {
              const T wgt = gOut * xc[i2] * yc[j2];
              if (cell >= 0) {
                lds_add(win + cell + c * kWaveCells + j2 * stride + i2, static_cast<double>(wgt));
              } else {
                atomic_add_g1(gp + c * plane + (by + j2) * w + bx + i2, wgt);
              }
            }
          }
        }
      }
      flush();
    }
  }
  if (valid) store_grid_grad<T>(grad_grid, ggl, n, pix, acc_x, acc_y);
}

// ---- host side: the argument check, the routing rule, the two entry points ---------------------------------------------------
// The level table of a call (entries beyond `mipmaps` repeat level 0), or what is wrong with it.  `grad_levels`: the backward's
// gradient pyramid (null in the forward); a level of it that has elements must exist.
int fill_table(
    LevelTable& lv, const void* const* levels, void* const* grad_levels, const int64_t* level_h,
    const int64_t* level_w, const int64_t* level_sN, int mipmaps, int64_t N, int64_t C) {
  if (mipmaps < 1 || mipmaps > kMaxLevels || !levels || !level_h || !level_w) return DRTK_ERR_INVALID_ARGUMENT;
  for (int i = 0; i < kMaxLevels; ++i) {
    const int j = i < mipmaps ? i : 0;
    if (level_h[j] <= 0 || level_w[j] <= 0 || level_h[j] * level_w[j] >= (int64_t(1) << 31)) return DRTK_ERR_INVALID_ARGUMENT;
    if (N * C > 0 && (!levels[j] || (grad_levels && !grad_levels[j]))) return DRTK_ERR_INVALID_ARGUMENT;
    lv.ptr[i] = levels[j];
    lv.grad[i] = grad_levels ? grad_levels[j] : nullptr;
    lv.h[i] = static_cast<int>(level_h[j]);
    lv.w[i] = static_cast<int>(level_w[j]);
    lv.sn[i] = level_sN ? level_sN[j] : C * level_h[j] * level_w[j];
    if (lv.sn[i] != 0 && lv.sn[i] < C * level_h[j] * level_w[j]) return DRTK_ERR_INVALID_ARGUMENT; // overlapping views
  }
  return DRTK_OK;
}

// The lean kernels and the wave-private bicubic backward address a texel as `channel_in_block * plane + offset` in 32 bits
// (at most three planes + one): a pyramid with a level beyond this size (a 23 171^2 level) takes the general kernels, whose
// plane offsets are 64-bit.
constexpr int64_t kMaxPlane32 = ((int64_t(1) << 31) - 1) / 4;
bool planes_fit_32bit(const LevelTable& lv, int mipmaps) {
  for (int i = 0; i < mipmaps; ++i) {
    if (int64_t(lv.h[i]) * lv.w[i] > kMaxPlane32) return false;
  }
  return true;
}

// The argument check of both entry points, complete before either writes anything (tests/test_mipmap_args_host.py pins every
// status; tests/test_gpu_mipmap_rejects.py that a rejected backward call has written nothing).  `grad_levels`: null in the
// forward.  `result`: the forward's `out`, the backward's `grad_grid`.  The per-pixel pointers and the grid layouts are judged
// only where there is a pixel to compute -- in the forward that takes a channel, too; the backward stores a grid gradient for
// every pixel, and reads `grad_out` where it has elements.  Fills `lv`, `gl` and (backward) `ggl`.
int check_sampler_args(
    bool backward, drtk_dtype_t dtype, const void* const* levels, void* const* grad_levels, const int64_t* level_h, const int64_t* level_w,
    const int64_t* level_sN, int mipmaps, const void* grid, const int64_t* grid_layout, const void* vt_dxdy_img, int64_t N, int64_t C,
    int64_t H, int64_t W, int max_aniso, int padding_mode, int interpolation_mode, const void* grad_out, const void* result,
    const int64_t* grad_grid_layout, LevelTable& lv, GridLayout& gl, GridLayout& ggl) {
  // (not bad_image(): this check puts no bound on H W)
  if (N < 0 || C < 0 || H < 0 || W < 0 || C >= (1 << 20) || max_aniso < 1 || padding_mode < 0 || padding_mode > 2 ||
      (interpolation_mode != 0 && interpolation_mode != 2) || !valid_dtype(dtype) || (backward && !grad_levels))
    return DRTK_ERR_INVALID_ARGUMENT;
  const int st = fill_table(lv, levels, grad_levels, level_h, level_w, level_sN, mipmaps, N, C);
  if (st != DRTK_OK) return st;
  if (N * H * W == 0 || (!backward && C == 0)) return DRTK_OK;
  if (!grid || !vt_dxdy_img || !result || (backward && C > 0 && !grad_out)) return DRTK_ERR_INVALID_ARGUMENT;
  const size_t es = dtype_size(dtype);
  if (make_grid_layout(gl, grid_layout, grid, H, W, es) != DRTK_OK) return DRTK_ERR_INVALID_ARGUMENT;
  if (backward && make_grid_layout(ggl, grad_grid_layout, result, H, W, es) != DRTK_OK) return DRTK_ERR_INVALID_ARGUMENT;
  return DRTK_OK;
}

// ONE routing rule for both passes (tests/test_gpu_mipmap_routes.py and tests/test_gpu_mipmap.py pin it).  The lean kernels
// (bilinear) and the wave-private bicubic backward -- LDS accumulators in double whatever the element type; float and double
// alike: the reference dispatches both, kernel_utils.h:35-57 -- run only where a view is a grid row of the launch, there is a
// channel and every level fits their 32-bit `c * plane + offset`.  Everything else -- a larger level, more than
// kMaxViewsPerLaunch views, a backward with C = 0 (which only stores a zero grid gradient), `no_windows` (the profiling build's
// flag 512; false in the product and in the forward) -- takes the general forward / the direct backward, whose offsets are 64-bit
// and whose views are a division.  There is no windowed bicubic forward: kWave means the general kernel there.
enum class SamplerRoute { kLean, kWave, kGeneral };
SamplerRoute sampler_route(int interpolation_mode, int64_t N, int64_t C, const LevelTable& lv, int mipmaps, bool no_windows) {
  if (N > kMaxViewsPerLaunch || C < 1 || !planes_fit_32bit(lv, mipmaps) || no_windows) return SamplerRoute::kGeneral;
  return interpolation_mode == 0 ? SamplerRoute::kLean : SamplerRoute::kWave;
}
// channels per sweep over the taps of the lean forward: as many as divide C
int forward_channels_per_sweep(int64_t C) { return C % 4 == 0 ? 4 : C % 3 == 0 ? 3 : C % 2 == 0 ? 2 : 1; }

} // namespace
} // namespace drtk_amd

using namespace drtk_amd;

extern "C" int drtk_amd_mipmap_grid_sampler_2d(
    drtk_dtype_t dtype, const void* const* levels, const int64_t* level_h, const int64_t* level_w, const int64_t* level_sN, int mipmaps,
    const void* grid, const int64_t* grid_layout, const void* vt_dxdy_img, int64_t N, int64_t C, int64_t H, int64_t W, int max_aniso,
    int padding_mode, int interpolation_mode, int align_corners, int force_max_aniso, int clip_grad, void* out,
    drtk_stream_t stream) {
  (void)align_corners; // ignored by the reference's forward kernel (:423)
  LevelTable lv;
  GridLayout gl, unused;
  const int st = check_sampler_args(
      false, dtype, levels, nullptr, level_h, level_w, level_sN, mipmaps, grid, grid_layout, vt_dxdy_img, N, C, H, W, max_aniso, padding_mode,
      interpolation_mode, nullptr, out, nullptr, lv, gl, unused);
  if (st != DRTK_OK) return st;
  const int64_t count = N * H * W;
  if (count == 0 || C == 0) return DRTK_OK;
  hipStream_t s = static_cast<hipStream_t>(stream);
  const SamplerRoute route = sampler_route(interpolation_mode, N, C, lv, mipmaps, false);
  return dispatch_dtype(dtype, [&](auto tag) {
    using T = decltype(tag);
    const T* grid_t = static_cast<const T*>(grid);
    const T* vt = static_cast<const T*>(vt_dxdy_img);
    const int strip = xcd_strip(ceil_div(16 * W, kBlock));
    with_constant<0, 2>(padding_mode, [&](auto pad) {
      constexpr int PAD = decltype(pad)::value;
      if (route == SamplerRoute::kLean) {
        with_constant<1, 4>(forward_channels_per_sweep(C), [&](auto cb) {
          constexpr int CB = decltype(cb)::value;
          static const std::string name = instance_name<PAD, CB>("mipmap_forward_lean_kernel");
          launch_as(
              name, mipmap_forward_lean_kernel<T, PAD, CB>, dim3(static_cast<unsigned>(ceil_div(H * W, kBlock)), static_cast<unsigned>(N)),
              kBlock, 0, s, lv, mipmaps, grid_t, gl, vt, (int)C, H * W, max_aniso, force_max_aniso != 0, clip_grad != 0,
              static_cast<T*>(out), strip);
        });
      } else { // bicubic, and the bilinear calls the lean kernel does not take
        with_constant<0, 1>(interpolation_mode / 2, [&](auto bicubic) {
          constexpr int MODE = 2 * decltype(bicubic)::value;
          static const std::string name = instance_name<MODE, PAD>("mipmap_forward_kernel");
          launch_as(
              name, mipmap_forward_kernel<T, MODE, PAD>, dim3(static_cast<unsigned>(ceil_div(count, kBlock))), kBlock, 0, s,
              lv, mipmaps, grid_t, gl, vt, count, (int)C, H * W, max_aniso, force_max_aniso != 0, clip_grad != 0, static_cast<T*>(out), strip);
        });
      }
    });
    DRTK_RETURN_IF_LAUNCH_FAILED();
    return DRTK_OK;
  });
}

extern "C" int drtk_amd_mipmap_grid_sampler_2d_backward(
    drtk_dtype_t dtype, const void* grad_out, const void* const* levels, const int64_t* level_h,
    const int64_t* level_w, const int64_t* level_sN, int mipmaps, const void* grid, const int64_t* grid_layout, const void* vt_dxdy_img,
    int64_t N, int64_t C, int64_t H, int64_t W, int max_aniso, int padding_mode, int interpolation_mode, int align_corners,
    int force_max_aniso, int clip_grad, void* const* grad_levels, void* grad_grid, const int64_t* grad_grid_layout,
    drtk_stream_t stream) {
  LevelTable lv;
  GridLayout gl, ggl;
  const int st = check_sampler_args(
      true, dtype, levels, grad_levels, level_h, level_w, level_sN, mipmaps, grid, grid_layout, vt_dxdy_img, N, C, H, W, max_aniso, padding_mode,
      interpolation_mode, grad_out, grad_grid, grad_grid_layout, lv, gl, ggl);
  if (st != DRTK_OK) return st;
  hipStream_t s = static_cast<hipStream_t>(stream);
  const size_t es = dtype_size(dtype);
  // :1120-1123 zeros_like -- also for a call with textures and no pixels.  Levels that lie back to back in memory (a caller that
  // carves the gradient pyramid out of one buffer, like the torch shim) are zeroed by one launch: the coarse levels are a few KB
  // each and a launch costs more than their fill.
  for (int i = 0; i < mipmaps;) {
    size_t bytes = es * N * C * level_h[i] * level_w[i];
    int j = i + 1;
    while (j < mipmaps && bytes > 0 && grad_levels[j] == static_cast<unsigned char*>(grad_levels[i]) + bytes &&
           es * N * C * level_h[j] * level_w[j] > 0) {
      bytes += es * N * C * level_h[j] * level_w[j];
      ++j;
    }
    if (bytes > 0 && fill_bytes_async(grad_levels[i], 0, bytes, s) != DRTK_OK) return DRTK_ERR_LAUNCH;
    i = j;
  }
  const int64_t count = N * H * W;
  if (count == 0) return DRTK_OK;
  const SamplerRoute route = sampler_route(interpolation_mode, N, C, lv, mipmaps, DRTK_DBG(debug_flags(), 512));
  return dispatch_dtype(dtype, [&](auto tag) -> int {
    using T = decltype(tag);
    const T* gout = static_cast<const T*>(grad_out);
    const T* grid_t = static_cast<const T*>(grid);
    const T* vt = static_cast<const T*>(vt_dxdy_img);
    T* ggrid = static_cast<T*>(grad_grid);
    if (route == SamplerRoute::kGeneral) {
      with_constant<0, 1>(interpolation_mode / 2, [&](auto bicubic) {
        constexpr int MODE = 2 * decltype(bicubic)::value;
        static const std::string name = instance_name<MODE>("mipmap_backward_kernel");
        launch_as(
            name, mipmap_backward_kernel<T, MODE>, dim3(static_cast<unsigned>(ceil_div(count, kBlock))), kBlock, 0, s, lv,
            mipmaps, gout, grid_t, gl, vt, count, (int)C, H * W, max_aniso, padding_mode, align_corners != 0, force_max_aniso != 0,
            clip_grad != 0, ggrid, ggl, xcd_strip(ceil_div(16 * W, kBlock)));
      });
      DRTK_RETURN_IF_LAUNCH_FAILED();
      return DRTK_OK;
    }
    const int tiles_x = static_cast<int>(ceil_div(W, kTileW)), tiles_y = static_cast<int>(ceil_div(H, kTileH));
    const dim3 tiles(static_cast<unsigned>(tiles_x * tiles_y), static_cast<unsigned>(N));
    int rc = DRTK_OK;
    with_constant<0, 2>(padding_mode, [&](auto pad) {
      with_constant<0, 1>(align_corners != 0, [&](auto align) {
        constexpr int PAD = decltype(pad)::value;
        constexpr bool ALIGN = decltype(align)::value != 0;
        if (route == SamplerRoute::kWave) {
          // bicubic, any C: 4 x 4 cells per tap in wave-private windows, channels in blocks of four inside the kernel
          const size_t lds = sizeof(double) * (C < kChBlock ? C : kChBlock) * kWaveCells * (kMipBlock / kWave);
          static const std::string name = instance_name<PAD, ALIGN>("mipmap_backward_wave_kernel");
          launch_as(
              name, mipmap_backward_wave_kernel<T, PAD, ALIGN>, tiles, kMipBlock, lds, s, lv, mipmaps, gout, grid_t, gl, vt, (int)H,
              (int)W, (int)C, tiles_x, max_aniso, force_max_aniso != 0, clip_grad != 0, ggrid, ggl, xcd_strip(tiles_x), debug_flags());
          if (hipGetLastError() != hipSuccess) rc = DRTK_ERR_LAUNCH;
          return;
        }
        // bilinear: the lean tile kernel, once per block of four channels (every launch after the first adds to the grid gradient)
        for (int c0 = 0; c0 < C && rc == DRTK_OK; c0 += 4) {
          with_constant<1, 4>(static_cast<int>(C - c0 < 4 ? C - c0 : 4), [&](auto cn) {
            constexpr int CN = decltype(cn)::value;
            static const std::string name = instance_name<PAD, ALIGN, CN>("mipmap_backward_lean_kernel");
            launch_as(
                name, mipmap_backward_lean_kernel<T, PAD, ALIGN, CN>, tiles, kMipBlock, sizeof(double) * CN * kWinLevels * lean_slot_cells<CN>(),
                s, lv, mipmaps, gout, grid_t, gl, vt, (int)H, (int)W, tiles_x, max_aniso, force_max_aniso != 0, clip_grad != 0, ggrid, ggl,
                xcd_strip(tiles_x), debug_flags(), (int)C, c0);
          });
          if (hipGetLastError() != hipSuccess) rc = DRTK_ERR_LAUNCH;
        }
      });
    });
    return rc;
  });
}
