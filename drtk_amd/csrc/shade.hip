// shade -- Blinn-Phong deferred shading of an interpolated G-buffer, forward and backward, one streaming kernel each way
// (no reference counterpart: the reference's tutorial writes it as about 25 PyTorch launches).
//
// Definition, per pixel of view n, in the tensors' own type, unit(x) = x / max(||x||, 1e-12):
//   L = unit(light_dir);  nv = unit(normal);  d = max(-(nv . L), 0);  col[c] = albedo[c] * (d + ambient[c])
//   with specular:  w = unit(pos);  h = unit(L - w);  b = max(-(h . nv), 1e-8);  col[c] += b^shininess * specular[c]
//   out[c] = col[c] where index != -1 (or there is no index), else background[c] (0 without one)   -- a select, not a blend
//   with gamma:  out[c] = max(out[c], 0)^(1 / gamma)                                                -- background included
// Gradients are the derivative of that, with these conventions at the non-smooth points: d passes a gradient only where
// -(nv . L) > 0, b only where -(h . nv) > 1e-8, the gamma step only where its argument is > 0 (else exactly 0, never NaN or
// inf), and unit(x) with ||x|| <= 1e-12 is a constant.  A pixel whose index is -1 reads none of the foreground images and
// gives them a zero gradient; a foreground pixel does not read the background and gives it a zero gradient.
//
// Layout: every image is [N, channels, H, W] with W stride 1 and element strides {sN, sC, sH}; outputs and gradients are
// contiguous.  One lane owns kShadePix consecutive pixels of one view (16 bytes) and moves each plane's share as one
// element-aligned vector; the ragged last lane of a plane goes pixel by pixel, and so does a lane whose pixels span two
// rows of an image whose rows are not W apart.  No LDS and no atomics in the forward.  The backward accumulates the at
// most 16 parameter terms of its pixels per lane in double, reduces them over the wave (a fixed butterfly) and over the
// four waves (in order, through LDS) and leaves one row of 16 doubles per workgroup in the workspace; shade_finalize_kernel
// adds the rows of a view -- row r of every kShadeFinalRows, in ascending order, then the kShadeFinalRows partial sums in
// order -- and a second launch of it adds the views' sums the same way for parameters shared by all views.  No atomics
// anywhere: bitwise reproducible.  Nothing is kept from the forward: the backward recomputes the shading.
//
// float32 evaluates x^y as exp2(y * log2(x)) on the hardware's v_log_f32 / v_exp_f32 (1 ulp each): the exponent's rounding
// costs |y log2 x| 2^-24 relative, times a result that is at most 2^-|y log2 x| -- below 1e-7 of the output's scale, against
// the 1e-5 the tests hold float32 to.  Square roots and divisions are the correctly rounded ones; float64 calls the library.
#include "common.hpp"

namespace drtk_amd {
namespace {

constexpr int kShadePixF32 = 4;       // pixels per lane, float32
constexpr int kShadePixF64 = 2;       // pixels per lane, float64
constexpr int kShadeTerms = 16;       // doubles per workspace row: light 0..2, shininess 3, albedo 4.., ambient 8.., specular 12..
constexpr int kShadeFinalRows = 64;   // rows the finalize kernel adds per pass
constexpr int kShadeFinalBlock = kShadeFinalRows * kShadeTerms;
constexpr int kShadeMaxChannels = 4;

template <typename T>
constexpr int kShadePix = sizeof(T) == 4 ? kShadePixF32 : kShadePixF64;

template <typename T>
struct ShadeImage {
  const T* p;
  int64_t sN, sC, sH;
};

template <typename T>
struct ShadeArgs {
  ShadeImage<T> normal, pos, albedo_img, bg; // p == NULL: absent
  const int32_t* index;                      // [N,H,W], strides {i_sN, i_sH}, or NULL: every pixel is foreground
  int64_t i_sN, i_sH;
  const T *light, *albedo, *ambient, *specular, *shininess; // per view (sN = count) or shared (sN = 0)
  int64_t l_sN, al_sN, am_sN, sp_sN, sh_sN;
  T inv_gamma; // 0: no gamma step
  int64_t HW;
  unsigned W;
  int flat; // every image's rows are W apart: a plane is one run of H W elements
  int strip;
  T* out; // [N,C,H,W]
  // backward
  const T* g_out;                      // [N,C,H,W]
  T *g_normal, *g_pos, *g_albedo_img, *g_bg; // contiguous, or NULL: not wanted
  double* rows;                        // [N][workgroups per view][kShadeTerms], or NULL: no parameter gradient is wanted
};

template <typename E, int P>
struct ShadeVec {
  typedef E type __attribute__((ext_vector_type(P), aligned(sizeof(E))));
};

// P consecutive elements at p: one element-aligned vector access when all P belong to the plane, else the first `rem`.
template <typename E, int P>
__device__ __forceinline__ void load_px(const E* __restrict__ p, int rem, E fill, E (&v)[P]) {
  if (rem == P) {
    const typename ShadeVec<E, P>::type q = *reinterpret_cast<const typename ShadeVec<E, P>::type*>(p);
#pragma unroll
    for (int j = 0; j < P; ++j) v[j] = q[j];
  } else {
#pragma unroll
    for (int j = 0; j < P; ++j) v[j] = j < rem ? p[j] : fill;
  }
}
template <typename E, int P>
__device__ __forceinline__ void store_px(E* __restrict__ p, int rem, const E (&v)[P]) {
  if (rem == P) {
    typename ShadeVec<E, P>::type q;
#pragma unroll
    for (int j = 0; j < P; ++j) q[j] = v[j];
    *reinterpret_cast<typename ShadeVec<E, P>::type*>(p) = q;
  } else {
#pragma unroll
    for (int j = 0; j < P; ++j) {
      if (j < rem) p[j] = v[j];
    }
  }
}

// Where a lane's pixels sit in an image: row y, column x of the first, and whether all `rem` lie in that row.  A flat
// image is one row of H W pixels.
struct ShadeSpan {
  int64_t y, x;
  bool one_row;
};
__device__ __forceinline__ ShadeSpan shade_span(int64_t pix0, int rem, unsigned W, bool flat) {
  if (flat) return {0, pix0, true};
  const unsigned p = static_cast<unsigned>(pix0), y = p / W, x = p - y * W;
  return {int64_t(y), int64_t(x), x + unsigned(rem) <= W};
}
template <typename E, int P>
__device__ __forceinline__ void load_span(
    const E* __restrict__ plane, int64_t sH, unsigned W, const ShadeSpan& s, int rem, E fill, E (&v)[P]) {
  if (s.one_row) {
    load_px<E, P>(plane + s.y * sH + s.x, rem, fill, v);
    return;
  }
  int64_t y = s.y, x = s.x;
#pragma unroll
  for (int j = 0; j < P; ++j) {
    v[j] = fill;
    if (j < rem) {
      v[j] = plane[y * sH + x];
      if (++x == int64_t(W)) x = 0, ++y;
    }
  }
}

template <typename T>
struct ShadeMath;
template <>
struct ShadeMath<float> {
  static __device__ __forceinline__ float sqrt(float x) { return ::sqrtf(x); }
  static __device__ __forceinline__ float log2(float x) { return __builtin_amdgcn_logf(x); }
  static __device__ __forceinline__ float exp2(float x) { return __builtin_amdgcn_exp2f(x); }
  // x^y and log2(x) for x > 0
  static __device__ __forceinline__ float pow(float x, float y, float& lg) {
    lg = log2(x);
    return exp2(y * lg);
  }
};
template <>
struct ShadeMath<double> {
  static __device__ __forceinline__ double sqrt(double x) { return ::sqrt(x); }
  static __device__ __forceinline__ double pow(double x, double y, double& lg) {
    lg = ::log2(x);
    return ::pow(x, y);
  }
};

// u = x / max(||x||, 1e-12); returns 1 / ||x||, or 0 where ||x|| <= 1e-12 (u is then a constant: no gradient)
template <typename T>
__device__ __forceinline__ T shade_unit(const T (&x)[3], T (&u)[3]) {
  const T nn = ShadeMath<T>::sqrt(x[0] * x[0] + x[1] * x[1] + x[2] * x[2]);
  const T inv = T(1) / (nn > T(1e-12) ? nn : T(1e-12));
#pragma unroll
  for (int k = 0; k < 3; ++k) u[k] = x[k] * inv;
  return nn > T(1e-12) ? inv : T(0);
}
// the gradient of x through u = unit(x), given that of u
template <typename T>
__device__ __forceinline__ void shade_unit_backward(const T (&u)[3], T inv, const T (&gu)[3], T (&gx)[3]) {
  const T dot = u[0] * gu[0] + u[1] * gu[1] + u[2] * gu[2];
#pragma unroll
  for (int k = 0; k < 3; ++k) gx[k] = (gu[k] - u[k] * dot) * inv;
}

// what is the same for every pixel of a view
template <typename T, int C>
struct ShadeView {
  T L[3], inv_l;
  T albedo[C], ambient[C], specular[C], shininess;
};
template <typename T, int C>
__device__ __forceinline__ ShadeView<T, C> shade_view(const ShadeArgs<T>& a, int n) {
  ShadeView<T, C> v;
  const T* lp = a.light + int64_t(n) * a.l_sN;
  const T l[3] = {lp[0], lp[1], lp[2]};
  v.inv_l = shade_unit<T>(l, v.L);
#pragma unroll
  for (int c = 0; c < C; ++c) {
    v.albedo[c] = a.albedo ? a.albedo[int64_t(n) * a.al_sN + c] : T(0);
    v.ambient[c] = a.ambient[int64_t(n) * a.am_sN + c];
    v.specular[c] = a.specular ? a.specular[int64_t(n) * a.sp_sN + c] : T(0);
  }
  v.shininess = a.specular ? a.shininess[int64_t(n) * a.sh_sN] : T(0);
  return v;
}

// the shading of one foreground pixel: everything the backward needs again
template <typename T>
struct ShadePixel {
  T nv[3], inv_n, ndl, d;         // unit normal, 1 / ||normal||, -(nv . L), max(ndl, 0)
  T w[3], inv_p, h[3], inv_h, hn; // unit position, unit half vector, -(h . nv)
  T b, s, log2b;                  // max(hn, 1e-8), b^shininess, log2(b)
};
template <typename T, int C>
__device__ __forceinline__ void shade_pixel(
    const ShadeView<T, C>& v, bool specular, const T (&normal)[3], const T (&pos)[3], ShadePixel<T>& q) {
  q.inv_n = shade_unit<T>(normal, q.nv);
  q.ndl = -(q.nv[0] * v.L[0] + q.nv[1] * v.L[1] + q.nv[2] * v.L[2]);
  q.d = q.ndl > T(0) ? q.ndl : T(0);
  q.s = T(0);
  if (specular) {
    q.inv_p = shade_unit<T>(pos, q.w);
    const T hv[3] = {v.L[0] - q.w[0], v.L[1] - q.w[1], v.L[2] - q.w[2]};
    q.inv_h = shade_unit<T>(hv, q.h);
    q.hn = -(q.h[0] * q.nv[0] + q.h[1] * q.nv[1] + q.h[2] * q.nv[2]);
    q.b = q.hn > T(1e-8) ? q.hn : T(1e-8);
    q.s = ShadeMath<T>::pow(q.b, v.shininess, q.log2b);
  }
}

// which of the lane's pixels are foreground (bit j), out of the `rem` it owns
template <typename T, int P>
__device__ __forceinline__ unsigned shade_foreground(const ShadeArgs<T>& a, int n, const ShadeSpan& span, int rem) {
  if (!a.index) return (1u << rem) - 1u;
  int32_t id[P];
  load_span<int32_t, P>(a.index + int64_t(n) * a.i_sN, a.i_sH, a.W, span, rem, -1, id);
  unsigned fg = 0;
#pragma unroll
  for (int j = 0; j < P; ++j) fg |= (id[j] != -1 ? 1u : 0u) << j;
  return fg;
}

template <typename T, int P>
__device__ __forceinline__ void shade_load3(
    const ShadeImage<T>& img, int n, unsigned W, const ShadeSpan& span, int rem, T (&v)[3][P]) {
  const T* p = img.p + int64_t(n) * img.sN;
#pragma unroll
  for (int k = 0; k < 3; ++k) load_span<T, P>(p + k * img.sC, img.sH, W, span, rem, T(0), v[k]);
}

template <typename T, int C>
__global__ __launch_bounds__(kBlock) void shade_forward_kernel(const ShadeArgs<T> a) {
  constexpr int P = kShadePix<T>;
  const int64_t pix0 = (int64_t(tile_index(a.strip)) * kBlock + threadIdx.x) * P;
  if (pix0 >= a.HW) return;
  const int n = blockIdx.y;
  const int rem = a.HW - pix0 < P ? static_cast<int>(a.HW - pix0) : P;
  const ShadeSpan span = shade_span(pix0, rem, a.W, a.flat);
  const unsigned fg = shade_foreground<T, P>(a, n, span, rem);
  const unsigned bgm = ((1u << rem) - 1u) & ~fg;
  const ShadeView<T, C> v = shade_view<T, C>(a, n);
  const bool specular = a.specular != nullptr;

  T col[C][P];
#pragma unroll
  for (int c = 0; c < C; ++c) {
#pragma unroll
    for (int j = 0; j < P; ++j) col[c][j] = T(0);
  }
  if (bgm && a.bg.p) {
    const T* bp = a.bg.p + int64_t(n) * a.bg.sN;
#pragma unroll
    for (int c = 0; c < C; ++c) load_span<T, P>(bp + c * a.bg.sC, a.bg.sH, a.W, span, rem, T(0), col[c]);
  }
  if (fg) {
    T nrm[3][P], pos[3][P], alb[C][P];
    shade_load3<T, P>(a.normal, n, a.W, span, rem, nrm);
    if (specular) shade_load3<T, P>(a.pos, n, a.W, span, rem, pos);
    if (a.albedo_img.p) {
      const T* ap = a.albedo_img.p + int64_t(n) * a.albedo_img.sN;
#pragma unroll
      for (int c = 0; c < C; ++c) load_span<T, P>(ap + c * a.albedo_img.sC, a.albedo_img.sH, a.W, span, rem, T(0), alb[c]);
    }
#pragma unroll
    for (int j = 0; j < P; ++j) {
      const T nj[3] = {nrm[0][j], nrm[1][j], nrm[2][j]};
      const T pj[3] = {specular ? pos[0][j] : T(0), specular ? pos[1][j] : T(0), specular ? pos[2][j] : T(0)};
      ShadePixel<T> q;
      shade_pixel<T, C>(v, specular, nj, pj, q);
      const bool on = (fg >> j) & 1u;
#pragma unroll
      for (int c = 0; c < C; ++c) {
        const T al = a.albedo_img.p ? alb[c][j] : v.albedo[c];
        T x = al * (q.d + v.ambient[c]);
        if (specular) x = x + q.s * v.specular[c];
        col[c][j] = on ? x : col[c][j]; // (a NaN next to a foreground pixel was loaded with it)
      }
    }
  }
  if (a.inv_gamma != T(0)) {
#pragma unroll
    for (int c = 0; c < C; ++c) {
#pragma unroll
      for (int j = 0; j < P; ++j) {
        T lg;
        const T x = col[c][j];
        col[c][j] = x > T(0) ? ShadeMath<T>::pow(x, a.inv_gamma, lg) : T(0);
      }
    }
  }
  T* op = a.out + (int64_t(n) * C) * a.HW + pix0;
#pragma unroll
  for (int c = 0; c < C; ++c) store_px<T, P>(op + c * a.HW, rem, col[c]);
}

__device__ __forceinline__ double shade_wave_sum(double x) {
#pragma unroll
  for (int m = kWave / 2; m >= 1; m >>= 1) x += __shfl_xor(x, m, kWave);
  return x;
}

template <typename T, int C>
__global__ __launch_bounds__(kBlock) void shade_backward_kernel(const ShadeArgs<T> a) {
  constexpr int P = kShadePix<T>;
  constexpr T kLn2 = T(0.69314718055994530942);
  __shared__ double s_red[kBlock / kWave][kShadeTerms];
  const int tile = tile_index(a.strip);
  const int64_t pix0 = (int64_t(tile) * kBlock + threadIdx.x) * P;
  const int n = blockIdx.y;
  const bool specular = a.specular != nullptr;
  const bool params = a.rows != nullptr;
  // the lane's share of the parameter gradients: light, shininess, albedo, ambient, specular
  double acc_l[3] = {0.0, 0.0, 0.0}, acc_sh = 0.0, acc_al[C], acc_am[C], acc_sp[C];
#pragma unroll
  for (int c = 0; c < C; ++c) acc_al[c] = acc_am[c] = acc_sp[c] = 0.0;

  if (pix0 < a.HW) {
    const int rem = a.HW - pix0 < P ? static_cast<int>(a.HW - pix0) : P;
    const ShadeSpan span = shade_span(pix0, rem, a.W, a.flat);
    const unsigned fg = shade_foreground<T, P>(a, n, span, rem);
    const unsigned bgm = ((1u << rem) - 1u) & ~fg;
    const ShadeView<T, C> v = shade_view<T, C>(a, n);
    const bool gamma = a.inv_gamma != T(0);

    T g[C][P], bgv[C][P], nrm[3][P], pos[3][P], alb[C][P];
    const T* gp = a.g_out + (int64_t(n) * C) * a.HW + pix0;
#pragma unroll
    for (int c = 0; c < C; ++c) load_px<T, P>(gp + c * a.HW, rem, T(0), g[c]);
#pragma unroll
    for (int c = 0; c < C; ++c) {
#pragma unroll
      for (int j = 0; j < P; ++j) bgv[c][j] = alb[c][j] = T(0);
    }
#pragma unroll
    for (int k = 0; k < 3; ++k) {
#pragma unroll
      for (int j = 0; j < P; ++j) nrm[k][j] = pos[k][j] = T(0);
    }
    // the background's value matters only to the gamma step
    if (bgm && a.bg.p && gamma) {
      const T* bp = a.bg.p + int64_t(n) * a.bg.sN;
#pragma unroll
      for (int c = 0; c < C; ++c) load_span<T, P>(bp + c * a.bg.sC, a.bg.sH, a.W, span, rem, T(0), bgv[c]);
    }
    if (fg) {
      shade_load3<T, P>(a.normal, n, a.W, span, rem, nrm);
      if (specular) shade_load3<T, P>(a.pos, n, a.W, span, rem, pos);
      if (a.albedo_img.p) {
        const T* ap = a.albedo_img.p + int64_t(n) * a.albedo_img.sN;
#pragma unroll
        for (int c = 0; c < C; ++c) load_span<T, P>(ap + c * a.albedo_img.sC, a.albedo_img.sH, a.W, span, rem, T(0), alb[c]);
      }
    }

    // per pixel; nrm, pos, alb and bgv end as the gradients of what they held
#pragma unroll
    for (int j = 0; j < P; ++j) {
      const bool on = (fg >> j) & 1u;
      if (on) {
        const T nj[3] = {nrm[0][j], nrm[1][j], nrm[2][j]};
        const T pj[3] = {pos[0][j], pos[1][j], pos[2][j]};
        ShadePixel<T> q;
        shade_pixel<T, C>(v, specular, nj, pj, q);
        T g_d = T(0), g_s = T(0);
#pragma unroll
        for (int c = 0; c < C; ++c) {
          const T al = a.albedo_img.p ? alb[c][j] : v.albedo[c];
          const T shade = q.d + v.ambient[c];
          T gc = g[c][j];
          if (gamma) {
            T x = al * shade, lg;
            if (specular) x = x + q.s * v.specular[c];
            gc = x > T(0) ? gc * a.inv_gamma * ShadeMath<T>::pow(x, a.inv_gamma, lg) / x : T(0);
          }
          const T g_al = gc * shade, g_am = gc * al;
          alb[c][j] = g_al;
          g_d = g_d + g_am;
          g_s = g_s + gc * v.specular[c];
          if (params) {
            acc_al[c] += double(g_al);
            acc_am[c] += double(g_am);
            if (specular) acc_sp[c] += double(gc * q.s);
          }
          bgv[c][j] = T(0);
        }
        T g_n[3] = {T(0), T(0), T(0)}, g_L[3] = {T(0), T(0), T(0)}, g_p[3] = {T(0), T(0), T(0)};
        if (specular) {
          const T g_b = q.hn > T(1e-8) ? g_s * v.shininess * q.s / q.b : T(0);
          if (params) acc_sh += double(g_s * q.s * (q.log2b * kLn2));
          const T g_h[3] = {-g_b * q.nv[0], -g_b * q.nv[1], -g_b * q.nv[2]};
          T g_hv[3];
          shade_unit_backward<T>(q.h, q.inv_h, g_h, g_hv);
          const T g_w[3] = {-g_hv[0], -g_hv[1], -g_hv[2]};
          shade_unit_backward<T>(q.w, q.inv_p, g_w, g_p);
#pragma unroll
          for (int k = 0; k < 3; ++k) g_n[k] = -g_b * q.h[k], g_L[k] = g_hv[k];
        }
        if (q.ndl > T(0)) {
#pragma unroll
          for (int k = 0; k < 3; ++k) g_n[k] = g_n[k] - g_d * v.L[k], g_L[k] = g_L[k] - g_d * q.nv[k];
        }
        T g_normal[3];
        shade_unit_backward<T>(q.nv, q.inv_n, g_n, g_normal);
#pragma unroll
        for (int k = 0; k < 3; ++k) nrm[k][j] = g_normal[k], pos[k][j] = g_p[k];
        if (params) {
          T g_light[3];
          shade_unit_backward<T>(v.L, v.inv_l, g_L, g_light);
#pragma unroll
          for (int k = 0; k < 3; ++k) acc_l[k] += double(g_light[k]);
        }
      } else {
#pragma unroll
        for (int c = 0; c < C; ++c) {
          T gc = g[c][j];
          if (gamma) {
            const T x = bgv[c][j];
            T lg;
            gc = x > T(0) ? gc * a.inv_gamma * ShadeMath<T>::pow(x, a.inv_gamma, lg) / x : T(0);
          }
          bgv[c][j] = gc;
          alb[c][j] = T(0);
        }
#pragma unroll
        for (int k = 0; k < 3; ++k) nrm[k][j] = pos[k][j] = T(0);
      }
    }

    if (a.g_normal) {
      T* p = a.g_normal + (int64_t(n) * 3) * a.HW + pix0;
#pragma unroll
      for (int k = 0; k < 3; ++k) store_px<T, P>(p + k * a.HW, rem, nrm[k]);
    }
    if (a.g_pos) {
      T* p = a.g_pos + (int64_t(n) * 3) * a.HW + pix0;
#pragma unroll
      for (int k = 0; k < 3; ++k) store_px<T, P>(p + k * a.HW, rem, pos[k]);
    }
    if (a.g_albedo_img) {
      T* p = a.g_albedo_img + (int64_t(n) * C) * a.HW + pix0;
#pragma unroll
      for (int c = 0; c < C; ++c) store_px<T, P>(p + c * a.HW, rem, alb[c]);
    }
    if (a.g_bg) {
      T* p = a.g_bg + (int64_t(n) * C) * a.HW + pix0;
#pragma unroll
      for (int c = 0; c < C; ++c) store_px<T, P>(p + c * a.HW, rem, bgv[c]);
    }
  }

  if (!params) return; // (uniform)
  double t[kShadeTerms];
#pragma unroll
  for (int i = 0; i < kShadeTerms; ++i) t[i] = 0.0;
#pragma unroll
  for (int k = 0; k < 3; ++k) t[k] = acc_l[k];
  t[3] = acc_sh;
#pragma unroll
  for (int c = 0; c < C; ++c) t[4 + c] = acc_al[c], t[8 + c] = acc_am[c], t[12 + c] = acc_sp[c];
  const int thread = static_cast<int>(threadIdx.x), wave = thread / kWave, lane = thread % kWave;
#pragma unroll
  for (int i = 0; i < kShadeTerms; ++i) {
    const bool used = i < 3 || (i == 3 ? true : ((i & 3) < C));
    const double s = used ? shade_wave_sum(t[i]) : 0.0;
    if (lane == 0) s_red[wave][i] = s;
  }
  __syncthreads();
  if (thread < kShadeTerms) {
    double s = s_red[0][thread];
    for (int wv = 1; wv < kBlock / kWave; ++wv) s += s_red[wv][thread];
    a.rows[(int64_t(n) * gridDim.x + tile) * kShadeTerms + thread] = s;
  }
}

// Where the sums of one group of rows go: the gradient of a parameter of `count` elements at term `first`, per group
// (stride = count) -- or nowhere (NULL).
template <typename T>
struct ShadeParamGrads {
  T *light, *shininess, *albedo, *ambient, *specular;
  int64_t l_s, sh_s, al_s, am_s, sp_s;
};

// One workgroup per group of `rows_per_group` rows: thread (r, i) adds term i of rows r, r + kShadeFinalRows, ... in ascending
// order, then thread i < 16 adds the kShadeFinalRows partial sums in order.  The sum goes to the parameter gradients that are
// given (element group * stride + index) and, if `sums`, to row `group` of it.
template <typename T>
__global__ __launch_bounds__(kShadeFinalBlock) void shade_finalize_kernel(
    const double* __restrict__ rows, int64_t rows_per_group, int C, ShadeParamGrads<T> g, double* __restrict__ sums) {
  __shared__ double s_part[kShadeFinalRows][kShadeTerms];
  const int thread = static_cast<int>(threadIdx.x), r = thread / kShadeTerms, i = thread % kShadeTerms;
  const int64_t group = blockIdx.x;
  const double* __restrict__ base = rows + group * rows_per_group * kShadeTerms;
  double t = 0.0;
  for (int64_t row = r; row < rows_per_group; row += kShadeFinalRows) t += base[row * kShadeTerms + i];
  s_part[r][i] = t;
  __syncthreads();
  if (thread >= kShadeTerms) return;
  t = s_part[0][i];
  for (int k = 1; k < kShadeFinalRows; ++k) t += s_part[k][i];
  if (sums) sums[group * kShadeTerms + i] = t;
  const int c = i & 3;
  if (i < 3) {
    if (g.light) g.light[group * g.l_s + i] = T(t);
  } else if (i == 3) {
    if (g.shininess) g.shininess[group * g.sh_s] = T(t);
  } else if (c < C) {
    if (i < 8) {
      if (g.albedo) g.albedo[group * g.al_s + c] = T(t);
    } else if (i < 12) {
      if (g.ambient) g.ambient[group * g.am_s + c] = T(t);
    } else {
      if (g.specular) g.specular[group * g.sp_s + c] = T(t);
    }
  }
}

// ---- host ---------------------------------------------------------------------------------------------------------------------

int64_t shade_blocks_per_view(drtk_dtype_t dtype, int64_t H, int64_t W) {
  const int P = dtype == DRTK_F32 ? kShadePixF32 : kShadePixF64;
  return ceil_div(H * W, int64_t(kBlock) * P);
}
// rows of the streaming kernel, then one row per view for the views' sums
size_t shade_workspace(drtk_dtype_t dtype, int64_t N, int64_t H, int64_t W) {
  return size_t(N) * size_t(shade_blocks_per_view(dtype, H, W) + 1) * kShadeTerms * sizeof(double);
}

int shade_validate(drtk_dtype_t dtype, int64_t N, int64_t C, int64_t H, int64_t W, double gamma) {
  constexpr int64_t kLimit = int64_t(1) << 31;
  if (!valid_dtype(dtype)) return DRTK_ERR_INVALID_ARGUMENT;
  if (H >= kLimit || W >= kLimit || bad_image(N, H, W)) return DRTK_ERR_INVALID_ARGUMENT;
  if (C < 1 || C > kShadeMaxChannels) return DRTK_ERR_INVALID_ARGUMENT;
  if (!(gamma >= 0.0) || !(gamma < 1e30)) return DRTK_ERR_INVALID_ARGUMENT; // 0: no gamma step
  return DRTK_OK;
}

bool shade_strides_ok(const int64_t* s, int count) {
  if (!s) return false;
  for (int i = 0; i < count; ++i) {
    if (s[i] < 0) return false;
  }
  return true;
}

// everything both entry points are given of the inputs, as the C ABI spells it
struct ShadeInputs {
  const void *normal, *pos, *albedo_img, *bg;
  const int64_t *normal_s, *pos_s, *albedo_img_s, *bg_s;
  const int32_t* index;
  const int64_t* index_s;
  const void *light, *albedo, *ambient, *specular, *shininess;
  int64_t l_sN, al_sN, am_sN, sp_sN, sh_sN;
  double gamma;
  int64_t N, C, H, W;
};

int shade_check_inputs(const ShadeInputs& in) {
  if (!in.normal || !shade_strides_ok(in.normal_s, 3) || !in.light || !in.ambient) return DRTK_ERR_INVALID_ARGUMENT;
  if ((in.albedo != nullptr) == (in.albedo_img != nullptr)) return DRTK_ERR_INVALID_ARGUMENT; // a vector or an image
  if (in.albedo_img && !shade_strides_ok(in.albedo_img_s, 3)) return DRTK_ERR_INVALID_ARGUMENT;
  if (in.specular && (!in.pos || !in.shininess || !shade_strides_ok(in.pos_s, 3))) return DRTK_ERR_INVALID_ARGUMENT;
  if (in.bg && !shade_strides_ok(in.bg_s, 3)) return DRTK_ERR_INVALID_ARGUMENT;
  if (in.index && !shade_strides_ok(in.index_s, 2)) return DRTK_ERR_INVALID_ARGUMENT;
  if (bad_view_stride(in.l_sN, 3) || bad_view_stride(in.am_sN, in.C)) return DRTK_ERR_INVALID_ARGUMENT;
  if (in.albedo && bad_view_stride(in.al_sN, in.C)) return DRTK_ERR_INVALID_ARGUMENT;
  if (in.specular && (bad_view_stride(in.sp_sN, in.C) || bad_view_stride(in.sh_sN, 1))) return DRTK_ERR_INVALID_ARGUMENT;
  return DRTK_OK;
}

template <typename T>
ShadeImage<T> shade_image(const void* p, const int64_t* s, int64_t n0) {
  if (!p) return {nullptr, 0, 0, 0};
  return {static_cast<const T*>(p) + n0 * s[0], s[0], s[1], s[2]};
}

// the kernel's arguments for views [n0, ...)
template <typename T>
ShadeArgs<T> shade_args(const ShadeInputs& in, int64_t n0) {
  ShadeArgs<T> a = {};
  a.normal = shade_image<T>(in.normal, in.normal_s, n0);
  a.pos = shade_image<T>(in.specular ? in.pos : nullptr, in.pos_s, n0); // (positions are read for the highlight only)
  a.albedo_img = shade_image<T>(in.albedo_img, in.albedo_img_s, n0);
  a.bg = shade_image<T>(in.bg, in.bg_s, n0);
  a.index = in.index ? in.index + n0 * in.index_s[0] : nullptr;
  if (in.index) a.i_sN = in.index_s[0], a.i_sH = in.index_s[1];
  const auto vec = [&](const void* p, int64_t sN) { return p ? static_cast<const T*>(p) + n0 * sN : nullptr; };
  a.light = vec(in.light, in.l_sN), a.l_sN = in.l_sN;
  a.albedo = vec(in.albedo, in.al_sN), a.al_sN = in.al_sN;
  a.ambient = vec(in.ambient, in.am_sN), a.am_sN = in.am_sN;
  a.specular = vec(in.specular, in.sp_sN), a.sp_sN = in.sp_sN;
  a.shininess = in.specular ? vec(in.shininess, in.sh_sN) : nullptr, a.sh_sN = in.sh_sN;
  a.inv_gamma = in.gamma > 0.0 ? T(1.0 / in.gamma) : T(0);
  a.HW = in.H * in.W, a.W = static_cast<unsigned>(in.W);
  const auto rows_flat = [&](const void* p, int64_t sH) { return !p || in.H <= 1 || sH == in.W; };
  a.flat = rows_flat(in.normal, in.normal_s[2]) && rows_flat(a.pos.p, a.pos.sH) && rows_flat(in.albedo_img, a.albedo_img.sH) &&
      rows_flat(in.bg, a.bg.sH) && rows_flat(in.index, a.i_sH);
  return a;
}

// the streaming kernel of either pass over all views, at most kMaxViewsPerLaunch per launch
template <typename T, bool BACKWARD, typename Fill>
int shade_stream(const ShadeInputs& in, hipStream_t stream, Fill&& fill) {
  constexpr int P = kShadePix<T>;
  const int64_t blocks = ceil_div(in.H * in.W, int64_t(kBlock) * P);
  return for_view_slices(in.N, [&](int64_t n0, int64_t n) {
    ShadeArgs<T> a = shade_args<T>(in, n0);
    a.strip = xcd_strip(ceil_div(16 * in.W, int64_t(kBlock) * P));
    fill(a, n0, blocks);
    const dim3 grid(static_cast<unsigned>(blocks), static_cast<unsigned>(n));
    with_constant<1, kShadeMaxChannels>(static_cast<int>(in.C), [&](auto cc) {
      constexpr int CC = decltype(cc)::value;
      if constexpr (BACKWARD) {
        static const std::string name = instance_name<CC>("shade_backward_kernel");
        launch_as(name, shade_backward_kernel<T, CC>, grid, kBlock, 0, stream, a);
      } else {
        static const std::string name = instance_name<CC>("shade_forward_kernel");
        launch_as(name, shade_forward_kernel<T, CC>, grid, kBlock, 0, stream, a);
      }
    });
    DRTK_RETURN_IF_LAUNCH_FAILED();
    return DRTK_OK;
  });
}

} // namespace
} // namespace drtk_amd

using namespace drtk_amd;

extern "C" int drtk_amd_shade_workspace_bytes(drtk_dtype_t dtype, int64_t N, int64_t H, int64_t W, size_t* bytes) {
  if (!bytes) return DRTK_ERR_INVALID_ARGUMENT;
  const int st = shade_validate(dtype, N, 1, H, W, 0.0);
  if (st != DRTK_OK) return st;
  *bytes = shade_workspace(dtype, N, H, W);
  return DRTK_OK;
}

extern "C" int drtk_amd_shade_forward(
    drtk_dtype_t dtype, const void* normal_img, const int64_t* normal_strides, const void* pos_img, const int64_t* pos_strides,
    const void* albedo_img, const int64_t* albedo_img_strides, const void* background, const int64_t* background_strides,
    const int32_t* index_img, const int64_t* index_strides, const void* light_dir, int64_t light_dir_sN, const void* albedo,
    int64_t albedo_sN, const void* ambient, int64_t ambient_sN, const void* specular, int64_t specular_sN, const void* shininess,
    int64_t shininess_sN, double gamma, int64_t N, int64_t C, int64_t H, int64_t W, void* out, drtk_stream_t stream) {
  const int st = shade_validate(dtype, N, C, H, W, gamma);
  if (st != DRTK_OK) return st;
  if (N == 0 || H * W == 0) return DRTK_OK;
  const ShadeInputs in = {normal_img, pos_img, albedo_img, background, normal_strides, pos_strides, albedo_img_strides,
                          background_strides, index_img, index_strides, light_dir, albedo, ambient, specular, shininess,
                          light_dir_sN, albedo_sN, ambient_sN, specular_sN, shininess_sN, gamma, N, C, H, W};
  const int bad = shade_check_inputs(in);
  if (bad != DRTK_OK) return bad;
  if (!out) return DRTK_ERR_INVALID_ARGUMENT;
  return dispatch_dtype(dtype, [&](auto tag) {
    using T = decltype(tag);
    return shade_stream<T, false>(in, static_cast<hipStream_t>(stream), [&](ShadeArgs<T>& a, int64_t n0, int64_t) {
      a.out = static_cast<T*>(out) + n0 * C * H * W;
    });
  });
}

extern "C" int drtk_amd_shade_backward(
    drtk_dtype_t dtype, const void* grad_out, const void* normal_img, const int64_t* normal_strides, const void* pos_img,
    const int64_t* pos_strides, const void* albedo_img, const int64_t* albedo_img_strides, const void* background,
    const int64_t* background_strides, const int32_t* index_img, const int64_t* index_strides, const void* light_dir,
    int64_t light_dir_sN, const void* albedo, int64_t albedo_sN, const void* ambient, int64_t ambient_sN, const void* specular,
    int64_t specular_sN, const void* shininess, int64_t shininess_sN, double gamma, int64_t N, int64_t C, int64_t H, int64_t W,
    void* grad_normal_img, void* grad_pos_img, void* grad_albedo_img, void* grad_background, void* grad_light_dir,
    int64_t grad_light_dir_sN, void* grad_albedo, int64_t grad_albedo_sN, void* grad_ambient, int64_t grad_ambient_sN,
    void* grad_specular, int64_t grad_specular_sN, void* grad_shininess, int64_t grad_shininess_sN, void* workspace,
    size_t workspace_bytes, drtk_stream_t stream) {
  const int st = shade_validate(dtype, N, C, H, W, gamma);
  if (st != DRTK_OK) return st;
  if (bad_view_stride(grad_light_dir_sN, 3) || bad_view_stride(grad_albedo_sN, C) || bad_view_stride(grad_ambient_sN, C) ||
      bad_view_stride(grad_specular_sN, C) || bad_view_stride(grad_shininess_sN, 1))
    return DRTK_ERR_INVALID_ARGUMENT;
  const bool params = grad_light_dir || grad_albedo || grad_ambient || grad_specular || grad_shininess;
  if (N > 0 && H * W > 0) {
    const ShadeInputs probe = {normal_img, pos_img, albedo_img, background, normal_strides, pos_strides, albedo_img_strides,
                               background_strides, index_img, index_strides, light_dir, albedo, ambient, specular, shininess,
                               light_dir_sN, albedo_sN, ambient_sN, specular_sN, shininess_sN, gamma, N, C, H, W};
    const int bad = shade_check_inputs(probe);
    if (bad != DRTK_OK) return bad;
    if (!grad_out) return DRTK_ERR_INVALID_ARGUMENT;
    if ((grad_pos_img || grad_specular || grad_shininess) && !specular) return DRTK_ERR_INVALID_ARGUMENT;
    if ((grad_albedo_img && !albedo_img) || (grad_albedo && !albedo) || (grad_background && !background))
      return DRTK_ERR_INVALID_ARGUMENT;
    if (params) {
      if (!workspace || (reinterpret_cast<uintptr_t>(workspace) & 15) != 0) return DRTK_ERR_INVALID_ARGUMENT;
      if (workspace_bytes < shade_workspace(dtype, N, H, W)) return DRTK_ERR_WORKSPACE_TOO_SMALL;
    }
  }
  if (N == 0 || H * W == 0) return DRTK_OK; // (the gradients of parameters shared by no view are the caller's zeros)
  if (!params && !grad_normal_img && !grad_pos_img && !grad_albedo_img && !grad_background) return DRTK_OK; // nothing is wanted
  const ShadeInputs in = {normal_img, pos_img, albedo_img, background, normal_strides, pos_strides, albedo_img_strides,
                          background_strides, index_img, index_strides, light_dir, albedo, ambient, specular, shininess,
                          light_dir_sN, albedo_sN, ambient_sN, specular_sN, shininess_sN, gamma, N, C, H, W};
  return dispatch_dtype(dtype, [&](auto tag) -> int {
    using T = decltype(tag);
    hipStream_t s = static_cast<hipStream_t>(stream);
    double* rows = params ? static_cast<double*>(workspace) : nullptr;
    const int rc = shade_stream<T, true>(in, s, [&](ShadeArgs<T>& a, int64_t n0, int64_t blocks) {
      const auto at = [&](void* p, int64_t channels) { return p ? static_cast<T*>(p) + n0 * channels * H * W : nullptr; };
      a.g_out = static_cast<const T*>(grad_out) + n0 * C * H * W;
      a.g_normal = at(grad_normal_img, 3), a.g_pos = at(grad_pos_img, 3);
      a.g_albedo_img = at(grad_albedo_img, C), a.g_bg = at(grad_background, C);
      a.rows = rows ? rows + n0 * blocks * kShadeTerms : nullptr;
    });
    if (rc != DRTK_OK || !params) return rc;
    // the rows of every view; a parameter with one gradient per view (or the only view's) is written here
    const int64_t blocks = shade_blocks_per_view(dtype, H, W);
    double* sums = rows + N * blocks * kShadeTerms;
    const auto pick = [&](bool per_view) {
      ShadeParamGrads<T> g = {};
      const auto take = [&](void* p, int64_t sN, int64_t count, T*& out, int64_t& stride) {
        const bool mine = p && (N == 1 || (sN != 0) == per_view);
        out = mine ? static_cast<T*>(p) : nullptr, stride = per_view ? (sN != 0 ? sN : count) : 0;
      };
      take(grad_light_dir, grad_light_dir_sN, 3, g.light, g.l_s);
      take(grad_shininess, grad_shininess_sN, 1, g.shininess, g.sh_s);
      take(grad_albedo, grad_albedo_sN, C, g.albedo, g.al_s);
      take(grad_ambient, grad_ambient_sN, C, g.ambient, g.am_s);
      take(grad_specular, grad_specular_sN, C, g.specular, g.sp_s);
      return g;
    };
    const ShadeParamGrads<T> per_view = pick(true), shared = pick(false);
    const bool any_shared =
        N > 1 && (shared.light || shared.shininess || shared.albedo || shared.ambient || shared.specular);
    DRTK_LAUNCH(
        shade_finalize_kernel<T>, dim3(static_cast<unsigned>(N)), dim3(kShadeFinalBlock), 0, s, rows, blocks, static_cast<int>(C),
        per_view, any_shared ? sums : nullptr);
    DRTK_RETURN_IF_LAUNCH_FAILED();
    if (any_shared) { // the views' sums, in the same fixed order
      DRTK_LAUNCH(
          shade_finalize_kernel<T>, dim3(1), dim3(kShadeFinalBlock), 0, s, sums, N, static_cast<int>(C), shared, nullptr);
      DRTK_RETURN_IF_LAUNCH_FAILED();
    }
    return DRTK_OK;
  });
}
