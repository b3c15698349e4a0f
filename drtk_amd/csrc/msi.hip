// msi -- multi-sphere-image background rendering (NeRF++ style), forward and backward.  A stack of L equirectangular
// RGB-sigma layers [L,4,H,W] sits on concentric spheres; one ray per pixel marches through them from the inside out and
// composites what it samples front to back.
//
// Reference: src/msi/msi_kernel.cu:18-409 (CUDA only).  Restated here, one lane per ray, 256-thread workgroups:
//   d = ray_d / |ray_d|, tc = -o.d, h2 = o.o - tc^2, n = L * sub_step_count, s = 1 / n
//   for i = 0 .. n-1:  a = (n - 1 - i + 0.5) / n, inv_r = (1 - a) max_inv_r + a min_inv_r, r = 1 / inv_r
//     det = r^2 - h2; det < 0: the ray misses this sphere, next i
//     pos = o + (tc + sqrt(det)) d;  u = atan2(pos.z, pos.x) / pi, v = 2 atan2(pos.y, |(pos.x, pos.z)|) / pi, w = 1 - 2a
//     sample(u, v, w): each coordinate unnormalised as ((c + 1) size - 1) / 2 and clipped to [0, size - 1] (grid_sample's
//       align_corners=False with border padding); bilinear in (x, y) -- the +1 neighbour of the last column / row has weight 0
//       and is not read --, cubic convolution (A = -0.75) over the layers floor(z) - 1 ... floor(z) + 2, each clipped to
//       [0, L - 1].  a, w and with them the four layers and their coefficients are the same for every ray of a step.
//       The texture is read in place: a tap is four loads H W apart, 64 scalar gathers per step.
//     sigma > 0:  p = sigma s, weight = exp(lt) (1 - exp(-p)), lt -= p, rgb_out += weight max(rgb, 0);
//                 exp(lt) < stop_thresh: lt = -1000, the ray ends
//   out = (rgb_out, lt)
// Non-finite rays sample a border texel (the clip maps NaN to 0): nothing is read or written out of range.
//
// Backward: a gradient for the texture only, grad_out[:, 3] is not read.  Each ray is marched again with g = grad_out[:, :3]
// and acc = g * out_rgb; at every sample that counts
//   colour gradient  [max(rgb, 0) == rgb] weight g        (a colour of exactly 0 passes its gradient on, as in the reference)
//   acc -= weight max(rgb, 0) g
//   sigma gradient   sum_ch( max(rgb, 0) g exp(-sigma) exp(lt_after) - acc )
// and the four values are added to the sixteen texels of the sample with the forward's weights: float atomics into a
// gradient this call has zero-filled, so the result is equal up to rounding from run to run, not bitwise (the reference's
// is atomic-ordered too).
// THE SIGMA GRADIENT IS THE REFERENCE'S EXPRESSION, NOT THE DERIVATIVE OF THE FORWARD.  With T = exp(lt_after) the
// derivative is  s * (ref + sum_ch max(rgb, 0) g T (1 - exp(-sigma))):  the reference leaves out the step size and writes
// exp(-sigma) where the forward has exp(-sigma s).  Kept as it is: what users of the reference trained against
// ("Multi-sphere background").
//
// Element types: float is the tuned path.  With a double texture the rays are promoted to double on load and everything
// -- the geometry too, which the reference keeps in float -- runs in double.
#include <type_traits>

#include "common.hpp"
#include "grid_coords.hpp"

namespace drtk_amd {
namespace {

// the sixteen taps of a sample: the north-west corner, whether its +1 neighbours exist, the bilinear weights (nw, ne, sw,
// se), the four layers and their cubic coefficients
template <typename T>
struct MsiTaps {
  int x0, y0;
  bool x1ok, y1ok;
  T wb[4];
  int layer[4];
  T co[4];
};

template <typename T>
__device__ __forceinline__ T msi_source(T c, int size) { // msi_kernel.cu:34-38; NaN -> 0, always inside [0, size - 1]
  return clip_plain(((c + T(1)) * T(size) - T(1)) / T(2), size);
}

template <typename T>
__device__ __forceinline__ void msi_taps(T u, T v, T w, int L, int H, int W, MsiTaps<T>& t) {
  const T x = msi_source(u, W), y = msi_source(v, H), z = msi_source(w, L);
  const T fx = floor(x), fy = floor(y), fz = floor(z);
  t.x0 = static_cast<int>(fx), t.y0 = static_cast<int>(fy);
  const int z0 = static_cast<int>(fz);
  t.x1ok = t.x0 + 1 < W, t.y1ok = t.y0 + 1 < H;
  const T wx0 = (fx + T(1)) - x, wx1 = x - fx, wy0 = (fy + T(1)) - y, wy1 = y - fy; // msi_kernel.cu:54-57
  t.wb[0] = wx0 * wy0, t.wb[1] = wx1 * wy0, t.wb[2] = wx0 * wy1, t.wb[3] = wx1 * wy1;
  cubic_coeffs(t.co, z - fz);
#pragma unroll
  for (int i = 0; i < 4; ++i) t.layer[i] = min(max(z0 - 1 + i, 0), L - 1);
}

// offset of texel (layer, y, x) of channel 0 in [L,4,H,W]; the channels are HW apart.  L * 4 * H * W < 2^31 (msi_validate).
__device__ __forceinline__ int msi_offset(int layer, int y, int x, int H, int W) {
  return (layer * 4 * H + y) * W + x;
}

template <typename T>
__device__ __forceinline__ void msi_sample(const T* __restrict__ tex, const MsiTaps<T>& t, int H, int W, T (&s)[4]) {
  const int HW = H * W;
#pragma unroll
  for (int c = 0; c < 4; ++c) s[c] = T(0);
#pragma unroll
  for (int i = 0; i < 4; ++i) {
    T a[4] = {T(0), T(0), T(0), T(0)};
#pragma unroll
    for (int k = 0; k < 4; ++k) {
      if (((k & 1) && !t.x1ok) || ((k & 2) && !t.y1ok)) continue;
      const T* p = tex + msi_offset(t.layer[i], t.y0 + (k >> 1), t.x0 + (k & 1), H, W);
#pragma unroll
      for (int c = 0; c < 4; ++c) a[c] = a[c] + p[c * HW] * t.wb[k];
    }
#pragma unroll
    for (int c = 0; c < 4; ++c) s[c] = s[c] + a[c] * t.co[i];
  }
}

// what a ray carries through the march
template <typename T>
struct MsiRay {
  T ox, oy, oz, dx, dy, dz, tc, h2;
};
template <typename T>
__device__ __forceinline__ MsiRay<T> msi_load_ray(const float* __restrict__ ray_o, const float* __restrict__ ray_d, int64_t ray) {
  MsiRay<T> r;
  r.ox = T(ray_o[3 * ray]), r.oy = T(ray_o[3 * ray + 1]), r.oz = T(ray_o[3 * ray + 2]);
  const T dx = T(ray_d[3 * ray]), dy = T(ray_d[3 * ray + 1]), dz = T(ray_d[3 * ray + 2]);
  const T len = sqrt(dx * dx + dy * dy + dz * dz);
  r.dx = dx / len, r.dy = dy / len, r.dz = dz / len;
  r.tc = -(r.ox * r.dx + r.oy * r.dy + r.oz * r.dz);
  r.h2 = (r.ox * r.ox + r.oy * r.oy + r.oz * r.oz) - r.tc * r.tc;
  return r;
}

// Step i of the march: false if the ray misses the sphere, else the taps of its sample.
template <typename T>
__device__ __forceinline__ bool msi_step(const MsiRay<T>& ray, int i, int n, double min_inv_r, double max_inv_r, int L, int H, int W, MsiTaps<T>& t) {
  const T a = (T(n - 1 - i) + T(0.5)) / T(n);
  // in double for float rays too, deliberately: the reference's mixed-precision expression (msi_kernel.cu:254-257; so is the
  // comparison of exp(lt) with stop_thresh in the kernels).  The same for every lane of a step.
  const T inv_r = static_cast<T>((1.0 - double(a)) * max_inv_r + double(a) * min_inv_r);
  const T r = T(1) / inv_r;
  const T det = r * r - ray.h2;
  if (det < T(0)) return false;
  const T tt = ray.tc + sqrt(det);
  const T px = tt * ray.dx + ray.ox, py = tt * ray.dy + ray.oy, pz = tt * ray.dz + ray.oz;
  constexpr T inv_pi = T(0.318309886183790671537767526745028724);
  const T u = atan2(pz, px) * inv_pi;
  const T v = (T(2) * atan2(py, sqrt(px * px + pz * pz))) * inv_pi;
  msi_taps<T>(u, v, T(1) - a * T(2), L, H, W, t);
  return true;
}

template <typename T>
__global__ __launch_bounds__(kBlock) void msi_forward_kernel(
    const float* __restrict__ ray_o, const float* __restrict__ ray_d, const T* __restrict__ tex, int64_t N, int L, int H, int W,
    int n, double min_inv_r, double max_inv_r, double stop_thresh, T* __restrict__ out) {
  const int64_t ray = int64_t(blockIdx.x) * kBlock + threadIdx.x;
  if (ray >= N) return;
  const MsiRay<T> r = msi_load_ray<T>(ray_o, ray_d, ray);
  const T step = T(1) / T(n);
  T o0 = T(0), o1 = T(0), o2 = T(0), lt = T(0);
  for (int i = 0; i < n; ++i) {
    MsiTaps<T> t;
    if (!msi_step<T>(r, i, n, min_inv_r, max_inv_r, L, H, W, t)) continue;
    T s[4];
    msi_sample<T>(tex, t, H, W, s);
    if (s[3] > T(0)) {
      const T p = s[3] * step;
      const T weight = exp(lt) * (T(1) - exp(-p));
      lt -= p;
      o0 = o0 + weight * (s[0] > T(0) ? s[0] : T(0));
      o1 = o1 + weight * (s[1] > T(0) ? s[1] : T(0));
      o2 = o2 + weight * (s[2] > T(0) ? s[2] : T(0));
      if (double(exp(lt)) < stop_thresh) {
        lt = T(-1000);
        break;
      }
    }
  }
  T* o = out + 4 * ray; // (element-aligned only: no vector store)
  o[0] = o0, o[1] = o1, o[2] = o2, o[3] = lt;
}

template <typename T>
__global__ __launch_bounds__(kBlock) void msi_backward_kernel(
    const T* __restrict__ grad_out, const T* __restrict__ fwd_out, const float* __restrict__ ray_o, const float* __restrict__ ray_d,
    const T* __restrict__ tex, int64_t N, int L, int H, int W, int n, double min_inv_r, double max_inv_r, double stop_thresh,
    T* __restrict__ grad_tex) {
  const int64_t ray = int64_t(blockIdx.x) * kBlock + threadIdx.x;
  if (ray >= N) return;
  const int HW = H * W;
  T g[3], acc[3];
#pragma unroll
  for (int c = 0; c < 3; ++c) g[c] = grad_out[4 * ray + c], acc[c] = g[c] * fwd_out[4 * ray + c];
  const MsiRay<T> r = msi_load_ray<T>(ray_o, ray_d, ray);
  const T step = T(1) / T(n);
  T lt = T(0);
  const GlobalPtr<T> gt = (GlobalPtr<T>)grad_tex;
  for (int i = 0; i < n; ++i) {
    MsiTaps<T> t;
    if (!msi_step<T>(r, i, n, min_inv_r, max_inv_r, L, H, W, t)) continue;
    T s[4];
    msi_sample<T>(tex, t, H, W, s);
    if (s[3] > T(0)) {
      const T p = s[3] * step;
      const T weight = exp(lt) * (T(1) - exp(-p));
      lt -= p;
      T g4[4]; // msi_kernel.cu:385-398
      const T e_sigma = exp(-s[3]), e_lt = exp(lt);
      T sum = T(0);
#pragma unroll
      for (int c = 0; c < 3; ++c) {
        const T rgb01 = s[c] > T(0) ? s[c] : T(0);
        g4[c] = (rgb01 == s[c] ? T(1) : T(0)) * weight * g[c];
        acc[c] -= weight * rgb01 * g[c];
        sum = sum + (rgb01 * g[c] * e_sigma * e_lt - acc[c]);
      }
      g4[3] = sum;
#pragma unroll
      for (int j = 0; j < 4; ++j) {
#pragma unroll
        for (int k = 0; k < 4; ++k) {
          if (((k & 1) && !t.x1ok) || ((k & 2) && !t.y1ok)) continue;
          const int at = msi_offset(t.layer[j], t.y0 + (k >> 1), t.x0 + (k & 1), H, W);
#pragma unroll
          for (int c = 0; c < 4; ++c) atomic_add_g1(gt + (at + c * HW), (t.wb[k] * g4[c]) * t.co[j]);
        }
      }
      if (double(e_lt) < stop_thresh) break;
    }
  }
}

int msi_validate(
    drtk_dtype_t dtype, int64_t N, int64_t L, int64_t H, int64_t W, int sub_step_count, double min_inv_r, double max_inv_r,
    double stop_thresh) {
  constexpr int64_t kLimit = int64_t(1) << 31;
  if (!valid_dtype(dtype)) return DRTK_ERR_INVALID_ARGUMENT;
  // (N counts rays, not views, and the whole texture is indexed in 31 bits, not one image: bounds of this file's own)
  if (N >= kLimit || L < 0 || L >= kLimit || H >= kLimit || W >= kLimit || bad_image(N, H, W)) return DRTK_ERR_INVALID_ARGUMENT;
  if (L * 4 * (H * W) >= kLimit) return DRTK_ERR_INVALID_ARGUMENT;
  if (sub_step_count < 1 || L * sub_step_count >= kLimit) return DRTK_ERR_INVALID_ARGUMENT;
  if (!(min_inv_r > max_inv_r) || !(stop_thresh > 0.0 && stop_thresh < 1.0)) return DRTK_ERR_INVALID_ARGUMENT; // (NaN fails too)
  return DRTK_OK;
}

} // namespace
} // namespace drtk_amd

using namespace drtk_amd;

extern "C" int drtk_amd_msi_forward(
    drtk_dtype_t dtype, const float* ray_o, const float* ray_d, const void* texture, int64_t N, int64_t L, int64_t H, int64_t W,
    int sub_step_count, double min_inv_r, double max_inv_r, double stop_thresh, void* out, drtk_stream_t stream) {
  const int st = msi_validate(dtype, N, L, H, W, sub_step_count, min_inv_r, max_inv_r, stop_thresh);
  if (st != DRTK_OK) return st;
  if (N == 0) return DRTK_OK;
  if (L == 0 || H == 0 || W == 0 || !ray_o || !ray_d || !texture || !out) return DRTK_ERR_INVALID_ARGUMENT;
  hipStream_t s = static_cast<hipStream_t>(stream);
  const dim3 grid_dim(static_cast<unsigned>(ceil_div(N, kBlock)));
  const int n = static_cast<int>(L * sub_step_count);
  return dispatch_dtype(dtype, [&](auto tag) {
    using T = decltype(tag);
    DRTK_LAUNCH(
        (msi_forward_kernel<T>), grid_dim, dim3(kBlock), 0, s, ray_o, ray_d, static_cast<const T*>(texture), N, (int)L, (int)H, (int)W, n,
        min_inv_r, max_inv_r, stop_thresh, static_cast<T*>(out));
    DRTK_RETURN_IF_LAUNCH_FAILED();
    return DRTK_OK;
  });
}

extern "C" int drtk_amd_msi_backward(
    drtk_dtype_t dtype, const void* grad_out, const void* out, const float* ray_o, const float* ray_d, const void* texture,
    int64_t N, int64_t L, int64_t H, int64_t W, int sub_step_count, double min_inv_r, double max_inv_r, double stop_thresh,
    void* grad_texture, drtk_stream_t stream) {
  const int st = msi_validate(dtype, N, L, H, W, sub_step_count, min_inv_r, max_inv_r, stop_thresh);
  if (st != DRTK_OK) return st;
  const int64_t texels = L * 4 * H * W;
  if (texels > 0 && !grad_texture) return DRTK_ERR_INVALID_ARGUMENT;
  if (N > 0 && (texels == 0 || !grad_out || !out || !ray_o || !ray_d || !texture)) return DRTK_ERR_INVALID_ARGUMENT;
  hipStream_t s = static_cast<hipStream_t>(stream);
  if (texels > 0 && fill_bytes_async(grad_texture, 0, dtype_size(dtype) * size_t(texels), s) != DRTK_OK) return DRTK_ERR_LAUNCH;
  if (N == 0) return DRTK_OK;
  const dim3 grid_dim(static_cast<unsigned>(ceil_div(N, kBlock)));
  const int n = static_cast<int>(L * sub_step_count);
  return dispatch_dtype(dtype, [&](auto tag) {
    using T = decltype(tag);
    DRTK_LAUNCH(
        (msi_backward_kernel<T>), grid_dim, dim3(kBlock), 0, s, static_cast<const T*>(grad_out), static_cast<const T*>(out), ray_o, ray_d,
        static_cast<const T*>(texture), N, (int)L, (int)H, (int)W, n, min_inv_r, max_inv_r, stop_thresh, static_cast<T*>(grad_texture));
    DRTK_RETURN_IF_LAUNCH_FAILED();
    return DRTK_OK;
  });
}
