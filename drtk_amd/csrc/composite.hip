// composite_layers -- front-to-back compositing of the K <= 8 layers of rasterize_layers, forward and backward, one
// streaming kernel each way (no reference counterpart: the reference stops at one layer).
//
// Definition, per pixel, in the tensors' own type and with exactly these operations in this order (the library is built
// with -ffp-contract=off, so the forward is the loop's result bit for bit):
//   img = 0, T = 1
//   for k = 0 .. K-1 (layer 0 is nearest):  a = alpha[k]          -- a layer whose index is -1 is SKIPPED: nothing of it is read
//     img[c] = img[c] + (T * a) * color[k][c];   T = T * (1 - a)
//   img[c] = img[c] + T * background[c]                           -- if there is a background
//   out = (img [N,C,H,W], T [N,1,H,W])
// Once T is exactly 0 the colours of the layers behind are not read (they would add (0 * a) * color = 0).
//
// Backward, division-free and back to front (exact at alpha == 1, where T_{k+1} / (1 - a_k) is 0 / 0).  With T_k the
// transmittance in front of layer k, a_k the alpha (0 where skipped), g = grad_img, d_k = sum_c color[k][c] g[c]:
//   R_K = grad_T + sum_c background[c] g[c]          (absent terms are 0)
//   k = K-1 .. 0:  grad_alpha[k] = T_k (d_k - R_{k+1});  R_k = a_k d_k + (1 - a_k) R_{k+1}
//   grad_color[k][c] = (T_k a_k) g[c];  grad_background[c] = T_K g[c]
// R_{k+1} is the derivative of the loss with respect to "what is seen through layer k", so the alpha gradient of an opaque
// layer needs the colours BEHIND it: the backward reads every layer that is present, whatever T.
//
// Layout: every H x W plane is contiguous; color and alpha (and their gradients) come with element strides for view, layer
// and channel, so split tensors, one [N,K,C+1,H,W] rgba tensor and channel slices of it are all read and written in place.
// One lane owns P consecutive pixels of one view (P * sizeof(T) = 16 bytes where the registers allow, see kPix below) and
// moves each plane's share as one element-aligned vector; the last lane of a plane whose pixel count is no multiple of P
// goes pixel by pixel.  K is a template parameter: T_k, a_k and d_k live in registers; C is a run-time loop.  The backward
// makes two sweeps over the channels -- d_k (colours read once), then, after the K-step recurrence, the gradient writes
// (grad_img read again rather than held) -- and writes every gradient element once, zeros at skipped layers included.
// No atomics, no LDS: bitwise reproducible.
#include "common.hpp"

namespace drtk_amd {
namespace {

template <typename T>
struct CompositeArgs {
  const T* color;
  int64_t c_sN, c_sK, c_sC;
  const T* alpha;
  int64_t a_sN, a_sK;
  const int32_t* index; // [N,K,H,W] contiguous, or NULL: every layer present
  const T* bg;          // [N,C,H,W] with view stride bg_sN (0: one background for all views), or NULL
  int64_t bg_sN;
  int64_t HW;
  int C;
  int strip;
  // forward
  T* img;   // [N,C,H,W]
  T* trans; // [N,1,H,W]
  // backward
  const T* g_img; // [N,C,H,W] or NULL
  const T* g_T;   // [N,1,H,W] or NULL
  T* g_color;     // or NULL
  int64_t gc_sN, gc_sK, gc_sC;
  T* g_alpha; // or NULL
  int64_t ga_sN, ga_sK;
  T* g_bg; // [N,C,H,W] or NULL
};

// Pixels per lane.  Forward: 16 bytes (the K weights and the K colour vectors of a channel in flight are 2 K P values).
// Backward: T_k, a_k, d_k and the colour vectors in flight are 4 K P values -- 16 bytes up to K = 4, 8 bytes beyond, which
// keeps K = 8 at 64 of them like K = 4 (DESIGN.md section 16 has the register counts).
template <typename T, int K, bool BACKWARD>
constexpr int kPix = (16 / int(sizeof(T))) / ((BACKWARD && K > 4) ? 2 : 1);

template <typename E, int P>
struct VecOf {
  typedef E type __attribute__((ext_vector_type(P), aligned(sizeof(E))));
};

// P consecutive elements at p: one element-aligned vector access when all P belong to the plane, else the first `rem`.
template <typename E, int P>
__device__ __forceinline__ void load_px(const E* __restrict__ p, int rem, E fill, E (&v)[P]) {
  if constexpr (P == 1) {
    v[0] = p[0];
  } else {
    if (rem == P) {
      const typename VecOf<E, P>::type q = *reinterpret_cast<const typename VecOf<E, P>::type*>(p);
#pragma unroll
      for (int j = 0; j < P; ++j) v[j] = q[j];
    } else {
#pragma unroll
      for (int j = 0; j < P; ++j) v[j] = j < rem ? p[j] : fill;
    }
  }
}
template <typename E, int P>
__device__ __forceinline__ void store_px(E* __restrict__ p, int rem, const E (&v)[P]) {
  if constexpr (P == 1) {
    p[0] = v[0];
  } else {
    if (rem == P) {
      typename VecOf<E, P>::type q;
#pragma unroll
      for (int j = 0; j < P; ++j) q[j] = v[j];
      *reinterpret_cast<typename VecOf<E, P>::type*>(p) = q;
    } else {
#pragma unroll
      for (int j = 0; j < P; ++j) {
        if (j < rem) p[j] = v[j];
      }
    }
  }
}

// What both passes start with: which of the lane's K x P (layer, pixel) pairs are present -- bit k * P + j of the result --
// their alphas (0 where absent) and the transmittance in front of every layer; t ends as T_K.
template <typename T, int K, int P>
__device__ __forceinline__ unsigned composite_front(
    const CompositeArgs<T>& a, int n, int64_t pix0, int rem, T (&al)[K][P], T (&tk)[K][P], T (&t)[P]) {
  constexpr unsigned kLane = (1u << P) - 1u;
  unsigned present = 0;
  if (a.index) {
    const int32_t* ip = a.index + (int64_t(n) * K) * a.HW + pix0;
    int32_t id[K][P];
#pragma unroll
    for (int k = 0; k < K; ++k) load_px<int32_t, P>(ip + k * a.HW, rem, -1, id[k]);
#pragma unroll
    for (int k = 0; k < K; ++k) {
#pragma unroll
      for (int j = 0; j < P; ++j) present |= (id[k][j] != -1 ? 1u : 0u) << (k * P + j);
    }
  } else {
#pragma unroll
    for (int k = 0; k < K; ++k) present |= ((1u << rem) - 1u) << (k * P);
  }
  const T* ap = a.alpha + int64_t(n) * a.a_sN + pix0;
#pragma unroll
  for (int k = 0; k < K; ++k) {
#pragma unroll
    for (int j = 0; j < P; ++j) al[k][j] = T(0);
    if ((present >> (k * P)) & kLane) load_px<T, P>(ap + k * a.a_sK, rem, T(0), al[k]);
  }
#pragma unroll
  for (int j = 0; j < P; ++j) t[j] = T(1);
#pragma unroll
  for (int k = 0; k < K; ++k) {
#pragma unroll
    for (int j = 0; j < P; ++j) {
      const bool on = (present >> (k * P + j)) & 1u;
      al[k][j] = on ? al[k][j] : T(0); // (a NaN next to a present pixel was loaded with it)
      tk[k][j] = t[j];
      t[j] = on ? t[j] * (T(1) - al[k][j]) : t[j];
    }
  }
  return present;
}

template <typename T, int K>
__global__ __launch_bounds__(kBlock) void composite_forward_kernel(const CompositeArgs<T> a) {
  constexpr int P = kPix<T, K, false>;
  constexpr unsigned kLane = (1u << P) - 1u;
  const int64_t pix0 = (int64_t(tile_index(a.strip)) * kBlock + threadIdx.x) * P;
  if (pix0 >= a.HW) return;
  const int n = blockIdx.y;
  const int rem = a.HW - pix0 < P ? static_cast<int>(a.HW - pix0) : P;
  T w[K][P], tk[K][P], t[P];
  const unsigned present = composite_front<T, K, P>(a, n, pix0, rem, w, tk, t);
  unsigned live = 0; // present, and something still shows through the layers in front
#pragma unroll
  for (int k = 0; k < K; ++k) {
#pragma unroll
    for (int j = 0; j < P; ++j) {
      const bool on = ((present >> (k * P + j)) & 1u) && tk[k][j] != T(0);
      live |= (on ? 1u : 0u) << (k * P + j);
      w[k][j] = tk[k][j] * w[k][j];
    }
  }
  store_px<T, P>(a.trans + int64_t(n) * a.HW + pix0, rem, t);
  const T* cp = a.color + int64_t(n) * a.c_sN + pix0;
  const T* bp = a.bg ? a.bg + int64_t(n) * a.bg_sN + pix0 : nullptr;
  T* op = a.img + (int64_t(n) * a.C) * a.HW + pix0;
  for (int c = 0; c < a.C; ++c) {
    T q[K][P], b[P];
    // the loads of a channel go out as one batch, the arithmetic follows
#pragma unroll
    for (int k = 0; k < K; ++k) {
#pragma unroll
      for (int j = 0; j < P; ++j) q[k][j] = T(0);
      if ((live >> (k * P)) & kLane) load_px<T, P>(cp + k * a.c_sK + c * a.c_sC, rem, T(0), q[k]);
    }
    if (bp) load_px<T, P>(bp + c * a.HW, rem, T(0), b);
    T acc[P];
#pragma unroll
    for (int j = 0; j < P; ++j) acc[j] = T(0);
#pragma unroll
    for (int k = 0; k < K; ++k) {
#pragma unroll
      for (int j = 0; j < P; ++j) acc[j] = ((live >> (k * P + j)) & 1u) ? acc[j] + w[k][j] * q[k][j] : acc[j];
    }
    if (bp) {
#pragma unroll
      for (int j = 0; j < P; ++j) acc[j] = acc[j] + t[j] * b[j];
    }
    store_px<T, P>(op + c * a.HW, rem, acc);
  }
}

template <typename T, int K>
__global__ __launch_bounds__(kBlock) void composite_backward_kernel(const CompositeArgs<T> a) {
  constexpr int P = kPix<T, K, true>;
  constexpr unsigned kLane = (1u << P) - 1u;
  const int64_t pix0 = (int64_t(tile_index(a.strip)) * kBlock + threadIdx.x) * P;
  if (pix0 >= a.HW) return;
  const int n = blockIdx.y;
  const int rem = a.HW - pix0 < P ? static_cast<int>(a.HW - pix0) : P;
  T al[K][P], tk[K][P], t[P];
  const unsigned present = composite_front<T, K, P>(a, n, pix0, rem, al, tk, t);
  const T* gp = a.g_img ? a.g_img + (int64_t(n) * a.C) * a.HW + pix0 : nullptr;

  if (a.g_alpha) {
    // sweep 1, front to back over the colours: d_k, and the background's share of R_K
    T d[K][P], r[P];
#pragma unroll
    for (int k = 0; k < K; ++k) {
#pragma unroll
      for (int j = 0; j < P; ++j) d[k][j] = T(0);
    }
#pragma unroll
    for (int j = 0; j < P; ++j) r[j] = T(0);
    if (gp) {
      const T* cp = a.color + int64_t(n) * a.c_sN + pix0;
      const T* bp = a.bg ? a.bg + int64_t(n) * a.bg_sN + pix0 : nullptr;
      for (int c = 0; c < a.C; ++c) {
        T q[K][P], g[P], b[P];
        load_px<T, P>(gp + c * a.HW, rem, T(0), g);
#pragma unroll
        for (int k = 0; k < K; ++k) {
#pragma unroll
          for (int j = 0; j < P; ++j) q[k][j] = T(0);
          if ((present >> (k * P)) & kLane) load_px<T, P>(cp + k * a.c_sK + c * a.c_sC, rem, T(0), q[k]);
        }
        if (bp) {
          load_px<T, P>(bp + c * a.HW, rem, T(0), b);
#pragma unroll
          for (int j = 0; j < P; ++j) r[j] = r[j] + b[j] * g[j];
        }
#pragma unroll
        for (int k = 0; k < K; ++k) {
#pragma unroll
          for (int j = 0; j < P; ++j) d[k][j] = ((present >> (k * P + j)) & 1u) ? d[k][j] + q[k][j] * g[j] : d[k][j];
        }
      }
    }
    if (a.g_T) {
      T gt[P];
      load_px<T, P>(a.g_T + int64_t(n) * a.HW + pix0, rem, T(0), gt);
#pragma unroll
      for (int j = 0; j < P; ++j) r[j] = gt[j] + r[j];
    }
    // the recurrence, back to front
    T* ap = a.g_alpha + int64_t(n) * a.ga_sN + pix0;
#pragma unroll
    for (int k = K - 1; k >= 0; --k) {
      T ga[P];
#pragma unroll
      for (int j = 0; j < P; ++j) {
        const bool on = (present >> (k * P + j)) & 1u;
        ga[j] = on ? tk[k][j] * (d[k][j] - r[j]) : T(0);
        r[j] = on ? al[k][j] * d[k][j] + (T(1) - al[k][j]) * r[j] : r[j];
      }
      store_px<T, P>(ap + k * a.ga_sK, rem, ga);
    }
  }

  if (!a.g_color && !a.g_bg) return;
  // sweep 2: the colour and background gradients, grad_img read again
#pragma unroll
  for (int k = 0; k < K; ++k) {
#pragma unroll
    for (int j = 0; j < P; ++j) tk[k][j] = tk[k][j] * al[k][j];
  }
  T* gcp = a.g_color ? a.g_color + int64_t(n) * a.gc_sN + pix0 : nullptr;
  T* gbp = a.g_bg ? a.g_bg + (int64_t(n) * a.C) * a.HW + pix0 : nullptr;
  for (int c = 0; c < a.C; ++c) {
    T g[P];
#pragma unroll
    for (int j = 0; j < P; ++j) g[j] = T(0);
    if (gp) load_px<T, P>(gp + c * a.HW, rem, T(0), g);
    if (gcp) {
#pragma unroll
      for (int k = 0; k < K; ++k) {
        T o[P];
#pragma unroll
        for (int j = 0; j < P; ++j) o[j] = ((present >> (k * P + j)) & 1u) ? tk[k][j] * g[j] : T(0);
        store_px<T, P>(gcp + k * a.gc_sK + c * a.gc_sC, rem, o);
      }
    }
    if (gbp) {
      T o[P];
#pragma unroll
      for (int j = 0; j < P; ++j) o[j] = t[j] * g[j];
      store_px<T, P>(gbp + c * a.HW, rem, o);
    }
  }
}

int composite_validate(drtk_dtype_t dtype, int64_t N, int64_t K, int64_t C, int64_t H, int64_t W) {
  constexpr int64_t kLimit = int64_t(1) << 31;
  if (!valid_dtype(dtype)) return DRTK_ERR_INVALID_ARGUMENT;
  // (H and W also one by one: an empty image of 2^31 rows is invalid here)
  if (C < 0 || C >= kLimit || H >= kLimit || W >= kLimit || bad_image(N, H, W)) return DRTK_ERR_INVALID_ARGUMENT;
  if (K < 1 || K > DRTK_AMD_MAX_RASTER_LAYERS) return DRTK_ERR_INVALID_ARGUMENT;
  if (N > 0 && H * W > 0 && C < 1) return DRTK_ERR_INVALID_ARGUMENT;
  return DRTK_OK;
}

bool strides_ok(const int64_t* s, int count) {
  if (!s) return false;
  for (int i = 0; i < count; ++i) {
    if (s[i] < 0) return false;
  }
  return true;
}

template <typename T, bool BACKWARD>
void composite_launch(const CompositeArgs<T>& args, int K, int64_t N, int64_t W, hipStream_t s) {
#define COMPOSITE_CASE(KK)                                                                                         \
  case KK: {                                                                                                       \
    constexpr int P = kPix<T, KK, BACKWARD>;                                                                       \
    CompositeArgs<T> a = args;                                                                                     \
    a.strip = xcd_strip(ceil_div(16 * W, int64_t(kBlock) * P));                                                    \
    const dim3 grid(static_cast<unsigned>(ceil_div(a.HW, int64_t(kBlock) * P)), static_cast<unsigned>(N));         \
    if constexpr (BACKWARD) {                                                                                      \
      DRTK_LAUNCH((composite_backward_kernel<T, KK>), grid, dim3(kBlock), 0, s, a);                                \
    } else {                                                                                                       \
      DRTK_LAUNCH((composite_forward_kernel<T, KK>), grid, dim3(kBlock), 0, s, a);                                 \
    }                                                                                                              \
  } break;
  switch (K) {
    COMPOSITE_CASE(1)
    COMPOSITE_CASE(2)
    COMPOSITE_CASE(3)
    COMPOSITE_CASE(4)
    COMPOSITE_CASE(5)
    COMPOSITE_CASE(6)
    COMPOSITE_CASE(7)
    COMPOSITE_CASE(8)
  }
#undef COMPOSITE_CASE
}

template <typename T>
CompositeArgs<T> composite_inputs(
    const void* color, const int64_t* cs, const void* alpha, const int64_t* as, const int32_t* index_img, const void* background,
    int64_t background_sN, int64_t C, int64_t HW) {
  CompositeArgs<T> a = {};
  a.color = static_cast<const T*>(color), a.c_sN = cs[0], a.c_sK = cs[1], a.c_sC = cs[2];
  a.alpha = static_cast<const T*>(alpha), a.a_sN = as[0], a.a_sK = as[1];
  a.index = index_img;
  a.bg = static_cast<const T*>(background), a.bg_sN = background_sN;
  a.HW = HW, a.C = static_cast<int>(C), a.strip = 1;
  return a;
}

} // namespace
} // namespace drtk_amd

using namespace drtk_amd;

extern "C" int drtk_amd_composite_layers(
    drtk_dtype_t dtype, const void* color, const int64_t* color_strides, const void* alpha, const int64_t* alpha_strides,
    const int32_t* index_img, const void* background, int64_t background_sN, int64_t N, int64_t K, int64_t C, int64_t H, int64_t W,
    void* img, void* transmittance, drtk_stream_t stream) {
  const int st = composite_validate(dtype, N, K, C, H, W);
  if (st != DRTK_OK) return st;
  if (N == 0 || H * W == 0) return DRTK_OK;
  if (!color || !alpha || !img || !transmittance || !strides_ok(color_strides, 3) || !strides_ok(alpha_strides, 2) || background_sN < 0)
    return DRTK_ERR_INVALID_ARGUMENT;
  const size_t es = dtype_size(dtype);
  if (N > kMaxViewsPerLaunch) return for_view_slices(N, [&](int64_t n0, int64_t n) {
    return drtk_amd_composite_layers(
        dtype, advance(color, n0 * color_strides[0], es), color_strides, advance(alpha, n0 * alpha_strides[0], es), alpha_strides,
        advance_typed(index_img, n0 * K * H * W), advance(background, n0 * background_sN, es), background_sN, n, K, C, H, W,
        advance(img, n0 * C * H * W, es), advance(transmittance, n0 * H * W, es), stream);
  });
  return dispatch_dtype(dtype, [&](auto tag) {
    using T = decltype(tag);
    auto a = composite_inputs<T>(color, color_strides, alpha, alpha_strides, index_img, background, background_sN, C, H * W);
    a.img = static_cast<T*>(img), a.trans = static_cast<T*>(transmittance);
    composite_launch<T, false>(a, static_cast<int>(K), N, W, static_cast<hipStream_t>(stream));
    DRTK_RETURN_IF_LAUNCH_FAILED();
    return DRTK_OK;
  });
}

extern "C" int drtk_amd_composite_layers_backward(
    drtk_dtype_t dtype, const void* grad_img, const void* grad_transmittance, const void* color, const int64_t* color_strides,
    const void* alpha, const int64_t* alpha_strides, const int32_t* index_img, const void* background, int64_t background_sN,
    int64_t N, int64_t K, int64_t C, int64_t H, int64_t W, void* grad_color, const int64_t* grad_color_strides, void* grad_alpha,
    const int64_t* grad_alpha_strides, void* grad_background, drtk_stream_t stream) {
  const int st = composite_validate(dtype, N, K, C, H, W);
  if (st != DRTK_OK) return st;
  if (N == 0 || H * W == 0) return DRTK_OK;
  if (!color || !alpha || !strides_ok(color_strides, 3) || !strides_ok(alpha_strides, 2) || background_sN < 0)
    return DRTK_ERR_INVALID_ARGUMENT;
  if ((grad_color && !strides_ok(grad_color_strides, 3)) || (grad_alpha && !strides_ok(grad_alpha_strides, 2)))
    return DRTK_ERR_INVALID_ARGUMENT;
  if (grad_background && !background) return DRTK_ERR_INVALID_ARGUMENT;
  if (!grad_color && !grad_alpha && !grad_background) return DRTK_OK; // nothing is wanted
  const size_t es = dtype_size(dtype);
  if (N > kMaxViewsPerLaunch) return for_view_slices(N, [&](int64_t n0, int64_t n) {
    return drtk_amd_composite_layers_backward(
        dtype, advance(grad_img, n0 * C * H * W, es), advance(grad_transmittance, n0 * H * W, es),
        advance(color, n0 * color_strides[0], es), color_strides, advance(alpha, n0 * alpha_strides[0], es), alpha_strides,
        advance_typed(index_img, n0 * K * H * W), advance(background, n0 * background_sN, es), background_sN, n, K, C, H, W,
        advance(grad_color, grad_color ? n0 * grad_color_strides[0] : 0, es), grad_color_strides,
        advance(grad_alpha, grad_alpha ? n0 * grad_alpha_strides[0] : 0, es), grad_alpha_strides,
        advance(grad_background, n0 * C * H * W, es), stream);
  });
  return dispatch_dtype(dtype, [&](auto tag) {
    using T = decltype(tag);
    auto a = composite_inputs<T>(color, color_strides, alpha, alpha_strides, index_img, background, background_sN, C, H * W);
    a.g_img = static_cast<const T*>(grad_img), a.g_T = static_cast<const T*>(grad_transmittance);
    a.g_color = static_cast<T*>(grad_color), a.g_alpha = static_cast<T*>(grad_alpha), a.g_bg = static_cast<T*>(grad_background);
    if (grad_color) a.gc_sN = grad_color_strides[0], a.gc_sK = grad_color_strides[1], a.gc_sC = grad_color_strides[2];
    if (grad_alpha) a.ga_sN = grad_alpha_strides[0], a.ga_sK = grad_alpha_strides[1];
    composite_launch<T, true>(a, static_cast<int>(K), N, W, static_cast<hipStream_t>(stream));
    DRTK_RETURN_IF_LAUNCH_FAILED();
    return DRTK_OK;
  });
}
