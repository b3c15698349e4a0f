// filter2d -- fused separable up/down-sampling FIR filters on [planes, H, W] images: zero-insertion by `up`, a k-tap 1-D
// filter along both axes, decimation by `down`, in ONE pass over memory (each input read once per tile, each output written
// once; neither the zero-stuffed image nor the result of the first pass ever exists in memory).
//
// Reference: src/filter2d/filter2d_kernel.cu (CUDA), restated per axis (the operator is separable; both axes use the same
// k, up, down):
//   pad0(k, up, down) = k / 2 if up == down == 1, (k - down + 1) / 2 if down != 1, else (k + up - 1) / 2
//   pad1(k, up, down) = (k - 1) / 2         |  (k - down) / 2                 |     (k - up) / 2        (floor divisions)
//   total = pad0 + pad1,  out = (in * up + total - k + down) / down
//   forward:        lead = pad0(k, up, down),                  F[j] = f[k - 1 - j]
//   `backward` set: lead = k - 1 - pad0(k, up = down, down = up), F[j] = f[j]   (the call is the gradient of that operator)
//   y[o] = sum_j Z[o * down + j - lead] F[j],  Z[u] = X[u / up] if up divides u, else 0
//   X[p] outside 0 .. n - 1: 0 (zeros) or one reflection that does not repeat the edge, p <- |p|, p <- (n - 1) - |n - 1 - p|.
// Gather form, what the kernel evaluates:  u = o * down + up - 1 - lead, i0 = floor(u / up), phase = (i0 + 1) up - u - 1,
//   y[o] = sum_t X[i0 + t] F[phase + t up]  while phase + t up < k,  t ascending, every product and sum rounded on its own.
// The horizontal pass runs first; its result stays in the accumulation type (float for half and float images, double for
// double) and is not rounded to the storage type before the vertical pass.
//
// UNDER REFLECTION THE `backward` CALL IS THE REFERENCE'S EXPRESSION, NOT THE DERIVATIVE OF THE FORWARD: within a filter's
// reach of the border the reference reflects the incoming gradient instead of folding the border contributions back.  Kept
// as it is ("Resampling filters"); with zeros padding the call is the exact adjoint.
//
// One 256-thread workgroup per tile of tow x toh outputs of one plane (f2d_plan):
//   1. the input tile with its halo -> LDS, borders resolved here (a reflected index, or a zero);
//   2. horizontal pass, LDS -> LDS: a wave per input row, a lane per output column (tow = 64; several rows per wave below);
//   3. vertical pass, LDS -> global: a wave per output row, a lane per output column.
// Passes 2 and 3 run over the whole tile without bounds tests -- lanes and rows past the image compute on LDS nobody
// filled, inside the allocation -- and only the store looks at the image size.  No workspace, no atomics: bitwise the
// same from run to run.
// The tuned instantiations know (up, down, k) at compile time and unroll the taps: with up == 1 they sit in registers and
// the input tile is stored de-interleaved by `down` (column c in plane c % down at c / down), so that consecutive lanes of
// pass 2 read consecutive dwords whatever `down` is; with up > 1 each lane keeps the k / up taps of its phase.  The generic
// instantiation takes the three numbers at run time and covers everything else, limited by LDS only.
#include <type_traits>

#include "common.hpp"

namespace drtk_amd {
namespace {

constexpr int kMaxTowShift = 6;         // a tile is at most 64 outputs wide: one wave across
constexpr size_t kLdsPerCu = 160 * 1024;

using half_t = _Float16; // storage only: loaded into, and stored from, float

template <typename T>
struct F2dAcc {
  using type = float;
};
template <>
struct F2dAcc<double> {
  using type = double;
};

struct F2dArgs {
  int H, W, OH, OW;          // one plane
  int k, up, down;           // (the tuned instantiations use their template arguments instead)
  int lead, tmax;            // tmax = ceil(k / up): the most taps an output has
  int reflect, reversed;     // reversed: F[j] = f[k - 1 - j]
  int tow_shift, toh;        // a tile is (1 << tow_shift) x toh outputs; narrower than a wave, a wave takes several rows at a time
  int tiles_x, tiles_y;
  int plane_w, si, ih_max;   // input tile in LDS: width of a de-interleaved plane, row stride, rows (of both LDS arrays)
  int sm;                    // row stride of the pass-2 result
};

__host__ __device__ inline int f2d_floor_div(int a, int b) {
  const int q = a / b;
  return (a % b != 0 && a < 0) ? q - 1 : q;
}

// Where X[p] of an axis of n elements is read from; -1: it is a zero.  The clamp is never active for an index a valid
// output needs (filter2d_validate: one reflection suffices); it only keeps everything else inside the image too.
__host__ __device__ inline int f2d_source(int p, int n, bool reflect) {
  if (!reflect) return (p < 0 || p >= n) ? -1 : p;
  p = p < 0 ? -p : p;
  int d = n - 1 - p;
  d = d < 0 ? -d : d;
  p = n - 1 - d;
  return p < 0 ? 0 : p;
}

// The three passes of one workgroup, as a function of (block, thread, pass) so that a host loop over the threads can stand
// in for the workgroup (how the index arithmetic was checked against the restatement above before it first ran on a GPU).
template <typename T, int UP, int DOWN, int K>
__host__ __device__ __forceinline__ void filter2d_pass(
    int pass, int block, int thread, const T* __restrict__ x, const float* __restrict__ f, T* __restrict__ y, const F2dArgs& a,
    unsigned char* lds) {
  using A = typename F2dAcc<T>::type;
  constexpr bool kTuned = K > 0;
  constexpr bool kRegTaps = kTuned && UP == 1;              // every output has the same K taps: registers
  constexpr int D = (kRegTaps && DOWN > 1) ? DOWN : 1;      // de-interleave factor of the input tile
  static_assert(!kTuned || UP == 1 || (DOWN == 1 && K % (UP > 0 ? UP : 1) == 0), "tuned: k is a multiple of up");
  const int up = kTuned ? UP : a.up, down = kTuned ? DOWN : a.down, k = kTuned ? K : a.k;
  A* __restrict__ s_in = reinterpret_cast<A*>(lds);
  A* __restrict__ s_mid = s_in + a.ih_max * a.si;
  A* __restrict__ s_f = s_mid + a.ih_max * a.sm;
  const int lane = thread & (kWave - 1), wave = thread / kWave;
  constexpr int kWaves = kBlock / kWave;
  // passes 2 and 3: a lane's column of the tile, and its row among the rows its wave takes at a time
  const int tow = 1 << a.tow_shift, col_l = lane & (tow - 1), rows_at_once = kWave >> a.tow_shift;
  const int row_first = wave * rows_at_once + (lane >> a.tow_shift), row_step = kWaves * rows_at_once;

  const int tiles = a.tiles_x * a.tiles_y;
  const int plane = block / tiles;
  const int tile = block - plane * tiles;
  const int ty = tile / a.tiles_x, tx = tile - ty * a.tiles_x;
  const int ox0 = tx * tow, oy0 = ty * a.toh;
  const int nox = a.OW - ox0 < tow ? a.OW - ox0 : tow, noy = a.OH - oy0 < a.toh ? a.OH - oy0 : a.toh;
  const int shift = up - 1 - a.lead;
  const int ix0 = f2d_floor_div(ox0 * down + shift, up), iy0 = f2d_floor_div(oy0 * down + shift, up);
  // what the tile's outputs inside the image read
  const int iw = f2d_floor_div((ox0 + nox - 1) * down + shift, up) + a.tmax - ix0;
  const int ih = f2d_floor_div((oy0 + noy - 1) * down + shift, up) + a.tmax - iy0;

  if (pass == 0) {
    const T* __restrict__ xp = x + int64_t(plane) * a.H * a.W;
    if (!kRegTaps) {
      for (int j = thread; j < k; j += kBlock) s_f[j] = A(f[a.reversed ? k - 1 - j : j]);
    }
    for (int r = wave; r < ih; r += kWaves) {
      const int py = f2d_source(iy0 + r, a.H, a.reflect != 0);
      A* __restrict__ row = s_in + r * a.si;
      for (int c = lane; c < iw; c += kWave) {
        const int px = f2d_source(ix0 + c, a.W, a.reflect != 0);
        A v = A(0);
        if (py >= 0 && px >= 0) v = A(xp[py * a.W + px]);
        row[D == 1 ? c : (c % D) * a.plane_w + c / D] = v;
      }
    }
    return;
  }

  if constexpr (kRegTaps) {
    A taps[K]; // wave-uniform: scalar loads
#pragma unroll
    for (int j = 0; j < K; ++j) taps[j] = A(f[a.reversed ? K - 1 - j : j]);
    if (pass == 1) {
      for (int r = row_first; r < ih; r += row_step) {
        const A* __restrict__ row = s_in + r * a.si + col_l; // column col_l * DOWN + t
        A acc = A(0);
#pragma unroll
        for (int t = 0; t < K; ++t) acc = acc + row[(t % D) * a.plane_w + t / D] * taps[t];
        s_mid[r * a.sm + col_l] = acc;
      }
    } else {
      T* __restrict__ yp = y + int64_t(plane) * a.OH * a.OW;
      for (int oy = row_first; oy < noy; oy += row_step) {
        const A* __restrict__ col = s_mid + oy * DOWN * a.sm + col_l;
        A acc = A(0);
#pragma unroll
        for (int t = 0; t < K; ++t) acc = acc + col[t * a.sm] * taps[t];
        if (col_l < nox) yp[(oy0 + oy) * a.OW + ox0 + col_l] = T(acc);
      }
    }
  } else {
    if (pass == 1) {
      const int u = (ox0 + col_l) * down + shift;
      const int i0 = f2d_floor_div(u, up);
      const int phase = (i0 + 1) * up - u - 1;
      const A* __restrict__ first = s_in + (i0 - ix0);
      if constexpr (kTuned) {
        constexpr int NT = K / (UP > 0 ? UP : 1);
        A taps[NT];
#pragma unroll
        for (int t = 0; t < NT; ++t) taps[t] = s_f[phase + t * UP];
        for (int r = row_first; r < ih; r += row_step) {
          const A* __restrict__ row = first + r * a.si;
          A acc = A(0);
#pragma unroll
          for (int t = 0; t < NT; ++t) acc = acc + row[t] * taps[t];
          s_mid[r * a.sm + col_l] = acc;
        }
      } else {
        for (int r = row_first; r < ih; r += row_step) {
          const A* __restrict__ row = first + r * a.si;
          A acc = A(0);
          for (int j = phase, t = 0; j < k; j += up, ++t) acc = acc + row[t] * s_f[j];
          s_mid[r * a.sm + col_l] = acc;
        }
      }
    } else {
      T* __restrict__ yp = y + int64_t(plane) * a.OH * a.OW;
      for (int oy = row_first; oy < noy; oy += row_step) {
        const int u = (oy0 + oy) * down + shift;
        const int i0 = f2d_floor_div(u, up);
        const int phase = (i0 + 1) * up - u - 1; // the same for every lane of a row
        const A* __restrict__ col = s_mid + (i0 - iy0) * a.sm + col_l;
        A acc = A(0);
        if constexpr (kTuned) {
          constexpr int NT = K / (UP > 0 ? UP : 1);
#pragma unroll
          for (int t = 0; t < NT; ++t) acc = acc + col[t * a.sm] * s_f[phase + t * UP];
        } else {
          for (int j = phase, t = 0; j < k; j += up, ++t) acc = acc + col[t * a.sm] * s_f[j];
        }
        if (col_l < nox) yp[(oy0 + oy) * a.OW + ox0 + col_l] = T(acc);
      }
    }
  }
}

template <typename T, int UP, int DOWN, int K>
__global__ __launch_bounds__(kBlock) void filter2d_kernel(
    const T* __restrict__ x, const float* __restrict__ f, T* __restrict__ y, F2dArgs a) {
  extern __shared__ __align__(16) unsigned char f2d_lds[];
  const int block = static_cast<int>(blockIdx.x), thread = static_cast<int>(threadIdx.x);
  filter2d_pass<T, UP, DOWN, K>(0, block, thread, x, f, y, a, f2d_lds);
  __syncthreads();
  filter2d_pass<T, UP, DOWN, K>(1, block, thread, x, f, y, a, f2d_lds);
  __syncthreads();
  filter2d_pass<T, UP, DOWN, K>(2, block, thread, x, f, y, a, f2d_lds);
}

// ---- host -----------------------------------------------------------------------------------------------------------
inline int64_t f2d_fdiv(int64_t a, int64_t b) {
  const int64_t q = a / b;
  return (a % b != 0 && a < 0) ? q - 1 : q;
}
inline int64_t f2d_pad0(int64_t k, int64_t up, int64_t down) {
  if (up == 1 && down == 1) return k / 2;
  return down != 1 ? f2d_fdiv(k - down + 1, 2) : f2d_fdiv(k + up - 1, 2);
}
inline int64_t f2d_pad1(int64_t k, int64_t up, int64_t down) {
  if (up == 1 && down == 1) return (k - 1) / 2;
  return down != 1 ? f2d_fdiv(k - down, 2) : f2d_fdiv(k - up, 2);
}

constexpr int64_t kF2dLimit = int64_t(1) << 31;
constexpr int64_t kF2dMaxFactor = 1 << 16, kF2dMaxTaps = 1 << 20;

// lead / total / out of one axis; DRTK_ERR_INVALID_ARGUMENT for factors, lengths and sizes the operator does not admit
int f2d_axis(int64_t in, int64_t k, int64_t up, int64_t down, bool backward, int64_t* lead, int64_t* total, int64_t* out) {
  if (in < 1 || k < 1 || up < 1 || down < 1 || in >= kF2dLimit || k > kF2dMaxTaps || up > kF2dMaxFactor || down > kF2dMaxFactor)
    return DRTK_ERR_INVALID_ARGUMENT;
  const int64_t tot = f2d_pad0(k, up, down) + f2d_pad1(k, up, down);
  const int64_t ld = backward ? k - 1 - f2d_pad0(k, down, up) : f2d_pad0(k, up, down);
  if (ld < 0 || tot - ld < 0) return DRTK_ERR_INVALID_ARGUMENT; // filter too short for the sampling factors
  const int64_t o = f2d_fdiv(in * up + tot - k + down, down);
  if (o < 1 || in * up + tot + down >= kF2dLimit) return DRTK_ERR_INVALID_ARGUMENT;
  *lead = ld, *total = tot, *out = o;
  return DRTK_OK;
}

int f2d_validate(
    drtk_dtype_t dtype, int64_t planes, int64_t H, int64_t W, int64_t k, int64_t up, int64_t down, bool reflect, bool backward,
    int64_t* lead, int64_t* OH, int64_t* OW) {
  if (!valid_dtype(dtype) && dtype != DRTK_F16) return DRTK_ERR_INVALID_ARGUMENT; // half: this operator only
  if (planes < 0) return DRTK_ERR_INVALID_ARGUMENT;
  int64_t total = 0;
  if (f2d_axis(H, k, up, down, backward, lead, &total, OH) != DRTK_OK) return DRTK_ERR_INVALID_ARGUMENT;
  if (f2d_axis(W, k, up, down, backward, lead, &total, OW) != DRTK_OK) return DRTK_ERR_INVALID_ARGUMENT;
  if (H * W >= kF2dLimit || *OH * *OW >= kF2dLimit) return DRTK_ERR_INVALID_ARGUMENT; // a plane is indexed with int
  if (reflect) { // torch's rule for reflect padding: the pad is smaller than the axis
    const int64_t before = ceil_div(*lead, up), after = ceil_div(total - *lead, up);
    if (before >= H || after >= H || before >= W || after >= W) return DRTK_ERR_INVALID_ARGUMENT;
  }
  return DRTK_OK;
}

// Tile geometry.  Candidates are 64, 32 or 16 outputs wide and 32, 16 ... 1 high; a candidate's LDS is the input tile
// with its halo plus the pass-2 result (plus the taps), its cost the inputs it loads per input it would load without a
// halo.  Taken: the cheapest tile that lets four workgroups share a CU's LDS, if it loads at most twice the ideal; failing
// that the same with two workgroups per CU; failing that the cheapest that fits at all (long filters, strong decimation,
// double).  false: nothing fits.
bool f2d_plan(F2dArgs& a, int D, size_t acc_size, bool with_taps, size_t* lds_bytes) {
  a.tmax = static_cast<int>(ceil_div(a.k, a.up));
  const size_t budgets[3] = {kLdsPerCu / 4, kLdsPerCu / 2, kLdsPerCu};
  const double ideal = double(a.down) * a.down / (double(a.up) * a.up); // inputs per output
  for (int b = 0; b < 3; ++b) {
    double best = -1.0;
    for (int shift = kMaxTowShift; shift >= 4; --shift) {
      const int tow = 1 << shift;
      const int iw_max = static_cast<int>(ceil_div(int64_t(tow - 1) * a.down, a.up)) + a.tmax;
      const int plane_w = static_cast<int>(ceil_div(iw_max, D)) | 1;
      int si = D * plane_w;
      if (si % 32 == 0) si += 1;
      for (int toh = 32; toh >= 1; toh /= 2) {
        const int64_t ih_max = ceil_div(int64_t(toh - 1) * a.down, a.up) + a.tmax;
        const size_t bytes = (size_t(ih_max) * size_t(si + tow + 1) + (with_taps ? size_t(a.k) : 0)) * acc_size;
        const double cost = double(iw_max) * double(ih_max) / (double(tow) * toh * ideal);
        if (bytes > budgets[b] || (best >= 0.0 && cost >= best)) continue;
        best = cost;
        a.tow_shift = shift, a.toh = toh, a.plane_w = plane_w, a.si = si, a.sm = tow + 1, a.ih_max = static_cast<int>(ih_max);
        *lds_bytes = bytes;
      }
    }
    if (best >= 0.0 && (best <= 2.0 || b == 2)) return true;
  }
  return false;
}

template <typename T, int UP, int DOWN, int K>
int f2d_launch(const void* x, const float* f, void* y, int64_t planes, F2dArgs a, hipStream_t stream) {
  using A = typename F2dAcc<T>::type;
  constexpr bool kRegTaps = K > 0 && UP == 1;
  constexpr int D = (kRegTaps && DOWN > 1) ? DOWN : 1;
  size_t lds_bytes = 0;
  if (!f2d_plan(a, D, sizeof(A), !kRegTaps, &lds_bytes)) return DRTK_ERR_UNSUPPORTED;
  a.tiles_x = static_cast<int>(ceil_div(a.OW, int64_t(1) << a.tow_shift)), a.tiles_y = static_cast<int>(ceil_div(a.OH, a.toh));
  const int64_t tiles = int64_t(a.tiles_x) * a.tiles_y;
  if (tiles >= kF2dLimit) return DRTK_ERR_INVALID_ARGUMENT;
  if (lds_bytes > 64 * 1024) {
    static bool raised = false; // (per instantiation; racing threads set the same value)
    if (!raised) {
      (void)hipFuncSetAttribute(
          reinterpret_cast<const void*>(&filter2d_kernel<T, UP, DOWN, K>), hipFuncAttributeMaxDynamicSharedMemorySize,
          static_cast<int>(kLdsPerCu));
      (void)hipGetLastError();
      raised = true;
    }
  }
  // planes are folded into gridDim.x, in slices where planes * tiles passes 2^31 - 1
  const int64_t per_launch = (kF2dLimit - 1) / tiles;
  const int64_t in_plane = int64_t(a.H) * a.W, out_plane = int64_t(a.OH) * a.OW;
  for (int64_t p0 = 0; p0 < planes; p0 += per_launch) {
    const int64_t n = planes - p0 < per_launch ? planes - p0 : per_launch;
    DRTK_LAUNCH(
        (filter2d_kernel<T, UP, DOWN, K>), dim3(static_cast<unsigned>(n * tiles)), dim3(kBlock), lds_bytes, stream,
        static_cast<const T*>(x) + p0 * in_plane, f, static_cast<T*>(y) + p0 * out_plane, a);
    DRTK_RETURN_IF_LAUNCH_FAILED();
  }
  return DRTK_OK;
}

// the families the reference tabulates (filter2d_kernel.cu); everything else takes the generic instantiation
#define F2D_TUNED(X)                                                                                               \
  X(1, 1, 3) X(1, 1, 5) X(1, 1, 7) X(1, 1, 9) X(1, 1, 11) X(1, 1, 13) X(1, 1, 17) X(1, 1, 25) X(1, 1, 33) X(1, 1, 49) \
  X(1, 1, 65)                                                                                                      \
  X(1, 2, 4) X(1, 2, 6) X(1, 2, 8) X(1, 2, 10) X(1, 2, 12) X(2, 1, 4) X(2, 1, 6) X(2, 1, 8) X(2, 1, 10) X(2, 1, 12)    \
  X(1, 4, 16) X(1, 4, 24) X(4, 1, 16) X(4, 1, 24) X(1, 8, 32) X(1, 8, 48) X(8, 1, 32) X(8, 1, 48)

template <typename T>
int f2d_dispatch(const void* x, const float* f, void* y, int64_t planes, const F2dArgs& a, bool force_generic, hipStream_t stream) {
  if (!force_generic) {
#define F2D_CASE(U, D, KK) \
  if (a.up == U && a.down == D && a.k == KK) return f2d_launch<T, U, D, KK>(x, f, y, planes, a, stream);
    F2D_TUNED(F2D_CASE)
#undef F2D_CASE
  }
  return f2d_launch<T, 0, 0, 0>(x, f, y, planes, a, stream);
}

} // namespace
} // namespace drtk_amd

using namespace drtk_amd;

extern "C" int drtk_amd_filter2d_output_size(int64_t in, int64_t k, int64_t up, int64_t down, int64_t* out) {
  int64_t lead = 0, total = 0, o = 0;
  if (!out) return DRTK_ERR_INVALID_ARGUMENT;
  const int st = f2d_axis(in, k, up, down, false, &lead, &total, &o);
  if (st != DRTK_OK) return st;
  *out = o;
  return DRTK_OK;
}

extern "C" int drtk_amd_filter2d(
    drtk_dtype_t dtype, const void* x, const float* f, int64_t planes, int64_t H, int64_t W, int64_t k, int64_t up, int64_t down,
    int reflect, int backward, int force_generic, void* y, drtk_stream_t stream) {
  int64_t lead = 0, OH = 0, OW = 0;
  const int st = f2d_validate(dtype, planes, H, W, k, up, down, reflect != 0, backward != 0, &lead, &OH, &OW);
  if (st != DRTK_OK) return st;
  if (planes == 0) return DRTK_OK;
  if (!x || !f || !y) return DRTK_ERR_INVALID_ARGUMENT;
  F2dArgs a = {};
  a.H = static_cast<int>(H), a.W = static_cast<int>(W), a.OH = static_cast<int>(OH), a.OW = static_cast<int>(OW);
  a.k = static_cast<int>(k), a.up = static_cast<int>(up), a.down = static_cast<int>(down), a.lead = static_cast<int>(lead);
  a.reflect = reflect != 0, a.reversed = backward == 0;
  hipStream_t s = static_cast<hipStream_t>(stream);
  if (dtype == DRTK_F16) return f2d_dispatch<half_t>(x, f, y, planes, a, force_generic != 0, s);
  return dispatch_dtype(dtype, [&](auto tag) {
    using T = decltype(tag);
    return f2d_dispatch<T>(x, f, y, planes, a, force_generic != 0, s);
  });
}
