// image_loss -- SSIM and the L1 / D-SSIM photometric loss of two [N,C,H,W] images under a per-pixel weight (the foreground
// mask of a render), one fused pass each way.  No reference counterpart; the definition (include/drtk_amd.h):
//   g[i] = exp(-(i - r)^2 / (2 sigma^2)) / sum, r = k / 2;  G*z: the separable blur of a channel with g, over zeros outside the
//   image ("same": the map domain D is the image) or over windows inside it only ("valid": D is the interior [H-2r, W-2r]);
//   mu_x = G*x, mu_y = G*y, s_x = G*(x x) - mu_x^2, s_y = G*(y y) - mu_y^2, s_xy = G*(x y) - mu_x mu_y
//   A1 = 2 mu_x mu_y + C1, A2 = 2 s_xy + C2, B1 = mu_x^2 + mu_y^2 + C1, B2 = s_x + s_y + C2, S = A1 A2 / (B1 B2)
//   ssim = sum_D(w S) / (C sum_D w),  l1 = sum(w |x - y|) / (C sum w) over the whole image; a weight sum of 0 gives 0.
// Gradient, with h the upstream gradient on D (zero outside):
//   dmu = 2 mu_y (A2 - A1) / (B1 B2) - 2 mu_x S (1 / B1 - 1 / B2),  dxx = -S / B2,  dxy = 2 A1 / (B1 B2)
//   grad_x = G*(h dmu) + 2 x G*(h dxx) + y G*(h dxy)  (+ the L1 term  l1_weight w sign(x - y) / (C sum w))
//
// Forward: one 256-thread workgroup per tile of kIlTileW x kIlTileH map elements of one view, channels looped inside:
//   1. the x and y tiles with a halo of r -> LDS, a wave per row, lanes along the row (row-contiguous loads); borders are
//      resolved here (a zero outside the image), and so is the weight tile, once per workgroup (1 inside the image without
//      a weight, 0 outside it in any case: the sums below need no bounds of their own);
//   2. horizontal pass, LDS -> LDS: a lane per tile row, kIlCols consecutive columns per lane in registers (k + kIlCols - 1
//      reads of x and y for kIlCols x 5 moment values; lanes walk rows, whose stride is odd: no bank conflicts);
//   3. vertical pass, LDS -> registers: a lane per column, kIlRows consecutive rows per lane (k + kIlRows - 1 reads per
//      moment); S, and with `maps` the three gradient maps, are formed and stored from registers.
//   |x - y| is taken from the tile in LDS, by the workgroup that owns the pixel (each pixel of the image has one owner,
//   also under "valid", where the border tiles own the rim the map does not cover).
//   Every workgroup reduces w S, w over D, w |x - y| and w over the image in double (row_shr DPP steps inside a row of 16
//   lanes, the four rows and then the four waves in a fixed order) and writes them to ITS slot of the workspace; a second,
//   one-workgroup kernel adds the slots -- thread t its slots t, t + 256, ... in ascending order, then the 256 sums in
//   ascending order -- and forms the scalars.  No atomics, no zero-fill: bitwise the same from run to run.
// Backward: one kernel, the same tile scheme over the IMAGE: the three maps times h, zero outside D, go to LDS with a
//   halo (h is the upstream map, or g w / (C sum w) from the scalars the forward left in device memory), two passes, and the
//   store combines the three blurs with x, y and the L1 term.
// The window travels by value in the kernel arguments: nothing is copied to the device, so the calls are capture-safe.
#include "common.hpp"

namespace drtk_amd {
namespace {

// A tile of map elements (forward) or pixels (backward); read by tests/test_gpu_image_loss.py.
constexpr int kIlTileW = 32;
constexpr int kIlTileH = 32;
constexpr int kIlCols = 4;       // consecutive columns a lane of the horizontal pass keeps in registers
constexpr int kIlRows = 4;       // consecutive rows a lane of the vertical pass keeps in registers
constexpr int kIlMinWindow = 3;
constexpr int kIlMaxWindow = 15;
constexpr int kIlSums = 4;       // sum_D w S, sum_D w, sum w |x - y|, sum w
constexpr int64_t kIlLimit = int64_t(1) << 31;
constexpr size_t kIlLdsPerCu = 160 * 1024;

static_assert(kIlTileW == 32 && kBlock == 256 && kWave == 64, "the lane maps below are written for these");
static_assert(kIlTileH == (kBlock / kIlTileW) * kIlRows, "vertical pass: every lane takes kIlRows rows of one column");
static_assert(kIlTileW == (kBlock / kWave) * 2 * kIlCols, "horizontal pass: a wave takes two groups of kIlCols columns");
static_assert(kIlTileH + 2 * (kIlMaxWindow / 2) <= kWave, "horizontal pass: a lane per tile row");

enum { IL_MAP = 0, IL_SSIM = 1, IL_PHOTOMETRIC = 2 };
enum { IL_W_NONE = 0, IL_W_BOOL = 1, IL_W_REAL = 2 };

template <typename T>
struct IlArgs {
  int C, H, W, OH, OW;       // the image and the map domain D
  int k, r, off;             // map (0, 0) is the window centred on pixel (off, off): 0 for "same", r for "valid"
  int tiles_x, tiles_y;
  int ih, iw, si, sm;        // LDS: rows and columns of a tile with its halo, its row stride, the row stride of pass 2's result
  int mode, weight_kind, write_maps;
  int64_t x_sN, x_sC, x_sH, y_sN, y_sC, y_sH, w_sN, w_sH;
  T c1, c2;
  T coef_ssim, coef_l1;      // backward: what the upstream scalar is multiplied by for the two terms
  T g[kIlMaxWindow];
};

template <typename T>
__device__ __forceinline__ T il_fma(T a, T b, T c);
template <>
__device__ __forceinline__ float il_fma<float>(float a, float b, float c) {
  return __builtin_fmaf(a, b, c);
}
template <>
__device__ __forceinline__ double il_fma<double>(double a, double b, double c) {
  return __builtin_fma(a, b, c);
}

// lane i receives lane i - n of its row of 16 lanes, lanes without such a source 0.0
template <int CTRL>
__device__ __forceinline__ double il_row_shr(double v) {
  const int lo = __builtin_amdgcn_update_dpp(0, __double2loint(v), CTRL, 0xf, 0xf, false);
  const int hi = __builtin_amdgcn_update_dpp(0, __double2hiint(v), CTRL, 0xf, 0xf, false);
  return __hiloint2double(hi, lo);
}
__device__ __forceinline__ double il_read_lane(double v, int lane) {
  return __hiloint2double(__builtin_amdgcn_readlane(__double2hiint(v), lane), __builtin_amdgcn_readlane(__double2loint(v), lane));
}
// The sum over the 64 lanes in one fixed order, in every lane.  All lanes must be active.
__device__ __forceinline__ double il_wave_sum(double v) {
  v += il_row_shr<0x111>(v); // row_shr:1
  v += il_row_shr<0x112>(v); // row_shr:2
  v += il_row_shr<0x114>(v); // row_shr:4
  v += il_row_shr<0x118>(v); // row_shr:8 -- lane 15 of every row now holds the row's sum
  return ((il_read_lane(v, 15) + il_read_lane(v, 31)) + il_read_lane(v, 47)) + il_read_lane(v, 63);
}

// LDS of both kernels: kBlock / kWave x kIlSums doubles for the reduction, then `planes_in` tiles with halo (ih x si) and
// `planes_mid` results of the horizontal pass (ih x sm).
__host__ __device__ inline size_t il_lds_bytes(int ih, int si, int sm, int planes_in, int planes_mid, size_t elem) {
  return size_t(kBlock / kWave) * kIlSums * sizeof(double) + (size_t(planes_in) * ih * si + size_t(planes_mid) * ih * sm) * elem;
}

// Vertical pass for the lane's column `col` and rows row0 .. row0 + kIlRows - 1 of M planes: acc[m][o] = sum_t g[t] mid_m[row0 + o + t][col],
// taps ascending.
template <typename T, int M>
__device__ __forceinline__ void il_vertical(const T* __restrict__ mid, int plane, int sm, int col, int row0, int k, const T* g, T (&acc)[M][kIlRows]) {
#pragma unroll
  for (int m = 0; m < M; ++m)
#pragma unroll
    for (int o = 0; o < kIlRows; ++o) acc[m][o] = T(0);
  for (int j = 0; j < k + kIlRows - 1; ++j) {
    T v[M];
#pragma unroll
    for (int m = 0; m < M; ++m) v[m] = mid[m * plane + (row0 + j) * sm + col];
#pragma unroll
    for (int o = 0; o < kIlRows; ++o) {
      const int t = j - o;
      if (t >= 0 && t < k) {
        const T gt = g[t];
#pragma unroll
        for (int m = 0; m < M; ++m) acc[m][o] = il_fma(gt, v[m], acc[m][o]);
      }
    }
  }
}

template <typename T>
__global__ __launch_bounds__(kBlock) void image_loss_forward_kernel(
    const T* __restrict__ x, const T* __restrict__ y, const void* __restrict__ weight, T* __restrict__ ssim_map, T* __restrict__ maps,
    int64_t map_plane_stride, double* __restrict__ slots, IlArgs<T> a) {
  extern __shared__ __align__(16) unsigned char il_lds[];
  double* __restrict__ s_red = reinterpret_cast<double*>(il_lds);
  T* __restrict__ s_x = reinterpret_cast<T*>(s_red + (kBlock / kWave) * kIlSums);
  const int tile_elems = a.ih * a.si, mid_plane = a.ih * a.sm;
  T* __restrict__ s_y = s_x + tile_elems;
  T* __restrict__ s_w = s_y + tile_elems;
  T* __restrict__ s_mid = s_w + tile_elems;

  const int thread = static_cast<int>(threadIdx.x), lane = thread & (kWave - 1), wave = thread / kWave;
  constexpr int kWaves = kBlock / kWave;
  const int tiles = a.tiles_x * a.tiles_y;
  const int block = static_cast<int>(blockIdx.x);
  const int n = block / tiles, tile = block - n * tiles;
  const int ty = tile / a.tiles_x, tx = tile - ty * a.tiles_x;
  const int ox0 = tx * kIlTileW, oy0 = ty * kIlTileH;
  // local (lr, lc) of the tile with halo is pixel (py0 + lr, px0 + lc)
  const int px0 = ox0 + a.off - a.r, py0 = oy0 + a.off - a.r;
  const bool sums = a.mode != IL_MAP;

  if (sums) { // the weight tile: once per workgroup
    for (int lr = wave; lr < a.ih; lr += kWaves) {
      const int py = py0 + lr, px = px0 + lane;
      if (lane < a.iw) {
        T v = T(0);
        if (py >= 0 && py < a.H && px >= 0 && px < a.W) {
          const int64_t at = int64_t(n) * a.w_sN + int64_t(py) * a.w_sH + px;
          v = a.weight_kind == IL_W_NONE   ? T(1)
              : a.weight_kind == IL_W_BOOL ? (static_cast<const unsigned char*>(weight)[at] != 0 ? T(1) : T(0))
                                           : static_cast<const T*>(weight)[at];
        }
        s_w[lr * a.si + lane] = v;
      }
    }
  }

  // the pixels this workgroup owns for the L1 term: its tile's centres, and on the border tiles the rim up to the image's edge
  const int own_y0 = ty == 0 ? 0 : oy0 + a.off, own_y1 = ty == a.tiles_y - 1 ? a.H : oy0 + a.off + kIlTileH;
  const int own_x0 = tx == 0 ? 0 : ox0 + a.off, own_x1 = tx == a.tiles_x - 1 ? a.W : ox0 + a.off + kIlTileW;
  const int own_lr0 = own_y0 - py0, own_lr1 = own_y1 - py0, own_lc0 = own_x0 - px0, own_lc1 = own_x1 - px0;

  // vertical pass: this lane's column and first row of the tile
  const int vcol = thread & (kIlTileW - 1), vrow0 = (thread / kIlTileW) * kIlRows;
  double sum_ws = 0.0, sum_wd = 0.0, sum_wl = 0.0, sum_w = 0.0;

  for (int ch = 0; ch < a.C; ++ch) {
    const T* __restrict__ xp = x + int64_t(n) * a.x_sN + int64_t(ch) * a.x_sC;
    const T* __restrict__ yp = y + int64_t(n) * a.y_sN + int64_t(ch) * a.y_sC;
    // 1. tiles with halo
    for (int lr = wave; lr < a.ih; lr += kWaves) {
      const int py = py0 + lr, px = px0 + lane;
      if (lane < a.iw) {
        T xv = T(0), yv = T(0);
        if (py >= 0 && py < a.H && px >= 0 && px < a.W) {
          xv = xp[int64_t(py) * a.x_sH + px];
          yv = yp[int64_t(py) * a.y_sH + px];
        }
        s_x[lr * a.si + lane] = xv;
        s_y[lr * a.si + lane] = yv;
      }
    }
    __syncthreads();
    if (a.mode == IL_PHOTOMETRIC) {
      for (int lr = own_lr0 + wave; lr < own_lr1; lr += kWaves) {
        const int lc = own_lc0 + lane;
        if (lc < own_lc1) {
          const T d = s_x[lr * a.si + lc] - s_y[lr * a.si + lc];
          const T w = s_w[lr * a.si + lc];
          sum_wl += double(w * (d < T(0) ? -d : d));
          if (ch == 0) sum_w += double(w);
        }
      }
    }
    // 2. horizontal pass: lane = row of the tile with halo, the wave's two groups of kIlCols columns
    if (lane < a.ih) {
      for (int grp = wave; grp < kIlTileW / kIlCols; grp += kWaves) {
        const T* __restrict__ rx = s_x + lane * a.si + grp * kIlCols;
        const T* __restrict__ ry = s_y + lane * a.si + grp * kIlCols;
        T acc[5][kIlCols];
#pragma unroll
        for (int m = 0; m < 5; ++m)
#pragma unroll
          for (int o = 0; o < kIlCols; ++o) acc[m][o] = T(0);
        for (int j = 0; j < a.k + kIlCols - 1; ++j) {
          const T xv = rx[j], yv = ry[j];
          const T v[5] = {xv, yv, xv * xv, yv * yv, xv * yv};
#pragma unroll
          for (int o = 0; o < kIlCols; ++o) {
            const int t = j - o;
            if (t >= 0 && t < a.k) {
              const T gt = a.g[t];
#pragma unroll
              for (int m = 0; m < 5; ++m) acc[m][o] = il_fma(gt, v[m], acc[m][o]);
            }
          }
        }
#pragma unroll
        for (int m = 0; m < 5; ++m)
#pragma unroll
          for (int o = 0; o < kIlCols; ++o) s_mid[m * mid_plane + lane * a.sm + grp * kIlCols + o] = acc[m][o];
      }
    }
    __syncthreads();
    // 3. vertical pass and the map
    T acc[5][kIlRows];
    il_vertical<T, 5>(s_mid, mid_plane, a.sm, vcol, vrow0, a.k, a.g, acc);
    const int64_t plane = int64_t(n) * a.C + ch;
#pragma unroll
    for (int o = 0; o < kIlRows; ++o) {
      const int oy = oy0 + vrow0 + o, ox = ox0 + vcol;
      const bool in = oy < a.OH && ox < a.OW;
      const T mu_x = acc[0][o], mu_y = acc[1][o];
      const T mxx = mu_x * mu_x, myy = mu_y * mu_y, mxy = mu_x * mu_y;
      const T s_xx = acc[2][o] - mxx, s_yy = acc[3][o] - myy, s_xy = acc[4][o] - mxy;
      const T A1 = T(2) * mxy + a.c1, A2 = T(2) * s_xy + a.c2;
      const T B1 = mxx + myy + a.c1, B2 = s_xx + s_yy + a.c2;
      const T inv_b = T(1) / (B1 * B2);
      const T S = A1 * A2 * inv_b;
      if (in) {
        const int64_t at = int64_t(oy) * a.OW + ox;
        if (a.mode == IL_MAP) ssim_map[plane * a.OH * a.OW + at] = S;
        if (a.write_maps) {
          T* __restrict__ mp = maps + plane * a.OH * a.OW + at;
          mp[0] = T(2) * mu_y * (A2 - A1) * inv_b - T(2) * mu_x * S * (T(1) / B1 - T(1) / B2);
          mp[map_plane_stride] = -S / B2;
          mp[2 * map_plane_stride] = T(2) * A1 * inv_b;
        }
        if (sums) {
          const T w = s_w[(vrow0 + o + a.r) * a.si + vcol + a.r];
          sum_ws += double(w * S);
          if (ch == 0) sum_wd += double(w);
        }
      }
    }
    // (the next channel's tiles are written after every wave has left pass 2, and pass 2 writes after the barrier that follows)
  }

  if (sums) {
    const double sums4[kIlSums] = {il_wave_sum(sum_ws), il_wave_sum(sum_wd), il_wave_sum(sum_wl), il_wave_sum(sum_w)};
    if (lane == 0) {
#pragma unroll
      for (int q = 0; q < kIlSums; ++q) s_red[wave * kIlSums + q] = sums4[q];
    }
    __syncthreads();
    if (thread < kIlSums) {
      double t = s_red[thread];
      for (int wv = 1; wv < kWaves; ++wv) t += s_red[wv * kIlSums + thread];
      slots[int64_t(block) * kIlSums + thread] = t;
    }
  }
}

// One workgroup: the slots' sums and the scalars.  scalars: ssim, l1, 1 / (C sum_D w), 1 / (C sum w), the inverses 0 where the sum is 0.
template <typename T>
__global__ __launch_bounds__(kBlock) void image_loss_finalize_kernel(
    const double* __restrict__ slots, int64_t nslots, int C, int mode, double l1_weight, double ssim_weight, T* __restrict__ out,
    double* __restrict__ scalars) {
  __shared__ double s_part[kBlock][kIlSums];
  const int thread = static_cast<int>(threadIdx.x);
  double t[kIlSums] = {0.0, 0.0, 0.0, 0.0};
  for (int64_t s = thread; s < nslots; s += kBlock) {
#pragma unroll
    for (int q = 0; q < kIlSums; ++q) t[q] += slots[s * kIlSums + q];
  }
#pragma unroll
  for (int q = 0; q < kIlSums; ++q) s_part[thread][q] = t[q];
  __syncthreads();
  if (thread == 0) {
    for (int i = 1; i < kBlock; ++i) {
#pragma unroll
      for (int q = 0; q < kIlSums; ++q) t[q] += s_part[i][q];
    }
    const double inv_d = t[1] > 0.0 ? 1.0 / (double(C) * t[1]) : 0.0;
    const double inv_l = t[3] > 0.0 ? 1.0 / (double(C) * t[3]) : 0.0;
    const double ssim = t[1] > 0.0 ? t[0] * inv_d : 0.0, l1 = t[3] > 0.0 ? t[2] * inv_l : 0.0;
    scalars[0] = ssim, scalars[1] = l1, scalars[2] = inv_d, scalars[3] = inv_l;
    out[0] = mode == IL_SSIM ? T(ssim) : T(l1_weight * l1 + ssim_weight * (1.0 - ssim));
  }
}

template <typename T>
__global__ __launch_bounds__(kBlock) void image_loss_backward_kernel(
    const T* __restrict__ x, const T* __restrict__ y, const void* __restrict__ weight, const T* __restrict__ maps, int64_t map_plane_stride,
    const T* __restrict__ grad_map, const T* __restrict__ grad_scalar, const double* __restrict__ scalars, T* __restrict__ grad_x,
    IlArgs<T> a) {
  extern __shared__ __align__(16) unsigned char il_lds[];
  double* __restrict__ s_red = reinterpret_cast<double*>(il_lds); // (unused here: one layout for both kernels)
  T* __restrict__ s_in = reinterpret_cast<T*>(s_red + (kBlock / kWave) * kIlSums);
  const int tile_elems = a.ih * a.si, mid_plane = a.ih * a.sm;
  T* __restrict__ s_w = s_in + 3 * tile_elems;
  T* __restrict__ s_mid = s_w + tile_elems;

  const int thread = static_cast<int>(threadIdx.x), lane = thread & (kWave - 1), wave = thread / kWave;
  constexpr int kWaves = kBlock / kWave;
  const int tiles = a.tiles_x * a.tiles_y;
  const int block = static_cast<int>(blockIdx.x);
  const int n = block / tiles, tile = block - n * tiles;
  const int ty = tile / a.tiles_x, tx = tile - ty * a.tiles_x;
  const int ix0 = tx * kIlTileW, iy0 = ty * kIlTileH; // pixels
  // local (lr, lc) is pixel (iy0 - r + lr, ix0 - r + lc), the map element at that pixel less (off, off)
  const int qx0 = ix0 - a.r - a.off, qy0 = iy0 - a.r - a.off;
  const bool means = a.mode != IL_MAP;

  T h_ssim = T(0), h_l1 = T(0);
  if (means) {
    const T gs = grad_scalar[0];
    h_ssim = gs * a.coef_ssim * T(scalars[2]);
    h_l1 = gs * a.coef_l1 * T(scalars[3]);
    for (int lr = wave; lr < a.ih; lr += kWaves) {
      const int py = iy0 - a.r + lr, px = ix0 - a.r + lane;
      if (lane < a.iw) {
        T v = T(0);
        if (py >= 0 && py < a.H && px >= 0 && px < a.W) {
          const int64_t at = int64_t(n) * a.w_sN + int64_t(py) * a.w_sH + px;
          v = a.weight_kind == IL_W_NONE   ? T(1)
              : a.weight_kind == IL_W_BOOL ? (static_cast<const unsigned char*>(weight)[at] != 0 ? T(1) : T(0))
                                           : static_cast<const T*>(weight)[at];
        }
        s_w[lr * a.si + lane] = v;
      }
    }
    __syncthreads();
  }

  const int vcol = thread & (kIlTileW - 1), vrow0 = (thread / kIlTileW) * kIlRows;
  const int64_t map_elems = int64_t(a.OH) * a.OW;

  for (int ch = 0; ch < a.C; ++ch) {
    const int64_t plane = int64_t(n) * a.C + ch;
    const T* __restrict__ mp = maps + plane * map_elems;
    // 1. h times the three maps, zero outside D
    for (int lr = wave; lr < a.ih; lr += kWaves) {
      const int qy = qy0 + lr, qx = qx0 + lane;
      if (lane < a.iw) {
        T va = T(0), vb = T(0), vc = T(0);
        if (qy >= 0 && qy < a.OH && qx >= 0 && qx < a.OW) {
          const int64_t at = int64_t(qy) * a.OW + qx;
          const T h = means ? s_w[lr * a.si + lane] * h_ssim : grad_map[plane * map_elems + at];
          va = h * mp[at], vb = h * mp[map_plane_stride + at], vc = h * mp[2 * map_plane_stride + at];
        }
        s_in[lr * a.si + lane] = va;
        s_in[tile_elems + lr * a.si + lane] = vb;
        s_in[2 * tile_elems + lr * a.si + lane] = vc;
      }
    }
    __syncthreads();
    // 2. horizontal pass
    if (lane < a.ih) {
      for (int grp = wave; grp < kIlTileW / kIlCols; grp += kWaves) {
        const T* __restrict__ row = s_in + lane * a.si + grp * kIlCols;
        T acc[3][kIlCols];
#pragma unroll
        for (int m = 0; m < 3; ++m)
#pragma unroll
          for (int o = 0; o < kIlCols; ++o) acc[m][o] = T(0);
        for (int j = 0; j < a.k + kIlCols - 1; ++j) {
          const T v[3] = {row[j], row[tile_elems + j], row[2 * tile_elems + j]};
#pragma unroll
          for (int o = 0; o < kIlCols; ++o) {
            const int t = j - o;
            if (t >= 0 && t < a.k) {
              const T gt = a.g[t];
#pragma unroll
              for (int m = 0; m < 3; ++m) acc[m][o] = il_fma(gt, v[m], acc[m][o]);
            }
          }
        }
#pragma unroll
        for (int m = 0; m < 3; ++m)
#pragma unroll
          for (int o = 0; o < kIlCols; ++o) s_mid[m * mid_plane + lane * a.sm + grp * kIlCols + o] = acc[m][o];
      }
    }
    __syncthreads();
    // 3. vertical pass and the gradient
    T acc[3][kIlRows];
    il_vertical<T, 3>(s_mid, mid_plane, a.sm, vcol, vrow0, a.k, a.g, acc);
    const T* __restrict__ xp = x + int64_t(n) * a.x_sN + int64_t(ch) * a.x_sC;
    const T* __restrict__ yp = y + int64_t(n) * a.y_sN + int64_t(ch) * a.y_sC;
#pragma unroll
    for (int o = 0; o < kIlRows; ++o) {
      const int py = iy0 + vrow0 + o, px = ix0 + vcol;
      if (py < a.H && px < a.W) {
        const T xv = xp[int64_t(py) * a.x_sH + px], yv = yp[int64_t(py) * a.y_sH + px];
        T gx = acc[0][o] + T(2) * xv * acc[1][o] + yv * acc[2][o];
        if (a.mode == IL_PHOTOMETRIC) {
          const T d = xv - yv;
          const T sgn = d > T(0) ? T(1) : (d < T(0) ? T(-1) : T(0));
          gx = gx + h_l1 * s_w[(vrow0 + o + a.r) * a.si + vcol + a.r] * sgn;
        }
        grad_x[plane * a.H * a.W + int64_t(py) * a.W + px] = gx;
      }
    }
  }
}

// ---- host -----------------------------------------------------------------------------------------------------------
struct IlShape {
  int64_t OH, OW, tiles_x, tiles_y, blocks; // of the forward
  int r, off;
};

int il_shape(int64_t N, int64_t C, int64_t H, int64_t W, int window_size, int valid, IlShape* s) {
  if (window_size < kIlMinWindow || window_size > kIlMaxWindow || window_size % 2 == 0) return DRTK_ERR_INVALID_ARGUMENT;
  if (N < 1 || C < 1 || H < 1 || W < 1 || H * W >= kIlLimit || C >= kIlLimit) return DRTK_ERR_INVALID_ARGUMENT;
  s->r = window_size / 2, s->off = valid ? s->r : 0;
  s->OH = H - 2 * s->off, s->OW = W - 2 * s->off;
  if (s->OH < 1 || s->OW < 1) return DRTK_ERR_INVALID_ARGUMENT; // "valid" needs H, W >= window_size
  s->tiles_x = ceil_div(s->OW, kIlTileW), s->tiles_y = ceil_div(s->OH, kIlTileH);
  s->blocks = N * s->tiles_x * s->tiles_y;
  // the backward's grid covers the image: it is the larger of the two
  if (N * ceil_div(W, kIlTileW) * ceil_div(H, kIlTileH) >= kIlLimit) return DRTK_ERR_INVALID_ARGUMENT;
  return DRTK_OK;
}

// the window, normalised in double
int il_window(int k, double sigma, double* g) {
  if (!(sigma > 0.0) || !(sigma < 1e30)) return DRTK_ERR_INVALID_ARGUMENT;
  const int r = k / 2;
  double sum = 0.0;
  for (int i = 0; i < k; ++i) sum += g[i] = std::exp(-double((i - r) * (i - r)) / (2.0 * sigma * sigma));
  for (int i = 0; i < k; ++i) g[i] /= sum;
  return DRTK_OK;
}

template <typename T>
void il_fill_args(
    IlArgs<T>& a, const IlShape& s, int64_t C, int64_t H, int64_t W, int k, const double* g, double data_range, int mode,
    int weight_kind, const int64_t* xs, const int64_t* ys, const int64_t* ws) {
  a.C = static_cast<int>(C), a.H = static_cast<int>(H), a.W = static_cast<int>(W);
  a.OH = static_cast<int>(s.OH), a.OW = static_cast<int>(s.OW);
  a.k = k, a.r = s.r, a.off = s.off;
  a.ih = kIlTileH + 2 * s.r, a.iw = kIlTileW + 2 * s.r, a.si = a.iw | 1, a.sm = kIlTileW + 1;
  a.mode = mode, a.weight_kind = weight_kind;
  a.x_sN = xs[0], a.x_sC = xs[1], a.x_sH = xs[2], a.y_sN = ys[0], a.y_sC = ys[1], a.y_sH = ys[2];
  a.w_sN = ws ? ws[0] : 0, a.w_sH = ws ? ws[1] : 0;
  a.c1 = T((0.01 * data_range) * (0.01 * data_range)), a.c2 = T((0.03 * data_range) * (0.03 * data_range));
  for (int i = 0; i < kIlMaxWindow; ++i) a.g[i] = i < k ? T(g[i]) : T(0);
}

// above 64 KiB (double) a kernel's dynamic-LDS limit is raised, once per kernel
template <auto KERNEL>
int il_raise_lds(size_t lds_bytes) {
  if (lds_bytes > kIlLdsPerCu) return DRTK_ERR_UNSUPPORTED;
  if (lds_bytes > 64 * 1024) {
    static bool raised = false; // (racing threads set the same value)
    if (!raised) {
      (void)hipFuncSetAttribute(reinterpret_cast<const void*>(KERNEL), hipFuncAttributeMaxDynamicSharedMemorySize, static_cast<int>(kIlLdsPerCu));
      (void)hipGetLastError();
      raised = true;
    }
  }
  return DRTK_OK;
}

bool il_strides_ok(const int64_t* s, int n) {
  if (!s) return false;
  for (int i = 0; i < n; ++i)
    if (s[i] < 0) return false;
  return true;
}

template <typename T>
int il_forward(
    const void* img, const int64_t* xs, const void* target, const int64_t* ys, const void* weight, int weight_kind, const int64_t* ws,
    int64_t N, int64_t C, int64_t H, int64_t W, int k, const double* g, const IlShape& s, double data_range, int mode, double l1_weight,
    double ssim_weight, void* out, void* maps, void* scalars, void* workspace, hipStream_t stream) {
  IlArgs<T> a = {};
  il_fill_args(a, s, C, H, W, k, g, data_range, mode, weight_kind, xs, ys, ws);
  a.tiles_x = static_cast<int>(s.tiles_x), a.tiles_y = static_cast<int>(s.tiles_y);
  a.write_maps = maps != nullptr;
  const size_t lds = il_lds_bytes(a.ih, a.si, a.sm, 3, 5, sizeof(T));
  const int st = il_raise_lds<&image_loss_forward_kernel<T>>(lds);
  if (st != DRTK_OK) return st;
  const int64_t map_plane_stride = N * C * s.OH * s.OW;
  DRTK_LAUNCH(
      image_loss_forward_kernel<T>, dim3(static_cast<unsigned>(s.blocks)), dim3(kBlock), lds, stream, static_cast<const T*>(img),
      static_cast<const T*>(target), weight, mode == IL_MAP ? static_cast<T*>(out) : nullptr, static_cast<T*>(maps), map_plane_stride,
      static_cast<double*>(workspace), a);
  DRTK_RETURN_IF_LAUNCH_FAILED();
  if (mode != IL_MAP) {
    DRTK_LAUNCH(
        image_loss_finalize_kernel<T>, dim3(1), dim3(kBlock), 0, stream, static_cast<const double*>(workspace), s.blocks,
        static_cast<int>(C), mode, l1_weight, ssim_weight, static_cast<T*>(out), static_cast<double*>(scalars));
    DRTK_RETURN_IF_LAUNCH_FAILED();
  }
  return DRTK_OK;
}

template <typename T>
int il_backward(
    const void* img, const int64_t* xs, const void* target, const int64_t* ys, const void* weight, int weight_kind, const int64_t* ws,
    int64_t N, int64_t C, int64_t H, int64_t W, int k, const double* g, const IlShape& s, double data_range, int mode, double l1_weight,
    double ssim_weight, const void* maps, const void* grad_out, const void* scalars, void* grad_img, hipStream_t stream) {
  IlArgs<T> a = {};
  il_fill_args(a, s, C, H, W, k, g, data_range, mode, weight_kind, xs, ys, ws);
  a.tiles_x = static_cast<int>(ceil_div(W, kIlTileW)), a.tiles_y = static_cast<int>(ceil_div(H, kIlTileH)); // over the image
  // ssim = +mean(S);  photometric = l1_weight l1 + ssim_weight (1 - mean(S))
  a.coef_ssim = mode == IL_SSIM ? T(1) : T(-ssim_weight);
  a.coef_l1 = mode == IL_PHOTOMETRIC ? T(l1_weight) : T(0);
  const size_t lds = il_lds_bytes(a.ih, a.si, a.sm, 4, 3, sizeof(T));
  const int st = il_raise_lds<&image_loss_backward_kernel<T>>(lds);
  if (st != DRTK_OK) return st;
  const int64_t map_plane_stride = N * C * s.OH * s.OW;
  const int64_t blocks = N * a.tiles_x * a.tiles_y;
  DRTK_LAUNCH(
      image_loss_backward_kernel<T>, dim3(static_cast<unsigned>(blocks)), dim3(kBlock), lds, stream, static_cast<const T*>(img),
      static_cast<const T*>(target), weight, static_cast<const T*>(maps), map_plane_stride,
      mode == IL_MAP ? static_cast<const T*>(grad_out) : nullptr, mode == IL_MAP ? nullptr : static_cast<const T*>(grad_out),
      static_cast<const double*>(scalars), static_cast<T*>(grad_img), a);
  DRTK_RETURN_IF_LAUNCH_FAILED();
  return DRTK_OK;
}

// everything both entry points judge before they look at a pointer
int il_validate(
    drtk_dtype_t dtype, int64_t N, int64_t C, int64_t H, int64_t W, int window_size, double sigma, double data_range, int valid, int mode,
    int weight_kind, double l1_weight, double ssim_weight, IlShape* s, double* g) {
  if (!valid_dtype(dtype)) return DRTK_ERR_INVALID_ARGUMENT;
  if (mode != IL_MAP && mode != IL_SSIM && mode != IL_PHOTOMETRIC) return DRTK_ERR_INVALID_ARGUMENT;
  if (weight_kind != IL_W_NONE && weight_kind != IL_W_BOOL && weight_kind != IL_W_REAL) return DRTK_ERR_INVALID_ARGUMENT;
  if (mode == IL_MAP && weight_kind != IL_W_NONE) return DRTK_ERR_INVALID_ARGUMENT;
  if (!(data_range > 0.0) || !(data_range < 1e30)) return DRTK_ERR_INVALID_ARGUMENT;
  if (!(l1_weight == l1_weight) || !(ssim_weight == ssim_weight)) return DRTK_ERR_INVALID_ARGUMENT;
  const int st = il_shape(N, C, H, W, window_size, valid, s);
  if (st != DRTK_OK) return st;
  return il_window(window_size, sigma, g);
}

} // namespace
} // namespace drtk_amd

using namespace drtk_amd;

extern "C" int drtk_amd_image_loss_workspace_bytes(int64_t N, int64_t H, int64_t W, int window_size, int valid, size_t* bytes) {
  IlShape s = {};
  if (!bytes) return DRTK_ERR_INVALID_ARGUMENT;
  const int st = il_shape(N, 1, H, W, window_size, valid, &s);
  if (st != DRTK_OK) return st;
  *bytes = size_t(s.blocks) * kIlSums * sizeof(double);
  return DRTK_OK;
}

extern "C" int drtk_amd_image_loss_forward(
    drtk_dtype_t dtype, const void* img, const int64_t* img_strides, const void* target, const int64_t* target_strides,
    const void* weight, int weight_kind, const int64_t* weight_strides, int64_t N, int64_t C, int64_t H, int64_t W, int window_size,
    double sigma, double data_range, int valid, int mode, double l1_weight, double ssim_weight, void* out, void* maps, void* scalars,
    void* workspace, size_t workspace_bytes, drtk_stream_t stream) {
  IlShape s = {};
  double g[kIlMaxWindow];
  const int st = il_validate(dtype, N, C, H, W, window_size, sigma, data_range, valid, mode, weight_kind, l1_weight, ssim_weight, &s, g);
  if (st != DRTK_OK) return st;
  if (!img || !target || !out || !il_strides_ok(img_strides, 3) || !il_strides_ok(target_strides, 3)) return DRTK_ERR_INVALID_ARGUMENT;
  if (weight_kind != IL_W_NONE && (!weight || !il_strides_ok(weight_strides, 2))) return DRTK_ERR_INVALID_ARGUMENT;
  if (mode != IL_MAP) {
    if (!scalars || !workspace) return DRTK_ERR_INVALID_ARGUMENT;
    if (workspace_bytes < size_t(s.blocks) * kIlSums * sizeof(double)) return DRTK_ERR_WORKSPACE_TOO_SMALL;
  }
  return dispatch_dtype(dtype, [&](auto tag) {
    using T = decltype(tag);
    return il_forward<T>(
        img, img_strides, target, target_strides, weight, weight_kind, weight_strides, N, C, H, W, window_size, g, s, data_range, mode,
        l1_weight, ssim_weight, out, maps, scalars, workspace, static_cast<hipStream_t>(stream));
  });
}

extern "C" int drtk_amd_image_loss_backward(
    drtk_dtype_t dtype, const void* img, const int64_t* img_strides, const void* target, const int64_t* target_strides,
    const void* weight, int weight_kind, const int64_t* weight_strides, int64_t N, int64_t C, int64_t H, int64_t W, int window_size,
    double sigma, double data_range, int valid, int mode, double l1_weight, double ssim_weight, const void* maps, const void* grad_out,
    const void* scalars, void* grad_img, drtk_stream_t stream) {
  IlShape s = {};
  double g[kIlMaxWindow];
  const int st = il_validate(dtype, N, C, H, W, window_size, sigma, data_range, valid, mode, weight_kind, l1_weight, ssim_weight, &s, g);
  if (st != DRTK_OK) return st;
  if (!img || !target || !maps || !grad_out || !grad_img || !il_strides_ok(img_strides, 3) || !il_strides_ok(target_strides, 3))
    return DRTK_ERR_INVALID_ARGUMENT;
  if (weight_kind != IL_W_NONE && (!weight || !il_strides_ok(weight_strides, 2))) return DRTK_ERR_INVALID_ARGUMENT;
  if (mode != IL_MAP && !scalars) return DRTK_ERR_INVALID_ARGUMENT;
  return dispatch_dtype(dtype, [&](auto tag) {
    using T = decltype(tag);
    return il_backward<T>(
        img, img_strides, target, target_strides, weight, weight_kind, weight_strides, N, C, H, W, window_size, g, s, data_range, mode,
        l1_weight, ssim_weight, maps, grad_out, scalars, grad_img, static_cast<hipStream_t>(stream));
  });
}
