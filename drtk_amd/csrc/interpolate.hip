// interpolate -- barycentric interpolation of per-vertex attributes, forward and backward.
//
// Reference: src/interpolate/interpolate_kernel.cu:38-111 (forward), :113-299 (backward).
// Forward: one lane = 4 adjacent pixels, so index/bary loads and every channel-plane store are
// 16-byte vectors; attribute rows are gathered through L1/L2 as float4 when C % 4 == 0.
// Backward: bary_grad is a per-pixel dot product; the vertex-attribute gradient goes through the
// wave-level run reduction of segscatter.hpp in chunks of 16 channels (3*16 = 48 of the wave's 64
// lanes own one (corner, channel) pair each), replacing the reference's per-channel
// WarpReduce + __syncthreads + atomics loop.
#include <string>

#include "common.hpp"
#include "segscatter.hpp"

namespace drtk_amd {
namespace {

template <typename T>
struct Vec4;
template <>
struct Vec4<float> {
  using type = float4;
};
template <>
struct Vec4<double> {
  using type = double4;
};

// (Two pixels per lane instead of four -- half the registers, twice the waves in flight for a kernel whose waves spend
// four gather round trips each -- was measured slower, 0.652 vs 0.543-0.577 ms: the 8-byte stores cost more than the
// occupancy buys.)
// PREFETCH (VEC = CV = 4, more than one channel chunk): the attribute rows of the NEXT chunk are requested before this
// chunk's products and stores.  A wave's life was four dependent gather round trips (SQ counters: 39 k cycles alive for
// 1.7 k cycles of vector issue); with the next chunk in flight the kernel takes 158 instead of 88 VGPRs -- 3 waves per
// SIMD instead of 5 -- and is still faster: 0.573 -> 0.548-0.560 ms on the bench shape, 2.46 -> 2.18 at 8 x 4096^2,
// 1.46 -> 1.30 at C = 32.  With a single chunk (C = 4) there is nothing to prefetch and only the registers are paid
// (0.216 -> 0.232 ms): that case keeps the plain loop.
// ANYW (VEC = 4): any W >= 4 and any element-aligned placement of index / bary / out -- the lane's four consecutive
// pixels may run over the end of a row (each gets its own coordinates for the background sweep), the accesses need the
// element's alignment only, and the last lane of a view whose pixel count is not a multiple of four goes pixel by pixel
// (round 4; before, such images took one pixel per lane: 1.2x the time at 2048 x 2046).
// (round 6: bounded to 4 waves per SIMD -- 128 registers -- the prefetching instantiation spills 30-38 of its 158)
// The index / barycentric quads of the aligned four-pixel lane are non-temporal loads: each is read once (profiles/NOTES.md R12).
template <typename T, int VEC, int CV, bool PREFETCH = false, bool ANYW = false>
__global__ __launch_bounds__(kBlock) void interpolate_kernel(
    const T* __restrict__ attrs, const int32_t* __restrict__ vi,
    const int32_t* __restrict__ index_img, const T* __restrict__ bary_img, int64_t V, int C,
    int64_t vi_sN, int H, int W, T* __restrict__ out, int zero_background, int strip) {
  using V4 = typename Vec4<T>::type;
  const int64_t HW = int64_t(H) * W;
  const int n = blockIdx.y;
  const int64_t pix0 = (int64_t(tile_index(strip)) * kBlock + threadIdx.x) * VEC;
  if (pix0 >= HW) return;
  const T* attrs_n = attrs + int64_t(n) * V * C;
  const int32_t* vi_n = vi + int64_t(n) * vi_sN;
  const int32_t* idx_p = index_img + int64_t(n) * HW + pix0;
  const T* bary_p = bary_img + int64_t(n) * 3 * HW + pix0;
  T* out_p = out + int64_t(n) * C * HW + pix0;

  typedef int32_t IQuad __attribute__((ext_vector_type(4), aligned(4)));
  typedef T TQuad __attribute__((ext_vector_type(4), aligned(sizeof(T))));
  static_assert(!ANYW || VEC == 4, "ANYW is a variant of the four-pixel lane");
  const bool whole = !ANYW || pix0 + 4 <= HW; // all four pixels belong to this view
  int32_t tr[VEC];
  T B0[VEC], B1[VEC], B2[VEC];
  if constexpr (ANYW) {
    if (whole) {
      const IQuad t4 = *reinterpret_cast<const IQuad*>(idx_p);
      tr[0] = t4.x, tr[1] = t4.y, tr[2] = t4.z, tr[3] = t4.w;
      const TQuad a = *reinterpret_cast<const TQuad*>(bary_p);
      const TQuad b = *reinterpret_cast<const TQuad*>(bary_p + HW);
      const TQuad c = *reinterpret_cast<const TQuad*>(bary_p + 2 * HW);
      B0[0] = a.x, B0[1] = a.y, B0[2] = a.z, B0[3] = a.w;
      B1[0] = b.x, B1[1] = b.y, B1[2] = b.z, B1[3] = b.w;
      B2[0] = c.x, B2[1] = c.y, B2[2] = c.z, B2[3] = c.w;
    } else {
#pragma unroll
      for (int j = 0; j < VEC; ++j) {
        const bool in = pix0 + j < HW;
        tr[j] = in ? idx_p[j] : -1;
        B0[j] = in ? bary_p[j] : T(0), B1[j] = in ? bary_p[HW + j] : T(0), B2[j] = in ? bary_p[2 * HW + j] : T(0);
      }
    }
  } else if constexpr (VEC == 4) {
    const NtQuad<int32_t> t4 = nt_load4(idx_p);
    tr[0] = t4.x, tr[1] = t4.y, tr[2] = t4.z, tr[3] = t4.w;
    const NtQuad<T> a = nt_load4(bary_p), b = nt_load4(bary_p + HW), c = nt_load4(bary_p + 2 * HW);
    B0[0] = a.x, B0[1] = a.y, B0[2] = a.z, B0[3] = a.w;
    B1[0] = b.x, B1[1] = b.y, B1[2] = b.z, B1[3] = b.w;
    B2[0] = c.x, B2[1] = c.y, B2[2] = c.z, B2[3] = c.w;
  } else {
    tr[0] = idx_p[0];
    B0[0] = bary_p[0], B1[0] = bary_p[HW], B2[0] = bary_p[2 * HW];
  }
  const int y = static_cast<int>(pix0 / W);
  const int x0 = static_cast<int>(pix0 - int64_t(y) * W);

  const T* a0[VEC];
  const T* a1[VEC];
  const T* a2[VEC];
  T bgx[VEC], bgy[VEC];
  // corner ids of the lane's pixels: UNCONDITIONAL loads (a background pixel reads face 0 and discards it) so that the
  // VEC x 3 of them form one batch -- under `if (covered)` every pixel's three loads sat in their own exec-masked region
  // with an s_waitcnt behind them: four dependent round trips per lane before the first attribute row was requested
  // (a lane with no covered pixel loads nothing -- with F = 0 there is no face to read --; in a lane that has one, its
  // background pixels read that pixel's triangle)
  int32_t t_any = tr[0];
#pragma unroll
  for (int j = 1; j < VEC; ++j) t_any = max(t_any, tr[j]);
  const bool any_cov = t_any != -1;
  int32_t fid[VEC][3];
#pragma unroll
  for (int j = 0; j < VEC; ++j) fid[j][0] = fid[j][1] = fid[j][2] = 0;
  if (any_cov) {
#pragma unroll
    for (int j = 0; j < VEC; ++j) {
      const int32_t* face = vi_n + int64_t(tr[j] != -1 ? tr[j] : t_any) * 3;
#pragma unroll
      for (int k = 0; k < 3; ++k) fid[j][k] = face[k];
    }
  }
#pragma unroll
  for (int j = 0; j < VEC; ++j) {
    a0[j] = attrs_n + int64_t(fid[j][0]) * C;
    a1[j] = attrs_n + int64_t(fid[j][1]) * C;
    a2[j] = attrs_n + int64_t(fid[j][2]) * C;
    // "undefined region" sweep (interpolate_kernel.cu:104-108, CPU twin interpolate_kernel_cpu.cpp:99-104)
    int xj = x0 + j, yj = y;
    if constexpr (ANYW) {
      if (xj >= W) xj -= W, yj += 1; // W >= 4: at most one row further
    }
    bgx[j] = (static_cast<T>(xj) * T(2.0) + T(1.0)) / static_cast<T>(W) - T(1.0);
    bgy[j] = (static_cast<T>(yj) * T(2.0) + T(1.0)) / static_cast<T>(H) - T(1.0);
  }
  // one row of four pixels' values to a channel plane
  auto store4 = [&](T* o, T r0, T r1, T r2, T r3) {
    if constexpr (ANYW) {
      if (whole) {
        *reinterpret_cast<TQuad*>(o) = TQuad{r0, r1, r2, r3};
      } else {
        const T r[4] = {r0, r1, r2, r3};
#pragma unroll
        for (int j = 0; j < 4; ++j)
          if (pix0 + j < HW) o[j] = r[j];
      }
    } else {
      *reinterpret_cast<V4*>(o) = V4{r0, r1, r2, r3}; // (non-temporal stores: 0.534 vs 0.538 ms, round 6 -- nothing)
    }
  };

  if constexpr (PREFETCH) {
    static_assert(CV == 4 && VEC == 4, "the prefetching loop is written for 4 pixels x 4 channels");
    V4 Q[VEC][3], Qn[VEC][3];
    // rows as 32-bit element offsets from attrs_n (V * C < 2^31 on this path, checked by the launcher): 12 registers
    // instead of 24 for the addresses
    uint32_t off[VEC][3];
#pragma unroll
    for (int j = 0; j < VEC; ++j) {
      off[j][0] = static_cast<uint32_t>(a0[j] - attrs_n);
      off[j][1] = static_cast<uint32_t>(a1[j] - attrs_n);
      off[j][2] = static_cast<uint32_t>(a2[j] - attrs_n);
    }
    auto fetch = [&](int c0, V4 (&q)[VEC][3]) {
#pragma unroll
      for (int j = 0; j < VEC; ++j) {
        if (tr[j] != -1) {
#pragma unroll
          for (int k = 0; k < 3; ++k) q[j][k] = *reinterpret_cast<const V4*>(attrs_n + off[j][k] + c0);
        }
      }
    };
    fetch(0, Q);
    for (int c0 = 0; c0 < C; c0 += CV) {
      if (c0 + CV < C) fetch(c0 + CV, Qn);
      T r[CV][VEC];
#pragma unroll
      for (int j = 0; j < VEC; ++j) {
        if (tr[j] != -1) {
          const T u0[4] = {Q[j][0].x, Q[j][0].y, Q[j][0].z, Q[j][0].w};
          const T u1[4] = {Q[j][1].x, Q[j][1].y, Q[j][1].z, Q[j][1].w};
          const T u2[4] = {Q[j][2].x, Q[j][2].y, Q[j][2].z, Q[j][2].w};
#pragma unroll
          for (int cc = 0; cc < CV; ++cc) r[cc][j] = u0[cc] * B0[j] + u1[cc] * B1[j] + u2[cc] * B2[j];
        } else {
#pragma unroll
          for (int cc = 0; cc < CV; ++cc) r[cc][j] = zero_background ? T(0) : (((c0 + cc) & 1) ? bgy[j] : bgx[j]);
        }
      }
#pragma unroll
      for (int cc = 0; cc < CV; ++cc) {
        store4(out_p + int64_t(c0 + cc) * HW, r[cc][0], r[cc][1], r[cc][2], r[cc][3]);
      }
#pragma unroll
      for (int j = 0; j < VEC; ++j) {
#pragma unroll
        for (int k = 0; k < 3; ++k) Q[j][k] = Qn[j][k];
      }
    }
    return;
  }
  for (int c0 = 0; c0 < C; c0 += CV) {
    T r[CV][VEC];
    // the block's attribute rows of all the lane's pixels first (unconditional: a background pixel reads vertex 0), the
    // products after: one round trip per channel block instead of one per pixel
    T u0[VEC][CV], u1[VEC][CV], u2[VEC][CV];
#pragma unroll
    for (int j = 0; j < VEC; ++j) {
      if (!any_cov) break;
      if constexpr (CV == 4) {
        const V4 q0 = *reinterpret_cast<const V4*>(a0[j] + c0);
        const V4 q1 = *reinterpret_cast<const V4*>(a1[j] + c0);
        const V4 q2 = *reinterpret_cast<const V4*>(a2[j] + c0);
        u0[j][0] = q0.x, u0[j][1] = q0.y, u0[j][2] = q0.z, u0[j][3] = q0.w;
        u1[j][0] = q1.x, u1[j][1] = q1.y, u1[j][2] = q1.z, u1[j][3] = q1.w;
        u2[j][0] = q2.x, u2[j][1] = q2.y, u2[j][2] = q2.z, u2[j][3] = q2.w;
      } else {
        u0[j][0] = a0[j][c0], u1[j][0] = a1[j][c0], u2[j][0] = a2[j][c0];
      }
    }
#pragma unroll
    for (int j = 0; j < VEC; ++j) {
      if (tr[j] != -1) {
#pragma unroll
        for (int cc = 0; cc < CV; ++cc) r[cc][j] = u0[j][cc] * B0[j] + u1[j][cc] * B1[j] + u2[j][cc] * B2[j];
      } else {
#pragma unroll
        for (int cc = 0; cc < CV; ++cc) r[cc][j] = zero_background ? T(0) : (((c0 + cc) & 1) ? bgy[j] : bgx[j]);
      }
    }
#pragma unroll
    for (int cc = 0; cc < CV; ++cc) {
      T* o = out_p + int64_t(c0 + cc) * HW;
      if constexpr (VEC == 4) {
        store4(o, r[cc][0], r[cc][1], r[cc][2], r[cc][3]);
      } else {
        o[0] = r[cc][0];
      }
    }
  }
}

// Backward.  A workgroup owns a 64 x 16 pixel tile; each of its 4 waves walks 4 adjacent rows of 64
// pixels (lane = pixel in phase 1) with a wave-private vertex table.  Channels are processed in
// chunks of 16 (outer loop).  No workgroup barrier is needed anywhere.
// CHUNK = channels staged per round.  CHUNK = 4 (C <= 4, e.g. the v_pix route of edge_grad) keeps
// a wave-private vertex table; CHUNK = 16 sends each run's sums straight to global memory -- its 16
// lanes per corner form one 64-byte request, and the smaller LDS footprint buys the occupancy
// that hides phase 1's gather latency (measured faster than the table at C = 16).
template <typename T, bool HAS_VERT, bool HAS_BARY, int CV, int CHUNK>
__global__ __launch_bounds__(kBlock) void interpolate_backward_kernel(
    const T* __restrict__ grad_out, const T* __restrict__ attrs, const int32_t* __restrict__ vi,
    const int32_t* __restrict__ index_img, const T* __restrict__ bary_img, int64_t V, int C,
    int64_t vi_sN, int H, int W, int tiles_x, T* __restrict__ attr_grad, T* __restrict__ bary_grad,
    int dbg, int strip) {
  using V4 = typename Vec4<T>::type;
  constexpr int kWaves = kBlock / kWave;
  constexpr int kPasses = kTileRows / kWaves;
  constexpr bool TABLE = HAS_VERT && CHUNK <= 4;
  __shared__ __attribute__((aligned(16))) T s_g[HAS_VERT ? kWaves : 1][HAS_VERT ? CHUNK * kRunPad : 4];
  __shared__ __attribute__((aligned(16))) T s_b[HAS_VERT ? kWaves : 1][HAS_VERT ? 3 * kRunPad : 4];
  __shared__ int32_t s_vid[HAS_VERT ? kWaves : 1][HAS_VERT ? 3 * kRunPad : 1];
  __shared__ int32_t s_slot[HAS_VERT ? kWaves : 1][HAS_VERT ? 3 * kRunPad : 1];
  __shared__ int32_t t_keys[TABLE ? kWaves : 1][TABLE ? kTableSlots : 1];
  __shared__ TableAcc t_vals[TABLE ? kWaves : 1][TABLE ? kTableSlots * CHUNK : 1];

  const int64_t HW = int64_t(H) * W;
  const int n = blockIdx.y;
  const int tile = tile_index(strip);
  const int tyi = tile / tiles_x, txi = tile - tyi * tiles_x;
  const int wave = threadIdx.x / kWave;
  const int lane = threadIdx.x & (kWave - 1);
  const int x = txi * kWave + lane;
  const T* attrs_n = attrs + int64_t(n) * V * C;
  const int32_t* vi_n = vi + int64_t(n) * vi_sN;
  T* attr_grad_n = HAS_VERT ? attr_grad + int64_t(n) * V * C : nullptr;

  if constexpr (TABLE) table_init(t_keys[wave]);

  for (int c0 = 0; c0 < C; c0 += CHUNK) {
    const int CC = min(CHUNK, C - c0);
    if constexpr (TABLE) {
      wave_lds_sync(); // previous chunk flushed, keys initialised
      for (int i = lane; i < kTableSlots * CHUNK; i += kWave) t_vals[wave][i] = 0;
      wave_lds_sync();
    }
    // software pipeline over the 4 row passes: the index of pass p+1 is requested at the top of
    // pass p and its triangle's vertex ids right before phase 2, so both dependent gathers fly
    // under the current pass instead of in front of the next one.
    auto load_tr = [&](int ps) -> int32_t {
      const int yy = tyi * kTileRows + wave * kPasses + ps;
      return (x < W && yy < H) ? index_img[int64_t(n) * HW + int64_t(yy) * W + x] : -1;
    };
    int32_t tr_next = load_tr(0);
    int32_t vn0 = 0, vn1 = 0, vn2 = 0;
    if (tr_next != -1) {
      const int32_t* face = vi_n + int64_t(tr_next) * 3;
      vn0 = face[0], vn1 = face[1], vn2 = face[2];
    }
#pragma unroll 1
    for (int ps = 0; ps < kPasses; ++ps) {
      const int y = tyi * kTileRows + wave * kPasses + ps;
      const bool in_range = x < W && y < H;
      const int64_t pix = int64_t(y) * W + x;
      const int32_t tr = tr_next;
      const bool covered = tr != -1;
      const int32_t vid0 = vn0, vid1 = vn1, vid2 = vn2;
      if (ps + 1 < kPasses) tr_next = load_tr(ps + 1);
      unsigned long long heads = 0, cov = 0;
      if constexpr (HAS_VERT) {
        T B0 = T(0), B1 = T(0), B2 = T(0);
        if (covered) {
          const T* bp = bary_img + int64_t(n) * 3 * HW + pix;
          B0 = bp[0], B1 = bp[HW], B2 = bp[2 * HW];
        }
        s_b[wave][0 * kRunPad + lane] = B0;
        s_b[wave][1 * kRunPad + lane] = B1;
        s_b[wave][2 * kRunPad + lane] = B2;
        s_vid[wave][0 * kRunPad + lane] = vid0;
        s_vid[wave][1 * kRunPad + lane] = vid1;
        s_vid[wave][2 * kRunPad + lane] = vid2;
        const bool use_table = TABLE && covered && !DRTK_DBG(dbg, 2) && vid0 != vid1 && vid0 != vid2 && vid1 != vid2;
        s_slot[wave][0 * kRunPad + lane] = use_table ? table_slot(t_keys[wave], vid0) : -1;
        s_slot[wave][1 * kRunPad + lane] = use_table ? table_slot(t_keys[wave], vid1) : -1;
        s_slot[wave][2 * kRunPad + lane] = use_table ? table_slot(t_keys[wave], vid2) : -1;
        run_masks(tr, heads, cov);
      }
      T bg0 = T(0), bg1 = T(0), bg2 = T(0);
      if constexpr (HAS_VERT) {
        if (!covered) { // phase 2 sums whole runs of the staging rows: uncovered pixels must read as 0
          for (int cb = 0; cb < CC; ++cb) s_g[wave][cb * kRunPad + lane] = T(0);
        }
      }
      if (covered) {
        const T* go_p = grad_out + int64_t(n) * C * HW + pix;
        const T* a0 = attrs_n + int64_t(vid0) * C;
        const T* a1 = attrs_n + int64_t(vid1) * C;
        const T* a2 = attrs_n + int64_t(vid2) * C;
        for (int cb = 0; cb < CC; cb += CV) {
          T g[CV];
#pragma unroll
          for (int cc = 0; cc < CV; ++cc) g[cc] = DRTK_DBG(dbg, 4) ? T(1) : go_p[int64_t(c0 + cb + cc) * HW];
          if constexpr (HAS_VERT) {
#pragma unroll
            for (int cc = 0; cc < CV; ++cc) s_g[wave][(cb + cc) * kRunPad + lane] = g[cc];
          }
          if (HAS_BARY && !DRTK_DBG(dbg, 8)) {
            T u0[CV], u1[CV], u2[CV];
            if constexpr (CV == 4) {
              const V4 q0 = *reinterpret_cast<const V4*>(a0 + c0 + cb);
              const V4 q1 = *reinterpret_cast<const V4*>(a1 + c0 + cb);
              const V4 q2 = *reinterpret_cast<const V4*>(a2 + c0 + cb);
              u0[0] = q0.x, u0[1] = q0.y, u0[2] = q0.z, u0[3] = q0.w;
              u1[0] = q1.x, u1[1] = q1.y, u1[2] = q1.z, u1[3] = q1.w;
              u2[0] = q2.x, u2[1] = q2.y, u2[2] = q2.z, u2[3] = q2.w;
            } else {
              u0[0] = a0[c0 + cb], u1[0] = a1[c0 + cb], u2[0] = a2[c0 + cb];
            }
#pragma unroll
            for (int cc = 0; cc < CV; ++cc) { // interpolate_kernel.cu:238-246 accumulation order
              bg0 += g[cc] * u0[cc];
              bg1 += g[cc] * u1[cc];
              bg2 += g[cc] * u2[cc];
            }
          }
        }
      }
      if constexpr (HAS_BARY) {
        if (in_range) { // channel chunks accumulate in ascending order, like the reference's loop
          T* bgp = bary_grad + int64_t(n) * 3 * HW + pix;
          if (c0 == 0) {
            bgp[0] = bg0, bgp[HW] = bg1, bgp[2 * HW] = bg2;
          } else if (covered) {
            bgp[0] += bg0, bgp[HW] += bg1, bgp[2 * HW] += bg2;
          }
        }
      }
      if (ps + 1 < kPasses) {
        vn0 = vn1 = vn2 = 0;
        if (tr_next != -1) {
          const int32_t* face = vi_n + int64_t(tr_next) * 3;
          vn0 = face[0], vn1 = face[1], vn2 = face[2];
        }
      }
      if constexpr (HAS_VERT) {
        wave_lds_sync();
        if (cov != 0 && !DRTK_DBG(dbg, 1)) {
          const T* sg = s_g[wave];
          const T* sb = s_b[wave];
          scatter_runs<T>(
              heads, cov, s_slot[wave], s_vid[wave], 3 * CC, CC, t_vals[wave], CHUNK, attr_grad_n, C, c0,
              [=](int k, int c, int g4, T* x) {
                if (DRTK_DBG(dbg, 64)) {
                  x[0] = x[1] = x[2] = x[3] = T(1);
                  return;
                }
                const V4 a = *reinterpret_cast<const V4*>(sg + c * kRunPad + 4 * g4);
                const V4 b = *reinterpret_cast<const V4*>(sb + k * kRunPad + 4 * g4);
                x[0] = a.x * b.x, x[1] = a.y * b.y, x[2] = a.z * b.z, x[3] = a.w * b.w;
              }, dbg);
        }
        wave_lds_sync();
      }
    }
    if constexpr (TABLE) {
      if (!DRTK_DBG(dbg, 16)) table_flush<T>(t_keys[wave], t_vals[wave], CHUNK, CC, attr_grad_n, C, c0);
    }
  }
}

// Backward for C <= 4 (the v_pix route of edge_grad_estimator with a hook, uv attributes, RGB attributes): lane = pixel
// like render backward; the 3 * CN products grad_out[c] * bary[k] stay in registers, a segmented scan over the 16-lane
// rows leaves each run's sums in its last lane (segscatter.hpp: run_sums_rows16), which alone updates the wave's vertex
// table (double accumulators) -- no LDS staging, no lane flip, no barrier in the loop.  The bary gradient is the
// reference's per-pixel dot products (interpolate_kernel.cu:238-246, channels ascending).
template <typename T, bool HAS_VERT, bool HAS_BARY, int CN>
__global__ __launch_bounds__(kBlock) void interpolate_backward_small_kernel(
    const T* __restrict__ grad_out, const T* __restrict__ attrs, const int32_t* __restrict__ vi,
    const int32_t* __restrict__ index_img, const T* __restrict__ bary_img, int64_t V, int64_t vi_sN, int H, int W,
    int tiles_x, T* __restrict__ attr_grad, T* __restrict__ bary_grad, int strip) {
  constexpr int kWaves = kBlock / kWave;
  constexpr int kPasses = kTileRows / kWaves;
  constexpr int kSlots = kTableSlots;
  constexpr int kStride = CN <= 4 ? 4 : CN <= 8 ? 8 : 12; // table entries per vertex
  static_assert(CN >= 1 && CN <= 12, "channels in registers");
  __shared__ int32_t t_keys[HAS_VERT ? kWaves : 1][HAS_VERT ? kSlots : 1];
  __shared__ TableAcc t_vals[HAS_VERT ? kWaves : 1][HAS_VERT ? kSlots * kStride : 1];

  const int64_t HW = int64_t(H) * W;
  const int n = blockIdx.y;
  const int tile = tile_index(strip);
  const int tyi = tile / tiles_x, txi = tile - tyi * tiles_x;
  const int wave = threadIdx.x / kWave;
  const int lane = threadIdx.x & (kWave - 1);
  const int x = txi * kWave + lane;
  const T* attrs_n = attrs + int64_t(n) * V * CN;
  const int32_t* vi_n = vi + int64_t(n) * vi_sN;
  T* attr_grad_n = HAS_VERT ? attr_grad + int64_t(n) * V * CN : nullptr;
  const T* go_n = grad_out + int64_t(n) * CN * HW;
  const T* bary_n = bary_img + int64_t(n) * 3 * HW;

  if constexpr (HAS_VERT) {
    table_init<kSlots>(t_keys[wave]);
    for (int i = lane; i < kSlots * kStride; i += kWave) t_vals[wave][i] = 0;
    wave_lds_sync();
  }
  auto load_tr = [&](int ps) -> int32_t {
    const int yy = tyi * kTileRows + wave * kPasses + ps;
    return (x < W && yy < H) ? index_img[int64_t(n) * HW + int64_t(yy) * W + x] : -1;
  };
  auto load_face = [&](int32_t t, int32_t (&f)[3]) {
    f[0] = f[1] = f[2] = 0;
    if (t != -1) {
      const int32_t* face = vi_n + int64_t(t) * 3;
      f[0] = face[0], f[1] = face[1], f[2] = face[2];
    }
  };
  int32_t tr_next = load_tr(0);
  int32_t vn[3];
  load_face(tr_next, vn);
#pragma unroll 1
  for (int ps = 0; ps < kPasses; ++ps) {
    const int y = tyi * kTileRows + wave * kPasses + ps;
    const bool in_range = x < W && y < H;
    const int64_t pix = int64_t(y) * W + x;
    const int32_t tr = tr_next;
    const bool covered = tr != -1;
    const int32_t cur[3] = {vn[0], vn[1], vn[2]};
    if (ps + 1 < kPasses) tr_next = load_tr(ps + 1);
    T g[CN], B[3] = {T(0), T(0), T(0)};
#pragma unroll
    for (int c = 0; c < CN; ++c) g[c] = T(0);
    if (covered) {
#pragma unroll
      for (int c = 0; c < CN; ++c) g[c] = go_n[int64_t(c) * HW + pix];
      if constexpr (HAS_VERT) {
#pragma unroll
        for (int k = 0; k < 3; ++k) B[k] = bary_n[int64_t(k) * HW + pix];
      }
    }
    if constexpr (HAS_BARY) {
      T bg[3] = {T(0), T(0), T(0)};
      if (covered) {
#pragma unroll
        for (int c = 0; c < CN; ++c) { // interpolate_kernel.cu:238-246 accumulation order
#pragma unroll
          for (int k = 0; k < 3; ++k) bg[k] += g[c] * attrs_n[int64_t(cur[k]) * CN + c];
        }
      }
      if (in_range) {
        T* bgp = bary_grad + int64_t(n) * 3 * HW + pix;
        bgp[0] = bg[0], bgp[HW] = bg[1], bgp[2 * HW] = bg[2];
      }
    }
    if (ps + 1 < kPasses) load_face(tr_next, vn);
    if constexpr (HAS_VERT) {
      int dist;
      bool tail;
      run_rows16(tr, dist, tail);
      if (__ballot(covered) != 0) {
        T p[3 * CN];
#pragma unroll
        for (int k = 0; k < 3; ++k) {
#pragma unroll
          for (int c = 0; c < CN; ++c) p[k * CN + c] = g[c] * B[k];
        }
        run_sums_rows16<T, 3 * CN>(p, dist);
        if (tail && covered) table_add<T, 3, CN, kSlots>(t_keys[wave], t_vals[wave], kStride, cur, p, attr_grad_n, CN);
      }
    }
  }
  if constexpr (HAS_VERT) {
    wave_lds_sync();
    table_flush<T, TableAcc, kSlots>(t_keys[wave], t_vals[wave], kStride, CN, attr_grad_n, CN, 0);
  }
}

// Backward, wide-channel path: the vertex gradient (with or without the bary gradient) for any C % 4 == 0, C >= 8,
// f32, 16-byte aligned attribute rows.  (Round 4: rounds 1-3 had this pipeline for C % 16 == 0 with both gradients only;
// every other shape fell back to the generic kernel above.)
//
// Same tiling as interpolate_backward_kernel -- a workgroup owns 64 x 16 pixels, each wave walks 4 adjacent rows of 64
// pixels, lane = pixel in phase 1, lane = (corner, channel) in phase 2 -- but written so that no memory round trip is
// ever waited for in isolation (the generic kernel's phase 1 is a chain of up to nine dependent global waits per row --
// index, corners, bary, then go/attribute loads per 4-channel block -- and PMC shows its waves parked on s_waitcnt
// 72 % of their life):
//   * ROW-outer, channel-chunk-inner: index, corner ids and barycentrics of a row are fetched and staged ONCE, whatever
//     C is, and the bary gradient of a pixel accumulates in registers over all chunks in the reference's channel order
//     (interpolate_kernel.cu:238-246) and is stored once -- a chunk-outer loop re-reads 16 B/px and read-modify-writes
//     24 B/px of bary_grad per extra chunk, i.e. costs more per channel at C = 64 than at C = 16;
//   * channels go in chunks of 16 with a last chunk of 4, 8 or 12 (scatter_runs folds 12 / 24 (corner, channel) pairs
//     into 4 / 2 pixel slices of the wave, so the lanes stay busy);
//   * every global load of a step (<= 16 grad_out planes, first half of the attribute rows) is issued in one batch, and
//     the NEXT step's grad_out planes (next chunk of this row, or first chunk + barycentrics of the next row) are
//     requested before the current step's phase 2, so they land while the wave is busy in LDS;
//   * the per-pixel bary-gradient dot products run after phase 2 and read grad_out back from the LDS staging rows, which
//     frees the registers for the prefetch.
//   * TABLE (round 4): the run sums do not go to global memory run by run but into a table of the WORKGROUP in LDS --
//     2^log2_slots vertices x C double accumulators, filled by all four waves with ds_add_f64, slots looked up once per
//     row by the lanes that start a run -- and the tile's 64 x 16 pixels cost one global atomic per vertex and channel at
//     the end.  Per-run atomics are what the counters show as write traffic beyond bary_grad (864 MB against 403 MB at
//     the bench shape), and on rows that are not a multiple of 64 bytes (C = 12, 24) they are several times slower still.
//     A vertex that finds no slot keeps the direct atomics.
//   * ANYC (round 5): channel counts that are not a multiple of four (C >= 5: position + normal = 6, RGB + k features) and
//     attribute tensors that are only element-aligned.  The last chunk is then 1 ... 15 channels: its grad_out planes are
//     still fetched in groups of four, the planes beyond C through a descriptor of ZERO records (they read 0.0 without
//     touching memory); the attribute rows' last, partial group of four is read as the four channels that END the row
//     (window shifted back by 4 - r: never a byte beyond the row, element alignment only) and its dot products skip the
//     channels the previous group already took; phase 2 is channel-count agnostic (J = 3 cc lanes).  Rows of such a C
//     are never whole 64-byte segments, so the run sums go through the workgroup's vertex table.
//   * double (round 5): the same pipeline in chunks of CH = 8 channels (the registers of 16 floats), 8-byte buffer loads.
// Waves per SIMD the wide kernel is compiled for: 4 (128 VGPRs) for every float flavour -- the chunk of 12 takes 104 with the bary
// gradient and spills 4-12 at 5 --, 3 for double (144-152 VGPRs; 32-50 spilled at 4).
constexpr int kWideWaves = 4;
constexpr int kWideWavesF64 = 3;
// Cache policy of the grad_out / bary plane loads: 2 = nt, each plane is read once per launch (0 = the default policy was slower).
constexpr int kPlaneLoadAux = 2;
// Groups of four attribute channels per corner requested BEFORE phase 2 (the rest after it): with ANYC and the bary gradient more
// than one spills at 4 waves per SIMD.
constexpr int kAttrGroupsAhead = 1;
// ANYC, 16-channel chunks: the last group is requested only after the products of the others (124 instead of 138 VGPRs: 4 waves).
constexpr bool kAnycSplitLastGroup = true;
template <typename T, bool HAS_BARY, bool TABLE, int CH, bool ANYC>
__global__ __launch_bounds__(kBlock, (sizeof(T) == 8 ? kWideWavesF64 : kWideWaves)) void interpolate_backward_wide_kernel(
    const T* __restrict__ grad_out, const T* __restrict__ attrs, const int32_t* __restrict__ vi,
    const int32_t* __restrict__ index_img, const T* __restrict__ bary_img, int64_t V, int C,
    int64_t vi_sN, int H, int W, int tiles_x, T* __restrict__ attr_grad, T* __restrict__ bary_grad,
    int dbg, int strip, int log2_slots, int CG) { // CG: elements between the rows of attr_grad (C, or the padded pitch of the workspace)
  using V4 = typename Vec4<T>::type;
  static_assert(CH % 4 == 0 && CH >= 8 && CH <= 16, "chunks of 8 or 16 channels");
  constexpr int kWaves = kBlock / kWave;
  constexpr int kPasses = kTileRows / kWaves;
  static_assert(kPasses == 4, "row pipeline below is written for 4 rows per wave");
  __shared__ __attribute__((aligned(16))) T s_g[kWaves][CH * kRunPad];
  __shared__ __attribute__((aligned(16))) T s_b[kWaves][3 * kRunPad];
  __shared__ int32_t s_vid[kWaves][3 * kRunPad];
  __shared__ int32_t s_slot[TABLE ? kWaves : 1][TABLE ? 3 * kRunPad : 1];
  extern __shared__ __attribute__((aligned(16))) unsigned char s_table_raw[]; // TABLE: [slots][C] doubles, then [slots] keys
  TableAcc* const t_vals = reinterpret_cast<TableAcc*>(s_table_raw);
  int32_t* const t_keys = reinterpret_cast<int32_t*>(t_vals + (TABLE ? (size_t(C) << log2_slots) : 0));

  const int64_t HW = int64_t(H) * W;
  const int n = blockIdx.y;
  const int tile = tile_index(strip);
  const int tyi = tile / tiles_x, txi = tile - tyi * tiles_x;
  const int wave = threadIdx.x / kWave;
  const int lane = threadIdx.x & (kWave - 1);
  const int x = txi * kWave + lane;
  const int y0 = tyi * kTileRows + wave * kPasses;
  const T* attrs_n = attrs + int64_t(n) * V * C;
  const int32_t* vi_n = vi + int64_t(n) * vi_sN;
  T* attr_grad_n = attr_grad + int64_t(n) * V * CG;
  const T* go_n = grad_out + int64_t(n) * C * HW;
  const T* bary_n = bary_img + int64_t(n) * 3 * HW;
  T* bgrad_n = HAS_BARY ? bary_grad + int64_t(n) * 3 * HW : nullptr;
  if constexpr (TABLE) {
    for (int i = threadIdx.x; i < (C << log2_slots); i += kBlock) t_vals[i] = 0;
    for (int i = threadIdx.x; i < (1 << log2_slots); i += kBlock) t_keys[i] = -1;
  }

  auto load_tr = [&](int ps) -> int32_t {
    const int y = y0 + ps;
    return (ps < kPasses && x < W && y < H) ? index_img[int64_t(n) * HW + int64_t(y) * W + x] : -1;
  };
  auto load_face = [&](int32_t t, int32_t& a0, int32_t& a1, int32_t& a2) {
    a0 = a1 = a2 = 0;
    if (t != -1) {
      const int32_t* face = vi_n + int64_t(t) * 3;
      a0 = face[0], a1 = face[1], a2 = face[2];
    }
  };

  // A wave whose 64 x 4 pixels are all background (43 % of them at the benchmark's coverage) has nothing to
  // scatter: it zeroes its part of bary_grad and leaves (TABLE: stays for the barriers of a tile that has foreground).
  bool wave_fg;
  {
    int32_t t4[kPasses];
#pragma unroll
    for (int ps = 0; ps < kPasses; ++ps) t4[ps] = load_tr(ps);
    const bool any_fg = (t4[0] & t4[1] & t4[2] & t4[3]) != -1;
    wave_fg = __ballot(any_fg) != 0;
    bool tile_fg = wave_fg;
    if constexpr (TABLE) tile_fg = __syncthreads_or(wave_fg) != 0; // (also orders the table's zero-fill before its first use)
    if (!wave_fg) {
      if constexpr (HAS_BARY) {
        int yz = y0; // (recomputed from a laundered copy: kept from the index loads above, the row predicates were spilled)
        asm volatile("" : "+v"(yz));
#pragma unroll
        for (int ps = 0; ps < kPasses; ++ps) {
          const int y = yz + ps;
          if (x < W && y < H) {
            T* bgp = bgrad_n + int64_t(y) * W + x;
            bgp[0] = T(0), bgp[HW] = T(0), bgp[2 * HW] = T(0);
          }
        }
      }
      if (!TABLE || !tile_fg) return;
    }
  }

  if (wave_fg) {
  T G[CH], B[3];
  // grad_out planes c0 .. c0 + cc - 1 of row ps (cc = 4, 8, 12 or 16: wave-uniform); zeros where uncovered
  // Loads of a row's operands: UNCONDITIONAL per lane (the offset of a lane off the canvas is clamped; what an uncovered
  // pixel reads is never used: phase 2 flushes covered runs only and restarts its sums at every run head, the bary
  // gradient is computed for covered pixels only), skipped for a row with no covered pixel at all (wave-uniform).  A
  // per-lane `covered ? load : 0` puts every group of loads into its own exec-masked region with its own s_waitcnt --
  // the prefetch became four dependent round trips (0.65 -> 0.72 ms at C = 16 when the tail chunks were introduced).
  // Plane bases are wave-uniform and the in-plane offset is a 32-bit lane value (H W < 2^31): SGPR base + VGPR offset.
  // The 16 + 3 plane loads of a row go through BUFFER loads: one descriptor per plane (wave-uniform: SGPRs) and ONE
  // 32-bit byte offset register for all of them (H W < 2^30 on this path, checked by the launcher; a lane off the canvas
  // is out of the plane's range and reads 0).  As global loads the compiler built a 64-bit address per load and, at the
  // register bound, recycled registers that were still load destinations as address temporaries -- an s_waitcnt
  // vmcnt(0) in the middle of the batch.
  const uint32_t plane_bytes = static_cast<uint32_t>(HW * int64_t(sizeof(T)));
  auto plane_load = [&](const T* plane, uint32_t byte_offset, bool exists) -> T { // `exists`: wave-uniform (ANYC: a plane < C)
    const __amdgpu_buffer_rsrc_t r = __builtin_amdgcn_make_buffer_rsrc(const_cast<T*>(plane), 0, exists ? static_cast<int>(plane_bytes) : 0, 0x00020000);
    if constexpr (sizeof(T) == 4) {
      return __builtin_bit_cast(T, __builtin_amdgcn_raw_buffer_load_b32(r, byte_offset, 0, kPlaneLoadAux));
    } else {
      return __builtin_bit_cast(T, __builtin_amdgcn_raw_buffer_load_b64(r, byte_offset, 0, kPlaneLoadAux));
    }
  };
  auto row_offset = [&](int ps) -> uint32_t { // beyond the plane for a lane off the canvas
    return (x < W && y0 + ps < H) ? static_cast<uint32_t>((y0 + ps) * W + x) * static_cast<uint32_t>(sizeof(T)) : plane_bytes;
  };
  // one call site, one offset register for grad_out and barycentrics (with an offset of its own the bary loads got a
  // freshly written register, and the compiler waited for the grad_out loads before writing it)
  // (plane bases by repeated addition of H W: written as go_n + (c0 + c) H W every plane cost a 64-bit scalar multiply,
  // eight scalar instructions -- the kernel issued more scalar than vector instructions, 152 M against 126 M per launch)
  auto load_row = [&](int ps, int c0, int cc, bool row_any, bool with_bary) {
    if (!row_any) return;
    const uint32_t bo = row_offset(ps);
    const T* plane = go_n + int64_t(c0) * HW;
#pragma unroll
    for (int q = 0; q < CH / 4; ++q) {
      if (4 * q < cc) {
#pragma unroll
        for (int c = 4 * q; c < 4 * q + 4; ++c) {
          G[c] = plane_load(plane, bo, !ANYC || c < cc);
          plane += HW;
        }
      }
    }
    if (with_bary) {
      const T* bplane = bary_n;
#pragma unroll
      for (int k = 0; k < 3; ++k) {
        B[k] = plane_load(bplane, bo, true);
        bplane += HW;
      }
    }
  };
  // rotating state: row ps (tr, v*), row ps+1 (tr_n, vn*), row ps+2 (tr_nn)
  int32_t tr = load_tr(0), tr_n = load_tr(1), tr_nn = -1;
  int32_t v0, v1, v2, vn0 = 0, vn1 = 0, vn2 = 0;
  load_face(tr, v0, v1, v2);
#pragma unroll
  for (int c = 0; c < CH; ++c) G[c] = T(0);
  B[0] = B[1] = B[2] = T(0);
  load_row(0, 0, min(CH, C), __ballot(tr != -1) != 0, true);
  // ONE loop over (row, chunk) steps, rows outer: as two nested loops the compiler kept ~45 more values live across the
  // inner one (173 instead of 128 VGPRs: spills at 4 waves per SIMD)
  unsigned long long heads = 0, cov = 0;
  T bg0 = T(0), bg1 = T(0), bg2 = T(0);
  int ps = 0, c0 = 0;
#pragma unroll 1
  for (;;) {
    const bool covered = tr != -1;
    if (c0 == 0) {
      // 0. the two CONDITIONAL fetches of the rows ahead come first: `cond ? load : default` compiles to a branch around
      //    the load with an s_waitcnt vmcnt(0) inside it; issued after the next row's 19 loads (as they used to be) that
      //    wait held the wave until all of them had landed, before the phase 2 they were meant to fly under (0.659 ->
      //    0.650 ms; making the two fetches unconditional instead cost registers and was slower, 0.675)
      if (ps + 1 < kPasses) {
        load_face(tr_n, vn0, vn1, vn2);
        tr_nn = load_tr(ps + 2);
      }
      // 1. what the row's chunks share: barycentrics, corner ids, run structure
#pragma unroll
      for (int k = 0; k < 3; ++k) s_b[wave][k * kRunPad + lane] = B[k];
      s_vid[wave][0 * kRunPad + lane] = v0;
      s_vid[wave][1 * kRunPad + lane] = v1;
      s_vid[wave][2 * kRunPad + lane] = v2;
      run_masks(tr, heads, cov);
      bg0 = bg1 = bg2 = T(0);
      if constexpr (TABLE) {
        // table slots of the row's runs, looked up by the lanes that START a covered run (phase 2 reads them there)
        int s0 = -1, s1 = -1, s2 = -1;
        if (covered && ((heads >> lane) & 1ull) && !DRTK_DBG(dbg, 2)) {
          s0 = table_slot_rt(t_keys, v0, log2_slots);
          s1 = table_slot_rt(t_keys, v1, log2_slots);
          s2 = table_slot_rt(t_keys, v2, log2_slots);
        }
        s_slot[wave][0 * kRunPad + lane] = s0;
        s_slot[wave][1 * kRunPad + lane] = s1;
        s_slot[wave][2 * kRunPad + lane] = s2;
      }
    }
    const int cc = min(CH, C - c0); // 4, 8, 12 or 16 (ANYC: anything from 1)
    const bool last_chunk = c0 + CH >= C;
    // 2. stage this chunk's grad_out
#pragma unroll
    for (int q = 0; q < CH / 4; ++q) {
      if (4 * q < cc) {
#pragma unroll
        for (int c = 4 * q; c < 4 * q + 4; ++c) s_g[wave][c * kRunPad + lane] = G[c];
      }
    }
    // 3. first half of the attribute rows of this row's triangles (consumed after phase 2)
    const T* a0 = attrs_n + int64_t(v0) * C + c0;
    const T* a1 = attrs_n + int64_t(v1) * C + c0;
    const T* a2 = attrs_n + int64_t(v2) * C + c0;
    // float4 per corner requested before / after phase 2 (kAttrGroupsAhead, kAnycSplitLastGroup: profiles/NOTES.md R12)
    constexpr int QA = kAttrGroupsAhead, QD = CH / 4 - QA;
    // group q of a row's chunk: channels 4q .. 4q+3, or (ANYC, the chunk's partial last group) the four that end the row
    typedef T TQuadU __attribute__((ext_vector_type(4), aligned(sizeof(T))));
    auto attr4 = [&](const T* row, int q) -> V4 {
      if constexpr (ANYC) {
        const int ws = 4 * q + 4 <= cc ? 4 * q : cc - 4; // wave-uniform; c0 + cc - 4 >= 1 (C >= 5)
        const TQuadU u = *reinterpret_cast<const TQuadU*>(row + ws);
        return V4{u.x, u.y, u.z, u.w};
      } else {
        return *reinterpret_cast<const V4*>(row + 4 * q);
      }
    };
    V4 A0[QA > 0 ? QA : 1], A1[QA > 0 ? QA : 1], A2[QA > 0 ? QA : 1];
    if constexpr (HAS_BARY) {
      if (covered) {
#pragma unroll
        for (int q = 0; q < QA; ++q) {
          if (4 * q < cc) {
            A0[q] = attr4(a0, q);
            A1[q] = attr4(a1, q);
            A2[q] = attr4(a2, q);
          }
        }
      }
    }
    // 4. the next step's operands fly under phase 2: the next chunk of this row, or the first chunk (and the
    //    barycentrics) of the next row
    //    (ONE load site for both cases: with two, the compiler loaded into temporaries and copied them into G behind an
    //    s_waitcnt vmcnt(0) straight after the loads -- the prefetch waited for itself)
    {
      const int n_ps = last_chunk ? ps + 1 : ps, n_c0 = last_chunk ? 0 : c0 + CH;
      const bool n_any = last_chunk ? (ps + 1 < kPasses && __ballot(tr_n != -1) != 0) : cov != 0;
      load_row(n_ps, n_c0, min(CH, C - n_c0), n_any, last_chunk);
    }
    wave_lds_sync();
    // 5. phase 2: run sums per (corner, channel) lane -> one 64-byte atomic request per corner and run
    //    (a per-vertex LDS table in front of the atomics was measured slower here, twice: 1.01 vs 0.83 ms in round 1;
    //    1.07 vs 0.65 ms in round 2 with a float table and slots looked up at run heads only -- the flush it saves is
    //    0.11 ms, but the table's bookkeeping takes the kernel from 126 to 171 VGPRs, i.e. from 4 to 2 waves per SIMD.
    //    A per-wave cache keyed by TRIANGLE instead -- the run loop is scalar, so the lookup is one v_cmp + s_ff1 on a
    //    VGPR of keys and costs no registers (128 VGPRs, 4 waves kept) -- merges the rows of the wave's 64 x 4 pixels
    //    and was also slower: 0.666 vs 0.654 ms with 16 float entries updated by read-add-write (the LDS round trip
    //    sits on every run's critical path), 0.692 with 8, 0.74 with 16 double entries and fire-and-forget ds_add_f64
    //    (51 KB of LDS per workgroup: 3 waves per SIMD).  Round 3: CARRYING the sums of the vertices two consecutive
    //    runs share (neighbouring triangles share an edge) from run to run instead of flushing them -- which corner
    //    continues as which decided by the scalar unit, the sums moved between the corner rows by one ds_bpermute, a
    //    third of the atomic requests -- is correct and much slower: 0.901 vs 0.648 ms (1.096 vs 0.731 at 250k
    //    triangles); the per-run scalar chain (vertex ids to SGPRs, nine compares, the permute's round trip) sits on
    //    the one wave's critical path, the atomics it saves were fire-and-forget)
    if (cov != 0 && !DRTK_DBG(dbg, 1)) {
      const T* sg = s_g[wave];
      const T* sb = s_b[wave];
      // (the table + bary variant sits at its register bound: it keeps the unpipelined reads)
      scatter_runs_rows<T, TableAcc, /*WIDE_ONLY=*/false, TABLE, 16, !(TABLE && HAS_BARY)>(
          heads, cov, TABLE ? s_slot[wave] : nullptr, s_vid[wave], 3 * cc, cc, t_vals, C, attr_grad_n, CG, c0, sg, sb, dbg,
          TABLE ? c0 : 0);
    }
    // 6. bary gradient: interpolate_kernel.cu:238-246 accumulation order (channels ascending, over all chunks)
    if constexpr (HAS_BARY) {
      if (covered && !DRTK_DBG(dbg, 8)) {
        V4 D0[QD], D1[QD], D2[QD]; // the rest: requested now, used after the first part's products
        // (row addresses rebuilt from laundered ids: carried over phase 2 as three 64-bit pointers they were spilled)
        int32_t w0 = v0, w1 = v1, w2 = v2;
        asm volatile("" : "+v"(w0), "+v"(w1), "+v"(w2));
        const T* d0 = attrs_n + int64_t(w0) * C + c0;
        const T* d1 = attrs_n + int64_t(w1) * C + c0;
        const T* d2 = attrs_n + int64_t(w2) * C + c0;
        // (ANYC at four waves per SIMD: the last group is requested only after the products of the others -- twelve registers
        // less in flight, one more round trip per chunk)
        constexpr int QD1 = (ANYC && CH == 16 && kAnycSplitLastGroup && QD > 1) ? QD - 1 : QD; // (12-channel chunks fit without: 0.69 vs 0.71 ms at C = 11)
#pragma unroll
        for (int q = 0; q < QD1; ++q) {
          if (4 * (QA + q) < cc) {
            D0[q] = attr4(d0, QA + q);
            D1[q] = attr4(d1, QA + q);
            D2[q] = attr4(d2, QA + q);
          }
        }
        auto dot4 = [&](int q4, const V4& u0, const V4& u1, const V4& u2) {
          if constexpr (ANYC) {
            if (4 * q4 + 4 > cc) { // the partial group: the window holds channels cc-4 .. cc-1, the first `skip` are done
              const int base = cc - 4, skip = 4 * q4 - base;
              const T* sgp = &s_g[wave][lane] + base * kRunPad;
              if (skip <= 1) {
                const T g1 = sgp[1 * kRunPad];
                bg0 += g1 * u0.y, bg1 += g1 * u1.y, bg2 += g1 * u2.y;
              }
              if (skip <= 2) {
                const T g2 = sgp[2 * kRunPad];
                bg0 += g2 * u0.z, bg1 += g2 * u1.z, bg2 += g2 * u2.z;
              }
              const T g3 = sgp[3 * kRunPad];
              bg0 += g3 * u0.w, bg1 += g3 * u1.w, bg2 += g3 * u2.w;
              return;
            }
          }
          const T g0 = s_g[wave][(4 * q4 + 0) * kRunPad + lane], g1 = s_g[wave][(4 * q4 + 1) * kRunPad + lane];
          const T g2 = s_g[wave][(4 * q4 + 2) * kRunPad + lane], g3 = s_g[wave][(4 * q4 + 3) * kRunPad + lane];
          bg0 += g0 * u0.x, bg1 += g0 * u1.x, bg2 += g0 * u2.x;
          bg0 += g1 * u0.y, bg1 += g1 * u1.y, bg2 += g1 * u2.y;
          bg0 += g2 * u0.z, bg1 += g2 * u1.z, bg2 += g2 * u2.z;
          bg0 += g3 * u0.w, bg1 += g3 * u1.w, bg2 += g3 * u2.w;
        };
#pragma unroll
        for (int q = 0; q < QA; ++q) {
          if (4 * q < cc) dot4(q, A0[q], A1[q], A2[q]);
        }
#pragma unroll
        for (int q = 0; q < QD1; ++q) {
          if (4 * (QA + q) < cc) dot4(QA + q, D0[q], D1[q], D2[q]);
        }
        if constexpr (QD1 < QD) {
          if (4 * (QA + QD1) < cc) {
            asm volatile("" ::: "memory"); // (keeps the request behind the products above)
            const V4 e0 = attr4(d0, QA + QD1), e1 = attr4(d1, QA + QD1), e2 = attr4(d2, QA + QD1);
            dot4(QA + QD1, e0, e1, e2);
          }
        }
      }
    }
    wave_lds_sync(); // the next step overwrites the staging rows
    c0 += CH;
    if (last_chunk) {
      if constexpr (HAS_BARY) {
        const int y = y0 + ps;
        if (x < W && y < H) {
          T* bgp = bgrad_n + int64_t(y) * W + x;
          bgp[0] = bg0, bgp[HW] = bg1, bgp[2 * HW] = bg2;
        }
      }
      tr = tr_n, v0 = vn0, v1 = vn1, v2 = vn2;
      tr_n = tr_nn;
      c0 = 0;
      if (++ps == kPasses) break;
    }
  }
  } // wave_fg
  if constexpr (TABLE) {
    // the tile's vertices to global memory: consecutive lanes = consecutive channels of a vertex (one request per 16)
    __syncthreads();
    if (!DRTK_DBG(dbg, 16)) {
      for (int e = threadIdx.x; e < (C << log2_slots); e += kBlock) {
        const int sl = e / C, c = e - sl * C;
        const int32_t key = t_keys[sl];
        if (key >= 0) {
          const T xv = static_cast<T>(t_vals[e]);
          if (xv != T(0)) atomic_add_global(attr_grad_n + int64_t(key) * CG + c, xv);
        }
      }
    }
  }
}

// rows of CG elements -> rows of C (the padded gradient workspace of the wide pipeline back into attr_grad)
template <typename T>
__global__ __launch_bounds__(kBlock) void compact_rows_kernel(const T* __restrict__ ws, T* __restrict__ out, int64_t count, int C, int CG) {
  const int64_t i = int64_t(blockIdx.x) * kBlock + threadIdx.x;
  if (i >= count) return;
  const int64_t r = i / C;
  out[i] = ws[r * CG + (i - r * C)];
}

// ---- launching -----------------------------------------------------------------------------------------------------------------
// The launch helpers of this file are templates: they name the instantiation they launch by its values (common.hpp:
// instance_name, launch_as), so that the timing report says which kernel ran.

// ---- forward -------------------------------------------------------------------------------------------------------------------
// double never prefetches: the prefetching loop needs 254 VGPRs there -- one wave per SIMD -- and loses to the plain one at two
template <typename T>
constexpr bool kForwardPrefetch = sizeof(T) == 4;

template <typename T>
struct ForwardCall {  // the entry point's arguments
  const T* attrs;
  const int32_t *vi, *index_img;
  const T* bary_img;
  int64_t N, V, C, vi_sN, H, W;
  T* out;
  int zero_background;
  hipStream_t stream;
};

template <typename T, int VEC, int CV, bool PREFETCH, bool ANYW>
void launch_forward(const ForwardCall<T>& c) {
  static const std::string name = instance_name<VEC, CV, PREFETCH, ANYW>("interpolate_kernel");
  launch_as(
      name, interpolate_kernel<T, VEC, CV, PREFETCH, ANYW>,
      dim3(static_cast<unsigned>(ceil_div(ceil_div(c.H * c.W, VEC), kBlock)), static_cast<unsigned>(c.N)), kBlock, 0, c.stream, c.attrs, c.vi,
      c.index_img, c.bary_img, c.V, (int)c.C, c.vi_sN, (int)c.H, (int)c.W, c.out, c.zero_background,
      xcd_strip(ceil_div(16 * c.W, int64_t(kBlock) * VEC)));
}
// CV and PREFETCH of a (VEC, ANYW) pair; the prefetching loop exists for four pixels x four channels of float only
template <typename T, int VEC, bool ANYW>
void launch_forward_channels(const ForwardCall<T>& c, bool cvec, bool prefetch) {
  if constexpr (VEC == 4 && kForwardPrefetch<T>) {
    if (prefetch) return launch_forward<T, 4, 4, true, ANYW>(c);
  }
  if (cvec) launch_forward<T, VEC, 4, false, ANYW>(c); else launch_forward<T, VEC, 1, false, ANYW>(c);
}

template <typename T>
int interpolate_impl(
    const T* attrs, const int32_t* vi, const int32_t* index_img, const T* bary_img, int64_t N,
    int64_t V, int64_t C, int64_t vi_sN, int64_t H, int64_t W, T* out, int zero_background, hipStream_t stream) {
  if (N * H * W * C == 0) return DRTK_OK;
  // whole 16-byte aligned quads of pixels: W % 4 == 0 and aligned images
  const bool pvec = (W % 4 == 0) && (reinterpret_cast<uintptr_t>(index_img) % 16 == 0) &&
      (reinterpret_cast<uintptr_t>(bary_img) % (4 * sizeof(T)) == 0) &&
      (reinterpret_cast<uintptr_t>(out) % (4 * sizeof(T)) == 0);
  // the four template arguments:
  const int vec = pvec || W >= 4 ? 4 : 1;  // VEC: pixels per lane
  const bool anyw = !pvec && W >= 4;       // ANYW: widths that are not a multiple of four, views into flat buffers
  const bool cvec = (C % 4 == 0) && (reinterpret_cast<uintptr_t>(attrs) % (4 * sizeof(T)) == 0);  // CV = 4: attribute rows as vectors
  // PREFETCH: more than one channel vector, and 32-bit row offsets in the prefetching loop
  const bool prefetch = kForwardPrefetch<T> && vec == 4 && cvec && C > 4 && V * C < (int64_t(1) << 31);
  const ForwardCall<T> c{attrs, vi, index_img, bary_img, N, V, C, vi_sN, H, W, out, zero_background, stream};
  if (anyw)
    launch_forward_channels<T, 4, true>(c, cvec, prefetch);
  else if (vec == 4)
    launch_forward_channels<T, 4, false>(c, cvec, prefetch);
  else
    launch_forward_channels<T, 1, false>(c, cvec, false);
  DRTK_RETURN_IF_LAUNCH_FAILED();
  return DRTK_OK;
}

// ---- backward: the routing plan ------------------------------------------------------------------------------------------------
// elements between the rows of the padded gradient workspace: whole 64-byte segments
template <typename T>
inline int64_t padded_row(int64_t C) {
  const int64_t seg = 64 / int64_t(sizeof(T));
  return (C + seg - 1) / seg * seg;
}
template <typename T>
inline bool rows_are_segments(int64_t C) {
  const size_t row_bytes = sizeof(T) * C;
  return row_bytes % 64 == 0 || 64 % row_bytes == 0;
}

// The thresholds of the rule; the measurements behind each are in profiles/NOTES.md R12.
// tests/scatter_table_cases.py builds its index images from five of them and reads them from this file BY SPELLING: the three
// macros below, and the literals of `int log2_slots = ...` and `table = log2_slots >= ...` in plan_backward.  Plain constants,
// not switches: nothing tests for a definition from outside.
// The register scan beats the wide pipeline while 3 C products per lane are few (the wide phase 2 keeps 3 C of 64 lanes busy).
#define DRTK_INTERP_SMALL_MAXC_F32 10
#define DRTK_INTERP_SMALL_MAXC_F64 7
template <typename T>
constexpr int kSmallMaxC = sizeof(T) == 4 ? DRTK_INTERP_SMALL_MAXC_F32 : DRTK_INTERP_SMALL_MAXC_F64;
// Channel counts the register scan is instantiated for; the bary gradient alone (no scatter) takes it up to here.
constexpr int kSmallInstMaxC = 12;
// double rows that are not 32-byte aligned (C % 4 != 0) stay with the register scan up to here: 9 measured, 10 / 11 by the trend.
constexpr int kSmallMaxCF64Unaligned = 11;
static_assert(kSmallMaxC<float> <= kSmallInstMaxC && kSmallMaxC<double> <= kSmallInstMaxC && kSmallMaxCF64Unaligned <= kSmallInstMaxC, "instantiated channel counts");
// Channels per round of the wide pipeline: 16 floats, or their registers' worth of doubles.
template <typename T>
constexpr int kWideChunk = sizeof(T) == 4 ? 16 : 8;
// float, element-aligned rows of 9 ... 12 channels with the bary gradient: ONE chunk of 12 (the 16-channel chunk's registers put
// that flavour at 3 waves per SIMD).
constexpr int kChunk12AboveC = 8;
constexpr int kChunk12MaxC = 12;
// Padded rows pay while the row is one chunk; with a tail chunk the table, which merges a vertex's chunks, wins.
constexpr int kPadMaxC = 16;
// The workgroup's vertex table: as many slots as fit this much LDS (the staging rows take 27 KB; 4 workgroups per CU leave 40 KB
// each), at most 2^7, and used from 2^4 -- below that, per-run atomics (the two literals in plan_backward).
#define DRTK_INTERP_TABLE_BYTES 12800

enum class BackwardRoute { kScan, kWide, kGeneric };
struct BackwardPlan {
  BackwardRoute route = BackwardRoute::kGeneric;
  // kWide: the run sums go through the workgroup's table of 2^log2_slots vertices (lds bytes) / into workspace rows padded to CG
  // elements, compacted afterwards; channels per round
  bool table = false, padded = false;
  int chunk = 0, log2_slots = 0, CG = 0;
  size_t lds = 0;
  // kGeneric: channels per attribute load, channels per round
  int cv = 1, generic_chunk = 16;
};

// Which kernel the backward launches, and how.  cvec: C % 4 == 0 and 16-byte (double: 32-byte) aligned attributes; ws_usable: a
// workspace is there and holds N V padded rows.  force_generic / no_table: the profiling build's flags 128 / 4096 (false in the
// product).
//   * register scan (interpolate_backward_small_kernel) for few channels,
//   * else the wide pipeline wherever the vertex gradient is wanted (any C >= 5, float and double; 32-bit byte offsets into a
//     plane), its run sums going -- rows of whole 64-byte segments: straight to global memory; other rows of one chunk, both
//     gradients, float, with a workspace: to PADDED rows, which then are such segments; other rows otherwise: through the table,
//   * else the generic kernel: the bary gradient alone beyond the register scan's counts (no scatter, covered pixels only: 0.95 of
//     the HBM peak), planes of 4 GB and more.
template <typename T>
BackwardPlan plan_backward(int64_t C, int64_t HW, bool want_attr, bool want_bary, bool cvec, bool ws_usable, bool force_generic, bool no_table) {
  BackwardPlan p;
  p.CG = static_cast<int>(C);
  const bool small_c = C <= kSmallMaxC<T> || (!want_attr && C <= kSmallInstMaxC) || (sizeof(T) == 8 && C % 4 != 0 && C <= kSmallMaxCF64Unaligned);
  if (force_generic || (!small_c && !(want_attr && HW * int64_t(sizeof(T)) < (int64_t(1) << 32)))) {
    p.route = BackwardRoute::kGeneric;
    // (attributes only: no attribute row is read; C <= 4 keeps a wave-private table, beyond it the run sums go to global memory)
    p.cv = cvec && want_bary ? 4 : 1;
    p.generic_chunk = want_attr && C <= 4 ? 4 : 16;
  } else if (small_c) {
    p.route = BackwardRoute::kScan;
  } else {
    p.route = BackwardRoute::kWide;
    p.padded = ws_usable && !rows_are_segments<T>(C) && want_bary && sizeof(T) == 4 && C <= kPadMaxC;
    if (p.padded) p.CG = static_cast<int>(padded_row<T>(C));
    int log2_slots = 7;
    while (log2_slots > 0 && (sizeof(TableAcc) * C + 4) * (size_t(1) << log2_slots) > DRTK_INTERP_TABLE_BYTES) --log2_slots;
    p.log2_slots = log2_slots;
    // on rows of whole segments the table's lookups and barriers cost more than the fire-and-forget atomics they replace
    p.table = log2_slots >= 4 && !p.padded && !rows_are_segments<T>(C) && !no_table;
    p.lds = p.table ? (sizeof(TableAcc) * C + 4) * (size_t(1) << p.log2_slots) : 0;
    const bool chunk12 = sizeof(T) == 4 && !cvec && C > kChunk12AboveC && C <= kChunk12MaxC && want_bary;
    p.chunk = chunk12 ? 12 : kWideChunk<T>;
  }
  return p;
}

// ---- backward: launching what the plan says ------------------------------------------------------------------------------------
template <typename T>
struct BackwardCall {  // what the three kernels share: their arguments in the kernels' order and types, the grid of 64 x 16 tiles
  const T *grad_out, *attrs;
  const int32_t *vi, *index_img;
  const T* bary_img;
  int64_t V;
  int C;
  int64_t vi_sN;
  int H, W, tiles_x;
  T *attr_grad, *bary_grad;
  int strip;
  dim3 grid;
  hipStream_t stream;
};

template <typename T, bool HAS_VERT, bool HAS_BARY, int CN>
void launch_scan(const BackwardCall<T>& c) {
  static const std::string name = instance_name<HAS_VERT, HAS_BARY, CN>("interpolate_backward_small_kernel");
  launch_as(
      name, interpolate_backward_small_kernel<T, HAS_VERT, HAS_BARY, CN>, c.grid, kBlock, 0, c.stream, c.grad_out, c.attrs, c.vi, c.index_img,
      c.bary_img, c.V, c.vi_sN, c.H, c.W, c.tiles_x, c.attr_grad, c.bary_grad, c.strip);
}
// the instantiation of c.C, 1 ... kSmallInstMaxC
template <typename T, bool HAS_VERT, bool HAS_BARY, int CN = kSmallInstMaxC>
void launch_scan_channels(const BackwardCall<T>& c) {
  if (c.C == CN)
    launch_scan<T, HAS_VERT, HAS_BARY, CN>(c);
  else if constexpr (CN > 1)
    launch_scan_channels<T, HAS_VERT, HAS_BARY, CN - 1>(c);
}

template <typename T, bool HAS_BARY, bool TABLE, int CH, bool ANYC>
void launch_wide(const BackwardCall<T>& c, const BackwardPlan& p, T* grad_dst) {
  static const std::string name = instance_name<HAS_BARY, TABLE, CH, ANYC>("interpolate_backward_wide_kernel");
  launch_as(
      name, interpolate_backward_wide_kernel<T, HAS_BARY, TABLE, CH, ANYC>, c.grid, kBlock, p.lds, c.stream, c.grad_out, c.attrs, c.vi,
      c.index_img, c.bary_img, c.V, c.C, c.vi_sN, c.H, c.W, c.tiles_x, grad_dst, c.bary_grad, debug_flags(), c.strip, p.log2_slots, p.CG);
}
// TABLE and CH of a (HAS_BARY, ANYC) pair; the chunk of 12 exists for float with the bary gradient on element-aligned rows only
template <typename T, bool HAS_BARY, bool ANYC>
void launch_wide_chunk(const BackwardCall<T>& c, const BackwardPlan& p, T* grad_dst) {
  if constexpr (sizeof(T) == 4 && HAS_BARY && ANYC) {
    if (p.chunk == 12) return p.table ? launch_wide<T, HAS_BARY, true, 12, ANYC>(c, p, grad_dst) : launch_wide<T, HAS_BARY, false, 12, ANYC>(c, p, grad_dst);
  }
  if (p.table)
    launch_wide<T, HAS_BARY, true, kWideChunk<T>, ANYC>(c, p, grad_dst);
  else
    launch_wide<T, HAS_BARY, false, kWideChunk<T>, ANYC>(c, p, grad_dst);
}

template <typename T, bool HAS_VERT, bool HAS_BARY, int CV, int CHUNK>
void launch_generic(const BackwardCall<T>& c) {
  static const std::string name = instance_name<HAS_VERT, HAS_BARY, CV, CHUNK>("interpolate_backward_kernel");
  launch_as(
      name, interpolate_backward_kernel<T, HAS_VERT, HAS_BARY, CV, CHUNK>, c.grid, kBlock, 0, c.stream, c.grad_out, c.attrs, c.vi, c.index_img,
      c.bary_img, c.V, c.C, c.vi_sN, c.H, c.W, c.tiles_x, c.attr_grad, c.bary_grad, debug_flags(), c.strip);
}

template <typename T>
int interpolate_backward_impl(
    const T* grad_out, const T* attrs, const int32_t* vi, const int32_t* index_img,
    const T* bary_img, int64_t N, int64_t V, int64_t C, int64_t vi_sN, int64_t H, int64_t W,
    T* attr_grad, T* bary_grad, T* ws, size_t ws_bytes, hipStream_t stream) {
  const int64_t HW = H * W;
  auto zero_grad = [&](bool to_ws) -> int {  // the zero-fill goes where the atomics will
    if (!attr_grad || N * V * C == 0) return DRTK_OK;
    return to_ws ? fill_bytes_async(ws, 0, sizeof(T) * N * V * padded_row<T>(C), stream) : fill_bytes_async(attr_grad, 0, sizeof(T) * N * V * C, stream);
  };
  if (N * HW == 0 || C == 0) {
    if (zero_grad(false) != DRTK_OK) return DRTK_ERR_LAUNCH;
  }
  if (N * HW == 0) return DRTK_OK;
  if (C == 0) {
    if (bary_grad && fill_bytes_async(bary_grad, 0, sizeof(T) * N * 3 * HW, stream) != DRTK_OK) return DRTK_ERR_LAUNCH;
    return DRTK_OK;
  }
  const bool cvec = (C % 4 == 0) && (reinterpret_cast<uintptr_t>(attrs) % (4 * sizeof(T)) == 0);
  const bool ws_usable = ws && N * V * C > 0 && ws_bytes >= sizeof(T) * size_t(N * V * padded_row<T>(C)) && padded_row<T>(C) < (int64_t(1) << 30);
  const BackwardPlan p = plan_backward<T>(
      C, HW, attr_grad != nullptr, bary_grad != nullptr, cvec, ws_usable, DRTK_DBG(debug_flags(), 128), DRTK_DBG(debug_flags(), 4096));
  if (zero_grad(p.padded) != DRTK_OK) return DRTK_ERR_LAUNCH;

  const int tiles_x = static_cast<int>(ceil_div(W, kWave)), tiles_y = static_cast<int>(ceil_div(H, kTileRows));
  const BackwardCall<T> c{
      grad_out, attrs, vi, index_img, bary_img, V, (int)C, vi_sN, (int)H, (int)W, tiles_x, attr_grad, bary_grad,
      xcd_strip(int64_t(tiles_x) * (16 / kTileRows)), dim3(static_cast<unsigned>(int64_t(tiles_x) * tiles_y), static_cast<unsigned>(N)), stream};
  const bool a = attr_grad != nullptr, b = bary_grad != nullptr, v4 = p.cv == 4, c4 = p.generic_chunk == 4;
  switch (p.route) {
    case BackwardRoute::kScan:
      if (a && b) launch_scan_channels<T, true, true>(c);
      else if (a) launch_scan_channels<T, true, false>(c);
      else launch_scan_channels<T, false, true>(c);
      break;
    case BackwardRoute::kWide: {  // ANYC = !cvec
      T* const grad_dst = p.padded ? ws : attr_grad;
      if (b && cvec) launch_wide_chunk<T, true, false>(c, p, grad_dst);
      else if (b) launch_wide_chunk<T, true, true>(c, p, grad_dst);
      else if (cvec) launch_wide_chunk<T, false, false>(c, p, grad_dst);
      else launch_wide_chunk<T, false, true>(c, p, grad_dst);
      break;
    }
    case BackwardRoute::kGeneric:
      if (a && b && c4) { if (v4) launch_generic<T, true, true, 4, 4>(c); else launch_generic<T, true, true, 1, 4>(c); }
      else if (a && b) { if (v4) launch_generic<T, true, true, 4, 16>(c); else launch_generic<T, true, true, 1, 16>(c); }
      else if (a) { if (c4) launch_generic<T, true, false, 1, 4>(c); else launch_generic<T, true, false, 1, 16>(c); }
      else { if (v4) launch_generic<T, false, true, 4, 16>(c); else launch_generic<T, false, true, 1, 16>(c); }
      break;
  }
  DRTK_RETURN_IF_LAUNCH_FAILED();
  if (p.padded) {
    const int64_t count = N * V * C;
    DRTK_LAUNCH((compact_rows_kernel<T>), dim3(static_cast<unsigned>(ceil_div(count, kBlock))), dim3(kBlock), 0, stream, ws, attr_grad, count, (int)C, p.CG);
    DRTK_RETURN_IF_LAUNCH_FAILED();
  }
  return DRTK_OK;
}

// ---- argument checks shared by the entry points ------------------------------------------------------------------------------------
bool bad_common(int64_t N, int64_t V, int64_t C, int64_t F, int64_t vi_sN, int64_t H, int64_t W) {
  return bad_image(N, H, W) || V < 0 || C < 0 || F < 0 || C >= (1 << 20) || bad_view_stride(vi_sN, F * 3);
}
// ... after the sizes, in this order: the per-pixel pointers (pixel_ptrs: the caller's are all there), the per-vertex ones, and
// the dtype last
bool bad_inputs(drtk_dtype_t dtype, const void* attrs, const int32_t* vi, bool pixel_ptrs, int64_t N, int64_t V, int64_t C, int64_t F, int64_t H, int64_t W) {
  if (N * H * W * C > 0 && !pixel_ptrs) return true;
  if ((N * V * C > 0 && !attrs) || (F > 0 && !vi)) return true;
  return !valid_dtype(dtype);
}

} // namespace
} // namespace drtk_amd

using namespace drtk_amd;

static int interpolate_entry(
    drtk_dtype_t dtype, const void* attrs, const int32_t* vi, const int32_t* index_img,
    const void* bary_img, int64_t N, int64_t V, int64_t C, int64_t F, int64_t vi_sN, int64_t H,
    int64_t W, void* out, int zero_background, drtk_stream_t stream) {
  if (bad_common(N, V, C, F, vi_sN, H, W)) return DRTK_ERR_INVALID_ARGUMENT;
  if (bad_inputs(dtype, attrs, vi, index_img && bary_img && out, N, V, C, F, H, W)) return DRTK_ERR_INVALID_ARGUMENT;
  const size_t es = dtype_size(dtype);
  if (N > kMaxViewsPerLaunch) return for_view_slices(N, [&](int64_t n0, int64_t n) {
    return interpolate_entry(
        dtype, advance(attrs, n0 * V * C, es), advance_typed(vi, n0 * vi_sN), advance_typed(index_img, n0 * H * W),
        advance(bary_img, n0 * 3 * H * W, es), n, V, C, F, vi_sN, H, W, advance(out, n0 * C * H * W, es), zero_background, stream);
  });
  return dispatch_dtype(dtype, [&](auto tag) {
    using T = decltype(tag);
    return interpolate_impl<T>(
        static_cast<const T*>(attrs), vi, index_img, static_cast<const T*>(bary_img), N, V, C, vi_sN, H, W, static_cast<T*>(out),
        zero_background, static_cast<hipStream_t>(stream));
  });
}

extern "C" int drtk_amd_interpolate(
    drtk_dtype_t dtype, const void* attrs, const int32_t* vi, const int32_t* index_img,
    const void* bary_img, int64_t N, int64_t V, int64_t C, int64_t F, int64_t vi_sN, int64_t H,
    int64_t W, void* out, drtk_stream_t stream) {
  return interpolate_entry(dtype, attrs, vi, index_img, bary_img, N, V, C, F, vi_sN, H, W, out, 0, stream);
}

extern "C" int drtk_amd_interpolate_masked(
    drtk_dtype_t dtype, const void* attrs, const int32_t* vi, const int32_t* index_img,
    const void* bary_img, int64_t N, int64_t V, int64_t C, int64_t F, int64_t vi_sN, int64_t H,
    int64_t W, void* out, drtk_stream_t stream) {
  return interpolate_entry(dtype, attrs, vi, index_img, bary_img, N, V, C, F, vi_sN, H, W, out, 1, stream);
}

// The workspace is the padded rows of the plan: the size is asked of the plan itself -- both gradients wanted, a workspace that
// is usable -- and is zero wherever it does not pad (the plan's padding depends on neither the image size nor the alignment).
extern "C" int drtk_amd_interpolate_backward_workspace_bytes(drtk_dtype_t dtype, int64_t N, int64_t V, int64_t C, size_t* bytes) {
  if (!bytes || N < 0 || V < 0 || C < 0) return DRTK_ERR_INVALID_ARGUMENT;
  return dispatch_dtype(dtype, [&](auto tag) {
    using T = decltype(tag);
    const BackwardPlan p = plan_backward<T>(C, 0, true, true, true, true, false, false);
    *bytes = (p.padded && N * V > 0) ? sizeof(T) * size_t(N * V * p.CG) : 0;
    return DRTK_OK;
  });
}

extern "C" int drtk_amd_interpolate_backward_ws(
    drtk_dtype_t dtype, const void* grad_out, const void* attrs, const int32_t* vi,
    const int32_t* index_img, const void* bary_img, int64_t N, int64_t V, int64_t C, int64_t F,
    int64_t vi_sN, int64_t H, int64_t W, void* attr_grad, void* bary_grad, void* workspace, size_t workspace_bytes,
    drtk_stream_t stream) {
  if (bad_common(N, V, C, F, vi_sN, H, W)) return DRTK_ERR_INVALID_ARGUMENT;
  if (!attr_grad && !bary_grad) {
    // A null output is one that was not requested OR is empty (N*V*C == 0 / N*H*W == 0; an empty tensor has no
    // storage): either way there is nothing to write.  Requesting nothing is an error only when both gradients
    // would have had elements.
    return (N * V * C > 0 && N * H * W > 0) ? DRTK_ERR_INVALID_ARGUMENT : DRTK_OK;
  }
  if (bad_inputs(dtype, attrs, vi, grad_out && index_img && bary_img, N, V, C, F, H, W)) return DRTK_ERR_INVALID_ARGUMENT;
  if (workspace && reinterpret_cast<uintptr_t>(workspace) % 64 != 0) return DRTK_ERR_INVALID_ARGUMENT; // rows of whole 64-byte segments
  const size_t es = dtype_size(dtype);
  // (slices of views reuse the workspace: each call leaves nothing in it)
  if (N > kMaxViewsPerLaunch) return for_view_slices(N, [&](int64_t n0, int64_t n) {
    return drtk_amd_interpolate_backward_ws(
        dtype, advance(grad_out, n0 * C * H * W, es), advance(attrs, n0 * V * C, es), advance_typed(vi, n0 * vi_sN),
        advance_typed(index_img, n0 * H * W), advance(bary_img, n0 * 3 * H * W, es), n, V, C, F, vi_sN, H, W,
        advance(attr_grad, n0 * V * C, es), advance(bary_grad, n0 * 3 * H * W, es), workspace, workspace_bytes, stream);
  });
  return dispatch_dtype(dtype, [&](auto tag) {
    using T = decltype(tag);
    return interpolate_backward_impl<T>(
        static_cast<const T*>(grad_out), static_cast<const T*>(attrs), vi, index_img, static_cast<const T*>(bary_img), N, V, C, vi_sN, H, W,
        static_cast<T*>(attr_grad), static_cast<T*>(bary_grad), static_cast<T*>(workspace), workspace_bytes, static_cast<hipStream_t>(stream));
  });
}

extern "C" int drtk_amd_interpolate_backward(
    drtk_dtype_t dtype, const void* grad_out, const void* attrs, const int32_t* vi,
    const int32_t* index_img, const void* bary_img, int64_t N, int64_t V, int64_t C, int64_t F,
    int64_t vi_sN, int64_t H, int64_t W, void* attr_grad, void* bary_grad, drtk_stream_t stream) {
  return drtk_amd_interpolate_backward_ws(dtype, grad_out, attrs, vi, index_img, bary_img, N, V, C, F, vi_sN, H, W, attr_grad, bary_grad, nullptr, 0, stream);
}
