// Closest-point queries: for every query p[n,i] the nearest target q[n,j] by brute force, and the gradients of the squared
// distance, without atomics (no counterpart in the reference's library).  The definition, the launch rule and the order of
// every sum are stated in include/drtk_amd.h ("Closest-point queries").
//
//   forward       a workgroup keeps kQueries = kBlock * kR queries of one view in registers, kR per lane as kR / 2 packed
//                 pairs, and walks its range of the targets in LDS tiles of kTile (x, y, z, pad: one 16-byte broadcast read
//                 per target for float, amortised over the lane's kR queries).  d2 = (dx*dx + dy*dy) + dz*dz, each operation
//                 rounded as written (the pairs compile to v_pk_add_f32 / v_pk_mul_f32, IEEE per element); the running minimum
//                 and its index stay in registers, and since j ascends the strict `<` keeps the lowest index.  A NaN or +inf d2
//                 never passes `d2 < best` (best starts at +inf), which is the whole rejection rule; the padding of a partial tile
//                 and the queries past P are NaN for the same reason.  Targets are taken in groups: the compare-and-select runs
//                 only for a group in which some query of the wave improves (see the loop).
//   merge         with S > 1 ranges: one lane per query takes the ranges' partials in ascending order with a strict `<`.
//   grad_p        one lane per query: a gather of q[idx] and a coalesced write; a shared p adds the views in double, n ascending.
//   grad_q        chunk pass: one workgroup per (view, chunk of kChunk sorted positions).  Lane l takes position c*kChunk + l of
//                 the caller's stable sort, forms its term -2 g (p - q) in double and stages it with its target in LDS; the lane
//                 at the head of a run of one target (inside the chunk) adds the run's terms in ascending position and stores the
//                 sum at the head's position of the workspace, and every lane stores its target to the sorted keys.
//                 target pass: one lane per target bisects the sorted keys for its run [lo, hi), adds the sums stored at lo and
//                 at the first position of every later chunk the run reaches, in ascending chunk order (shared q: then the
//                 views, n ascending), rounds once and writes -- zeros for an empty run.  It is the only writer of grad_q.
#include "common.hpp"

#include <limits>

namespace drtk_amd {
namespace {

constexpr int kR = DRTK_NEAREST_R;            // queries per lane
constexpr int kQueries = DRTK_NEAREST_QUERIES; // queries per workgroup
constexpr int kTile = DRTK_NEAREST_TILE;       // targets per LDS tile
constexpr int kSplitBlocks = DRTK_NEAREST_SPLIT_BLOCKS;
constexpr int kChunk = DRTK_NEAREST_CHUNK;     // sorted positions per workgroup of the grad_q chunk pass
constexpr int kUnroll = 8;                     // targets per step of the inner loop; a partial tile is padded to it with NaN
static_assert(kQueries == kBlock * kR && kR % 2 == 0 && kTile % kUnroll == 0 && kChunk == kBlock, "include/drtk_amd.h");

template <typename T>
using Pair = T __attribute__((ext_vector_type(2)));

// fmin: the operand that is not NaN when one is (v_min_f32 / v_min_f64 under IEEE rules)
__device__ __forceinline__ float min_num(float a, float b) { return __builtin_fminf(a, b); }
__device__ __forceinline__ double min_num(double a, double b) { return __builtin_fmin(a, b); }

// The launch rule of include/drtk_amd.h: S ranges of L targets each.
struct Split {
  int64_t S, L;
};
inline Split split_rule(int64_t N, int64_t P, int64_t M) {
  const int64_t B = N * ceil_div(P, kQueries);
  if (B <= 0 || B >= kSplitBlocks || M <= kTile) return {1, M};
  const int64_t tiles = ceil_div(M, kTile);
  const int64_t want = ceil_div(kSplitBlocks, B);
  const int64_t S0 = want < tiles ? want : tiles;
  const int64_t L = ceil_div(ceil_div(M, S0), kTile) * kTile;
  return {ceil_div(M, L), L};
}

template <typename T>
__global__ __launch_bounds__(kBlock) void nearest_forward_kernel(
    const T* __restrict__ p, int64_t p_sN, int64_t p_sP, const T* __restrict__ q, int64_t q_sN, int64_t q_sM, int32_t P,
    int32_t M, int32_t blocks_per_view, int32_t S, int32_t L, T* __restrict__ out_d, int32_t* __restrict__ out_i) {
  __shared__ __attribute__((aligned(16))) T tile[kTile * 4];
  const T nan = std::numeric_limits<T>::quiet_NaN();
  const T inf = std::numeric_limits<T>::infinity();
  const int64_t b = int64_t(blockIdx.x) / S;
  const int32_t s = int32_t(int64_t(blockIdx.x) - b * S);
  const int64_t n = b / blocks_per_view;
  const int32_t i0 = int32_t(b - n * blocks_per_view) * kQueries + int32_t(threadIdx.x); // < P + kQueries <= 2^31 + 1023: checked by the entry point

  Pair<T> px[kR / 2], py[kR / 2], pz[kR / 2], best[kR / 2];
  int32_t bi[kR];
  const T* pn = p + n * p_sN;
#pragma unroll
  for (int r = 0; r < kR; ++r) {
    const int32_t i = i0 + r * kBlock;
    const bool in = i < P;
    const T* pi = pn + int64_t(in ? i : 0) * p_sP;
    px[r / 2][r % 2] = in ? pi[0] : nan;
    py[r / 2][r % 2] = in ? pi[1] : nan;
    pz[r / 2][r % 2] = in ? pi[2] : nan;
    best[r / 2][r % 2] = inf;
    bi[r] = -1;
  }

  const int64_t begin64 = int64_t(s) * L;
  const int32_t begin = int32_t(begin64 < M ? begin64 : M);
  const int32_t end = int32_t(begin64 + L < M ? begin64 + L : M);
  const T* qn = q + n * q_sN;
  for (int32_t j0 = begin; j0 < end; j0 += kTile) {
    const int32_t cnt = end - j0 < kTile ? end - j0 : kTile;
    const int32_t padded = (cnt + kUnroll - 1) / kUnroll * kUnroll;
    __syncthreads(); // the previous tile has been read by every wave
    for (int32_t t = threadIdx.x; t < padded; t += kBlock) {
      T x = nan, y = nan, z = nan;
      if (t < cnt) {
        const T* qj = qn + int64_t(j0 + t) * q_sM;
        x = qj[0], y = qj[1], z = qj[2];
      }
      tile[t * 4] = x, tile[t * 4 + 1] = y, tile[t * 4 + 2] = z, tile[t * 4 + 3] = T(0);
    }
    __syncthreads();
    // A group of G targets at a time: the distances, then their minimum per query (min ignores a NaN operand, and a
    // minimum that is NaN or +inf is not below `best`).  Only when some query of the wave has a distance below its best
    // -- a handful of times per query over the whole range -- are the group's targets taken one by one with the strict
    // `<`, which is then exactly the sequential scan: no distance of a skipped group would have passed it.
    constexpr int G = sizeof(T) == 4 ? kUnroll : kUnroll / 2;
    for (int32_t t = 0; t < padded; t += G) {
      Pair<T> d[G][kR / 2];
#pragma unroll
      for (int u = 0; u < G; ++u) {
        const T qx = tile[(t + u) * 4], qy = tile[(t + u) * 4 + 1], qz = tile[(t + u) * 4 + 2];
#pragma unroll
        for (int h = 0; h < kR / 2; ++h) {
          const Pair<T> dx = px[h] - qx, dy = py[h] - qy, dz = pz[h] - qz;
          d[u][h] = (dx * dx + dy * dy) + dz * dz;
        }
      }
      bool below = false;
#pragma unroll
      for (int h = 0; h < kR / 2; ++h) {
#pragma unroll
        for (int e = 0; e < 2; ++e) {
          T m = d[0][h][e];
#pragma unroll
          for (int u = 1; u < G; ++u) m = min_num(m, d[u][h][e]);
          below = below | (m < best[h][e]);
        }
      }
      if (__builtin_amdgcn_ballot_w64(below) != 0) { // wave-uniform
#pragma unroll
        for (int u = 0; u < G; ++u) {
          const int32_t j = j0 + t + u;
#pragma unroll
          for (int h = 0; h < kR / 2; ++h) {
#pragma unroll
            for (int e = 0; e < 2; ++e) {
              const bool lt = d[u][h][e] < best[h][e];
              best[h][e] = lt ? d[u][h][e] : best[h][e];
              bi[h * 2 + e] = lt ? j : bi[h * 2 + e];
            }
          }
        }
      }
    }
  }

  // S == 1: the outputs [N,P]; S > 1: the partials [N,S,P]
  const int64_t row = (n * S + s) * int64_t(P);
#pragma unroll
  for (int r = 0; r < kR; ++r) {
    const int32_t i = i0 + r * kBlock;
    if (i < P) {
      out_d[row + i] = best[r / 2][r % 2];
      out_i[row + i] = bi[r];
    }
  }
}

template <typename T>
__global__ __launch_bounds__(kBlock) void nearest_merge_kernel(
    const T* __restrict__ part_d, const int32_t* __restrict__ part_i, int64_t N, int64_t P, int32_t S, T* __restrict__ dist2,
    int32_t* __restrict__ idx) {
  const int64_t t = int64_t(blockIdx.x) * kBlock + threadIdx.x;
  if (t >= N * P) return;
  const int64_t n = t / P, i = t - n * P;
  T best = std::numeric_limits<T>::infinity();
  int32_t bi = -1;
  for (int32_t s = 0; s < S; ++s) {
    const int64_t o = (n * S + s) * P + i;
    const T d = part_d[o];
    if (d < best) best = d, bi = part_i[o];
  }
  dist2[t] = best;
  idx[t] = bi;
}

// one lane per (view, query), or per query over the views (sum_views)
template <typename T>
__global__ __launch_bounds__(kBlock) void nearest_grad_p_kernel(
    const T* __restrict__ g, const T* __restrict__ p, int64_t p_sN, int64_t p_sP, const T* __restrict__ q, int64_t q_sN,
    int64_t q_sM, const int32_t* __restrict__ idx, int64_t N, int64_t P, bool sum_views, T* __restrict__ grad_p) {
  const int64_t t = int64_t(blockIdx.x) * kBlock + threadIdx.x;
  if (t >= (sum_views ? P : N * P)) return;
  const int64_t n0 = sum_views ? 0 : t / P, n1 = sum_views ? N : n0 + 1, i = sum_views ? t : t - n0 * P;
  double acc[3] = {0.0, 0.0, 0.0};
  T one[3] = {T(0), T(0), T(0)};
  for (int64_t n = n0; n < n1; ++n) {
    const int32_t j = idx[n * P + i];
    one[0] = one[1] = one[2] = T(0);
    if (j >= 0) {
      const T two_g = T(2) * g[n * P + i];
      const T* pi = p + n * p_sN + i * p_sP;
      const T* qj = q + n * q_sN + int64_t(j) * q_sM;
#pragma unroll
      for (int a = 0; a < 3; ++a) one[a] = two_g * (pi[a] - qj[a]);
    }
#pragma unroll
    for (int a = 0; a < 3; ++a) acc[a] += double(one[a]);
  }
  T* o = grad_p + t * 3;
#pragma unroll
  for (int a = 0; a < 3; ++a) o[a] = sum_views ? T(acc[a]) : one[a];
}

// chunk pass of grad_q: one workgroup per (view, chunk)
template <typename T>
__global__ __launch_bounds__(kBlock) void nearest_grad_q_chunk_kernel(
    const T* __restrict__ g, const T* __restrict__ p, int64_t p_sN, int64_t p_sP, const T* __restrict__ q, int64_t q_sN,
    int64_t q_sM, const int32_t* __restrict__ idx, const int32_t* __restrict__ order, int64_t P, int64_t chunks_per_view,
    double* __restrict__ sums, int32_t* __restrict__ keys) {
  __shared__ double term[3][kChunk];
  __shared__ int32_t key[kChunk];
  const int64_t n = int64_t(blockIdx.x) / chunks_per_view;
  const int64_t c = int64_t(blockIdx.x) - n * chunks_per_view;
  const int l = threadIdx.x;
  const int64_t pos = c * kChunk + l;
  const int cnt = int(P - c * kChunk < kChunk ? P - c * kChunk : kChunk);
  int32_t j = -1;
  double v[3] = {0.0, 0.0, 0.0};
  if (l < cnt) {
    const int64_t i = order[n * P + pos];
    j = idx[n * P + i];
    keys[n * P + pos] = j;
    if (j >= 0) {
      const double m2g = -2.0 * double(g[n * P + i]);
      const T* pi = p + n * p_sN + i * p_sP;
      const T* qj = q + n * q_sN + int64_t(j) * q_sM;
#pragma unroll
      for (int a = 0; a < 3; ++a) v[a] = m2g * (double(pi[a]) - double(qj[a]));
    }
  }
  key[l] = j;
#pragma unroll
  for (int a = 0; a < 3; ++a) term[a][l] = v[a];
  __syncthreads();
  if (l < cnt && j >= 0 && (l == 0 || key[l - 1] != j)) {
    double s[3] = {v[0], v[1], v[2]};
    for (int m = l + 1; m < cnt && key[m] == j; ++m) {
#pragma unroll
      for (int a = 0; a < 3; ++a) s[a] += term[a][m];
    }
    double* o = sums + (n * P + pos) * 3;
    o[0] = s[0], o[1] = s[1], o[2] = s[2];
  }
}

// first position in keys[0, P) whose key is >= j (keys ascending)
__device__ __forceinline__ int64_t lower_bound_key(const int32_t* __restrict__ keys, int64_t P, int64_t j) {
  int64_t lo = 0, hi = P;
  while (lo < hi) {
    const int64_t mid = (lo + hi) >> 1;
    if (keys[mid] < j) lo = mid + 1;
    else hi = mid;
  }
  return lo;
}

// target pass of grad_q: one lane per (view, target), or per target over the views (sum_views)
template <typename T>
__global__ __launch_bounds__(kBlock) void nearest_grad_q_target_kernel(
    const double* __restrict__ sums, const int32_t* __restrict__ keys, int64_t N, int64_t P, int64_t M, bool sum_views,
    T* __restrict__ grad_q) {
  const int64_t t = int64_t(blockIdx.x) * kBlock + threadIdx.x;
  if (t >= (sum_views ? M : N * M)) return;
  const int64_t n0 = sum_views ? 0 : t / M, n1 = sum_views ? N : n0 + 1, j = sum_views ? t : t - n0 * M;
  double total[3] = {0.0, 0.0, 0.0};
  for (int64_t n = n0; n < n1; ++n) {
    const int32_t* kn = keys + n * P;
    const int64_t lo = lower_bound_key(kn, P, j);
    if (lo >= P || kn[lo] != j) continue;
    const int64_t hi = lower_bound_key(kn, P, j + 1);
    const double* sn = sums + n * P * 3;
    double s[3] = {sn[lo * 3], sn[lo * 3 + 1], sn[lo * 3 + 2]};
    const int64_t c1 = (hi - 1) / kChunk;
    int64_t c = lo / kChunk + 1;
    // eight chunk sums in flight, added in chunk order (at the start of a fit one target holds every chunk of a view)
    for (; c + 8 <= c1 + 1; c += 8) {
      double x[8][3];
#pragma unroll
      for (int u = 0; u < 8; ++u)
#pragma unroll
        for (int a = 0; a < 3; ++a) x[u][a] = sn[(c + u) * kChunk * 3 + a];
#pragma unroll
      for (int u = 0; u < 8; ++u)
#pragma unroll
        for (int a = 0; a < 3; ++a) s[a] += x[u][a];
    }
    for (; c <= c1; ++c)
#pragma unroll
      for (int a = 0; a < 3; ++a) s[a] += sn[c * kChunk * 3 + a];
#pragma unroll
    for (int a = 0; a < 3; ++a) total[a] = sum_views ? total[a] + s[a] : s[a];
  }
  T* o = grad_q + t * 3;
#pragma unroll
  for (int a = 0; a < 3; ++a) o[a] = T(total[a]);
}

constexpr int64_t kMaxBlocks = (int64_t(1) << 31) - 1;
constexpr int64_t kMaxPoints = (int64_t(1) << 31) - kQueries; // i0 + r * kBlock stays an int32

bool bad_sizes(int64_t N, int64_t P, int64_t M) {
  return N < 0 || P < 0 || M < 0 || P >= kMaxPoints || M >= kMaxPoints || (N > 0 && ceil_div(P, kBlock) > kMaxBlocks / N) ||
         (N > 0 && ceil_div(M, kBlock) > kMaxBlocks / N);
}
// a point is 3 consecutive elements; points at least 3 apart; views overlap nothing (or stride 0: shared)
bool bad_point_strides(int64_t sN, int64_t sP, int64_t count) {
  return sP < 3 || sN < 0 || (sN != 0 && count > 0 && sN < (count - 1) * sP + 3);
}
inline dim3 grid_1d(int64_t items) {
  return dim3(static_cast<unsigned>(ceil_div(items, kBlock)));
}
// the size rounded up to a multiple of 8 bytes
inline size_t align8(size_t b) { return (b + 7) & ~size_t(7); }

} // namespace
} // namespace drtk_amd

using namespace drtk_amd;

extern "C" int drtk_amd_nearest_forward_workspace_bytes(drtk_dtype_t dtype, int64_t N, int64_t P, int64_t M, size_t* bytes) {
  if (!valid_dtype(dtype) || !bytes || bad_sizes(N, P, M)) return DRTK_ERR_INVALID_ARGUMENT;
  const Split sp = split_rule(N, P, M);
  *bytes = sp.S == 1 ? 0 : size_t(N) * size_t(sp.S) * size_t(P) * (dtype_size(dtype) + sizeof(int32_t));
  return DRTK_OK;
}

extern "C" int drtk_amd_nearest_forward(
    drtk_dtype_t dtype, const void* p, int64_t p_sN, int64_t p_sP, const void* q, int64_t q_sN, int64_t q_sM, int64_t N,
    int64_t P, int64_t M, void* dist2, int32_t* idx, void* workspace, size_t workspace_bytes, drtk_stream_t stream) {
  if (!valid_dtype(dtype)) return DRTK_ERR_INVALID_ARGUMENT;
  if (bad_sizes(N, P, M) || bad_point_strides(p_sN, p_sP, P) || bad_point_strides(q_sN, q_sM, M)) return DRTK_ERR_INVALID_ARGUMENT;
  if (N * P == 0) return DRTK_OK;
  if (!p || !dist2 || !idx || (M > 0 && !q)) return DRTK_ERR_INVALID_ARGUMENT;
  const Split sp = split_rule(N, P, M);
  size_t need = 0;
  drtk_amd_nearest_forward_workspace_bytes(dtype, N, P, M, &need);
  if (need > 0 && (!workspace || workspace_bytes < need)) return DRTK_ERR_WORKSPACE_TOO_SMALL;
  if (need > 0 && (reinterpret_cast<uintptr_t>(workspace) & 7) != 0) return DRTK_ERR_INVALID_ARGUMENT;
  return dispatch_dtype(dtype, [&](auto tag) -> int {
    using T = decltype(tag);
    const hipStream_t s = static_cast<hipStream_t>(stream);
    const int64_t bpv = ceil_div(P, kQueries);
    T* part_d = sp.S == 1 ? static_cast<T*>(dist2) : static_cast<T*>(workspace);
    int32_t* part_i = sp.S == 1 ? idx : reinterpret_cast<int32_t*>(static_cast<T*>(workspace) + N * sp.S * P);
    DRTK_LAUNCH((nearest_forward_kernel<T>), dim3(static_cast<unsigned>(N * bpv * sp.S)), dim3(kBlock), 0, s,
                static_cast<const T*>(p), p_sN, p_sP, static_cast<const T*>(q), q_sN, q_sM, int32_t(P), int32_t(M),
                int32_t(bpv), int32_t(sp.S), int32_t(sp.L), part_d, part_i);
    DRTK_RETURN_IF_LAUNCH_FAILED();
    if (sp.S > 1) {
      DRTK_LAUNCH((nearest_merge_kernel<T>), grid_1d(N * P), dim3(kBlock), 0, s, part_d, part_i, N, P, int32_t(sp.S),
                  static_cast<T*>(dist2), idx);
      DRTK_RETURN_IF_LAUNCH_FAILED();
    }
    return DRTK_OK;
  });
}

extern "C" int drtk_amd_nearest_backward_workspace_bytes(drtk_dtype_t dtype, int64_t N, int64_t P, int64_t M,
                                                         int need_grad_q, size_t* bytes) {
  if (!valid_dtype(dtype) || !bytes || bad_sizes(N, P, M)) return DRTK_ERR_INVALID_ARGUMENT;
  // the chunk sums [N,P,3] in double for either dtype, then the sorted keys [N,P] int32
  *bytes = need_grad_q ? align8(size_t(N) * size_t(P) * (3 * sizeof(double) + sizeof(int32_t))) : 0;
  return DRTK_OK;
}

extern "C" int drtk_amd_nearest_backward(
    drtk_dtype_t dtype, const void* grad_dist2, const void* p, int64_t p_sN, int64_t p_sP, const void* q, int64_t q_sN,
    int64_t q_sM, const int32_t* idx, const int32_t* order, int64_t N, int64_t P, int64_t M, int64_t grad_p_B, void* grad_p,
    int64_t grad_q_B, void* grad_q, void* workspace, size_t workspace_bytes, drtk_stream_t stream) {
  if (!valid_dtype(dtype)) return DRTK_ERR_INVALID_ARGUMENT;
  if (bad_sizes(N, P, M) || bad_point_strides(p_sN, p_sP, P) || bad_point_strides(q_sN, q_sM, M)) return DRTK_ERR_INVALID_ARGUMENT;
  if (!grad_p && !grad_q) return DRTK_ERR_INVALID_ARGUMENT;
  if (grad_p && grad_p_B != 1 && grad_p_B != N) return DRTK_ERR_INVALID_ARGUMENT;
  if (grad_q && grad_q_B != 1 && grad_q_B != N) return DRTK_ERR_INVALID_ARGUMENT;
  // (N = 0 with a summed gradient: the empty sum, zeros)
  const bool p_pass = grad_p && P > 0 && (N > 0 || grad_p_B == 1);
  const bool q_pass = grad_q && M > 0 && (N > 0 || grad_q_B == 1);
  if (!p_pass && !q_pass) return DRTK_OK;
  const bool pairs = N * P > 0 && M > 0; // without them every idx is -1 or there is none
  if (N * P > 0 && (!grad_dist2 || !idx || !p)) return DRTK_ERR_INVALID_ARGUMENT;
  if (pairs && !q) return DRTK_ERR_INVALID_ARGUMENT;
  const bool chunk_pass = q_pass && N * P > 0;
  size_t need = 0;
  if (chunk_pass) {
    if (!order) return DRTK_ERR_INVALID_ARGUMENT;
    drtk_amd_nearest_backward_workspace_bytes(dtype, N, P, M, 1, &need);
    if (!workspace || workspace_bytes < need) return DRTK_ERR_WORKSPACE_TOO_SMALL;
    if ((reinterpret_cast<uintptr_t>(workspace) & 7) != 0) return DRTK_ERR_INVALID_ARGUMENT;
  }
  return dispatch_dtype(dtype, [&](auto tag) -> int {
    using T = decltype(tag);
    const hipStream_t s = static_cast<hipStream_t>(stream);
    const T *g = static_cast<const T*>(grad_dist2), *pp = static_cast<const T*>(p), *qq = static_cast<const T*>(q);
    if (p_pass) {
      const bool sum_views = grad_p_B == 1;
      DRTK_LAUNCH((nearest_grad_p_kernel<T>), grid_1d(sum_views ? P : N * P), dim3(kBlock), 0, s, g, pp, p_sN, p_sP, qq, q_sN,
                  q_sM, idx, N, P, sum_views, static_cast<T*>(grad_p));
      DRTK_RETURN_IF_LAUNCH_FAILED();
    }
    if (q_pass) {
      double* sums = static_cast<double*>(workspace);
      int32_t* keys = reinterpret_cast<int32_t*>(sums + N * P * 3);
      if (chunk_pass) {
        const int64_t cpv = ceil_div(P, kChunk);
        DRTK_LAUNCH((nearest_grad_q_chunk_kernel<T>), dim3(static_cast<unsigned>(N * cpv)), dim3(kBlock), 0, s, g, pp, p_sN,
                    p_sP, qq, q_sN, q_sM, idx, order, P, cpv, sums, keys);
        DRTK_RETURN_IF_LAUNCH_FAILED();
      }
      const bool sum_views = grad_q_B == 1;
      // (P = 0: every bisection ends at once without reading the keys, every run is empty)
      DRTK_LAUNCH((nearest_grad_q_target_kernel<T>), grid_1d(sum_views ? M : N * M), dim3(kBlock), 0, s, sums, keys, N, P, M,
                  sum_views, static_cast<T*>(grad_q));
      DRTK_RETURN_IF_LAUNCH_FAILED();
    }
    return DRTK_OK;
  });
}
