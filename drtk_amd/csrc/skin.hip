// Linear blend skinning: out[n,i] = sum_k w[i,k] (R[n,j] v[n,i] + t[n,j]), j = joint_idx[i,k], forward and the three
// gradients, without float atomics (no counterpart in the reference's library).
//
//   forward          one lane per (view, vertex); a workgroup stays inside one view and stages that view's J x 12 values
//                    in LDS while J <= kSkinLdsJoints (above it the lanes read them from memory, where L2 serves them).
//                    The 3x4 is blended first, k ascending, then applied: M = sum_k w_k T_j;  out = M [v; 1].
//   vertex backward  one lane per vertex, looping over the views with the vertex's (index, weight) row in registers:
//                    grad_v[n,i] = M^T g[n,i] (a shared v: the views' rows added in ascending n, here) and
//                    grad_w[i,k] = sum_n dot(g[n,i], R[n,j] v[n,i] + t[n,j]), n ascending.  The half that is not asked
//                    for is skipped.
//   joint backward   grad_T[n,j] = sum over the entries (i,k) that name j of w[i,k] g[n,i] [v[n,i]; 1]^T, through the joint
//                    incidence (CSR over joints, entries i*K+k ascending), EVERY row cut into chunks of kSkinChunk entries:
//                    stage one, one wave per (view, chunk): lane l takes the chunk's entries l, l + 64, ... in that order
//                    into 12 double accumulators, the wave adds the lanes' sums in a fixed butterfly (xor 32, 16, ... 1) and
//                    stores one partial row; stage two, one lane per output element, adds the joint's partial rows in chunk
//                    order and rounds once to the output dtype.  Row 3 of a 4x4 output and a joint nobody names get 0.
// Every sum has one fixed order that depends on the inputs' shapes only, so results are bitwise reproducible and
// independent of the launch shape.
#include "common.hpp"

namespace drtk_amd {
namespace {

constexpr int kSkinChunk = 512;      // DRTK_SKIN_CHUNK of include/drtk_amd.h
constexpr int kSkinLdsJoints = 512;  // forward: stage the view's transforms in LDS up to this many joints (48 KiB of double)
constexpr int kSkinMaxSlots = 8;     // DRTK_SKIN_MAX_SLOTS
static_assert(kSkinChunk == DRTK_SKIN_CHUNK && kSkinMaxSlots == DRTK_SKIN_MAX_SLOTS, "include/drtk_amd.h");

template <typename T, bool LDS>
__global__ __launch_bounds__(kBlock) void skin_forward_kernel(
    const T* __restrict__ v, int64_t v_sN, const int32_t* __restrict__ idx, const T* __restrict__ w,
    const T* __restrict__ tr, int64_t t_sN, int64_t t_sJ, int64_t V, int J, int K, int64_t blocks_per_view,
    T* __restrict__ out) {
  extern __shared__ __attribute__((aligned(16))) unsigned char skin_lds_raw[];
  T* lds = reinterpret_cast<T*>(skin_lds_raw);
  const int64_t n = int64_t(blockIdx.x) / blocks_per_view;
  const int64_t tile = int64_t(blockIdx.x) - n * blocks_per_view;
  const T* tn = tr + n * t_sN;
  if (LDS) {
    for (int q = threadIdx.x; q < J * 12; q += kBlock) {
      const int j = q / 12;
      lds[q] = tn[int64_t(j) * t_sJ + (q - j * 12)]; // rows 0..2 of a joint: 12 consecutive elements
    }
    __syncthreads();
  }
  const int64_t i = tile * kBlock + threadIdx.x;
  if (i >= V) return;
  T m[12];
#pragma unroll
  for (int q = 0; q < 12; ++q) m[q] = T(0);
  bool any = false;
  for (int k = 0; k < K; ++k) {
    const int32_t j = idx[i * K + k];
    if (j < 0) continue; // an empty slot: its weight is not read
    any = true;
    const T wk = w[i * K + k];
    if (LDS) {
      const T* tj = lds + j * 12;
#pragma unroll
      for (int q = 0; q < 12; ++q) m[q] += wk * tj[q];
    } else {
      const T* tj = tn + int64_t(j) * t_sJ;
#pragma unroll
      for (int q = 0; q < 12; ++q) m[q] += wk * tj[q];
    }
  }
  T* o = out + (n * V + i) * 3;
  if (!any) {
    o[0] = o[1] = o[2] = T(0);
    return;
  }
  const T* p = v + n * v_sN + i * 3;
  const T x = p[0], y = p[1], z = p[2];
#pragma unroll
  for (int a = 0; a < 3; ++a) o[a] = m[a * 4] * x + m[a * 4 + 1] * y + m[a * 4 + 2] * z + m[a * 4 + 3];
}

// KMAX: 4 or 8 register slots (K <= KMAX; slots past K read as empty)
template <typename T, int KMAX, bool NEED_V, bool NEED_W>
__global__ __launch_bounds__(kBlock) void skin_vertex_backward_kernel(
    const T* __restrict__ g, const T* __restrict__ v, int64_t v_sN, const int32_t* __restrict__ idx,
    const T* __restrict__ w, const T* __restrict__ tr, int64_t t_sN, int64_t t_sJ, int64_t N, int64_t V, int K,
    bool sum_views, T* __restrict__ grad_v, T* __restrict__ grad_w) {
  const int64_t i = int64_t(blockIdx.x) * kBlock + threadIdx.x;
  if (i >= V) return;
  int32_t js[KMAX];
  T ws[KMAX], gw[KMAX];
#pragma unroll
  for (int k = 0; k < KMAX; ++k) {
    js[k] = k < K ? idx[i * K + k] : -1;
    ws[k] = NEED_V && js[k] >= 0 ? w[i * K + k] : T(0);
    gw[k] = T(0);
  }
  T acc[3] = {T(0), T(0), T(0)};
  for (int64_t n = 0; n < N; ++n) {
    const T* gp = g + (n * V + i) * 3;
    const T g0 = gp[0], g1 = gp[1], g2 = gp[2];
    const T* p = v + n * v_sN + i * 3;
    T x = T(0), y = T(0), z = T(0);
    if (NEED_W) x = p[0], y = p[1], z = p[2];
    const T* tn = tr + n * t_sN;
    T m[9];
#pragma unroll
    for (int q = 0; q < 9; ++q) m[q] = T(0);
#pragma unroll
    for (int k = 0; k < KMAX; ++k) {
      if (js[k] < 0) continue;
      const T* tj = tn + int64_t(js[k]) * t_sJ;
      T r[12];
#pragma unroll
      for (int a = 0; a < 3; ++a) {
#pragma unroll
        for (int b = 0; b < 3; ++b) r[a * 4 + b] = tj[a * 4 + b];
        r[a * 4 + 3] = NEED_W ? tj[a * 4 + 3] : T(0);
      }
      if (NEED_V) {
#pragma unroll
        for (int a = 0; a < 3; ++a)
#pragma unroll
          for (int b = 0; b < 3; ++b) m[a * 3 + b] += ws[k] * r[a * 4 + b];
      }
      if (NEED_W) {
        const T p0 = r[0] * x + r[1] * y + r[2] * z + r[3];
        const T p1 = r[4] * x + r[5] * y + r[6] * z + r[7];
        const T p2 = r[8] * x + r[9] * y + r[10] * z + r[11];
        gw[k] += g0 * p0 + g1 * p1 + g2 * p2;
      }
    }
    if (NEED_V) {
      T gv[3];
#pragma unroll
      for (int b = 0; b < 3; ++b) gv[b] = m[b] * g0 + m[3 + b] * g1 + m[6 + b] * g2;
      if (sum_views) {
#pragma unroll
        for (int b = 0; b < 3; ++b) acc[b] += gv[b];
      } else {
        T* o = grad_v + (n * V + i) * 3;
        o[0] = gv[0], o[1] = gv[1], o[2] = gv[2];
      }
    }
  }
  if (NEED_V && sum_views) {
    T* o = grad_v + i * 3;
    o[0] = acc[0], o[1] = acc[1], o[2] = acc[2];
  }
  if (NEED_W) {
#pragma unroll
    for (int k = 0; k < KMAX; ++k)
      if (k < K) grad_w[i * K + k] = gw[k]; // (an empty slot: 0)
  }
}

// stage one of the joint backward: one wave per (view, chunk)
template <typename T>
__global__ __launch_bounds__(kBlock) void skin_joint_chunk_kernel(
    const T* __restrict__ g, const T* __restrict__ v, int64_t v_sN, const T* __restrict__ w,
    const int32_t* __restrict__ crow, const int32_t* __restrict__ entries, const int32_t* __restrict__ chunk_begin,
    const int32_t* __restrict__ chunk_joint, int64_t num_chunks, int64_t N, int64_t V, int K,
    double* __restrict__ partial) {
  const int64_t item = int64_t(blockIdx.x) * (kBlock / kWave) + threadIdx.x / kWave; // wave-uniform
  if (item >= N * num_chunks) return;
  const int lane = threadIdx.x % kWave;
  const int64_t n = item / num_chunks, c = item - n * num_chunks;
  const int32_t beg = chunk_begin[c];
  const int32_t row_end = crow[chunk_joint[c] + 1];
  const int32_t end = beg + kSkinChunk < row_end ? beg + kSkinChunk : row_end;
  const T* gn = g + n * V * 3;
  const T* vn = v + n * v_sN;
  double acc[12];
#pragma unroll
  for (int q = 0; q < 12; ++q) acc[q] = 0.0;
  for (int32_t pos = beg + lane; pos < end; pos += kWave) {
    const int32_t e = entries[pos];
    const int64_t i = e / K;
    const double we = double(w[e]);
    const double h[4] = {double(vn[i * 3]), double(vn[i * 3 + 1]), double(vn[i * 3 + 2]), 1.0};
#pragma unroll
    for (int a = 0; a < 3; ++a) {
      const double wg = we * double(gn[i * 3 + a]);
#pragma unroll
      for (int b = 0; b < 4; ++b) acc[a * 4 + b] += wg * h[b];
    }
  }
#pragma unroll
  for (int mask = kWave / 2; mask >= 1; mask >>= 1) {
#pragma unroll
    for (int q = 0; q < 12; ++q) {
      const double other = __shfl_xor(acc[q], mask, kWave);
      acc[q] += other;
    }
  }
  if (lane == 0) {
    double* o = partial + item * 12;
#pragma unroll
    for (int q = 0; q < 12; ++q) o[q] = acc[q];
  }
}

// stage two: one lane per element of grad_T [N,J,rows,4]
template <typename T>
__global__ __launch_bounds__(kBlock) void skin_joint_sum_kernel(
    const double* __restrict__ partial, const int32_t* __restrict__ chunk_ptr, int64_t num_chunks, int64_t N, int64_t J,
    int rows, T* __restrict__ grad_t) {
  const int64_t i = int64_t(blockIdx.x) * kBlock + threadIdx.x;
  const int per = rows * 4;
  if (i >= N * J * per) return;
  const int64_t nj = i / per;
  const int q = int(i - nj * per);
  const int64_t n = nj / J, j = nj - n * J;
  double s = 0.0;
  if (q < 12) {
    const int32_t c1 = chunk_ptr[j + 1];
    const double* p = partial + n * num_chunks * 12 + q;
    int32_t c = chunk_ptr[j];
    // eight loads in flight, added in chunk order (a root joint has hundreds of chunks: one load at a time is a chain
    // of memory latencies)
    for (; c + 8 <= c1; c += 8) {
      double t[8];
#pragma unroll
      for (int u = 0; u < 8; ++u) t[u] = p[int64_t(c + u) * 12];
#pragma unroll
      for (int u = 0; u < 8; ++u) s += t[u];
    }
    for (; c < c1; ++c) s += p[int64_t(c) * 12];
  }
  grad_t[i] = T(s);
}

inline dim3 grid_1d(int64_t items) {
  return dim3(static_cast<unsigned>(ceil_div(items, kBlock)));
}
constexpr int64_t kMaxBlocks = (int64_t(1) << 31) - 1;

// sizes every entry point shares; i*K+k and n*V*3 offsets are 64-bit, incidence entries 32-bit
bool bad_sizes(int64_t N, int64_t V, int64_t J, int64_t K) {
  return N < 0 || V < 0 || J < 0 || K < 1 || K > kSkinMaxSlots || J >= (int64_t(1) << 27) ||
         V * K >= (int64_t(1) << 31) || (N > 0 && ceil_div(V, kBlock) > kMaxBlocks / N);
}
// rows 0..2 of a joint are 12 consecutive elements; joints 12 ([3,4]) or 16 ([4,4]) elements apart or, in a view of a
// larger tensor, further; views at least J joints apart
bool bad_transform_strides(int64_t t_sN, int64_t t_sJ, int64_t J) {
  return t_sJ < 12 || t_sN < 0 || (t_sN != 0 && J > 0 && t_sN < (J - 1) * t_sJ + 12);
}

} // namespace
} // namespace drtk_amd

using namespace drtk_amd;

extern "C" int drtk_amd_skin_forward(
    drtk_dtype_t dtype, const void* v, int64_t v_sN, const int32_t* joint_idx, const void* joint_weights,
    const void* transforms, int64_t t_sN, int64_t t_sJ, int64_t N, int64_t V, int64_t J, int64_t K, void* out,
    drtk_stream_t stream) {
  if (!valid_dtype(dtype)) return DRTK_ERR_INVALID_ARGUMENT;
  if (bad_sizes(N, V, J, K) || bad_view_stride(v_sN, V * 3) || bad_transform_strides(t_sN, t_sJ, J))
    return DRTK_ERR_INVALID_ARGUMENT;
  if (N * V == 0) return DRTK_OK;
  if (!v || !joint_idx || !joint_weights || !out || (J > 0 && !transforms)) return DRTK_ERR_INVALID_ARGUMENT;
  return dispatch_dtype(dtype, [&](auto tag) -> int {
    using T = decltype(tag);
    const hipStream_t s = static_cast<hipStream_t>(stream);
    const int64_t bpv = ceil_div(V, kBlock);
    const dim3 grid(static_cast<unsigned>(N * bpv));
    if (J <= kSkinLdsJoints) {
      DRTK_LAUNCH((skin_forward_kernel<T, true>), grid, dim3(kBlock), size_t(J) * 12 * sizeof(T), s,
                  static_cast<const T*>(v), v_sN, joint_idx, static_cast<const T*>(joint_weights),
                  static_cast<const T*>(transforms), t_sN, t_sJ, V, int(J), int(K), bpv, static_cast<T*>(out));
    } else {
      DRTK_LAUNCH((skin_forward_kernel<T, false>), grid, dim3(kBlock), 0, s, static_cast<const T*>(v), v_sN, joint_idx,
                  static_cast<const T*>(joint_weights), static_cast<const T*>(transforms), t_sN, t_sJ, V, int(J), int(K),
                  bpv, static_cast<T*>(out));
    }
    DRTK_RETURN_IF_LAUNCH_FAILED();
    return DRTK_OK;
  });
}

extern "C" int drtk_amd_skin_backward_workspace_bytes(drtk_dtype_t dtype, int64_t N, int64_t num_chunks, size_t* bytes) {
  if (!valid_dtype(dtype) || !bytes || N < 0 || num_chunks < 0) return DRTK_ERR_INVALID_ARGUMENT;
  *bytes = size_t(N) * size_t(num_chunks) * 12 * sizeof(double); // one partial row per (view, chunk), double for either dtype
  return DRTK_OK;
}

namespace drtk_amd {
namespace {
template <typename T, int KMAX>
int vertex_backward_impl(const void* g, const void* v, int64_t v_sN, const int32_t* idx, const void* w, const void* tr,
                         int64_t t_sN, int64_t t_sJ, int64_t N, int64_t V, int K, bool sum_views, void* grad_v,
                         void* grad_w, hipStream_t s) {
#define DRTK_SKIN_VERTEX_BACKWARD(NV, NW)                                                                              \
  DRTK_LAUNCH((skin_vertex_backward_kernel<T, KMAX, NV, NW>), grid_1d(V), dim3(kBlock), 0, s, static_cast<const T*>(g), \
              static_cast<const T*>(v), v_sN, idx, static_cast<const T*>(w), static_cast<const T*>(tr), t_sN, t_sJ, N, V, \
              K, sum_views, static_cast<T*>(grad_v), static_cast<T*>(grad_w))
  if (grad_v && grad_w) DRTK_SKIN_VERTEX_BACKWARD(true, true);
  else if (grad_v) DRTK_SKIN_VERTEX_BACKWARD(true, false);
  else DRTK_SKIN_VERTEX_BACKWARD(false, true);
#undef DRTK_SKIN_VERTEX_BACKWARD
  DRTK_RETURN_IF_LAUNCH_FAILED();
  return DRTK_OK;
}
} // namespace
} // namespace drtk_amd

extern "C" int drtk_amd_skin_backward(
    drtk_dtype_t dtype, const void* grad_out, const void* v, int64_t v_sN, const int32_t* joint_idx,
    const void* joint_weights, const void* transforms, int64_t t_sN, int64_t t_sJ, const int32_t* crow,
    const int32_t* entries, const int32_t* chunk_ptr, const int32_t* chunk_begin, const int32_t* chunk_joint,
    int64_t num_chunks, int64_t N, int64_t V, int64_t J, int64_t K, int64_t grad_v_B, void* grad_v, void* grad_weights,
    int64_t grad_t_rows, void* grad_transforms, void* workspace, size_t workspace_bytes, drtk_stream_t stream) {
  if (!valid_dtype(dtype)) return DRTK_ERR_INVALID_ARGUMENT;
  if (bad_sizes(N, V, J, K) || bad_view_stride(v_sN, V * 3) || bad_transform_strides(t_sN, t_sJ, J) || num_chunks < 0)
    return DRTK_ERR_INVALID_ARGUMENT;
  if (!grad_v && !grad_weights && !grad_transforms) return DRTK_ERR_INVALID_ARGUMENT;
  if (grad_v && grad_v_B != 1 && grad_v_B != N) return DRTK_ERR_INVALID_ARGUMENT;
  if (grad_transforms && grad_t_rows != 3 && grad_t_rows != 4) return DRTK_ERR_INVALID_ARGUMENT;
  if (N > 0 && (num_chunks > kMaxBlocks / N || J * 16 > kMaxBlocks / N)) return DRTK_ERR_INVALID_ARGUMENT;
  const bool vertex_pass = (grad_v || grad_weights) && V > 0 && (N > 0 || grad_weights || grad_v_B == 1);
  const bool joint_pass = grad_transforms && N * J > 0;
  if (!vertex_pass && !joint_pass) return DRTK_OK;
  if ((V > 0 && (!joint_idx || !joint_weights)) || (N * V > 0 && (!grad_out || !v)) || (N * V > 0 && J > 0 && !transforms))
    return DRTK_ERR_INVALID_ARGUMENT;
  if (joint_pass) {
    if (!chunk_ptr || (num_chunks > 0 && (!crow || !entries || !chunk_begin || !chunk_joint)))
      return DRTK_ERR_INVALID_ARGUMENT;
    size_t need = 0;
    drtk_amd_skin_backward_workspace_bytes(dtype, N, num_chunks, &need);
    if (need > 0 && (!workspace || workspace_bytes < need || (reinterpret_cast<uintptr_t>(workspace) & 7) != 0))
      return !workspace || workspace_bytes < need ? DRTK_ERR_WORKSPACE_TOO_SMALL : DRTK_ERR_INVALID_ARGUMENT;
  }
  return dispatch_dtype(dtype, [&](auto tag) -> int {
    using T = decltype(tag);
    const hipStream_t s = static_cast<hipStream_t>(stream);
    if (vertex_pass) {
      // (N = 0 with a summed grad_v or grad_weights: the empty sums, zeros)
      const bool sum_views = grad_v_B == 1;
      const int rc = K <= 4 ? vertex_backward_impl<T, 4>(grad_out, v, v_sN, joint_idx, joint_weights, transforms, t_sN, t_sJ, N, V, int(K), sum_views, grad_v, grad_weights, s)
                            : vertex_backward_impl<T, 8>(grad_out, v, v_sN, joint_idx, joint_weights, transforms, t_sN, t_sJ, N, V, int(K), sum_views, grad_v, grad_weights, s);
      if (rc != DRTK_OK) return rc;
    }
    if (joint_pass) {
      double* partial = static_cast<double*>(workspace);
      if (num_chunks > 0) {
        DRTK_LAUNCH((skin_joint_chunk_kernel<T>), dim3(static_cast<unsigned>(ceil_div(N * num_chunks, kBlock / kWave))),
                    dim3(kBlock), 0, s, static_cast<const T*>(grad_out), static_cast<const T*>(v), v_sN,
                    static_cast<const T*>(joint_weights), crow, entries, chunk_begin, chunk_joint, num_chunks, N, V,
                    int(K), partial);
        DRTK_RETURN_IF_LAUNCH_FAILED();
      }
      DRTK_LAUNCH((skin_joint_sum_kernel<T>), grid_1d(N * J * grad_t_rows * 4), dim3(kBlock), 0, s, partial, chunk_ptr,
                  num_chunks, N, J, int(grad_t_rows), static_cast<T*>(grad_transforms));
      DRTK_RETURN_IF_LAUNCH_FAILED();
    }
    return DRTK_OK;
  });
}
