// Mesh geometry of drtk.utils (face_info, vert_normals, face_attribute_to_vert, face_dpdt, vert_binormals) in two
// passes and without float atomics.
//
// Reference: drtk/utils/geometry.py (pure PyTorch: per-view index_select, cross / norm / clamp / divide, scatter_add
// over the (face, corner) pairs, F.normalize).  Here:
//   face pass     one lane per (view, face): the per-face results (normal, area, edges, dpdt_t, v012) forward; backward
//                 the gradient of the three corners of the face, written as plain per-corner rows [N,F,3,3] (positions)
//                 and [N,F,3,2] (UVs).  Where the upstream gradient is per vertex (vert_normals, vert_binormals,
//                 face_attribute_to_vert) the pass gathers it at its three corners itself, applying F.normalize's
//                 backward from the saved unnormalised sums inline.
//   vertex pass   one lane per (view, vertex): the sum of the rows (per face or per (face, corner)) listed in the
//                 vertex's incidence row (CSR, entries f*3+k ascending -- the order in which a single-threaded
//                 scatter_add visits them), optionally normalised (keeping the sum for the backward).
// Rows longer than DRTK_GEOMETRY_CHUNK entries are split into chunks of that length: one lane per (view, chunk) sums a
// chunk, and the vertex pass adds the chunk sums in chunk order.  Every sum has one fixed order, so results are
// bitwise reproducible and independent of the launch shape.
//
// The mesh regulariser rides on the same structure: cotangent weights are a face pass each way (backward: per-corner
// rows, reduced by the vertex pass), and the weighted graph Laplacian sum_j w_ij (x_j - x_i) is a vertex pass that
// walks the incidence row and reads the face's indices and weights per entry -- no vertex-vertex adjacency, nothing
// padded; it is symmetric, so its backward with respect to x is itself, and the weights' gradient is a face pass.
#include "common.hpp"

namespace drtk_amd {
namespace {

constexpr int kChunk = DRTK_GEOMETRY_CHUNK;

template <typename T>
__device__ __forceinline__ void cross3(const T a[3], const T b[3], T c[3]) {
  c[0] = a[1] * b[2] - a[2] * b[1];
  c[1] = a[2] * b[0] - a[0] * b[2];
  c[2] = a[0] * b[1] - a[1] * b[0];
}

template <typename T>
__device__ __forceinline__ T norm3(const T c[3]) {
  return sqrt(c[0] * c[0] + c[1] * c[1] + c[2] * c[2]);
}

// Backward of  y = s / max(|s|, eps)  (the composite's divide, clamp and vector_norm, branch for branch): below eps the
// clamp passes no gradient to the norm, and the norm passes none at s = 0.
template <typename T>
__device__ __forceinline__ void normalize_backward(const T g[3], const T s[3], T eps, T extra_norm_grad, T gs[3]) {
  const T nrm = norm3(s);
  const T d = nrm < eps ? eps : nrm;
  const T gd = -(g[0] * s[0] + g[1] * s[1] + g[2] * s[2]) / (d * d);
  const T gn = (nrm < eps ? T(0) : gd) + extra_norm_grad;
  const T k = nrm > T(0) ? gn / nrm : T(0);
#pragma unroll
  for (int j = 0; j < 3; ++j) gs[j] = g[j] / d + k * s[j];
}

template <typename T>
__device__ __forceinline__ void load_corners(const T* __restrict__ v, const int32_t* __restrict__ fi, T p[3][3]) {
#pragma unroll
  for (int k = 0; k < 3; ++k) {
    const T* q = v + int64_t(fi[k]) * 3;
#pragma unroll
    for (int j = 0; j < 3; ++j) p[k][j] = q[j];
  }
}

template <typename T>
__device__ __forceinline__ void load_uv_corners(const T* __restrict__ vt, const int32_t* __restrict__ fi, T t[3][2]) {
#pragma unroll
  for (int k = 0; k < 3; ++k) {
    const T* q = vt + int64_t(fi[k]) * 2;
    t[k][0] = q[0];
    t[k][1] = q[1];
  }
}

// dpdt_t = inv([t1-t0; t2-t0]) @ [p1-p0; p2-p0], the inverse in closed form (a singular UV matrix gives inf / nan).
// In double whatever T is (a few operations per face): det = a0 b1 - a1 b0 cancels on a sliver UV triangle, and carried in
// float such a face -- the largest entries of the output, and of the gradients through M^T gM M^T -- lost its condition
// number times 2^-24, several times what a pivoted float inverse of the same matrix loses (tests/fuzz_geometry.py, seeds
// 13, 99, 155 and 207).  The edge differences of float corners are exact in double, so a float result is the correctly
// rounded one up to the last products.
struct Dpdt {
  double m[2][2]; // inv(dtdb_t)
  double P[2][3]; // dpdb_t
};
template <typename T>
__device__ __forceinline__ Dpdt dpdt_setup(const T p[3][3], const T t[3][2]) {
  Dpdt r;
  const double a0 = double(t[1][0]) - double(t[0][0]), a1 = double(t[1][1]) - double(t[0][1]);
  const double b0 = double(t[2][0]) - double(t[0][0]), b1 = double(t[2][1]) - double(t[0][1]);
  const double det = a0 * b1 - a1 * b0;
  r.m[0][0] = b1 / det, r.m[0][1] = -a1 / det;
  r.m[1][0] = -b0 / det, r.m[1][1] = a0 / det;
#pragma unroll
  for (int j = 0; j < 3; ++j)
    r.P[0][j] = double(p[1][j]) - double(p[0][j]), r.P[1][j] = double(p[2][j]) - double(p[0][j]);
  return r;
}

template <typename T>
__global__ __launch_bounds__(kBlock) void geom_face_forward_kernel(
    const T* __restrict__ v, int64_t v_sN, const int32_t* __restrict__ vi, int64_t vi_sN, const T* __restrict__ vt,
    int64_t vt_sN, const int32_t* __restrict__ vti, int64_t N, int64_t F, T* __restrict__ normals,
    T* __restrict__ areas, T* __restrict__ edges, T* __restrict__ dpdt, T* __restrict__ dpdt_u, T* __restrict__ v012) {
  const int64_t i = int64_t(blockIdx.x) * kBlock + threadIdx.x;
  if (i >= N * F) return;
  const int64_t n = i / F, f = i - n * F;
  T p[3][3];
  load_corners(v + n * v_sN, vi + n * vi_sN + f * 3, p);
  if (normals || areas) {
    T a[3], b[3], c[3];
#pragma unroll
    for (int j = 0; j < 3; ++j) a[j] = p[0][j] - p[2][j], b[j] = p[1][j] - p[0][j];
    cross3(a, b, c);
    const T nrm = norm3(c);
    if (areas) areas[i] = T(0.5) * nrm;
    if (normals) {
      const T d = nrm < T(1e-8) ? T(1e-8) : nrm;
#pragma unroll
      for (int j = 0; j < 3; ++j) normals[i * 3 + j] = c[j] / d;
    }
  }
  if (edges) {
#pragma unroll
    for (int j = 0; j < 3; ++j) {
      edges[i * 9 + j] = p[1][j] - p[0][j];
      edges[i * 9 + 3 + j] = p[0][j] - p[2][j];
      edges[i * 9 + 6 + j] = p[2][j] - p[1][j];
    }
  }
  if (v012) {
#pragma unroll
    for (int k = 0; k < 3; ++k)
#pragma unroll
      for (int j = 0; j < 3; ++j) v012[i * 9 + k * 3 + j] = p[k][j];
  }
  if (dpdt || dpdt_u) {
    T t[3][2];
    load_uv_corners(vt + n * vt_sN, vti + f * 3, t);
    const Dpdt q = dpdt_setup(p, t);
#pragma unroll
    for (int r = 0; r < 2; ++r)
#pragma unroll
      for (int j = 0; j < 3; ++j) {
        const T x = T(q.m[r][0] * q.P[0][j] + q.m[r][1] * q.P[1][j]);
        if (dpdt) dpdt[i * 6 + r * 3 + j] = x;
        if (dpdt_u && r == 0) dpdt_u[i * 3 + j] = x;
      }
  }
}

// Sum over the face's three corners of the per-vertex gradient g [N,V,3] (through F.normalize's backward when the
// unnormalised sums are given).
template <typename T>
__device__ __forceinline__ void gather_corner_grads(
    const T* __restrict__ g_vert, const T* __restrict__ sums, const int32_t* __restrict__ fi, int64_t row0, T out[3]) {
  out[0] = out[1] = out[2] = T(0);
#pragma unroll
  for (int k = 0; k < 3; ++k) {
    const int64_t o = (row0 + fi[k]) * 3;
    T g[3] = {g_vert[o], g_vert[o + 1], g_vert[o + 2]};
    if (sums) {
      const T s[3] = {sums[o], sums[o + 1], sums[o + 2]};
      normalize_backward(g, s, T(1e-12), T(0), g);
    }
#pragma unroll
    for (int j = 0; j < 3; ++j) out[j] += g[j];
  }
}

// Backward of the face pass.  DPDT = false: face_info (normals, areas, edges); true: face_dpdt (dpdt_t, v012).
// g_vert/sums, when given, add the per-vertex gradient of vert_normals (DPDT false) or vert_binormals (DPDT true: it
// is the gradient of dpdt_t's first row).  Output: per-corner rows, positions [N,F,3,3] and (DPDT) UVs [N,F,3,2].
template <typename T, bool DPDT>
__global__ __launch_bounds__(kBlock) void geom_face_backward_kernel(
    const T* __restrict__ v, int64_t v_sN, const int32_t* __restrict__ vi, int64_t vi_sN, const T* __restrict__ vt,
    int64_t vt_sN, const int32_t* __restrict__ vti, int64_t N, int64_t V, int64_t F, const T* __restrict__ g_vert,
    const T* __restrict__ sums, const T* __restrict__ g_normals, const T* __restrict__ g_areas,
    const T* __restrict__ g_edges, const T* __restrict__ g_dpdt, const T* __restrict__ g_v012,
    T* __restrict__ pos_rows, T* __restrict__ uv_rows) {
  const int64_t i = int64_t(blockIdx.x) * kBlock + threadIdx.x;
  if (i >= N * F) return;
  const int64_t n = i / F, f = i - n * F;
  const int32_t* fi = vi + n * vi_sN + f * 3;
  T p[3][3];
  load_corners(v + n * v_sN, fi, p);
  T gv[3] = {T(0), T(0), T(0)};
  if (g_vert) gather_corner_grads(g_vert, sums, fi, n * V, gv);
  T gp[3][3];
  if (!DPDT) {
    T a[3], b[3], c[3], gc[3] = {T(0), T(0), T(0)};
#pragma unroll
    for (int j = 0; j < 3; ++j) a[j] = p[0][j] - p[2][j], b[j] = p[1][j] - p[0][j];
    cross3(a, b, c);
    const T ga_area = g_areas ? T(0.5) * g_areas[i] : T(0);
    if (g_normals || g_vert) {
      T gn[3];
#pragma unroll
      for (int j = 0; j < 3; ++j) gn[j] = (g_normals ? g_normals[i * 3 + j] : T(0)) + gv[j];
      normalize_backward(gn, c, T(1e-8), ga_area, gc);
    } else if (g_areas) {
      const T nrm = norm3(c);
      const T k = nrm > T(0) ? ga_area / nrm : T(0);
#pragma unroll
      for (int j = 0; j < 3; ++j) gc[j] = k * c[j];
    }
    // c = a x b:  ga = b x gc, gb = gc x a;  a = p0 - p2, b = p1 - p0
    T ga[3], gb[3];
    cross3(b, gc, ga);
    cross3(gc, a, gb);
#pragma unroll
    for (int j = 0; j < 3; ++j) {
      gp[0][j] = ga[j] - gb[j];
      gp[1][j] = gb[j];
      gp[2][j] = -ga[j];
    }
    if (g_edges) { // edges = (p1 - p0, p0 - p2, p2 - p1)
      const T* ge = g_edges + i * 9;
#pragma unroll
      for (int j = 0; j < 3; ++j) {
        gp[0][j] += ge[3 + j] - ge[j];
        gp[1][j] += ge[j] - ge[6 + j];
        gp[2][j] += ge[6 + j] - ge[3 + j];
      }
    }
  } else {
    T t[3][2];
    load_uv_corners(vt + n * vt_sN, vti + f * 3, t);
    const Dpdt q = dpdt_setup(p, t);
    double gD[2][3];
#pragma unroll
    for (int r = 0; r < 2; ++r)
#pragma unroll
      for (int j = 0; j < 3; ++j) gD[r][j] = double((g_dpdt ? g_dpdt[i * 6 + r * 3 + j] : T(0)) + (r == 0 ? gv[j] : T(0)));
    // D = M P:  gM = gD P^T, gP = M^T gD;  M = inv(A):  gA = -M^T gM M^T  (in double, as M is)
    double gM[2][2], gA[2][2], gP[2][3];
#pragma unroll
    for (int r = 0; r < 2; ++r)
#pragma unroll
      for (int s = 0; s < 2; ++s) gM[r][s] = gD[r][0] * q.P[s][0] + gD[r][1] * q.P[s][1] + gD[r][2] * q.P[s][2];
#pragma unroll
    for (int r = 0; r < 2; ++r)
#pragma unroll
      for (int j = 0; j < 3; ++j) gP[r][j] = q.m[0][r] * gD[0][j] + q.m[1][r] * gD[1][j];
#pragma unroll
    for (int r = 0; r < 2; ++r)
#pragma unroll
      for (int s = 0; s < 2; ++s) {
        // (M^T gM M^T)[r][s] = sum_kl M[k][r] gM[k][l] M[s][l]
        const double x0 = q.m[0][r] * gM[0][0] + q.m[1][r] * gM[1][0];
        const double x1 = q.m[0][r] * gM[0][1] + q.m[1][r] * gM[1][1];
        gA[r][s] = -(x0 * q.m[s][0] + x1 * q.m[s][1]);
      }
    T* uv = uv_rows + i * 6;
#pragma unroll
    for (int j = 0; j < 2; ++j) {
      uv[j] = T(-(gA[0][j] + gA[1][j]));
      uv[2 + j] = T(gA[0][j]);
      uv[4 + j] = T(gA[1][j]);
    }
#pragma unroll
    for (int j = 0; j < 3; ++j) {
      gp[0][j] = T(-(gP[0][j] + gP[1][j]));
      gp[1][j] = T(gP[0][j]);
      gp[2][j] = T(gP[1][j]);
    }
    if (g_v012) {
#pragma unroll
      for (int k = 0; k < 3; ++k)
#pragma unroll
        for (int j = 0; j < 3; ++j) gp[k][j] += g_v012[i * 9 + k * 3 + j];
    }
  }
  T* o = pos_rows + i * 9;
#pragma unroll
  for (int k = 0; k < 3; ++k)
#pragma unroll
    for (int j = 0; j < 3; ++j) o[k * 3 + j] = gp[k][j];
}

// Backward of face_attribute_to_vert (and of vert_normals' fnorms): out[n,f,:] = sum over the three corners of the
// per-vertex gradient [N,V,A], through F.normalize's backward when `sums` is given (A = 3 then).
template <typename T>
__global__ __launch_bounds__(kBlock) void geom_face_gather_kernel(
    const T* __restrict__ g_vert, const T* __restrict__ sums, const int32_t* __restrict__ vi, int64_t vi_sN,
    int64_t N, int64_t V, int64_t F, int64_t A, T* __restrict__ out) {
  const int64_t i = int64_t(blockIdx.x) * kBlock + threadIdx.x;
  if (i >= N * F) return;
  const int64_t n = i / F, f = i - n * F;
  const int32_t* fi = vi + n * vi_sN + f * 3;
  if (sums) {
    T g[3];
    gather_corner_grads(g_vert, sums, fi, n * V, g);
#pragma unroll
    for (int j = 0; j < 3; ++j) out[i * 3 + j] = g[j];
    return;
  }
  const T* g0 = g_vert + (n * V + fi[0]) * A;
  const T* g1 = g_vert + (n * V + fi[1]) * A;
  const T* g2 = g_vert + (n * V + fi[2]) * A;
  for (int64_t a = 0; a < A; ++a) out[i * A + a] = (g0[a] + g1[a]) + g2[a];
}

// Sum of one chunk of a long incidence row: lane per (replica, chunk); replica = view when the topology is shared.
template <typename T>
__global__ __launch_bounds__(kBlock) void geom_vertex_chunk_kernel(
    const T* __restrict__ src, int64_t src_sN, int per_corner, int64_t A, const int32_t* __restrict__ crow,
    const int32_t* __restrict__ entries, const int32_t* __restrict__ chunk_begin, const int32_t* __restrict__ chunk_row,
    int64_t C, int64_t reps, int64_t V, bool shared, T* __restrict__ partial) {
  const int64_t i = int64_t(blockIdx.x) * kBlock + threadIdx.x;
  if (i >= reps * C) return;
  const int64_t rep = i / C, c = i - rep * C;
  const int64_t r = chunk_row[c];
  const int64_t n = shared ? rep : r / V;
  const int32_t beg = chunk_begin[c];
  const int32_t end = min(beg + kChunk, crow[r + 1]);
  const T* s = src + n * src_sN;
  for (int64_t a0 = 0; a0 < A; a0 += 4) {
    T acc[4] = {T(0), T(0), T(0), T(0)};
#pragma unroll 4
    for (int32_t j = beg; j < end; ++j) {
      const int64_t e = entries[j];
      const T* x = s + (per_corner ? e : e / 3) * A + a0;
#pragma unroll
      for (int q = 0; q < 4; ++q)
        if (a0 + q < A) acc[q] += x[q];
    }
#pragma unroll
    for (int q = 0; q < 4; ++q)
      if (a0 + q < A) partial[i * A + a0 + q] = acc[q];
  }
}

// out[n,v,:] = sum of the rows of the vertex's incidence row (in CSR order; a long row: its chunk sums in chunk
// order), NORMALIZE: out = sum / max(|sum|, 1e-12) and sums = sum (A = 3).
template <typename T, bool NORMALIZE>
__global__ __launch_bounds__(kBlock) void geom_vertex_gather_kernel(
    const T* __restrict__ src, int64_t src_sN, int per_corner, int64_t A_, const int32_t* __restrict__ crow,
    const int32_t* __restrict__ entries, const int32_t* __restrict__ chunk_ptr, const T* __restrict__ partial,
    int64_t C, bool shared, int64_t N, int64_t V, T* __restrict__ out, T* __restrict__ sums) {
  const int64_t i = int64_t(blockIdx.x) * kBlock + threadIdx.x;
  if (i >= N * V) return;
  const int64_t A = NORMALIZE ? 3 : A_;
  const int64_t n = i / V, v = i - n * V;
  const int64_t r = (shared ? 0 : n * V) + v;
  const T* s = src + n * src_sN;
  const int32_t c0 = chunk_ptr ? chunk_ptr[r] : 0, c1 = chunk_ptr ? chunk_ptr[r + 1] : 0;
  const int32_t beg = crow[r], end = crow[r + 1];
  for (int64_t a0 = 0; a0 < A; a0 += 4) {
    T acc[4] = {T(0), T(0), T(0), T(0)};
    if (c1 > c0) {
      const T* part = partial + (shared ? n * C : 0) * A + a0;
      for (int32_t c = c0; c < c1; ++c) {
#pragma unroll
        for (int q = 0; q < 4; ++q)
          if (a0 + q < A) acc[q] += part[int64_t(c) * A + q];
      }
    } else {
#pragma unroll 4
      for (int32_t j = beg; j < end; ++j) {
        const int64_t e = entries[j];
        const T* x = s + (per_corner ? e : e / 3) * A + a0;
#pragma unroll
        for (int q = 0; q < 4; ++q)
          if (a0 + q < A) acc[q] += x[q];
      }
    }
    if (NORMALIZE) {
      const T nrm = norm3(acc);
      const T d = nrm < T(1e-12) ? T(1e-12) : nrm;
#pragma unroll
      for (int q = 0; q < 3; ++q) {
        out[i * 3 + q] = acc[q] / d;
        if (sums) sums[i * 3 + q] = acc[q];
      }
    } else {
#pragma unroll
      for (int q = 0; q < 4; ++q)
        if (a0 + q < A) out[i * A + a0 + q] = acc[q];
    }
  }
}

// ---- cotangent weights and the mesh Laplacian ---------------------------------------------------------------------
// w[n,f,k] = dot(p_{k+1} - p_k, p_{k+2} - p_k) / (2 |c|) = cot(angle at corner k) / 2, c of the face pass; exactly 0 for
// all three k where |c| > 0 is false (c zero: duplicate or collinear corners; c NaN).
template <typename T>
__global__ __launch_bounds__(kBlock) void cot_weights_face_kernel(
    const T* __restrict__ v, int64_t v_sN, const int32_t* __restrict__ vi, int64_t vi_sN, int64_t N, int64_t F,
    T* __restrict__ w) {
  const int64_t i = int64_t(blockIdx.x) * kBlock + threadIdx.x;
  if (i >= N * F) return;
  const int64_t n = i / F, f = i - n * F;
  T p[3][3];
  load_corners(v + n * v_sN, vi + n * vi_sN + f * 3, p);
  T a[3], b[3], c[3];
#pragma unroll
  for (int j = 0; j < 3; ++j) a[j] = p[0][j] - p[2][j], b[j] = p[1][j] - p[0][j];
  cross3(a, b, c);
  const T nrm = norm3(c);
  const bool ok = nrm > T(0);
#pragma unroll
  for (int k = 0; k < 3; ++k) {
    const int k1 = (k + 1) % 3, k2 = (k + 2) % 3;
    T d = T(0);
#pragma unroll
    for (int j = 0; j < 3; ++j) d += (p[k1][j] - p[k][j]) * (p[k2][j] - p[k][j]);
    w[i * 3 + k] = ok ? d / (T(2) * nrm) : T(0);
  }
}

// Backward of the above: the per-corner rows [N,F,3,3] of grad_v from g_w [N,F,3]; a face whose weights are the
// degenerate zeros gives zero rows.
template <typename T>
__global__ __launch_bounds__(kBlock) void cot_weights_face_backward_kernel(
    const T* __restrict__ v, int64_t v_sN, const int32_t* __restrict__ vi, int64_t vi_sN, int64_t N, int64_t F,
    const T* __restrict__ g_w, T* __restrict__ pos_rows) {
  const int64_t i = int64_t(blockIdx.x) * kBlock + threadIdx.x;
  if (i >= N * F) return;
  const int64_t n = i / F, f = i - n * F;
  T p[3][3];
  load_corners(v + n * v_sN, vi + n * vi_sN + f * 3, p);
  T a[3], b[3], c[3];
#pragma unroll
  for (int j = 0; j < 3; ++j) a[j] = p[0][j] - p[2][j], b[j] = p[1][j] - p[0][j];
  cross3(a, b, c);
  const T nrm = norm3(c);
  T gp[3][3] = {{T(0), T(0), T(0)}, {T(0), T(0), T(0)}, {T(0), T(0), T(0)}};
  if (nrm > T(0)) {
    const T two_nrm = T(2) * nrm;
    T gn = T(0); // gradient of |c|:  w_k = d_k / (2 |c|)
#pragma unroll
    for (int k = 0; k < 3; ++k) {
      const int k1 = (k + 1) % 3, k2 = (k + 2) % 3;
      T e1[3], e2[3], d = T(0);
#pragma unroll
      for (int j = 0; j < 3; ++j) {
        e1[j] = p[k1][j] - p[k][j], e2[j] = p[k2][j] - p[k][j];
        d += e1[j] * e2[j];
      }
      const T g = g_w[i * 3 + k];
      const T gd = g / two_nrm;
      gn -= (g * d) / (two_nrm * nrm);
#pragma unroll
      for (int j = 0; j < 3; ++j) {
        gp[k1][j] += gd * e2[j];
        gp[k2][j] += gd * e1[j];
        gp[k][j] -= gd * (e1[j] + e2[j]);
      }
    }
    // |c| -> c = a x b:  gc = gn c / |c|, ga = b x gc, gb = gc x a;  a = p0 - p2, b = p1 - p0
    T gc[3], ga[3], gb[3];
#pragma unroll
    for (int j = 0; j < 3; ++j) gc[j] = gn * (c[j] / nrm);
    cross3(b, gc, ga);
    cross3(gc, a, gb);
#pragma unroll
    for (int j = 0; j < 3; ++j) {
      gp[0][j] += ga[j] - gb[j];
      gp[1][j] += gb[j];
      gp[2][j] -= ga[j];
    }
  }
  T* o = pos_rows + i * 9;
#pragma unroll
  for (int k = 0; k < 3; ++k)
#pragma unroll
    for (int j = 0; j < 3; ++j) o[k * 3 + j] = gp[k][j];
}

// The entries [beg, end) of vertex i's incidence row, channels c0 .. c0+3 of C: per entry (f, k), i = a_k, the bracket
//   w[f,k+1] * (x[a_{k+2}] - x[i]) + w[f,k+2] * (x[a_{k+1}] - x[i])
// evaluated as written and then added to acc, in entry order.  x, vi, w: the view's.  WEIGHTED false: every w is 1/2 and
// w is not read.
template <typename T, bool WEIGHTED>
__device__ __forceinline__ void laplacian_entries(
    const T* __restrict__ x, const int32_t* __restrict__ vi, const T* __restrict__ w,
    const int32_t* __restrict__ entries, int32_t beg, int32_t end, const T xi[4], int64_t C, int64_t c0, T acc[4]) {
#pragma unroll 2
  for (int32_t j = beg; j < end; ++j) {
    const int32_t e = entries[j];
    const int32_t f = e / 3, k = e - f * 3;
    const int k1 = k == 2 ? 0 : k + 1, k2 = k == 0 ? 2 : k - 1;
    const int64_t f3 = int64_t(f) * 3;
    const T* x1 = x + int64_t(vi[f3 + k1]) * C + c0;
    const T* x2 = x + int64_t(vi[f3 + k2]) * C + c0;
    const T w1 = WEIGHTED ? w[f3 + k1] : T(0.5);
    const T w2 = WEIGHTED ? w[f3 + k2] : T(0.5);
#pragma unroll
    for (int q = 0; q < 4; ++q)
      if (c0 + q < C) acc[q] += w1 * (x2[q] - xi[q]) + w2 * (x1[q] - xi[q]);
  }
}

// One chunk of a long incidence row: lane per (replica, chunk); replica = view when the topology is shared.
template <typename T, bool WEIGHTED>
__global__ __launch_bounds__(kBlock) void laplacian_chunk_kernel(
    const T* __restrict__ x, int64_t C, const int32_t* __restrict__ vi, int64_t vi_sN, const T* __restrict__ w,
    int64_t w_sN, const int32_t* __restrict__ crow, const int32_t* __restrict__ entries,
    const int32_t* __restrict__ chunk_begin, const int32_t* __restrict__ chunk_row, int64_t num_chunks, int64_t reps,
    int64_t V, bool shared, T* __restrict__ partial) {
  const int64_t i = int64_t(blockIdx.x) * kBlock + threadIdx.x;
  if (i >= reps * num_chunks) return;
  const int64_t rep = i / num_chunks, c = i - rep * num_chunks;
  const int64_t r = chunk_row[c];
  const int64_t b = r / V, vert = r - b * V;
  const int64_t n = shared ? rep : b;
  const int32_t beg = chunk_begin[c];
  const int32_t end = min(beg + kChunk, crow[r + 1]);
  const T* xn = x + n * V * C;
  for (int64_t c0 = 0; c0 < C; c0 += 4) {
    T xi[4], acc[4] = {T(0), T(0), T(0), T(0)};
#pragma unroll
    for (int q = 0; q < 4; ++q) xi[q] = c0 + q < C ? xn[vert * C + c0 + q] : T(0);
    laplacian_entries<T, WEIGHTED>(xn, vi + n * vi_sN, WEIGHTED ? w + n * w_sN : nullptr, entries, beg, end, xi, C, c0, acc);
#pragma unroll
    for (int q = 0; q < 4; ++q)
      if (c0 + q < C) partial[i * C + c0 + q] = acc[q];
  }
}

// out[n,i,:] = sum_j w_ij (x_j - x_i): lane per (view, vertex) over its incidence row in CSR order; a long row: its
// chunk sums in chunk order.
template <typename T, bool WEIGHTED>
__global__ __launch_bounds__(kBlock) void laplacian_vertex_kernel(
    const T* __restrict__ x, int64_t C, const int32_t* __restrict__ vi, int64_t vi_sN, const T* __restrict__ w,
    int64_t w_sN, const int32_t* __restrict__ crow, const int32_t* __restrict__ entries,
    const int32_t* __restrict__ chunk_ptr, const T* __restrict__ partial, int64_t num_chunks, bool shared, int64_t N,
    int64_t V, T* __restrict__ out) {
  const int64_t i = int64_t(blockIdx.x) * kBlock + threadIdx.x;
  if (i >= N * V) return;
  const int64_t n = i / V, vert = i - n * V;
  const int64_t r = (shared ? 0 : n * V) + vert;
  const int32_t c0_ = chunk_ptr ? chunk_ptr[r] : 0, c1_ = chunk_ptr ? chunk_ptr[r + 1] : 0;
  const int32_t beg = crow[r], end = crow[r + 1];
  const T* xn = x + n * V * C;
  for (int64_t c0 = 0; c0 < C; c0 += 4) {
    T acc[4] = {T(0), T(0), T(0), T(0)};
    if (c1_ > c0_) {
      const T* part = partial + (shared ? n * num_chunks : 0) * C + c0;
      for (int32_t c = c0_; c < c1_; ++c) {
#pragma unroll
        for (int q = 0; q < 4; ++q)
          if (c0 + q < C) acc[q] += part[int64_t(c) * C + q];
      }
    } else {
      T xi[4];
#pragma unroll
      for (int q = 0; q < 4; ++q) xi[q] = c0 + q < C ? xn[vert * C + c0 + q] : T(0);
      laplacian_entries<T, WEIGHTED>(xn, vi + n * vi_sN, WEIGHTED ? w + n * w_sN : nullptr, entries, beg, end, xi, C, c0, acc);
    }
#pragma unroll
    for (int q = 0; q < 4; ++q)
      if (c0 + q < C) out[i * C + c0 + q] = acc[q];
  }
}

// grad_w[n,f,k] = -dot(g[a_{k+1}] - g[a_{k+2}], x[a_{k+1}] - x[a_{k+2}]) over the channels, ascending; shared weights:
// lane per face, the views' dots subtracted from 0 in ascending n.
template <typename T>
__global__ __launch_bounds__(kBlock) void laplacian_grad_weights_kernel(
    const T* __restrict__ g, const T* __restrict__ x, int64_t C, const int32_t* __restrict__ vi, int64_t vi_sN,
    int64_t N, int64_t V, int64_t F, bool shared_w, T* __restrict__ grad_w) {
  const int64_t i = int64_t(blockIdx.x) * kBlock + threadIdx.x;
  if (i >= (shared_w ? 1 : N) * F) return;
  const int64_t nw = i / F, f = i - nw * F;
  const int64_t n0 = shared_w ? 0 : nw, n1 = shared_w ? N : nw + 1;
  T acc[3] = {T(0), T(0), T(0)};
  for (int64_t n = n0; n < n1; ++n) {
    const int32_t* fi = vi + n * vi_sN + f * 3;
    const T* gn = g + n * V * C;
    const T* xn = x + n * V * C;
    const int64_t a[3] = {int64_t(fi[0]) * C, int64_t(fi[1]) * C, int64_t(fi[2]) * C};
    T d[3] = {T(0), T(0), T(0)};
    for (int64_t c = 0; c < C; ++c) {
      const T gv[3] = {gn[a[0] + c], gn[a[1] + c], gn[a[2] + c]};
      const T xv[3] = {xn[a[0] + c], xn[a[1] + c], xn[a[2] + c]};
#pragma unroll
      for (int k = 0; k < 3; ++k) {
        const int k1 = (k + 1) % 3, k2 = (k + 2) % 3;
        d[k] += (gv[k1] - gv[k2]) * (xv[k1] - xv[k2]);
      }
    }
#pragma unroll
    for (int k = 0; k < 3; ++k) acc[k] -= d[k];
  }
#pragma unroll
  for (int k = 0; k < 3; ++k) grad_w[i * 3 + k] = acc[k];
}

inline dim3 grid_1d(int64_t items) {
  return dim3(static_cast<unsigned>(ceil_div(items, kBlock)));
}
constexpr int64_t kMaxLanes = (int64_t(1) << 31) * kBlock - kBlock; // grid.x < 2^31 blocks

template <typename T>
int face_forward_impl(const void* v, int64_t v_sN, const int32_t* vi, int64_t vi_sN, const void* vt, int64_t vt_sN,
                      const int32_t* vti, int64_t N, int64_t F, void* normals, void* areas, void* edges, void* dpdt,
                      void* dpdt_u, void* v012, hipStream_t s) {
  DRTK_LAUNCH((geom_face_forward_kernel<T>), grid_1d(N * F), dim3(kBlock), 0, s, static_cast<const T*>(v), v_sN, vi,
              vi_sN, static_cast<const T*>(vt), vt_sN, vti, N, F, static_cast<T*>(normals), static_cast<T*>(areas),
              static_cast<T*>(edges), static_cast<T*>(dpdt), static_cast<T*>(dpdt_u), static_cast<T*>(v012));
  DRTK_RETURN_IF_LAUNCH_FAILED();
  return DRTK_OK;
}

template <typename T>
int face_backward_impl(const void* v, int64_t v_sN, const int32_t* vi, int64_t vi_sN, const void* vt, int64_t vt_sN,
                       const int32_t* vti, int64_t N, int64_t V, int64_t F, const void* g_vert, const void* sums,
                       const void* g_normals, const void* g_areas, const void* g_edges, const void* g_dpdt,
                       const void* g_v012, void* pos_rows, void* uv_rows, hipStream_t s) {
  const T* cv = static_cast<const T*>(v);
  const T* cvt = static_cast<const T*>(vt);
  if (vt) {
    DRTK_LAUNCH((geom_face_backward_kernel<T, true>), grid_1d(N * F), dim3(kBlock), 0, s, cv, v_sN, vi, vi_sN, cvt,
                vt_sN, vti, N, V, F, static_cast<const T*>(g_vert), static_cast<const T*>(sums),
                static_cast<const T*>(g_normals), static_cast<const T*>(g_areas), static_cast<const T*>(g_edges),
                static_cast<const T*>(g_dpdt), static_cast<const T*>(g_v012), static_cast<T*>(pos_rows),
                static_cast<T*>(uv_rows));
  } else {
    DRTK_LAUNCH((geom_face_backward_kernel<T, false>), grid_1d(N * F), dim3(kBlock), 0, s, cv, v_sN, vi, vi_sN, cvt,
                vt_sN, vti, N, V, F, static_cast<const T*>(g_vert), static_cast<const T*>(sums),
                static_cast<const T*>(g_normals), static_cast<const T*>(g_areas), static_cast<const T*>(g_edges),
                static_cast<const T*>(g_dpdt), static_cast<const T*>(g_v012), static_cast<T*>(pos_rows),
                static_cast<T*>(uv_rows));
  }
  DRTK_RETURN_IF_LAUNCH_FAILED();
  return DRTK_OK;
}

template <typename T>
int face_gather_impl(const void* g_vert, const void* sums, const int32_t* vi, int64_t vi_sN, int64_t N, int64_t V,
                     int64_t F, int64_t A, void* out, hipStream_t s) {
  DRTK_LAUNCH((geom_face_gather_kernel<T>), grid_1d(N * F), dim3(kBlock), 0, s, static_cast<const T*>(g_vert),
              static_cast<const T*>(sums), vi, vi_sN, N, V, F, A, static_cast<T*>(out));
  DRTK_RETURN_IF_LAUNCH_FAILED();
  return DRTK_OK;
}

template <typename T>
int vertex_gather_impl(const void* src, int64_t src_sN, int per_corner, int64_t A, const int32_t* crow,
                       const int32_t* entries, const int32_t* chunk_ptr, const int32_t* chunk_begin,
                       const int32_t* chunk_row, int64_t C, int64_t B, int64_t N, int64_t V, void* out, void* sums,
                       int normalize, void* workspace, hipStream_t s) {
  const bool shared = B == 1;
  T* partial = static_cast<T*>(workspace);
  if (C > 0) {
    const int64_t reps = shared ? N : 1;
    DRTK_LAUNCH((geom_vertex_chunk_kernel<T>), grid_1d(reps * C), dim3(kBlock), 0, s, static_cast<const T*>(src),
                src_sN, per_corner, A, crow, entries, chunk_begin, chunk_row, C, reps, V, shared, partial);
    DRTK_RETURN_IF_LAUNCH_FAILED();
  }
  if (N * V == 0) return DRTK_OK;
  if (normalize) {
    DRTK_LAUNCH((geom_vertex_gather_kernel<T, true>), grid_1d(N * V), dim3(kBlock), 0, s, static_cast<const T*>(src),
                src_sN, per_corner, A, crow, entries, C > 0 ? chunk_ptr : nullptr, partial, C, shared, N, V,
                static_cast<T*>(out), static_cast<T*>(sums));
  } else {
    DRTK_LAUNCH((geom_vertex_gather_kernel<T, false>), grid_1d(N * V), dim3(kBlock), 0, s, static_cast<const T*>(src),
                src_sN, per_corner, A, crow, entries, C > 0 ? chunk_ptr : nullptr, partial, C, shared, N, V,
                static_cast<T*>(out), static_cast<T*>(sums));
  }
  DRTK_RETURN_IF_LAUNCH_FAILED();
  return DRTK_OK;
}

template <typename T, bool WEIGHTED>
int laplacian_impl(const void* x, int64_t C, const int32_t* vi, int64_t vi_sN, const void* w, int64_t w_sN,
                   const int32_t* crow, const int32_t* entries, const int32_t* chunk_ptr, const int32_t* chunk_begin,
                   const int32_t* chunk_row, int64_t num_chunks, int64_t B, int64_t N, int64_t V, void* out,
                   void* workspace, hipStream_t s) {
  const bool shared = B == 1;
  T* partial = static_cast<T*>(workspace);
  if (num_chunks > 0) {
    const int64_t reps = shared ? N : 1;
    DRTK_LAUNCH((laplacian_chunk_kernel<T, WEIGHTED>), grid_1d(reps * num_chunks), dim3(kBlock), 0, s,
                static_cast<const T*>(x), C, vi, vi_sN, static_cast<const T*>(w), w_sN, crow, entries, chunk_begin,
                chunk_row, num_chunks, reps, V, shared, partial);
    DRTK_RETURN_IF_LAUNCH_FAILED();
  }
  DRTK_LAUNCH((laplacian_vertex_kernel<T, WEIGHTED>), grid_1d(N * V), dim3(kBlock), 0, s, static_cast<const T*>(x), C,
              vi, vi_sN, static_cast<const T*>(w), w_sN, crow, entries, num_chunks > 0 ? chunk_ptr : nullptr, partial,
              num_chunks, shared, N, V, static_cast<T*>(out));
  DRTK_RETURN_IF_LAUNCH_FAILED();
  return DRTK_OK;
}

// (no image here, so no bad_image(): the limits are 32-bit vertex and corner indices and kMaxLanes, one lane per face or vertex)
bool bad_sizes(int64_t N, int64_t V, int64_t F) {
  return N < 0 || V < 0 || F < 0 || V >= (int64_t(1) << 31) || F >= (int64_t(1) << 31) / 3 ||
         (N > 0 && (F > kMaxLanes / N || V > kMaxLanes / N));
}

} // namespace
} // namespace drtk_amd

using namespace drtk_amd;

extern "C" int drtk_amd_geometry_face_forward(
    drtk_dtype_t dtype, const void* v, int64_t v_sN, const int32_t* vi, int64_t vi_sN, const void* vt, int64_t vt_sN,
    const int32_t* vti, int64_t N, int64_t V, int64_t T_, int64_t F, void* normals, void* areas, void* edges,
    void* dpdt, void* dpdt_u, void* v012, drtk_stream_t stream) {
  if (!valid_dtype(dtype)) return DRTK_ERR_INVALID_ARGUMENT;
  if (bad_sizes(N, V, F) || T_ < 0 || T_ >= (int64_t(1) << 31)) return DRTK_ERR_INVALID_ARGUMENT;
  if (bad_view_stride(v_sN, V * 3) || bad_view_stride(vi_sN, F * 3) || bad_view_stride(vt_sN, T_ * 2)) return DRTK_ERR_INVALID_ARGUMENT;
  const bool uv = dpdt || dpdt_u;
  if (N * F == 0) return DRTK_OK; // (outputs without elements may be NULL)
  if (!normals && !areas && !edges && !uv && !v012) return DRTK_ERR_INVALID_ARGUMENT;
  if (!v || !vi || V == 0 || (uv && (!vt || !vti || T_ == 0))) return DRTK_ERR_INVALID_ARGUMENT;
  return dispatch_dtype(dtype, [&](auto tag) {
    using T = decltype(tag);
    return face_forward_impl<T>(v, v_sN, vi, vi_sN, vt, vt_sN, vti, N, F, normals, areas, edges, dpdt, dpdt_u, v012, static_cast<hipStream_t>(stream));
  });
}

extern "C" int drtk_amd_geometry_face_backward(
    drtk_dtype_t dtype, const void* v, int64_t v_sN, const int32_t* vi, int64_t vi_sN, const void* vt, int64_t vt_sN,
    const int32_t* vti, int64_t N, int64_t V, int64_t T_, int64_t F, const void* grad_vert, const void* vert_sums,
    const void* grad_normals, const void* grad_areas, const void* grad_edges, const void* grad_dpdt,
    const void* grad_v012, void* pos_rows, void* uv_rows, drtk_stream_t stream) {
  if (!valid_dtype(dtype)) return DRTK_ERR_INVALID_ARGUMENT;
  if (bad_sizes(N, V, F) || T_ < 0 || T_ >= (int64_t(1) << 31)) return DRTK_ERR_INVALID_ARGUMENT;
  if (bad_view_stride(v_sN, V * 3) || bad_view_stride(vi_sN, F * 3) || bad_view_stride(vt_sN, T_ * 2)) return DRTK_ERR_INVALID_ARGUMENT;
  const bool dp = vt != nullptr;
  if (dp ? (grad_normals || grad_areas || grad_edges || !uv_rows || !vti) : (grad_dpdt || grad_v012 || uv_rows))
    return DRTK_ERR_INVALID_ARGUMENT;
  if (vert_sums && !grad_vert) return DRTK_ERR_INVALID_ARGUMENT;
  if (N * F == 0) return DRTK_OK;
  if (!v || !vi || !pos_rows || V == 0 || (dp && T_ == 0)) return DRTK_ERR_INVALID_ARGUMENT;
  return dispatch_dtype(dtype, [&](auto tag) {
    using T = decltype(tag);
    return face_backward_impl<T>(
        v, v_sN, vi, vi_sN, vt, vt_sN, vti, N, V, F, grad_vert, vert_sums, grad_normals, grad_areas, grad_edges, grad_dpdt, grad_v012,
        pos_rows, uv_rows, static_cast<hipStream_t>(stream));
  });
}

extern "C" int drtk_amd_geometry_face_gather(
    drtk_dtype_t dtype, const void* grad_vert, const void* vert_sums, const int32_t* vi, int64_t vi_sN, int64_t N,
    int64_t V, int64_t F, int64_t A, void* out, drtk_stream_t stream) {
  if (!valid_dtype(dtype)) return DRTK_ERR_INVALID_ARGUMENT;
  if (bad_sizes(N, V, F) || A < 1 || (vert_sums && A != 3) || bad_view_stride(vi_sN, F * 3))
    return DRTK_ERR_INVALID_ARGUMENT;
  if (N * F == 0) return DRTK_OK;
  if (!grad_vert || !vi || !out || V == 0) return DRTK_ERR_INVALID_ARGUMENT;
  return dispatch_dtype(dtype, [&](auto tag) {
    using T = decltype(tag);
    return face_gather_impl<T>(grad_vert, vert_sums, vi, vi_sN, N, V, F, A, out, static_cast<hipStream_t>(stream));
  });
}

extern "C" int drtk_amd_geometry_vertex_gather_workspace_bytes(
    drtk_dtype_t dtype, int64_t N, int64_t B, int64_t num_chunks, int64_t A, size_t* bytes) {
  if (!valid_dtype(dtype) || !bytes || N < 0 || num_chunks < 0 || A < 1 || (B != 1 && B != N))
    return DRTK_ERR_INVALID_ARGUMENT;
  *bytes = size_t((B == 1 ? N : 1) * num_chunks * A) * dtype_size(dtype);
  return DRTK_OK;
}

extern "C" int drtk_amd_geometry_vertex_gather(
    drtk_dtype_t dtype, const void* src, int64_t src_sN, int per_corner, int64_t A, const int32_t* crow,
    const int32_t* entries, const int32_t* chunk_ptr, const int32_t* chunk_begin, const int32_t* chunk_row,
    int64_t num_chunks, int64_t B, int64_t N, int64_t V, int64_t F, int normalize, void* out, void* vert_sums,
    void* workspace, size_t workspace_bytes, drtk_stream_t stream) {
  if (!valid_dtype(dtype)) return DRTK_ERR_INVALID_ARGUMENT;
  if (bad_sizes(N, V, F) || A < 1 || num_chunks < 0 || (normalize && A != 3) || (vert_sums && !normalize))
    return DRTK_ERR_INVALID_ARGUMENT;
  if ((B != 1 && B != N) || (per_corner != 0 && per_corner != 1) || src_sN != F * A * (per_corner ? 3 : 1))
    return DRTK_ERR_INVALID_ARGUMENT;
  if (N > 0 && (num_chunks > kMaxLanes / N || 3 * F * B >= (int64_t(1) << 31))) return DRTK_ERR_INVALID_ARGUMENT;
  if (N * V == 0) return DRTK_OK;
  if (!crow || !out || (F > 0 && (!src || !entries))) return DRTK_ERR_INVALID_ARGUMENT;
  if (num_chunks > 0) {
    if (!chunk_ptr || !chunk_begin || !chunk_row) return DRTK_ERR_INVALID_ARGUMENT;
    size_t need = 0;
    drtk_amd_geometry_vertex_gather_workspace_bytes(dtype, N, B, num_chunks, A, &need);
    if (!workspace || workspace_bytes < need) return DRTK_ERR_WORKSPACE_TOO_SMALL;
  }
  return dispatch_dtype(dtype, [&](auto tag) {
    using T = decltype(tag);
    return vertex_gather_impl<T>(
        src, src_sN, per_corner, A, crow, entries, chunk_ptr, chunk_begin, chunk_row, num_chunks, B, N, V, out, vert_sums, normalize,
        workspace, static_cast<hipStream_t>(stream));
  });
}

extern "C" int drtk_amd_geometry_cot_weights(
    drtk_dtype_t dtype, const void* v, int64_t v_sN, const int32_t* vi, int64_t vi_sN, int64_t N, int64_t V, int64_t F,
    void* weights, drtk_stream_t stream) {
  if (!valid_dtype(dtype)) return DRTK_ERR_INVALID_ARGUMENT;
  if (bad_sizes(N, V, F) || bad_view_stride(v_sN, V * 3) || bad_view_stride(vi_sN, F * 3)) return DRTK_ERR_INVALID_ARGUMENT;
  if (N * F == 0) return DRTK_OK;
  if (!v || !vi || !weights || V == 0) return DRTK_ERR_INVALID_ARGUMENT;
  return dispatch_dtype(dtype, [&](auto tag) -> int {
    using T = decltype(tag);
    const hipStream_t s = static_cast<hipStream_t>(stream);
    DRTK_LAUNCH((cot_weights_face_kernel<T>), grid_1d(N * F), dim3(kBlock), 0, s, static_cast<const T*>(v), v_sN, vi, vi_sN, N, F, static_cast<T*>(weights));
    DRTK_RETURN_IF_LAUNCH_FAILED();
    return DRTK_OK;
  });
}

extern "C" int drtk_amd_geometry_cot_weights_backward(
    drtk_dtype_t dtype, const void* v, int64_t v_sN, const int32_t* vi, int64_t vi_sN, int64_t N, int64_t V, int64_t F,
    const void* grad_weights, void* pos_rows, drtk_stream_t stream) {
  if (!valid_dtype(dtype)) return DRTK_ERR_INVALID_ARGUMENT;
  if (bad_sizes(N, V, F) || bad_view_stride(v_sN, V * 3) || bad_view_stride(vi_sN, F * 3)) return DRTK_ERR_INVALID_ARGUMENT;
  if (N * F == 0) return DRTK_OK;
  if (!v || !vi || !grad_weights || !pos_rows || V == 0) return DRTK_ERR_INVALID_ARGUMENT;
  return dispatch_dtype(dtype, [&](auto tag) -> int {
    using T = decltype(tag);
    const hipStream_t s = static_cast<hipStream_t>(stream);
    DRTK_LAUNCH((cot_weights_face_backward_kernel<T>), grid_1d(N * F), dim3(kBlock), 0, s, static_cast<const T*>(v), v_sN, vi, vi_sN, N, F, static_cast<const T*>(grad_weights), static_cast<T*>(pos_rows));
    DRTK_RETURN_IF_LAUNCH_FAILED();
    return DRTK_OK;
  });
}

extern "C" int drtk_amd_geometry_laplacian_workspace_bytes(
    drtk_dtype_t dtype, int64_t N, int64_t B, int64_t num_chunks, int64_t C, size_t* bytes) {
  return drtk_amd_geometry_vertex_gather_workspace_bytes(dtype, N, B, num_chunks, C, bytes); // one partial row per (replica, chunk)
}

extern "C" int drtk_amd_geometry_laplacian(
    drtk_dtype_t dtype, const void* x, int64_t C, const int32_t* vi, int64_t vi_sN, const void* weights, int64_t w_sN,
    const int32_t* crow, const int32_t* entries, const int32_t* chunk_ptr, const int32_t* chunk_begin,
    const int32_t* chunk_row, int64_t num_chunks, int64_t B, int64_t N, int64_t V, int64_t F, void* out, void* workspace,
    size_t workspace_bytes, drtk_stream_t stream) {
  if (!valid_dtype(dtype)) return DRTK_ERR_INVALID_ARGUMENT;
  if (bad_sizes(N, V, F) || C < 1 || num_chunks < 0 || (B != 1 && B != N)) return DRTK_ERR_INVALID_ARGUMENT;
  // the topology the incidence was built from: shared (B = 1, stride 0) or one per view
  if (bad_view_stride(vi_sN, F * 3) || (N > 1 && (vi_sN != 0) != (B == N))) return DRTK_ERR_INVALID_ARGUMENT;
  if (bad_view_stride(w_sN, F * 3) || (!weights && w_sN != 0)) return DRTK_ERR_INVALID_ARGUMENT;
  if (N > 0 && (num_chunks > kMaxLanes / N || 3 * F * B >= (int64_t(1) << 31))) return DRTK_ERR_INVALID_ARGUMENT;
  if (N * V == 0) return DRTK_OK;
  if (!x || !crow || !out || (F > 0 && (!vi || !entries))) return DRTK_ERR_INVALID_ARGUMENT;
  if (num_chunks > 0) {
    if (!chunk_ptr || !chunk_begin || !chunk_row) return DRTK_ERR_INVALID_ARGUMENT;
    size_t need = 0;
    drtk_amd_geometry_laplacian_workspace_bytes(dtype, N, B, num_chunks, C, &need);
    if (!workspace || workspace_bytes < need) return DRTK_ERR_WORKSPACE_TOO_SMALL;
  }
  return dispatch_dtype(dtype, [&](auto tag) -> int {
    using T = decltype(tag);
    const hipStream_t s = static_cast<hipStream_t>(stream);
    if (weights)
      return laplacian_impl<T, true>(x, C, vi, vi_sN, weights, w_sN, crow, entries, chunk_ptr, chunk_begin, chunk_row, num_chunks, B, N, V, out, workspace, s);
    return laplacian_impl<T, false>(x, C, vi, vi_sN, nullptr, 0, crow, entries, chunk_ptr, chunk_begin, chunk_row, num_chunks, B, N, V, out, workspace, s);
  });
}

extern "C" int drtk_amd_geometry_laplacian_grad_weights(
    drtk_dtype_t dtype, const void* grad_out, const void* x, int64_t C, const int32_t* vi, int64_t vi_sN, int64_t N,
    int64_t V, int64_t F, int64_t weights_B, void* grad_weights, drtk_stream_t stream) {
  if (!valid_dtype(dtype)) return DRTK_ERR_INVALID_ARGUMENT;
  if (bad_sizes(N, V, F) || C < 1 || bad_view_stride(vi_sN, F * 3) || (weights_B != 1 && weights_B != N))
    return DRTK_ERR_INVALID_ARGUMENT;
  if (weights_B * F == 0) return DRTK_OK;
  if (!vi || !grad_weights || (N > 0 && (!grad_out || !x || V == 0))) return DRTK_ERR_INVALID_ARGUMENT;
  const bool shared_w = weights_B == 1; // (N = 0 with shared weights: the empty sum, zeros)
  return dispatch_dtype(dtype, [&](auto tag) -> int {
    using T = decltype(tag);
    const hipStream_t s = static_cast<hipStream_t>(stream);
    DRTK_LAUNCH((laplacian_grad_weights_kernel<T>), grid_1d(weights_B * F), dim3(kBlock), 0, s, static_cast<const T*>(grad_out), static_cast<const T*>(x), C, vi, vi_sN, N, V, F, shared_w, static_cast<T*>(grad_weights));
    DRTK_RETURN_IF_LAUNCH_FAILED();
    return DRTK_OK;
  });
}
