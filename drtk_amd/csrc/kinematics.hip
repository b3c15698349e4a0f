// Forward kinematics along a joint tree: pose (axis-angle vectors or rotation matrices) and rest joints to the skinning
// matrices `skin` reads and the posed joint positions, forward and the gradients to the rotations, the rest joints and the
// root translation, without atomics (no counterpart in the reference's library).
//
//   With p = parents[j] (-1: a root, else p < j), R_j the local rotation, c_j the rest joint:
//     root:   G_j.R = R_j             G_j.t = c_j + translation
//     child:  G_j.R = G_p.R R_j       G_j.t = G_p.R (c_j - c_p) + G_p.t
//     posed[n,j] = G_j.t              transforms[n,j] = [ G_j.R | G_j.t - G_j.R c_j ]
//
//   forward   one wave-sized workgroup per view.  Lanes stride over the joints and form the local [R_j | c_j - c_p] in LDS
//             (Rodrigues runs here, off the dependent chain); then the levels of the tree in order, a barrier after each:
//             the lane of a joint reads its parent's G from LDS and writes its own over its local; finally the lanes write
//             both outputs with consecutive stores.
//   backward  the same workgroup recomputes the forward (locals in one LDS array, G in a second), then walks the levels in
//             reverse as a PULL: the lane of joint j adds its own output gradients and its children's messages (in
//             child_entries order), writes gG_j's message for its parent over its local, emits its row of grad_joints, and
//             leaves gR_j = G_p.R^T gG_j.R in G's slot, which nobody reads any more.  After the walk the lanes stride
//             over the joints again and pull gR_j back through Rodrigues (again off the chain); lane 0 adds the roots'
//             gG.t in index order for grad_translation.  A rest pose shared by N > 1 views gets its per-view rows in a
//             workspace and a second tiny launch adds them in view order, in double.
// The data is a few kilobytes: the cost is the launch and the chain of dependent levels, not bandwidth.  Every sum has
// one fixed order that the schedule fixes, so results are bitwise reproducible.
#include "common.hpp"

#include <type_traits>

namespace drtk_amd {
namespace {

constexpr int kFkMaxJoints = 320; // DRTK_FK_MAX_JOINTS: two LDS arrays of 12 doubles per joint = 61440 bytes <= 64 KiB
constexpr int kFkLanes = kWave;   // one wave per view
static_assert(kFkMaxJoints == DRTK_FK_MAX_JOINTS, "include/drtk_amd.h");
static_assert(2 * 12 * sizeof(double) * kFkMaxJoints <= 65536, "the backward's LDS state is static");

// Below this theta^2 the coefficients of the exponential map and their derivatives are Taylor series in theta^2 (five
// terms: the first neglected one is below 1e-13 of the leading one at either threshold); above it they are closed forms,
// whose cancellation (cos(theta) - a, a - 2b) is of relative size eps / theta^2 and enters the gradient times theta^2.
constexpr double kFkTaylorTheta2F32 = 0.0625;
constexpr double kFkTaylorTheta2F64 = 0.00390625;

template <typename T>
struct ExpCoeff {
  T a, b, da, db; // a = sin(t)/t, b = (1 - cos t)/t^2, da = da/d(t^2), db = db/d(t^2)
};

template <typename T, bool DERIV>
__device__ inline ExpCoeff<T> exp_coeff(T s) {
  ExpCoeff<T> c;
  c.da = c.db = T(0);
  const T thr = std::is_same<T, float>::value ? T(kFkTaylorTheta2F32) : T(kFkTaylorTheta2F64);
  if (s < thr) {
    c.a = T(1) + s * (T(-1.0 / 6) + s * (T(1.0 / 120) + s * (T(-1.0 / 5040) + s * T(1.0 / 362880))));
    c.b = T(0.5) + s * (T(-1.0 / 24) + s * (T(1.0 / 720) + s * (T(-1.0 / 40320) + s * T(1.0 / 3628800))));
    if (DERIV) {
      c.da = T(-1.0 / 6) + s * (T(2.0 / 120) + s * (T(-3.0 / 5040) + s * (T(4.0 / 362880) + s * T(-5.0 / 39916800))));
      c.db = T(-1.0 / 24) + s * (T(2.0 / 720) + s * (T(-3.0 / 40320) + s * (T(4.0 / 3628800) + s * T(-5.0 / 479001600))));
    }
  } else {
    const T t = sqrt(s);
    const T h = T(0.5) * t;
    const T sh = sin(h) / h;
    c.a = sin(t) / t;
    c.b = T(0.5) * (sh * sh); // not (1 - cos t)/t^2: no cancellation
    if (DERIV) {
      c.da = (cos(t) - c.a) / (T(2) * s);
      c.db = (c.a - T(2) * c.b) / (T(2) * s);
    }
  }
  return c;
}

// R = I + a K + b K^2, K the skew matrix of r, K^2 = r r^T - theta^2 I
template <typename T>
__device__ inline void rodrigues(T x, T y, T z, T* R) {
  const T s = x * x + y * y + z * z;
  const ExpCoeff<T> c = exp_coeff<T, false>(s);
  R[0] = T(1) + c.b * (x * x - s), R[1] = c.b * (x * y) - c.a * z, R[2] = c.b * (x * z) + c.a * y;
  R[3] = c.b * (x * y) + c.a * z, R[4] = T(1) + c.b * (y * y - s), R[5] = c.b * (y * z) - c.a * x;
  R[6] = c.b * (x * z) - c.a * y, R[7] = c.b * (y * z) + c.a * x, R[8] = T(1) + c.b * (z * z - s);
}

// the gradient to r of a gradient M to R = exp(skew(r))
template <typename T>
__device__ inline void rodrigues_pullback(T x, T y, T z, const T* M, T* g) {
  const T s = x * x + y * y + z * z;
  const ExpCoeff<T> c = exp_coeff<T, true>(s);
  const T r[3] = {x, y, z};
  const T w[3] = {M[7] - M[5], M[2] - M[6], M[3] - M[1]}; // <M, dK/dr_k>
  const T tr = M[0] + M[4] + M[8];
  T mr[3], mtr[3];
#pragma unroll
  for (int k = 0; k < 3; ++k) {
    mr[k] = M[k * 3] * x + M[k * 3 + 1] * y + M[k * 3 + 2] * z;
    mtr[k] = M[k] * x + M[3 + k] * y + M[6 + k] * z;
  }
  const T mk = x * w[0] + y * w[1] + z * w[2];                    // <M, K>
  const T mk2 = (x * mr[0] + y * mr[1] + z * mr[2]) - s * tr;     // <M, K^2>
  const T radial = T(2) * (c.da * mk + c.db * mk2);
#pragma unroll
  for (int k = 0; k < 3; ++k) g[k] = c.a * w[k] + c.b * ((mr[k] + mtr[k]) - T(2) * (r[k] * tr)) + r[k] * radial;
}

struct FkIn {
  const void* rot;      // axis-angle [N,J,3] or matrices [N,J,3,3], read through the strides
  int64_t r_sN, r_sJ, r_sA, r_sB;
  const void* joints;   // [J,3] (c_sN = 0) or [N,J,3] (c_sN = 3J), contiguous rows
  int64_t c_sN;
  const void* tr;       // [N,3] or null
  const int32_t *parents, *order, *level_start, *child_crow, *child_entries;
  int J, D;
};

// the local [R_j | c_j - c_p] (a root: [R_j | c_j + translation]), 12 values
template <typename T, bool MAT>
__device__ inline void fk_local(const FkIn& in, int64_t n, int j, int p, T* L) {
  const T* r = static_cast<const T*>(in.rot) + n * in.r_sN + int64_t(j) * in.r_sJ;
  if (MAT) {
#pragma unroll
    for (int a = 0; a < 3; ++a)
#pragma unroll
      for (int b = 0; b < 3; ++b) L[a * 3 + b] = r[a * in.r_sA + b * in.r_sB];
  } else {
    rodrigues<T>(r[0], r[in.r_sA], r[2 * in.r_sA], L);
  }
  const T* c = static_cast<const T*>(in.joints) + n * in.c_sN;
  if (p >= 0) {
#pragma unroll
    for (int a = 0; a < 3; ++a) L[9 + a] = c[j * 3 + a] - c[p * 3 + a];
  } else {
    const T* t = static_cast<const T*>(in.tr);
#pragma unroll
    for (int a = 0; a < 3; ++a) L[9 + a] = t ? c[j * 3 + a] + t[n * 3 + a] : c[j * 3 + a];
  }
}

// G = G_p o L
template <typename T>
__device__ inline void fk_compose(const T* P, const T* L, T* G) {
#pragma unroll
  for (int a = 0; a < 3; ++a) {
#pragma unroll
    for (int b = 0; b < 3; ++b) G[a * 3 + b] = P[a * 3] * L[b] + P[a * 3 + 1] * L[3 + b] + P[a * 3 + 2] * L[6 + b];
    G[9 + a] = (P[a * 3] * L[9] + P[a * 3 + 1] * L[10] + P[a * 3 + 2] * L[11]) + P[9 + a];
  }
}

template <typename T, bool MAT>
__global__ __launch_bounds__(kFkLanes) void fk_forward_kernel(FkIn in, T* __restrict__ transforms, T* __restrict__ posed) {
  __shared__ T G[kFkMaxJoints * 12];
  const int64_t n = blockIdx.x;
  const int lane = threadIdx.x, J = in.J;
  for (int j = lane; j < J; j += kFkLanes) {
    T L[12];
    fk_local<T, MAT>(in, n, j, in.parents[j], L);
#pragma unroll
    for (int q = 0; q < 12; ++q) G[j * 12 + q] = L[q];
  }
  __syncthreads();
  for (int l = 1; l < in.D; ++l) { // (level 0, the roots: G is the local)
    const int end = in.level_start[l + 1];
    for (int i = in.level_start[l] + lane; i < end; i += kFkLanes) {
      const int j = in.order[i];
      const int p = in.parents[j];
      T P[12], L[12], O[12];
#pragma unroll
      for (int q = 0; q < 12; ++q) P[q] = G[p * 12 + q], L[q] = G[j * 12 + q];
      fk_compose(P, L, O);
#pragma unroll
      for (int q = 0; q < 12; ++q) G[j * 12 + q] = O[q];
    }
    __syncthreads();
  }
  const T* c = static_cast<const T*>(in.joints) + n * in.c_sN;
  T* tn = transforms + n * J * 12;
  for (int q = lane; q < J * 12; q += kFkLanes) {
    const int j = q / 12, e = q - j * 12, a = e >> 2, b = e & 3;
    const T* g = G + j * 12;
    tn[q] = b < 3 ? g[a * 3 + b] : g[9 + a] - (g[a * 3] * c[j * 3] + g[a * 3 + 1] * c[j * 3 + 1] + g[a * 3 + 2] * c[j * 3 + 2]);
  }
  T* pn = posed + n * J * 3;
  for (int q = lane; q < J * 3; q += kFkLanes) {
    const int j = q / 3;
    pn[q] = G[j * 12 + 9 + (q - j * 3)];
  }
}

// grad_transforms [N,J,3,4] and grad_posed [N,J,3] may each be null (zero).  grad_rot: [N,J,3] / [N,J,3,3]; grad_joints:
// one row [J,3] per view (the output itself, or the workspace of a shared rest pose); grad_tr [N,3].
template <typename T, bool MAT, bool NEED_R, bool NEED_C, bool NEED_TR>
__global__ __launch_bounds__(kFkLanes) void fk_backward_kernel(
    FkIn in, const T* __restrict__ grad_transforms, const T* __restrict__ grad_posed, T* __restrict__ grad_rot,
    T* __restrict__ grad_joints, T* __restrict__ grad_tr) {
  __shared__ T G[kFkMaxJoints * 12];   // G_j; after joint j's turn in the reverse walk: gR_j
  __shared__ T Msg[kFkMaxJoints * 12]; // the local of joint j; after its turn: its message [gG_j.R R_j^T + gG_j.t d_j^T | gG_j.t]
  const int64_t n = blockIdx.x;
  const int lane = threadIdx.x, J = in.J;
  for (int j = lane; j < J; j += kFkLanes) {
    T L[12];
    const int p = in.parents[j];
    fk_local<T, MAT>(in, n, j, p, L);
#pragma unroll
    for (int q = 0; q < 12; ++q) Msg[j * 12 + q] = L[q];
    if (p < 0) {
#pragma unroll
      for (int q = 0; q < 12; ++q) G[j * 12 + q] = L[q];
    }
  }
  __syncthreads();
  for (int l = 1; l < in.D; ++l) {
    const int end = in.level_start[l + 1];
    for (int i = in.level_start[l] + lane; i < end; i += kFkLanes) {
      const int j = in.order[i];
      const int p = in.parents[j];
      T P[12], L[12], O[12];
#pragma unroll
      for (int q = 0; q < 12; ++q) P[q] = G[p * 12 + q], L[q] = Msg[j * 12 + q];
      fk_compose(P, L, O);
#pragma unroll
      for (int q = 0; q < 12; ++q) G[j * 12 + q] = O[q];
    }
    __syncthreads();
  }
  const T* c = static_cast<const T*>(in.joints) + n * in.c_sN;
  for (int l = in.D - 1; l >= 0; --l) {
    const int end = in.level_start[l + 1];
    for (int i = in.level_start[l] + lane; i < end; i += kFkLanes) {
      const int j = in.order[i];
      const int p = in.parents[j];
      const T cj[3] = {c[j * 3], c[j * 3 + 1], c[j * 3 + 2]};
      T gA[12]; // [n,j,a,b] at a*4+b
#pragma unroll
      for (int q = 0; q < 12; ++q) gA[q] = grad_transforms ? grad_transforms[(n * J + j) * 12 + q] : T(0);
      T gR[9], gt[3], sum_t[3] = {T(0), T(0), T(0)};
#pragma unroll
      for (int a = 0; a < 3; ++a) {
        gt[a] = grad_posed ? gA[a * 4 + 3] + grad_posed[(n * J + j) * 3 + a] : gA[a * 4 + 3];
#pragma unroll
        for (int b = 0; b < 3; ++b) gR[a * 3 + b] = gA[a * 4 + b] - gA[a * 4 + 3] * cj[b];
      }
      const int c1 = in.child_crow[j + 1];
      for (int e = in.child_crow[j]; e < c1; ++e) {
        const T* m = Msg + in.child_entries[e] * 12;
#pragma unroll
        for (int q = 0; q < 9; ++q) gR[q] += m[q];
#pragma unroll
        for (int a = 0; a < 3; ++a) gt[a] += m[9 + a], sum_t[a] += m[9 + a];
      }
      T Gj[9], P[9], L[12];
#pragma unroll
      for (int q = 0; q < 9; ++q) Gj[q] = G[j * 12 + q], P[q] = p >= 0 ? G[p * 12 + q] : T(0);
#pragma unroll
      for (int q = 0; q < 12; ++q) L[q] = Msg[j * 12 + q];
      if (NEED_C) {
        // -G_j.R^T gA.t + G_p.R^T gG_j.t (a root: gG_j.t) - G_j.R^T sum over the children of gG_c.t
        T* o = grad_joints + (n * J + j) * 3;
#pragma unroll
        for (int b = 0; b < 3; ++b) {
          const T own = Gj[b] * gA[3] + Gj[3 + b] * gA[7] + Gj[6 + b] * gA[11];
          const T up = p >= 0 ? P[b] * gt[0] + P[3 + b] * gt[1] + P[6 + b] * gt[2] : gt[b];
          const T down = Gj[b] * sum_t[0] + Gj[3 + b] * sum_t[1] + Gj[6 + b] * sum_t[2];
          o[b] = (up - own) - down;
        }
      }
      // the message to the parent (a root's is read for grad_translation only), over the local
#pragma unroll
      for (int a = 0; a < 3; ++a) {
#pragma unroll
        for (int b = 0; b < 3; ++b)
          Msg[j * 12 + a * 3 + b] =
              (gR[a * 3] * L[b * 3] + gR[a * 3 + 1] * L[b * 3 + 1] + gR[a * 3 + 2] * L[b * 3 + 2]) + gt[a] * L[9 + b];
        Msg[j * 12 + 9 + a] = gt[a];
      }
      if (NEED_R) {
        // gR_j = G_p.R^T gG_j.R into G's slot of joint j: its readers (its children) have had their turn
#pragma unroll
        for (int a = 0; a < 3; ++a)
#pragma unroll
          for (int b = 0; b < 3; ++b)
            G[j * 12 + a * 3 + b] = p >= 0 ? P[a] * gR[b] + P[3 + a] * gR[3 + b] + P[6 + a] * gR[6 + b] : gR[a * 3 + b];
      }
    }
    __syncthreads();
  }
  if (NEED_R) {
    if (MAT) {
      T* o = grad_rot + n * J * 9;
      for (int q = lane; q < J * 9; q += kFkLanes) {
        const int j = q / 9;
        o[q] = G[j * 12 + (q - j * 9)];
      }
    } else {
      for (int j = lane; j < J; j += kFkLanes) {
        const T* r = static_cast<const T*>(in.rot) + n * in.r_sN + int64_t(j) * in.r_sJ;
        T M[9], g[3];
#pragma unroll
        for (int q = 0; q < 9; ++q) M[q] = G[j * 12 + q];
        rodrigues_pullback<T>(r[0], r[in.r_sA], r[2 * in.r_sA], M, g);
        T* o = grad_rot + (n * J + j) * 3;
        o[0] = g[0], o[1] = g[1], o[2] = g[2];
      }
    }
  }
  if (NEED_TR && lane < 3) {
    T s = T(0);
    const int end = in.D > 0 ? in.level_start[1] : 0;
    for (int i = 0; i < end; ++i) s += Msg[in.order[i] * 12 + 9 + lane]; // the roots, ascending
    grad_tr[n * 3 + lane] = s;
  }
}

// a shared rest pose: the views' rows added in view order, in double
template <typename T>
__global__ __launch_bounds__(kBlock) void fk_joint_sum_kernel(const T* __restrict__ rows, int64_t N, int64_t per_view,
                                                              T* __restrict__ out) {
  const int64_t i = int64_t(blockIdx.x) * kBlock + threadIdx.x;
  if (i >= per_view) return;
  double s = 0.0;
  int64_t n = 0;
  // sixteen loads in flight, added in view order (one load at a time is a chain of N memory latencies)
  for (; n + 16 <= N; n += 16) {
    T t[16];
#pragma unroll
    for (int u = 0; u < 16; ++u) t[u] = rows[(n + u) * per_view + i];
#pragma unroll
    for (int u = 0; u < 16; ++u) s += double(t[u]);
  }
  for (; n < N; ++n) s += double(rows[n * per_view + i]);
  out[i] = T(s);
}

constexpr int64_t kMaxBlocks = (int64_t(1) << 31) - 1;

bool fk_bad_args(int64_t N, int64_t J, int64_t num_levels, int rot_is_matrix, int64_t c_sN) {
  return N < 0 || N > kMaxBlocks || J < 0 || J > kFkMaxJoints || num_levels < 0 || num_levels > J ||
         (J > 0 && num_levels == 0) || (rot_is_matrix != 0 && rot_is_matrix != 1) || bad_view_stride(c_sN, J * 3);
}

FkIn fk_in(const void* rot, const int64_t* rs, const void* joints, int64_t c_sN, const void* tr, const int32_t* parents,
           const int32_t* order, const int32_t* level_start, int64_t num_levels, const int32_t* child_crow,
           const int32_t* child_entries, int64_t J) {
  return FkIn{rot, rs[0], rs[1], rs[2], rs[3], joints, c_sN, tr, parents, order, level_start, child_crow, child_entries,
              int(J), int(num_levels)};
}

} // namespace
} // namespace drtk_amd

using namespace drtk_amd;

extern "C" int drtk_amd_kinematics_forward(
    drtk_dtype_t dtype, const void* rotations, int rot_is_matrix, const int64_t* rot_strides, const void* joints,
    int64_t c_sN, const void* translation, const int32_t* parents, const int32_t* order, const int32_t* level_start,
    int64_t num_levels, int64_t N, int64_t J, void* transforms, void* posed_joints, drtk_stream_t stream) {
  if (!valid_dtype(dtype) || !rot_strides) return DRTK_ERR_INVALID_ARGUMENT;
  if (fk_bad_args(N, J, num_levels, rot_is_matrix, c_sN)) return DRTK_ERR_INVALID_ARGUMENT;
  if (N * J == 0) return DRTK_OK;
  if (!rotations || !joints || !parents || !order || !level_start || !transforms || !posed_joints)
    return DRTK_ERR_INVALID_ARGUMENT;
  return dispatch_dtype(dtype, [&](auto tag) -> int {
    using T = decltype(tag);
    const hipStream_t s = static_cast<hipStream_t>(stream);
    const FkIn in = fk_in(rotations, rot_strides, joints, c_sN, translation, parents, order, level_start, num_levels,
                          nullptr, nullptr, J);
    const dim3 grid(static_cast<unsigned>(N));
    if (rot_is_matrix)
      DRTK_LAUNCH((fk_forward_kernel<T, true>), grid, dim3(kFkLanes), 0, s, in, static_cast<T*>(transforms),
                  static_cast<T*>(posed_joints));
    else
      DRTK_LAUNCH((fk_forward_kernel<T, false>), grid, dim3(kFkLanes), 0, s, in, static_cast<T*>(transforms),
                  static_cast<T*>(posed_joints));
    DRTK_RETURN_IF_LAUNCH_FAILED();
    return DRTK_OK;
  });
}

extern "C" int drtk_amd_kinematics_backward_workspace_bytes(drtk_dtype_t dtype, int64_t N, int64_t J, int64_t grad_joints_B,
                                                            size_t* bytes) {
  if (!valid_dtype(dtype) || !bytes || N < 0 || J < 0 || J > kFkMaxJoints || (grad_joints_B != 0 && grad_joints_B != 1 && grad_joints_B != N))
    return DRTK_ERR_INVALID_ARGUMENT;
  // one row [J,3] per view, in the tensor dtype, where a shared rest pose of more than one view gets a gradient
  const bool second = grad_joints_B == 1 && N > 1;
  *bytes = second ? size_t(N) * size_t(J) * 3 * (dtype == DRTK_F32 ? 4 : 8) : 0;
  return DRTK_OK;
}

namespace drtk_amd {
namespace {
// the unrequested halves compiled out; the launch site spells the flags as values, which is what the timing report shows
template <typename T>
int fk_backward_launch(bool mat, const FkIn& in, int64_t N, const void* gA, const void* gP, void* g_rot, void* g_joint_rows,
                       void* g_tr, hipStream_t s) {
  const dim3 grid(static_cast<unsigned>(N));
#define DRTK_FK_BACKWARD(M, NR, NC, NT)                                                                                \
  DRTK_LAUNCH((fk_backward_kernel<T, M, NR, NC, NT>), grid, dim3(kFkLanes), 0, s, in, static_cast<const T*>(gA),        \
              static_cast<const T*>(gP), static_cast<T*>(g_rot), static_cast<T*>(g_joint_rows), static_cast<T*>(g_tr))
  const int which = (mat ? 8 : 0) | (g_rot ? 4 : 0) | (g_joint_rows ? 2 : 0) | (g_tr ? 1 : 0);
  switch (which) {
    case 1: DRTK_FK_BACKWARD(false, false, false, true); break;
    case 2: DRTK_FK_BACKWARD(false, false, true, false); break;
    case 3: DRTK_FK_BACKWARD(false, false, true, true); break;
    case 4: DRTK_FK_BACKWARD(false, true, false, false); break;
    case 5: DRTK_FK_BACKWARD(false, true, false, true); break;
    case 6: DRTK_FK_BACKWARD(false, true, true, false); break;
    case 7: DRTK_FK_BACKWARD(false, true, true, true); break;
    case 9: DRTK_FK_BACKWARD(true, false, false, true); break;
    case 10: DRTK_FK_BACKWARD(true, false, true, false); break;
    case 11: DRTK_FK_BACKWARD(true, false, true, true); break;
    case 12: DRTK_FK_BACKWARD(true, true, false, false); break;
    case 13: DRTK_FK_BACKWARD(true, true, false, true); break;
    case 14: DRTK_FK_BACKWARD(true, true, true, false); break;
    case 15: DRTK_FK_BACKWARD(true, true, true, true); break;
    default: return DRTK_ERR_INVALID_ARGUMENT; // (no output: refused by the entry point)
  }
#undef DRTK_FK_BACKWARD
  DRTK_RETURN_IF_LAUNCH_FAILED();
  return DRTK_OK;
}
} // namespace
} // namespace drtk_amd

extern "C" int drtk_amd_kinematics_backward(
    drtk_dtype_t dtype, const void* grad_transforms, const void* grad_posed, const void* rotations, int rot_is_matrix,
    const int64_t* rot_strides, const void* joints, int64_t c_sN, const void* translation, const int32_t* parents,
    const int32_t* order, const int32_t* level_start, int64_t num_levels, const int32_t* child_crow,
    const int32_t* child_entries, int64_t N, int64_t J, void* grad_rotations, int64_t grad_joints_B, void* grad_joints,
    void* grad_translation, void* workspace, size_t workspace_bytes, drtk_stream_t stream) {
  if (!valid_dtype(dtype) || !rot_strides) return DRTK_ERR_INVALID_ARGUMENT;
  if (fk_bad_args(N, J, num_levels, rot_is_matrix, c_sN)) return DRTK_ERR_INVALID_ARGUMENT;
  if (!grad_rotations && !grad_joints && !grad_translation) return DRTK_ERR_INVALID_ARGUMENT;
  if (grad_joints && grad_joints_B != 1 && grad_joints_B != N) return DRTK_ERR_INVALID_ARGUMENT;
  size_t need = 0;
  if (drtk_amd_kinematics_backward_workspace_bytes(dtype, N, J, grad_joints ? grad_joints_B : 0, &need) != DRTK_OK)
    return DRTK_ERR_INVALID_ARGUMENT;
  if (need > 0 && (!workspace || workspace_bytes < need || (reinterpret_cast<uintptr_t>(workspace) & 7) != 0))
    return !workspace || workspace_bytes < need ? DRTK_ERR_WORKSPACE_TOO_SMALL : DRTK_ERR_INVALID_ARGUMENT;
  const bool main_pass = N * J > 0;
  // N = 0 with a summed grad_joints: the empty sum, zeros; J = 0 with a grad_translation: no roots, zeros
  const bool zero_joints = grad_joints && grad_joints_B == 1 && N == 0 && J > 0;
  const bool zero_tr = grad_translation && J == 0 && N > 0;
  if (!main_pass && !zero_joints && !zero_tr) return DRTK_OK;
  if (main_pass && (!rotations || !joints || !parents || !order || !level_start || !child_crow || (J > 1 && !child_entries)))
    return DRTK_ERR_INVALID_ARGUMENT;
  return dispatch_dtype(dtype, [&](auto tag) -> int {
    using T = decltype(tag);
    const hipStream_t s = static_cast<hipStream_t>(stream);
    if (zero_joints && fill_bytes_async(grad_joints, 0, size_t(J) * 3 * sizeof(T), s) != DRTK_OK) return DRTK_ERR_LAUNCH;
    if (zero_tr && fill_bytes_async(grad_translation, 0, size_t(N) * 3 * sizeof(T), s) != DRTK_OK) return DRTK_ERR_LAUNCH;
    if (!main_pass) return DRTK_OK;
    const FkIn in = fk_in(rotations, rot_strides, joints, c_sN, translation, parents, order, level_start, num_levels,
                          child_crow, child_entries, J);
    void* rows = need > 0 ? workspace : grad_joints;
    const int rc = fk_backward_launch<T>(rot_is_matrix != 0, in, N, grad_transforms, grad_posed, grad_rotations, rows, grad_translation, s);
    if (rc != DRTK_OK) return rc;
    if (need > 0) {
      DRTK_LAUNCH((fk_joint_sum_kernel<T>), dim3(static_cast<unsigned>(ceil_div(J * 3, kBlock))), dim3(kBlock), 0, s,
                  static_cast<const T*>(workspace), N, J * 3, static_cast<T*>(grad_joints));
      DRTK_RETURN_IF_LAUNCH_FAILED();
    }
    return DRTK_OK;
  });
}
