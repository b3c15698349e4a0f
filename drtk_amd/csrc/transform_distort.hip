// transform with the distortion camera models -- radial-tangential, fisheye, fisheye62 (+ lookup table) -- in one kernel
// each way, on the template of transform.hip.
//
// Reference: drtk/utils/projection.py:56-310 (the three models) and :618-644 (the fisheye62 cull), pure PyTorch: ~60
// launches forward and >100 backward, boolean-mask indexing for a per-view mode list.  Here the mode is a per-view integer
// (wave-uniform: the view is blockIdx.y), one thread per (view, vertex) computes v_cam, the pinhole division, the model
// and, fisheye62 only, the bilinear lookup-table offset.  The backward recomputes the forward, forms the 2x2 Jacobian of
// the model (and of the table) in registers and applies its transpose; with shared [1,V,3] vertices one thread per vertex
// walks the N views and writes the sum -- no atomics, bitwise reproducible.
//
// Quirks of the reference that are reproduced (each is spelled where it happens):
//   * every clamp has zero gradient where it is active (torch.clamp);
//   * radial-tangential: r^2 is clamped to fov^2, the tangential terms use p clamped per component, p * R the unclamped p;
//     the coefficient count decides which powers are EVALUATED (fov = inf and a camera-plane vertex: r2^3 overflows in
//     float32 and 0 * inf would plant a NaN the reference does not produce);
//   * fisheye62: the lookup table's x is normalised by size(2) - 1 and y by size(3) - 1, while grid_sample reads x along
//     size(3); z = -1 beyond fov only when the caller asks for the cull.
// One deviation: for r < 1e-8 (the optical axis) the scale theta_d / r is taken as constant -- a finite gradient where the
// reference's sqrt yields NaN.
#include "common.hpp"

namespace drtk_amd {
namespace {

enum : int { kPinhole = 0, kRadTan = 1, kFisheye = 2, kFisheye62 = 3 };

template <typename T>
struct DistortArgs {
  const T* v;
  const T* campos;
  const T* camrot;
  const T* focal;
  const T* princpt;
  const T* coeff;
  const T* fov;
  const T* lut;
  const T* lut_spacing;
  const int32_t* mode_per_view;
  int64_t v_sN;
  int mode_all, ncoef, cull, Hl, Wl, N, V;
};

// what is constant over a view
template <typename T>
struct View {
  T pos[3], rot[9], focal[4], pp[2], D[8], fov, sp[2];
  const T* lut; // this view's [2,Hl,Wl] table, or null
  int mode;
};

template <typename T>
__host__ __device__ __forceinline__ View<T> load_view(const DistortArgs<T>& a, int64_t n) {
  View<T> c;
#pragma unroll
  for (int i = 0; i < 3; ++i) c.pos[i] = a.campos[n * 3 + i];
#pragma unroll
  for (int i = 0; i < 9; ++i) c.rot[i] = a.camrot[n * 9 + i];
#pragma unroll
  for (int i = 0; i < 4; ++i) c.focal[i] = a.focal[n * 4 + i];
  c.pp[0] = a.princpt[n * 2 + 0];
  c.pp[1] = a.princpt[n * 2 + 1];
#pragma unroll
  for (int i = 0; i < 8; ++i) c.D[i] = i < a.ncoef ? a.coeff[n * a.ncoef + i] : T(0);
  c.fov = a.fov[n];
  const int m = a.mode_per_view ? a.mode_per_view[n] : a.mode_all;
  c.mode = (m >= kPinhole && m <= kFisheye62) ? m : kPinhole;
  c.lut = nullptr;
  c.sp[0] = c.sp[1] = T(1);
  if (a.lut && c.mode == kFisheye62) {
    c.lut = a.lut + n * 2 * a.Hl * a.Wl;
    c.sp[0] = a.lut_spacing[n * 2 + 0];
    c.sp[1] = a.lut_spacing[n * 2 + 1];
  }
  return c;
}

// projection.py:47-48 : z < 0 ? min(z, -1e-8) : max(z, 1e-8)
template <typename T>
__host__ __device__ __forceinline__ T clamp_z(T z, bool& clamped) {
  const T e = T(1e-8);
  const T zc = z < T(0) ? (z < -e ? z : -e) : (z > e ? z : e);
  clamped = zc != z;
  return zc;
}

// torch.clamp(x, -b, b) and whether its gradient passes
template <typename T>
__host__ __device__ __forceinline__ T clamp_sym(T x, T b, T& pass) {
  pass = (x >= -b && x <= b) ? T(1) : T(0);
  return x < -b ? -b : (x > b ? b : x);
}

template <typename T>
__host__ __device__ __forceinline__ T atan_t(T x);
template <>
__host__ __device__ __forceinline__ float atan_t<float>(float x) { return atanf(x); }
template <>
__host__ __device__ __forceinline__ double atan_t<double>(double x) { return atan(x); }
template <typename T>
__host__ __device__ __forceinline__ T sqrt_t(T x);
template <>
__host__ __device__ __forceinline__ float sqrt_t<float>(float x) { return sqrtf(x); }
template <>
__host__ __device__ __forceinline__ double sqrt_t<double>(double x) { return sqrt(x); }
template <typename T>
__host__ __device__ __forceinline__ T floor_t(T x);
template <>
__host__ __device__ __forceinline__ float floor_t<float>(float x) { return floorf(x); }
template <>
__host__ __device__ __forceinline__ double floor_t<double>(double x) { return floor(x); }

// a 2x2 Jacobian d(out x, out y) / d(in x, in y), row-major
template <typename T>
struct J2 {
  T xx, xy, yx, yy;
};

// projection.py:87-131 : (px, py) -> distorted normalised point
template <typename T, bool JAC>
__host__ __device__ __forceinline__ void radtan(const View<T>& c, int ncoef, T px, T py, T& xd, T& yd, J2<T>& J) {
  const T r2u = px * px + py * py;
  const T fov2 = c.fov * c.fov;
  const bool in = !(r2u > fov2); // clamp(max=fov^2): the gradient passes up to and including the bound
  const T r2 = in ? r2u : fov2;
  T mx, my;
  const T xc = clamp_sym(px, c.fov, mx), yc = clamp_sym(py, c.fov, my);
  const T k1 = c.D[0], k2 = c.D[1], p1 = c.D[2], p2 = c.D[3];
  T R = T(1) + k1 * r2 + k2 * (r2 * r2);
  T dR = k1 + T(2) * k2 * r2;
  if (ncoef >= 5) { // the powers a 4-coefficient call never forms must not be formed here either
    const T r4 = r2 * r2, r6 = r4 * r2;
    R = R + c.D[4] * r6;
    dR += T(3) * c.D[4] * r4;
    if (ncoef == 8) {
      const T den = T(1) + c.D[5] * r2 + c.D[6] * r4 + c.D[7] * r6;
      const T dden = c.D[5] + T(2) * c.D[6] * r2 + T(3) * c.D[7] * r4;
      R = R / den;
      dR = (dR - R * dden) / den;
    }
  }
  xd = px * R + T(2) * xc * yc * p1 + r2 * p2 + T(2) * p2 * (xc * xc);
  yd = py * R + T(2) * xc * yc * p2 + r2 * p1 + T(2) * p1 * (yc * yc);
  if (JAC) {
    const T rx = in ? T(2) * px : T(0), ry = in ? T(2) * py : T(0); // d r2 / d p
    const T ax = px * dR + p2, ay = py * dR + p1;                 // d xd / d r2, d yd / d r2
    J.xx = R + ax * rx + mx * (T(2) * yc * p1 + T(4) * p2 * xc);
    J.xy = ax * ry + my * (T(2) * xc * p1);
    J.yx = ay * rx + mx * (T(2) * yc * p2);
    J.yy = R + ay * ry + my * (T(2) * xc * p2 + T(4) * p1 * yc);
  }
}

// projection.py:165-180 (NK = 4) and :224-260 (NK = 6): (px, py) -> (px, py) * theta_d(atan(r)) / r, r clamped to [1e-8, fov]
template <typename T, int NK, bool JAC>
__host__ __device__ __forceinline__ void fisheye_scale(const View<T>& c, T px, T py, T& xs, T& ys, J2<T>& J) {
  const T ru = sqrt_t(px * px + py * py);
  const T lo = T(1e-8);
  const bool in = ru >= lo && ru <= c.fov;
  T r = ru < lo ? lo : ru; // clamp(min, max) = min(max(r, lo), fov)
  r = r > c.fov ? c.fov : r;
  const T th = atan_t(r), t2 = th * th;
  T poly = T(1), dpoly = T(1), tp = T(1); // theta_d = theta * poly, d theta_d / d theta = dpoly
#pragma unroll
  for (int k = 0; k < NK; ++k) {
    tp *= t2;
    poly += c.D[k] * tp;
    dpoly += T(2 * k + 3) * c.D[k] * tp;
  }
  const T s = th * poly / r;
  xs = px * s;
  ys = py * s;
  if (JAC) {
    // beyond fov and below 1e-8 the scale is a constant; inside, d s / d r = (d theta_d / d r - s) / r
    const T g = in ? (dpoly / (T(1) + r * r) - s) / r / ru : T(0);
    J.xx = s + px * px * g;
    J.xy = px * py * g;
    J.yx = J.xy;
    J.yy = s + py * py * g;
  }
}

// projection.py:262-273 : per-component clamp of the scaled point to +-fov, then the tangential terms
template <typename T, bool JAC>
__host__ __device__ __forceinline__ void fisheye62(const View<T>& c, T px, T py, T& xd, T& yd, J2<T>& J) {
  T xs, ys;
  J2<T> A;
  fisheye_scale<T, 6, JAC>(c, px, py, xs, ys, A);
  T mx, my;
  const T xr = clamp_sym(xs, c.fov, mx), yr = clamp_sym(ys, c.fov, my);
  const T p0 = c.D[6], p1 = c.D[7];
  const T rr = xr * xr + yr * yr;
  xd = xr + ((T(2) * xr * xr + rr) * p0 + (T(2) * xr * yr) * p1);
  yd = yr + ((T(2) * xr * yr) * p0 + (T(2) * yr * yr + rr) * p1);
  if (JAC) {
    const T bxx = T(1) + T(6) * xr * p0 + T(2) * yr * p1, bxy = T(2) * yr * p0 + T(2) * xr * p1;
    const T byy = T(1) + T(2) * xr * p0 + T(6) * yr * p1;
    // J = B diag(mx, my) A   (B symmetric off the diagonal: byx = bxy)
    const T axx = mx * A.xx, axy = mx * A.xy, ayx = my * A.yx, ayy = my * A.yy;
    J.xx = bxx * axx + bxy * ayx;
    J.xy = bxx * axy + bxy * ayy;
    J.yx = bxy * axx + byy * ayx;
    J.yy = bxy * axy + byy * ayy;
  }
}

// projection.py:277-307 : the pixel-space offset sampled from the [2,Hl,Wl] table (grid_sample: bilinear, zeros padding,
// align_corners=True), zero where the normalised position leaves [-1, 1].  L = d(u + off_x, v + off_y) / d(u, v).
template <typename T, bool JAC>
__host__ __device__ __forceinline__ void lut_offset(const View<T>& c, int Hl, int Wl, T& u, T& v, J2<T>& L) {
  if (JAC) L.xx = L.yy = T(1), L.xy = L.yx = T(0);
  // x is normalised by size(2) - 1 = Hl - 1 and y by size(3) - 1 = Wl - 1, as the reference does it
  const T nx = u / c.sp[0] / T(Hl - 1) * T(2) - T(1);
  const T ny = v / c.sp[1] / T(Wl - 1) * T(2) - T(1);
  if (!(nx >= T(-1) && nx <= T(1) && ny >= T(-1) && ny <= T(1))) {
    if (nx != nx || ny != ny) u = v = nx + ny; // a NaN position stays a NaN
    return;
  }
  // grid_sample reads x along the last axis (Wl) and y along Hl
  const T ix = (nx + T(1)) / T(2) * T(Wl - 1), iy = (ny + T(1)) / T(2) * T(Hl - 1);
  const T fx = floor_t(ix), fy = floor_t(iy);
  const int x0 = static_cast<int>(fx), y0 = static_cast<int>(fy); // in [0, Wl-1] x [0, Hl-1]: nx, ny are in [-1, 1]
  const T tx = ix - fx, ty = iy - fy;
  const bool x0ok = x0 >= 0 && x0 < Wl, x1ok = x0 + 1 >= 0 && x0 + 1 < Wl;
  const bool y0ok = y0 >= 0 && y0 < Hl, y1ok = y0 + 1 >= 0 && y0 + 1 < Hl;
  T off[2], dix[2], diy[2];
#pragma unroll
  for (int ch = 0; ch < 2; ++ch) {
    const T* p = c.lut + int64_t(ch) * Hl * Wl;
    const T nw = (x0ok && y0ok) ? p[int64_t(y0) * Wl + x0] : T(0);
    const T ne = (x1ok && y0ok) ? p[int64_t(y0) * Wl + x0 + 1] : T(0);
    const T sw = (x0ok && y1ok) ? p[int64_t(y0 + 1) * Wl + x0] : T(0);
    const T se = (x1ok && y1ok) ? p[int64_t(y0 + 1) * Wl + x0 + 1] : T(0);
    off[ch] = nw * ((T(1) - tx) * (T(1) - ty)) + ne * (tx * (T(1) - ty)) + sw * ((T(1) - tx) * ty) + se * (tx * ty);
    dix[ch] = (T(1) - ty) * (ne - nw) + ty * (se - sw);
    diy[ch] = (T(1) - tx) * (sw - nw) + tx * (se - ne);
  }
  if (JAC) {
    const T dxu = T(Wl - 1) / (c.sp[0] * T(Hl - 1)); // d ix / d u
    const T dyv = T(Hl - 1) / (c.sp[1] * T(Wl - 1)); // d iy / d v
    L.xx = T(1) + dix[0] * dxu;
    L.xy = diy[0] * dyv;
    L.yx = dix[1] * dxu;
    L.yy = T(1) + diy[1] * dyv;
  }
  u += off[0];
  v += off[1];
}

// camera space -> (pixel x, pixel y, z); with JAC also what the backward needs
template <typename T>
struct Projected {
  T u, v, z;
  T zc;         // clamped z
  bool clamped; // the z clamp was active
  bool culled;  // z was replaced by -1
  J2<T> J, L;   // model and table Jacobians
};

template <typename T, bool JAC>
__host__ __device__ __forceinline__ Projected<T> project(const View<T>& c, const DistortArgs<T>& a, T cx, T cy, T cz) {
  Projected<T> o;
  o.zc = clamp_z(cz, o.clamped);
  const T px = cx / o.zc, py = cy / o.zc;
  T xd = px, yd = py;
  if (JAC) o.J.xx = o.J.yy = T(1), o.J.xy = o.J.yx = T(0);
  if (c.mode == kRadTan) {
    radtan<T, JAC>(c, a.ncoef, px, py, xd, yd, o.J);
  } else if (c.mode == kFisheye) {
    fisheye_scale<T, 4, JAC>(c, px, py, xd, yd, o.J);
  } else if (c.mode == kFisheye62) {
    fisheye62<T, JAC>(c, px, py, xd, yd, o.J);
  }
  o.u = c.focal[0] * xd + c.focal[1] * yd + c.pp[0];
  o.v = c.focal[2] * xd + c.focal[3] * yd + c.pp[1];
  if (JAC) o.L.xx = o.L.yy = T(1), o.L.xy = o.L.yx = T(0);
  if (c.lut) lut_offset<T, JAC>(c, a.Hl, a.Wl, o.u, o.v, o.L);
  // projection.py:623-642 : fisheye62 with a fov given by the caller -- beyond it z = -1, the rasterizer culls the triangle
  o.culled = a.cull && c.mode == kFisheye62 && sqrt_t(px * px + py * py) > c.fov;
  o.z = o.culled ? T(-1) : cz;
  return o;
}

// one (view, vertex) of the forward
template <typename T>
__host__ __device__ __forceinline__ void forward_point(
    const DistortArgs<T>& a, int n, int i, T* __restrict__ v_pix, T* __restrict__ v_cam_out) {
  const View<T> c = load_view<T>(a, n);
  const T* p = a.v + int64_t(n) * a.v_sN + int64_t(i) * 3;
  const T dx = p[0] - c.pos[0], dy = p[1] - c.pos[1], dz = p[2] - c.pos[2];
  const T cx = c.rot[0] * dx + c.rot[1] * dy + c.rot[2] * dz;
  const T cy = c.rot[3] * dx + c.rot[4] * dy + c.rot[5] * dz;
  const T cz = c.rot[6] * dx + c.rot[7] * dy + c.rot[8] * dz;
  const Projected<T> r = project<T, false>(c, a, cx, cy, cz);
  T* o = v_pix + (int64_t(n) * a.V + i) * 3;
  o[0] = r.u, o[1] = r.v, o[2] = r.z;
  if (v_cam_out) {
    T* q = v_cam_out + (int64_t(n) * a.V + i) * 3;
    q[0] = cx, q[1] = cy, q[2] = cz;
  }
}

template <typename T>
__global__ __launch_bounds__(kBlock) void transform_distort_kernel(
    const DistortArgs<T> a, T* __restrict__ v_pix, T* __restrict__ v_cam_out) {
  const int i = blockIdx.x * kBlock + threadIdx.x;
  if (i < a.V) forward_point<T>(a, blockIdx.y, i, v_pix, v_cam_out);
}

// grad_v[view or 0, i, :] of one vertex; SHARED: v is [1,V,3] and the gradient is summed over the N views here.
template <typename T, bool SHARED>
__host__ __device__ __forceinline__ void backward_point(
    const DistortArgs<T>& a, int view, int i, const T* __restrict__ grad_v_pix, const T* __restrict__ grad_v_cam,
    T* __restrict__ grad_v) {
  const int n_begin = SHARED ? 0 : view, n_end = SHARED ? a.N : view + 1;
  T ax = T(0), ay = T(0), az = T(0);
  for (int n = n_begin; n < n_end; ++n) {
    const View<T> c = load_view<T>(a, n);
    const T* p = a.v + (SHARED ? int64_t(0) : int64_t(n) * a.V * 3) + int64_t(i) * 3;
    const T dx = p[0] - c.pos[0], dy = p[1] - c.pos[1], dz = p[2] - c.pos[2];
    const T cx = c.rot[0] * dx + c.rot[1] * dy + c.rot[2] * dz;
    const T cy = c.rot[3] * dx + c.rot[4] * dy + c.rot[5] * dz;
    const T cz = c.rot[6] * dx + c.rot[7] * dy + c.rot[8] * dz;
    T gcx = T(0), gcy = T(0), gcz = T(0);
    if (grad_v_pix) {
      const Projected<T> r = project<T, true>(c, a, cx, cy, cz);
      const T* g = grad_v_pix + (int64_t(n) * a.V + i) * 3;
      // (u, v) + table offset  ->  transpose of L
      const T gu = r.L.xx * g[0] + r.L.yx * g[1];
      const T gv = r.L.xy * g[0] + r.L.yy * g[1];
      // (u, v) = focal @ d + pp  ->  d d = focal^T g
      const T gdx = c.focal[0] * gu + c.focal[2] * gv;
      const T gdy = c.focal[1] * gu + c.focal[3] * gv;
      // d = model(p)  ->  d p = J^T d d
      const T gpx = r.J.xx * gdx + r.J.yx * gdy;
      const T gpy = r.J.xy * gdx + r.J.yy * gdy;
      gcx = gpx / r.zc;
      gcy = gpy / r.zc;
      const T gzc = -(gpx * cx + gpy * cy) / (r.zc * r.zc);
      gcz = (r.clamped ? T(0) : gzc) + (r.culled ? T(0) : g[2]);
    }
    if (grad_v_cam) {
      const T* h = grad_v_cam + (int64_t(n) * a.V + i) * 3;
      gcx += h[0], gcy += h[1], gcz += h[2];
    }
    // v_cam = R (v - campos)  ->  d v = R^T d v_cam
    ax += c.rot[0] * gcx + c.rot[3] * gcy + c.rot[6] * gcz;
    ay += c.rot[1] * gcx + c.rot[4] * gcy + c.rot[7] * gcz;
    az += c.rot[2] * gcx + c.rot[5] * gcy + c.rot[8] * gcz;
  }
  T* o = grad_v + (SHARED ? int64_t(0) : int64_t(view) * a.V * 3) + int64_t(i) * 3;
  o[0] = ax, o[1] = ay, o[2] = az;
}

template <typename T, bool SHARED>
__global__ __launch_bounds__(kBlock) void transform_distort_backward_kernel(
    const DistortArgs<T> a, const T* __restrict__ grad_v_pix, const T* __restrict__ grad_v_cam, T* __restrict__ grad_v) {
  const int i = blockIdx.x * kBlock + threadIdx.x;
  if (i < a.V) backward_point<T, SHARED>(a, blockIdx.y, i, grad_v_pix, grad_v_cam, grad_v);
}

struct RawArgs {
  const void *v, *campos, *camrot, *focal, *princpt, *coeff, *fov, *lut, *lut_spacing;
  const int32_t* mode_per_view;
  int64_t v_sN, N, V, Hl, Wl;
  int mode_all, ncoef, cull;
};

template <typename T>
DistortArgs<T> typed(const RawArgs& r) {
  DistortArgs<T> a;
  a.v = static_cast<const T*>(r.v);
  a.campos = static_cast<const T*>(r.campos);
  a.camrot = static_cast<const T*>(r.camrot);
  a.focal = static_cast<const T*>(r.focal);
  a.princpt = static_cast<const T*>(r.princpt);
  a.coeff = static_cast<const T*>(r.coeff);
  a.fov = static_cast<const T*>(r.fov);
  a.lut = static_cast<const T*>(r.lut);
  a.lut_spacing = static_cast<const T*>(r.lut_spacing);
  a.mode_per_view = r.mode_per_view;
  a.v_sN = r.v_sN;
  a.mode_all = r.mode_all, a.ncoef = r.ncoef, a.cull = r.cull;
  a.Hl = static_cast<int>(r.Hl), a.Wl = static_cast<int>(r.Wl);
  a.N = static_cast<int>(r.N), a.V = static_cast<int>(r.V);
  return a;
}

// the arguments both directions share; everything is decided on the host, before any launch
bool valid(drtk_dtype_t dtype, const RawArgs& r) {
  if (!valid_dtype(dtype)) return false;
  if (r.N < 0 || r.V < 0 || r.V >= (int64_t(1) << 31) || r.N >= (int64_t(1) << 31)) return false;
  if (bad_view_stride(r.v_sN, r.V * 3)) return false;
  if (r.mode_all < kPinhole || r.mode_all > kFisheye62) return false;
  if (r.ncoef != 4 && r.ncoef != 5 && r.ncoef != 8) return false;
  if (!r.mode_per_view && r.mode_all == kFisheye62 && r.ncoef != 8) return false;
  if (r.lut && (!r.lut_spacing || r.Hl < 1 || r.Wl < 1 || r.Hl >= (int64_t(1) << 31) || r.Wl >= (int64_t(1) << 31))) return false;
  if (r.N * r.V > 0 && (!r.v || !r.campos || !r.camrot || !r.focal || !r.princpt || !r.coeff || !r.fov)) return false;
  return true;
}

RawArgs slice(const RawArgs& r, int64_t n0, int64_t n, size_t es) {
  RawArgs s = r;
  s.v = advance(r.v, n0 * r.v_sN, es);
  s.campos = advance(r.campos, n0 * 3, es);
  s.camrot = advance(r.camrot, n0 * 9, es);
  s.focal = advance(r.focal, n0 * 4, es);
  s.princpt = advance(r.princpt, n0 * 2, es);
  s.coeff = advance(r.coeff, n0 * r.ncoef, es);
  s.fov = advance(r.fov, n0, es);
  s.lut = advance(r.lut, n0 * 2 * r.Hl * r.Wl, es);
  s.lut_spacing = advance(r.lut_spacing, n0 * 2, es);
  s.mode_per_view = advance_typed(r.mode_per_view, n0);
  s.N = n;
  return s;
}

template <typename T>
int forward_impl(const RawArgs& r, void* v_pix, void* v_cam, hipStream_t stream) {
  const size_t es = sizeof(T);
  return for_view_slices(r.N, [&](int64_t n0, int64_t n) { // the view is blockIdx.y: one launch per slice
    const DistortArgs<T> a = typed<T>(slice(r, n0, n, es));
    const dim3 grid(static_cast<unsigned>(ceil_div(r.V, kBlock)), static_cast<unsigned>(n));
    DRTK_LAUNCH((transform_distort_kernel<T>), grid, dim3(kBlock), 0, stream, a,
                static_cast<T*>(advance(v_pix, n0 * r.V * 3, es)), static_cast<T*>(advance(v_cam, n0 * r.V * 3, es)));
    DRTK_RETURN_IF_LAUNCH_FAILED();
    return DRTK_OK;
  });
}

template <typename T>
int backward_impl(const RawArgs& r, const void* grad_v_pix, const void* grad_v_cam, void* grad_v, hipStream_t stream) {
  const size_t es = sizeof(T);
  if (r.v_sN == 0) { // shared vertices: ONE launch sums the views in-kernel, any N
    const dim3 grid(static_cast<unsigned>(ceil_div(r.V, kBlock)), 1);
    DRTK_LAUNCH((transform_distort_backward_kernel<T, true>), grid, dim3(kBlock), 0, stream, typed<T>(r),
                static_cast<const T*>(grad_v_pix), static_cast<const T*>(grad_v_cam), static_cast<T*>(grad_v));
    DRTK_RETURN_IF_LAUNCH_FAILED();
    return DRTK_OK;
  }
  return for_view_slices(r.N, [&](int64_t n0, int64_t n) {
    const DistortArgs<T> a = typed<T>(slice(r, n0, n, es));
    const dim3 grid(static_cast<unsigned>(ceil_div(r.V, kBlock)), static_cast<unsigned>(n));
    DRTK_LAUNCH((transform_distort_backward_kernel<T, false>), grid, dim3(kBlock), 0, stream, a,
                static_cast<const T*>(advance(grad_v_pix, n0 * r.V * 3, es)),
                static_cast<const T*>(advance(grad_v_cam, n0 * r.V * 3, es)),
                static_cast<T*>(advance(grad_v, n0 * r.V * 3, es)));
    DRTK_RETURN_IF_LAUNCH_FAILED();
    return DRTK_OK;
  });
}

} // namespace
} // namespace drtk_amd

using namespace drtk_amd;

extern "C" int drtk_amd_transform_distort(
    drtk_dtype_t dtype, const void* v, int64_t v_sN, const void* campos, const void* camrot, const void* focal,
    const void* princpt, int mode_all, const int32_t* mode_per_view, const void* coeff, int ncoef, const void* fov,
    int cull_outside_fov, const void* lut, const void* lut_spacing, int64_t Hl, int64_t Wl, int64_t N, int64_t V,
    void* v_pix, void* v_cam, drtk_stream_t stream) {
  const RawArgs r{v, campos, camrot, focal, princpt, coeff, fov, lut, lut_spacing, mode_per_view, v_sN, N, V, Hl, Wl,
                  mode_all, ncoef, cull_outside_fov != 0};
  if (!valid(dtype, r)) return DRTK_ERR_INVALID_ARGUMENT;
  if (N * V > 0 && !v_pix) return DRTK_ERR_INVALID_ARGUMENT;
  if (N * V == 0) return DRTK_OK;
  return dispatch_dtype(dtype, [&](auto tag) {
    using T = decltype(tag);
    return forward_impl<T>(r, v_pix, v_cam, static_cast<hipStream_t>(stream));
  });
}

extern "C" int drtk_amd_transform_distort_backward(
    drtk_dtype_t dtype, const void* v, int64_t v_sN, const void* campos, const void* camrot, const void* focal,
    const void* princpt, int mode_all, const int32_t* mode_per_view, const void* coeff, int ncoef, const void* fov,
    int cull_outside_fov, const void* lut, const void* lut_spacing, int64_t Hl, int64_t Wl, const void* grad_v_pix,
    const void* grad_v_cam, int64_t N, int64_t V, void* grad_v, drtk_stream_t stream) {
  const RawArgs r{v, campos, camrot, focal, princpt, coeff, fov, lut, lut_spacing, mode_per_view, v_sN, N, V, Hl, Wl,
                  mode_all, ncoef, cull_outside_fov != 0};
  if (!valid(dtype, r)) return DRTK_ERR_INVALID_ARGUMENT;
  if (N * V > 0 && (!grad_v || (!grad_v_pix && !grad_v_cam))) return DRTK_ERR_INVALID_ARGUMENT;
  if (N * V == 0) return DRTK_OK;
  return dispatch_dtype(dtype, [&](auto tag) {
    using T = decltype(tag);
    return backward_impl<T>(r, grad_v_pix, grad_v_cam, grad_v, static_cast<hipStream_t>(stream));
  });
}
