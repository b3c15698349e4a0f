// edge_grad backward -- gradients of the rasterized image at visibility discontinuities
// (Pidhorskyi et al., arXiv 2405.02508).
//
// Reference: src/edge_grad/edge_grad_kernel.cu:217-449.  There every interior pixel acts as the
// centre of a (centre, right, down) stencil, reads img / grad_output for both pixels of a pair
// only where the triangle index changes (sparse 4-byte loads), and scatters 9 atomicAdds per
// pixel (zeros included) into a zero-filled grad_v_pix_img [N,3,H,W].
//
// CDNA4 mapping: three routes, chosen on the host (the launchers at the end of this file).
//   Hook route (drtk_amd_edge_grad_backward: a v_pix_img hook needs the per-pixel image) -- dots + gather, no atomics, no
//   zero-fill:
//     edge_dots_kernel (dense body) streams img and grad_output with 16-byte loads and writes, for every pixel, the two
//     pair terms  gdx = sum_c (img_R - img_C) * 0.5 (g_R + g_C)  and the same downwards (gdy): 8 B/px of workspace.
//     edge_gather4_kernel / edge_gather_kernel: every pixel OWNS its output, classifies the four pairs it takes part in
//     exactly like the reference and sums the at most four contributions in the single-threaded reference order.  Pairs
//     are classified twice (once by each member), which costs ALU only.
//   Fused route (drtk_amd_edge_grad_backward_fused: no hook, the gradient goes straight to the vertices, grad_v_pix
//   [N,V,3]), double and float calls below a megapixel -- dots + scatter_pairs:
//     edge_dots_kernel (dense body) as above; it also clears grad_v_pix, spread over its grid.
//     edge_scatter_pairs_kernel: the unit of work is the differing PAIR, evaluated once, both ends' contributions times
//     their pixels' barycentrics scattered with atomics through a wave-private vertex table (segscatter.hpp).
//   Fused route, float, at least a megapixel and 32-bit addressable -- one pass:
//     a fill of grad_v_pix, then edge_dots_kernel (one-pass body): the wave classifies its differing pairs FIRST
//     (needed_pair_flags), streams img / grad_output only where a pair's term is used -- the reference selects 0 for a pair
//     of two foreground pixels of which neither lies inside the other's triangle (edge_grad_kernel.cu:338-341, 391-410),
//     and on a rendered surface nearly every differing pair is such a seam -- and scatters its own pairs.  No workspace.
// The measurements behind every constant and rule of this file are in profiles/NOTES.md (sections 3.5, R7.1, R8.1, R10, R11).
#include <cstdlib>

#include "common.hpp"
#include "segscatter.hpp"

namespace drtk_amd {
namespace {

// ---------------------------------------------------------------------------------------------
// Small helpers
// ---------------------------------------------------------------------------------------------
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

// Four adjacent pixels of an image row as ONE 16 / 32-byte access that needs the alignment of its element only: rows
// of an image whose width is not a multiple of four start at any element, and so do contiguous views into a flat buffer.
// The hardware serves dword-aligned wide accesses (a wave's 64 such loads touch one cache line more than aligned ones).
template <typename T>
using Quad = T __attribute__((ext_vector_type(4), aligned(sizeof(T))));

// The batched loads of the one-pass body (edge_dots_onepass) go through raw buffer descriptors: a wave-uniform
// base with the exact byte size of what it covers -- one view's plane, one view's corner or vertex table -- and a 32-bit
// byte offset per lane.  The hardware checks every dword of an access against that size: what lies beyond it is not
// fetched and reads as 0, so a lane that has nothing to load is given the size itself as its offset instead of a branch
// around the load, and a batch of such loads is issued back to back under one wait.  (A load under a lane condition is
// compiled as a branch with its own s_waitcnt vmcnt(0): one round trip per load.)
using BufferRsrc = __amdgpu_buffer_rsrc_t;
__device__ __forceinline__ BufferRsrc buffer_rsrc(const void* base, uint32_t bytes) { // both wave-uniform
  return __builtin_amdgcn_make_buffer_rsrc(const_cast<void*>(base), 0, static_cast<int>(bytes), 0x00020000);
}
// (a loaded vector's element passes through this argument: __builtin_bit_cast applied to the element expression itself
// reads element 0 whichever is named)
__device__ __forceinline__ float as_float(uint32_t bits) {
  return __builtin_bit_cast(float, bits);
}
__device__ __forceinline__ int32_t buffer_load_i32(BufferRsrc r, uint32_t byte_offset) {
  return static_cast<int32_t>(__builtin_amdgcn_raw_buffer_load_b32(r, byte_offset, 0, 0));
}

// exclusive prefix over the lanes of a 0..4 count, and its wave total, from three ballots (lt = the lanes below this one)
__device__ __forceinline__ int prefix4(int cnt, unsigned long long lt, int& total) {
  const unsigned long long b0 = __ballot(cnt & 1), b1 = __ballot(cnt & 2), b2 = __ballot(cnt & 4);
  total = __popcll(b0) + 2 * __popcll(b1) + 4 * __popcll(b2);
  return __popcll(b0 & lt) + 2 * __popcll(b1 & lt) + 4 * __popcll(b2 & lt);
}

// Compaction step of a list build: the set bits of each lane's four flags `f` are appended to the wave's LDS list in
// lane order, entry(j) for bit j; n_all = the list's length, before and after.  Wave-collective.
template <typename E, typename EntryOf>
__device__ __forceinline__ void append_flagged(uint32_t f, unsigned long long lt, int& n_all, E* list, EntryOf entry) {
  int t;
  int pos = n_all + prefix4(__popc(f), lt, t);
  n_all += t;
#pragma unroll
  for (int j = 0; j < 4; ++j) {
    if (f & (1u << j)) list[pos++] = entry(j);
  }
}

// ---------------------------------------------------------------------------------------------
// The reference's pair maths
// ---------------------------------------------------------------------------------------------
// edge_grad_kernel.cu:18-28,72-87
template <typename T>
struct TriInfo {
  T p0x, p0y, p1x, p1y;
  T v01x, v01y, v02x, v02y, v12x, v12y;
  T den;
  T nx, ny, nz; // face normal, filled lazily
  int32_t i0, i1, i2;
};

// the edge vectors and the doubled area from the three corners' positions (t.i0 .. t.i2 are the caller's)
template <typename T>
__device__ __forceinline__ void tri_setup(TriInfo<T>& t, T p0x, T p0y, T p1x, T p1y, T p2x, T p2y) {
  t.p0x = p0x;
  t.p0y = p0y;
  t.p1x = p1x;
  t.p1y = p1y;
  t.v01x = t.p1x - t.p0x;
  t.v01y = t.p1y - t.p0y;
  t.v02x = p2x - t.p0x;
  t.v02y = p2y - t.p0y;
  t.v12x = p2x - t.p1x;
  t.v12y = p2y - t.p1y;
  t.den = t.v01x * t.v02y - t.v01y * t.v02x;
}

template <typename T>
__device__ __forceinline__ void load_tri(
    const T* __restrict__ v_n, const int32_t* __restrict__ vi_n, int32_t idx, TriInfo<T>& t) {
  // invalid triangles use vertex (0,0,0) like the reference (edge_grad_kernel.cu:296-301)
  t.i0 = t.i1 = t.i2 = 0;
  if (idx >= 0) {
    const int32_t* f = vi_n + int64_t(idx) * 3;
    t.i0 = f[0], t.i1 = f[1], t.i2 = f[2];
  }
  const T p0x = v_n[3 * (int64_t)t.i0 + 0], p0y = v_n[3 * (int64_t)t.i0 + 1];
  const T p1x = v_n[3 * (int64_t)t.i1 + 0], p1y = v_n[3 * (int64_t)t.i1 + 1];
  const T p2x = v_n[3 * (int64_t)t.i2 + 0], p2y = v_n[3 * (int64_t)t.i2 + 1];
  tri_setup<T>(t, p0x, p0y, p1x, p1y, p2x, p2y);
}

// edge_grad_kernel.cu:30-70 : rasterizer's top-left rule on NON-canonical edge functions
template <typename T>
__device__ __forceinline__ bool pix_in_tri(const TriInfo<T>& t, int x, int y) {
  if (t.den != T(0)) {
    const T px = static_cast<T>(x), py = static_cast<T>(y);
    const T vp0x = px - t.p0x, vp0y = py - t.p0y;
    const T vp1x = px - t.p1x, vp1y = py - t.p1y;
    T b0 = vp1y * t.v12x - vp1x * t.v12y;
    T b1 = vp0x * t.v02y - vp0y * t.v02x;
    T b2 = vp0y * t.v01x - vp0x * t.v01y;
    const T s = t.den > T(0) ? T(1) : (t.den < T(0) ? T(-1) : T(0));
    b0 *= s;
    b1 *= s;
    b2 *= s;
    const bool inside = (b0 >= T(0)) && (b1 >= T(0)) && (b2 >= T(0));
    const bool on0 = b0 == T(0), on1 = b1 == T(0), on2 = b2 == T(0);
    const bool pos = t.den > T(0);
    const bool tl0 = pos ? (t.v12y < T(0) || (t.v12y == T(0) && t.v12x > T(0)))
                         : (t.v12y > T(0) || (t.v12y == T(0) && t.v12x < T(0)));
    const bool tl1 = pos ? (t.v02y > T(0) || (t.v02y == T(0) && t.v02x < T(0)))
                         : (t.v02y < T(0) || (t.v02y == T(0) && t.v02x > T(0)));
    const bool tl2 = pos ? (t.v01y < T(0) || (t.v01y == T(0) && t.v01x > T(0)))
                         : (t.v01y > T(0) || (t.v01y == T(0) && t.v01x < T(0)));
    return inside && !((on0 && !tl0) || (on1 && !tl1) || (on2 && !tl2));
  }
  return false;
}

// Correctly rounded square roots, as the reference's host path gets from libm.  NOT `__fsqrt_rn`: without
// OCML_BASIC_ROUNDED_OPERATIONS the toolchain defines it as __ocml_native_sqrt_f32 (the bare 1-ulp v_sqrt_f32,
// __clang_hip_math.h), and one ulp in a normal's length is enough to flip the sign that get_dp_dr takes from a
// near-zero `d` -- a difference of 2 * max_dp_dr in the output of that pixel.  The builtin is lowered with the
// compiler's correction steps (HIP's default -fhip-fp32-correctly-rounded-divide-sqrt).
__device__ __forceinline__ float sqrt_t(float x) {
  return __builtin_sqrtf(x);
}
__device__ __forceinline__ double sqrt_t(double x) {
  return __builtin_sqrt(x);
}

// edge_grad_kernel.cu:89-100 ; normalize = v * (1 / sqrt(dot)) as on the reference's host path
template <typename T>
__device__ __forceinline__ void tri_normal(const T* __restrict__ v_n, TriInfo<T>& t) {
  const T* p0 = v_n + 3 * (int64_t)t.i0;
  const T* p1 = v_n + 3 * (int64_t)t.i1;
  const T* p2 = v_n + 3 * (int64_t)t.i2;
  const T ax = p0[0] - p2[0], ay = p0[1] - p2[1], az = p0[2] - p2[2];
  const T bx = p1[0] - p0[0], by = p1[1] - p0[1], bz = p1[2] - p0[2];
  const T cx = ay * bz - az * by;
  const T cy = az * bx - ax * bz;
  const T cz = ax * by - ay * bx;
  const T inv = T(1.0) / sqrt_t(cx * cx + cy * cy + cz * cz);
  t.nx = cx * inv;
  t.ny = cy * inv;
  t.nz = cz * inv;
}

// edge_grad_kernel.cu:102-203
template <typename T>
__device__ __forceinline__ void get_dp_dr(T nvx, T nvy, T nfx, T nfy, T M, T& ox, T& oy) {
  const T inv_v = T(1.0) / sqrt_t(nvx * nvx + nvy * nvy);
  const T nv_x = nvx * inv_v, nv_y = nvy * inv_v;
  const T inv_f = T(1.0) / sqrt_t(nfx * nfx + nfy * nfy);
  const T nf_x = nfx * inv_f, nf_y = nfy * inv_f;
  const T bx = -nf_y, by = nf_x;
  const T d = bx * nv_x + by * nv_y;
  T q;
  if (M > T(0)) {
    const T abs_d = d < T(0) ? -d : d;
    const T abs_bx = bx < T(0) ? -bx : bx;
    const T lim = abs_bx / M;
    const T m = abs_d < lim ? lim : abs_d;
    const T safe_d = (d >= T(0) ? T(1) : T(-1)) * epsclamp(m);
    q = bx / safe_d;
  } else {
    q = bx / epsclamp(d);
  }
  ox = q * nv_x;
  oy = q * nv_y;
}

// Contributions of one pixel pair A (centre role) - B (right/down role).
//   AXIS 0: B = A + (1,0), normals use (x,z);  AXIS 1: B = A + (0,1), normals use (y,z).
// gA/gB: in-plane component (x or y), zA/zB: z component.  edge_grad_kernel.cu:303-425.
template <typename T, int AXIS>
__device__ __forceinline__ void eval_pair(
    const T* __restrict__ v_n, TriInfo<T>& tA, TriInfo<T>& tB, int32_t idxA, int32_t idxB, int xa,
    int ya, T grad_dot, T M, T& gA, T& zA, T& gB, T& zB) {
  gA = zA = gB = zB = T(0);
  const bool a_valid = idxA >= 0, b_valid = idxB >= 0;
  const bool both = a_valid && b_valid;
  const int xb = xa + (AXIS == 0 ? 1 : 0), yb = ya + (AXIS == 1 ? 1 : 0);
  const bool a_in_b = both && pix_in_tri(tB, xa, ya);
  const bool b_in_a = both && pix_in_tri(tA, xb, yb);
  const bool a_over_b = a_in_b && !b_in_a;
  const bool b_over_a = b_in_a && !a_in_b;
  const bool inter = a_in_b && b_in_a;
  const bool adjacent = both && !a_in_b && !b_in_a;
  if (!inter) {
    gA = (!a_valid || b_over_a || adjacent) ? T(0) : grad_dot;
    gB = (!b_valid || a_over_b || adjacent) ? T(0) : grad_dot;
  } else {
    tri_normal(v_n, tA);
    tri_normal(v_n, tB);
    const T a_in = AXIS == 0 ? tA.nx : tA.ny;
    const T b_in = AXIS == 0 ? tB.nx : tB.ny;
    T dx, dz;
    get_dp_dr<T>(a_in, tA.nz, b_in, tB.nz, M, dx, dz);
    gA = grad_dot * dx;
    zA = grad_dot * dz;
    get_dp_dr<T>(b_in, tB.nz, a_in, tA.nz, M, dx, dz);
    gB = grad_dot * dx;
    zB = grad_dot * dz;
  }
}

// ---------------------------------------------------------------------------------------------
// The pair phase of the fused route (edge_scatter_pairs_kernel and the one-pass body of edge_dots_kernel)
// ---------------------------------------------------------------------------------------------
// slots of a wave's vertex table (segscatter.hpp).  128 against 64 slots: no difference (profiles/NOTES.md R11).
constexpr int kEdgeSlots = 64;

// One round of the pair phase: every lane with `act` holds one pair A = (px, y), B = A + (1,0) [AXIS 0] or A + (0,1)
// [AXIS 1] whose indices differ, and the pair's dot term; the wave evaluates its pairs, sums runs of lanes that hit the
// same two triangles and adds the runs' sums to the vertices through its table.  Wave-collective: called by all lanes of
// the wave, the idle ones with act = false.
// (A pair's six barycentrics requested together with its two ids instead of after the evaluation: measured and not kept,
// profiles/NOTES.md R10, lever b.)
template <typename T, int AXIS, int SLOTS>
__device__ __forceinline__ void scatter_pair_round(
    bool act, int px, int y, T term, const int32_t* __restrict__ idx_n, const T* __restrict__ v_n,
    const int32_t* __restrict__ vi_n, const T* __restrict__ bary_n, int64_t HW, int W, T M, int32_t* keys,
    TableAcc* vals, T* __restrict__ grad_n) {
  int32_t ia = -1, ib = -1;
  T ga = T(0), za = T(0), gb = T(0), zb = T(0); // -(in-plane), -(z) contributions to pixel A / pixel B
  T Ba[3] = {T(0), T(0), T(0)}, Bb[3] = {T(0), T(0), T(0)};
  int32_t va[3] = {0, 0, 0}, vb[3] = {0, 0, 0};
  if (act) {
    const int64_t pa = int64_t(y) * W + px;
    const int64_t pb = AXIS == 0 ? pa + 1 : pa + W;
    ia = idx_n[pa];
    ib = idx_n[pb];
    TriInfo<T> ta, tb;
    load_tri<T>(v_n, vi_n, ia, ta);
    load_tri<T>(v_n, vi_n, ib, tb);
    T gA, zA, gB, zB;
    eval_pair<T, AXIS>(v_n, ta, tb, ia, ib, px, y, term, M, gA, zA, gB, zB);
    ga = -gA, za = -zA, gb = -gB, zb = -zB; // edge_grad_kernel.cu:427-445 negates
    va[0] = ta.i0, va[1] = ta.i1, va[2] = ta.i2;
    vb[0] = tb.i0, vb[1] = tb.i1, vb[2] = tb.i2;
    if (ia >= 0) Ba[0] = bary_n[pa], Ba[1] = bary_n[HW + pa], Ba[2] = bary_n[2 * HW + pa];
    if (ib >= 0) Bb[0] = bary_n[pb], Bb[1] = bary_n[HW + pb], Bb[2] = bary_n[2 * HW + pb];
  }
  // a side takes part if its pixel is foreground and it received something
  const bool a_on = ia >= 0 && (ga != T(0) || za != T(0));
  const bool b_on = ib >= 0 && (gb != T(0) || zb != T(0));
  // twelve terms per pair: corner slots A0..A2, B0..B2, two components each -- the pair's axis (x or y) and z
  T g[12];
#pragma unroll
  for (int k = 0; k < 3; ++k) {
    g[2 * k + 0] = a_on ? ga * Ba[k] : T(0);
    g[2 * k + 1] = a_on ? za * Ba[k] : T(0);
    g[6 + 2 * k + 0] = b_on ? gb * Bb[k] : T(0);
    g[6 + 2 * k + 1] = b_on ? zb * Bb[k] : T(0);
  }
  // a run = consecutive lanes with the same two triangles and the same participation; its sums end up in its
  // last lane (segscatter.hpp: run_sums_rows16), which alone touches the vertex table
  const int32_t key_a = a_on ? ia : -1, key_b = b_on ? ib : -1;
  int dist;
  bool tail;
  const int32_t left_a = __shfl_up(key_a, 1), left_b = __shfl_up(key_b, 1); // both BEFORE the ||: a shuffle under a
  run_rows16_heads(key_a != left_a || key_b != left_b, dist, tail);           // short-circuit runs with lanes switched off
  if (__ballot(a_on || b_on) != 0) {
    run_sums_rows16<T, 12>(g, dist);
    // components {axis, z}: x,z = 0 + c*2 ; y,z = 1 + c*1
    constexpr int c_off = AXIS == 0 ? 0 : 1, c_step = AXIS == 0 ? 2 : 1;
    if (tail && a_on) table_add<T, 3, 2, SLOTS>(keys, vals, 4, va, g, grad_n, 3, c_off, c_step);
    if (tail && b_on) table_add<T, 3, 2, SLOTS>(keys, vals, 4, vb, g + 6, grad_n, 3, c_off, c_step);
  }
}

// What the rounds of one wave work on: one view's tensors and the wave's own vertex table (LDS).
template <typename T>
struct PairView {
  const int32_t* idx_n;
  const T* v_n;
  const int32_t* vi_n;
  const T* bary_n;
  T* grad_n;
  int64_t HW;
  int W;
  T M;
  int32_t* keys;
  TableAcc* vals;
};

// scatter_pair_round with the axis (wave-uniform) known at run time only: the round itself wants it as a constant
template <typename T>
__device__ __forceinline__ void scatter_pair_axis(int axis, bool act, int px, int y, T term, const PairView<T>& v) {
  if (axis == 0) {
    scatter_pair_round<T, 0, kEdgeSlots>(act, px, y, term, v.idx_n, v.v_n, v.vi_n, v.bary_n, v.HW, v.W, v.M, v.keys, v.vals, v.grad_n);
  } else {
    scatter_pair_round<T, 1, kEdgeSlots>(act, px, y, term, v.idx_n, v.v_n, v.vi_n, v.bary_n, v.HW, v.W, v.M, v.keys, v.vals, v.grad_n);
  }
}

// Rounds of 64 pairs that needed_pair_flags keeps in flight.  Three: slower; four spill at the kernel's 80 registers
// (profiles/NOTES.md R10, levers; profiles/r10/edge_chain_ab.txt).
constexpr int kClassifyRounds = 2;

// Classification phase of the one-pass body: of the wave's differing pairs (`flags`, the body's layout),
// those whose term reaches the output.  eval_pair discards the term of an `adjacent` pair -- both pixels foreground,
// neither inside the other's triangle -- with a select, and scatter_pair_round then drops the pair (a_on / b_on); every
// other pair is needed.  The verdict is eval_pair's own: the same load_tri, the same pix_in_tri on the same arguments
// (no contraction, no fast-math: the same bits), and nothing else of it -- no normals, square roots, barycentrics.
// The pairs' positions are compacted into `list` (uint32 per pair: owner lane << 5 | flag bit; row-major per axis, so
// that a round's index gathers run along image rows) and taken one per lane; a pair with a background pixel is needed
// without a look at its triangle.  A needed pair sets its bit in its owner's word of `mask` (one word per lane).
// Wave-collective; `list` and `mask` are wave-private LDS, free for other use on return.
// P rounds of 64 pairs are in flight at a time, and each of a pair's three dependent gathers is issued for all of them
// before the first is waited for -- the two ids of P pairs, then their two faces, then their six vertices, then the tests:
// three round trips per 64 P pairs.  The gathers go through descriptors of exactly this view's index plane, corner
// table and vertex table (idx_bytes, vi_bytes, v_bytes: their sizes, which as an offset mean "nothing to load").
template <typename T, int R, int P>
__device__ __forceinline__ uint32_t needed_pair_flags(
    uint32_t flags, int lane, int strip_x0, int y0, BufferRsrc idx_rsrc, uint32_t idx_bytes, BufferRsrc v_rsrc,
    uint32_t v_bytes, BufferRsrc vi_rsrc, uint32_t vi_bytes, int W, uint32_t* list, uint32_t* mask) {
  const unsigned long long lt = (1ull << lane) - 1ull;
  mask[lane] = 0;
  int n_all = 0;
#pragma unroll
  for (int g = 0; g < 2 * R; ++g) {
    append_flagged((flags >> (4 * g)) & 15u, lt, n_all, list, [&](int j) { return static_cast<uint32_t>((lane << 5) | (4 * g + j)); });
  }
  wave_lds_sync();
  for (int t0 = 0; t0 < n_all; t0 += kWave * P) {
    bool valid[P], both[P];
    uint32_t entry[P];
    int xa[P], ya[P], xb[P], yb[P];
    int32_t id[P][2], corner[P][2][3];
    T pos[P][2][3][2];
#pragma unroll
    for (int p = 0; p < P; ++p) {
      const int t = t0 + p * kWave + lane;
      valid[p] = t < n_all;
      entry[p] = list[valid[p] ? t : 0]; // (entry 0 exists: n_all > 0)
    }
    // 1. the two ids.  A listed pair lies in the stencil domain, so both of its pixels are pixels of this view; a lane
    //    without a pair loads nothing.
#pragma unroll
    for (int p = 0; p < P; ++p) {
      const int bit = static_cast<int>(entry[p] & 31u), owner = static_cast<int>(entry[p] >> 5);
      const bool vertical = bit >= 4 * R;
      const int k = vertical ? bit - 4 * R : bit;
      xa[p] = strip_x0 + owner * 4 + (k & 3), ya[p] = y0 + (k >> 2);
      xb[p] = vertical ? xa[p] : xa[p] + 1, yb[p] = vertical ? ya[p] + 1 : ya[p];
      id[p][0] = buffer_load_i32(idx_rsrc, valid[p] ? static_cast<uint32_t>(ya[p] * W + xa[p]) * 4u : idx_bytes);
      id[p][1] = buffer_load_i32(idx_rsrc, valid[p] ? static_cast<uint32_t>(yb[p] * W + xb[p]) * 4u : idx_bytes);
    }
    // 2. the two faces of a pair of two foreground pixels (`both` of eval_pair); an id that is no triangle of this view
    //    lies beyond the corner table and reads the corners 0, 0, 0
#pragma unroll
    for (int p = 0; p < P; ++p) {
      both[p] = valid[p] && id[p][0] >= 0 && id[p][1] >= 0;
#pragma unroll
      for (int s = 0; s < 2; ++s) {
        const auto f = __builtin_amdgcn_raw_buffer_load_b96(vi_rsrc, both[p] ? static_cast<uint32_t>(id[p][s]) * 12u : vi_bytes, 0, 0);
#pragma unroll
        for (int k = 0; k < 3; ++k) corner[p][s][k] = static_cast<int32_t>(f[k]);
      }
    }
    // 3. x and y of the six vertices; a corner that is no vertex of this view lies beyond the vertex table and reads 0, 0
#pragma unroll
    for (int p = 0; p < P; ++p) {
#pragma unroll
      for (int s = 0; s < 2; ++s) {
#pragma unroll
        for (int k = 0; k < 3; ++k) {
          const auto xy = __builtin_amdgcn_raw_buffer_load_b64(v_rsrc, both[p] ? static_cast<uint32_t>(corner[p][s][k]) * 12u : v_bytes, 0, 0);
          pos[p][s][k][0] = as_float(xy[0]), pos[p][s][k][1] = as_float(xy[1]);
        }
      }
    }
    // 4. the tests of eval_pair
#pragma unroll
    for (int p = 0; p < P; ++p) {
      TriInfo<T> ta, tb;
      tri_setup<T>(ta, pos[p][0][0][0], pos[p][0][0][1], pos[p][0][1][0], pos[p][0][1][1], pos[p][0][2][0], pos[p][0][2][1]);
      tri_setup<T>(tb, pos[p][1][0][0], pos[p][1][0][1], pos[p][1][1][0], pos[p][1][1][1], pos[p][1][2][0], pos[p][1][2][1]);
      const bool a_in_b = pix_in_tri(tb, xa[p], ya[p]);
      const bool b_in_a = pix_in_tri(ta, xb[p], yb[p]);
      const bool need = valid[p] && (!both[p] || a_in_b || b_in_a); // not `adjacent`
      if (need) atomicOr(&mask[entry[p] >> 5], 1u << (entry[p] & 31u));
    }
  }
  wave_lds_sync();
  return mask[lane];
}

// ---------------------------------------------------------------------------------------------
// edge_dots_kernel: the channel dots of every pixel pair, stored (dense body) or scattered at once (one-pass body)
// ---------------------------------------------------------------------------------------------
// One wave = strip of 63*4 pixels (+ 4 halo pixels in lane 63) x R rows; the WAVES waves of a workgroup are stacked
// vertically on the same pixel columns (WAVES*R rows per workgroup), so the extra "row below" every wave needs is the
// first row of its sibling wave and is served by this CU's L1 -- HBM sees each row (WAVES*R+1)/(WAVES*R) times.
// Strips are 63 lanes wide: lane 63 holds the first pixels of the next strip and only feeds lane 62's pair term.
// Rows per wave x waves per workgroup, settled in round 2 (2 x 4 against 2 x 8, 1 x 4, 1 x 8, 3 x 4, 4 x 2, 4 x 4:
// profiles/NOTES.md R11, "rows and waves").
constexpr int kStripRows = 2;
constexpr int kDotsWaves = 4;
// Entries of the one-pass body's pair list (tests/test_gpu_edge_chain.py overflows exactly this), and the waves per SIMD
// that body is compiled for: 80 registers; without the bound 85, five waves (profiles/NOTES.md R7.1).
constexpr int kOnepassCap = 512;
constexpr int kOnepassWaves = 6;

// where a wave's strip lies: view, strip column, lane, first row, the lane's first pixel
struct StripPos {
  int n, sx, lane, y0, x;
};
template <int R, int WAVES>
__device__ __forceinline__ StripPos strip_pos(int strips_x, int strip) {
  const int tile = tile_index(strip);
  const int by = tile / strips_x, sx = tile - by * strips_x;
  const int lane = threadIdx.x & (kWave - 1);
  return {static_cast<int>(blockIdx.y), sx, lane, (by * WAVES + static_cast<int>(threadIdx.x / kWave)) * R, (sx * (kWave - 1) + lane) * 4};
}

// four adjacent pixels of one row of one plane, and the next lane's first
template <typename T>
struct Row {
  T v[4];
  T next; // pixel x + 4 (first pixel of the next lane)
};

// Both bodies' products: gdx[y][x] pairs (x,y)-(x+1,y), gdy[y][x] pairs (x,y)-(x,y+1); one channel's share, the
// channels accumulated in ascending order (edge_grad_kernel.cu:353-380).  ri / rg: rows y0 .. y0+R of img / grad_output.
template <typename T, int R>
__device__ __forceinline__ void add_pair_products(const Row<T> (&ri)[R + 1], const Row<T> (&rg)[R + 1], T (&ax)[R][4], T (&ay)[R][4]) {
#pragma unroll
  for (int r = 0; r < R; ++r) {
#pragma unroll
    for (int j = 0; j < 4; ++j) {
      const T inext = (j + 1 < 4) ? ri[r].v[(j + 1) % 4] : ri[r].next;
      const T gnext = (j + 1 < 4) ? rg[r].v[(j + 1) % 4] : rg[r].next;
      ax[r][j] += (inext - ri[r].v[j]) * (T(0.5) * (gnext + rg[r].v[j]));
      ay[r][j] += (ri[r + 1].v[j] - ri[r].v[j]) * (T(0.5) * (rg[r + 1].v[j] + rg[r].v[j]));
    }
  }
}

// (dense body) a lane's four pixels of one row, or zeros.  Plain cached loads: as non-temporal loads the fused route ran
// slower (profiles/NOTES.md R6.6, R11).
template <typename T>
__device__ __forceinline__ Row<T> load_row(const T* __restrict__ plane, int64_t row_off, int x, int W, bool x_ok) {
  Row<T> r;
  if (x_ok) {
    if (x + 4 <= W) {
      const Quad<T> q = *reinterpret_cast<const Quad<T>*>(plane + row_off + x);
      r.v[0] = q.x, r.v[1] = q.y, r.v[2] = q.z, r.v[3] = q.w;
    } else { // the lane that holds the end of a row whose width is not a multiple of four
#pragma unroll
      for (int j = 0; j < 4; ++j) r.v[j] = x + j < W ? plane[row_off + x + j] : T(0);
    }
  } else {
#pragma unroll
    for (int j = 0; j < 4; ++j) r.v[j] = T(0);
  }
  r.next = __shfl_down(r.v[0], 1); // lane 63's is never used: it is the halo lane
  return r;
}

// The dense body (any T): every pair term of the strip goes to the workspace planes gdx / gdy.
template <typename T, int R, int WAVES>
__device__ __forceinline__ void edge_dots_dense(
    const T* img, const T* grad_output, const int32_t* index_img, int C, int H, int W, int strips_x, T* gdx, T* gdy, int strip) {
  const int64_t HW = int64_t(H) * W;
  const StripPos p = strip_pos<R, WAVES>(strips_x, strip);
  const int n = p.n, lane = p.lane, y0 = p.y0, x = p.x;
  if (y0 >= H) return;
  const T* img_n = img + int64_t(n) * C * HW;
  const T* go_n = grad_output + int64_t(n) * C * HW;

  // Pair terms are only ever read where the triangle index changes, and a pair of two background
  // pixels never does: a lane whose pixels, their left / right neighbours and the halo row are all
  // background neither loads nor stores anything (its part of the workspace is never read), so the
  // background of the image costs 4 B/px of index instead of 8C B/px of img + grad_output.
  bool any_fg = false;
  const int32_t* idx_n = index_img + int64_t(n) * HW;
#pragma unroll
  for (int r = 0; r <= R; ++r) {
    const int y = y0 + r;
    if (y < H) { // wave-uniform
      bool fg = false;
      int32_t first = -1, last = -1;
      if (x < W) {
        Quad<int32_t> q;
        if (x + 4 <= W) {
          q = *reinterpret_cast<const Quad<int32_t>*>(idx_n + int64_t(y) * W + x);
        } else {
          const int32_t* rp = idx_n + int64_t(y) * W + x;
          q.x = rp[0], q.y = x + 1 < W ? rp[1] : -1, q.z = x + 2 < W ? rp[2] : -1, q.w = -1;
        }
        fg = (q.x & q.y & q.z & q.w) != -1;
        first = q.x, last = q.w;
      }
      int32_t left = __shfl_up(last, 1), right = __shfl_down(first, 1);
      if (lane == 0) left = (x >= 1 && x < W) ? idx_n[int64_t(y) * W + x - 1] : -1;
      if (lane == kWave - 1) right = (x + 4 < W) ? idx_n[int64_t(y) * W + x + 4] : -1;
      any_fg = any_fg || fg || left != -1 || right != -1;
    }
  }
  if (__ballot(any_fg) == 0) return;
  const bool x_ok = x < W && any_fg;

  T ax[R][4], ay[R][4];
#pragma unroll
  for (int r = 0; r < R; ++r)
#pragma unroll
    for (int j = 0; j < 4; ++j) ax[r][j] = ay[r][j] = T(0);

  for (int c = 0; c < C; ++c) {
    const T* ip = img_n + int64_t(c) * HW;
    const T* gp = go_n + int64_t(c) * HW;
    Row<T> ri[R + 1], rg[R + 1];
#pragma unroll
    for (int r = 0; r <= R; ++r) {
      const bool y_ok = (y0 + r) < H; // wave-uniform
      ri[r] = load_row<T>(ip, int64_t(y0 + r) * W, x, W, x_ok && y_ok);
      rg[r] = load_row<T>(gp, int64_t(y0 + r) * W, x, W, x_ok && y_ok);
    }
    add_pair_products<T, R>(ri, rg, ax, ay);
  }
  if (!x_ok || lane == kWave - 1) return;
  T* ox = gdx + int64_t(n) * HW;
  T* oy = gdy + int64_t(n) * HW;
#pragma unroll
  for (int r = 0; r < R; ++r) {
    const int y = y0 + r;
    if (y >= H) break;
    const int64_t o = int64_t(y) * W + x;
    if (x + 4 <= W) {
      *reinterpret_cast<Quad<T>*>(ox + o) = Quad<T>{ax[r][0], ax[r][1], ax[r][2], ax[r][3]};
      *reinterpret_cast<Quad<T>*>(oy + o) = Quad<T>{ay[r][0], ay[r][1], ay[r][2], ay[r][3]};
    } else {
#pragma unroll
      for (int j = 0; j < 4; ++j)
        if (x + j < W) ox[o + j] = ax[r][j], oy[o + j] = ay[r][j];
    }
  }
}

// What the one-pass body needs beside the images (the arguments of edge_scatter_pairs_kernel).
template <typename T>
struct PairArgs {
  const T* v_pix;
  const int32_t* vi;
  const T* bary_img;
  T* grad_v_pix;
  int64_t V, vi_sN, F;
  T M;
};

// The one-pass body (float): the wave does not store its pair terms.  It OWNS the pairs whose terms it
// holds -- (x,y)-(x+1,y) and (x,y)-(x,y+1) for the pixels of lanes 0..62 in rows y0 .. y0+R-1 inside the reference's
// stencil domain (x < W-1, y < H-1); lane 62's last pixel pairs with lane 63's first, row R-1 with the halo row, lane 63
// owns nothing -- and runs the pair phase of edge_scatter_pairs_kernel on them right after its channel loop: the pairs
// whose indices differ (flags taken from the index rows, one register across the channel loop)
// go into a wave-private LDS list of (position, term) entries, are evaluated one per lane with the axis as a compile-time
// constant and scattered through the wave's vertex table into grad_v_pix, which the host has cleared BEFORE the launch
// (other workgroups' atomics would race a fill spread over this grid).  Nothing crosses a wave: no workgroup barrier, no
// workspace.
// Most differing pairs are seams between two neighbouring triangles of one surface (both pixels foreground, neither inside
// the other's triangle: `adjacent` in eval_pair), and for those the reference selects 0 whatever the term is
// (edge_grad_kernel.cu:338-341,391-410) -- on the bench scene 0.18 pairs per pixel differ and 0.12 % of the pixels receive
// anything.  So the wave classifies its differing pairs first (needed_pair_flags: positions only, one pair per lane, the
// pixel-in-triangle tests of eval_pair and nothing else) and keeps the flags of the NEEDED pairs -- a background pixel, an
// overlap or an intersection: silhouettes and self-occlusion contours.  What a lane loads follows those flags: a lane
// without a needed pair (and whose first pixel its left neighbour does not need) loads nothing, a wave without one returns
// before the channel loop (four strips in five on the bench scene), and the pair phase sees the needed pairs only.
// Such a wave is a chain of dependent loads, not a stream, so every phase issues its loads TOGETHER and
// waits once (BufferRsrc above: range-checked loads instead of branches): the R + 1 index rows, then per P rounds of the
// classification all ids, all faces, all vertices, then per channel the 2 (R + 1) image rows; the shuffles that hand a
// lane's first pixel to its left neighbour come after the loads of their phase.  (Written with a load under each lane
// condition: six round trips for the index rows, three per round of 64 pairs, five to six per channel.)
template <int R, int WAVES>
__device__ __forceinline__ void edge_dots_onepass(
    const float* img, const float* grad_output, const int32_t* index_img, int C, int H, int W, int strips_x, int strip,
    const PairArgs<float>& pairs) {
  static_assert(8 * R <= 32, "the flags of a lane's pairs are one register");
  // Wave-private LDS.  The list holds the flagged pairs only: a dense staging of the terms (4 KB per wave) plus a
  // worst-case list would not fit 24 waves into a CU's 160 KB.  kOnepassCap entries of 8 bytes + the table = 6.3 KB per
  // wave; a strip with more needed pairs than that -- an index image may differ at every pixel -- takes the list-free
  // path below.
  constexpr int kSlots = kEdgeSlots;
  constexpr int kCap = kOnepassCap;
  __shared__ uint2 s_list[WAVES][kCap]; // .x = (row << 8) | pixel of the strip, .y = the pair's term
  __shared__ int32_t t_keys[WAVES][kSlots];
  __shared__ TableAcc t_vals[WAVES][kSlots * 4];
  const int64_t HW = int64_t(H) * W;
  const StripPos p = strip_pos<R, WAVES>(strips_x, strip);
  const int n = p.n, lane = p.lane, y0 = p.y0, x = p.x;
  if (y0 >= H) return;
  const int strip_x0 = p.sx * (kWave - 1) * 4;
  const float* img_n = img + int64_t(n) * C * HW;
  const float* go_n = grad_output + int64_t(n) * C * HW;

  // the pairs this lane owns whose indices differ -- bit 4r+j: (x+j,y0+r)-(x+j+1,y0+r), bit 4R+4r+j: (x+j,y0+r)-(x+j,y0+r+1)
  uint32_t flags = 0;
  // What the batched loads of a plane of this view take -- the plane's size in bytes (H W <= 2^30 - 8 on this path,
  // checked by the launcher) and, per row of the strip, the byte offset of this lane's four pixels in the plane; a lane
  // off the canvas and a row below the image get the plane's size: beyond the descriptor, nothing is fetched
  const uint32_t plane_bytes = static_cast<uint32_t>(HW) * 4u;
  uint32_t row_off[R + 1];
#pragma unroll
  for (int r = 0; r <= R; ++r) row_off[r] = (x < W && y0 + r < H) ? static_cast<uint32_t>((y0 + r) * W + x) * 4u : plane_bytes;
  const BufferRsrc idx_rsrc = buffer_rsrc(index_img + int64_t(n) * HW, plane_bytes);
  {
    // The quads of all R + 1 index rows in ONE round trip, the shuffles after them.  Each load stays inside this view's
    // index plane: the descriptor covers exactly its H W elements, and an element of a quad that lies beyond the end of
    // its row (the next row's first pixels, or nothing) is replaced by -1 after the load.  Neither lane 0's left
    // neighbour nor lane 63's right one is loaded: lane 63 owns no pair, and no pair looks to the left.
    int32_t cur[R + 1][4];
#pragma unroll
    for (int r = 0; r <= R; ++r) {
      const auto q = __builtin_amdgcn_raw_buffer_load_b128(idx_rsrc, row_off[r], 0, 0);
#pragma unroll
      for (int j = 0; j < 4; ++j) cur[r][j] = static_cast<int32_t>(q[j]);
    }
#pragma unroll
    for (int r = 0; r <= R; ++r)
#pragma unroll
      for (int j = 0; j < 4; ++j) cur[r][j] = (x + j < W && y0 + r < H) ? cur[r][j] : -1;
    int32_t right[R + 1]; // the next lane's first pixel (the halo row has no horizontal pair)
#pragma unroll
    for (int r = 0; r < R; ++r) right[r] = __shfl_down(cur[r][0], 1);
    right[R] = -1;
#pragma unroll
    for (int r = 0; r <= R; ++r) {
      const int y = y0 + r;
#pragma unroll
      for (int j = 0; j < 4; ++j) {
        const bool in_x = lane != kWave - 1 && x + j < W - 1; // stencil domain of the reference; lane 63 owns nothing
        // vertical pairs of the row before, if this row exists (then y - 1 < H - 1)
        if (r > 0 && y < H && in_x && cur[r > 0 ? r - 1 : 0][j] != cur[r][j]) flags |= 1u << (4 * R + 4 * (r - 1) + j);
        const int32_t nr = j < 3 ? cur[r][(j + 1) & 3] : right[r];
        if (r < R && in_x && y < H - 1 && cur[r][j] != nr) flags |= 1u << (4 * r + j);
      }
    }
  }
  if (__ballot(flags != 0) == 0) return; // (wave-uniform) no pair of this strip differs: nothing to add anywhere
  {
    // the differing pairs whose term is used; the list's storage holds their positions (all of a strip's 63 x 4 x R x 2
    // pairs fit, so this phase has no dense form), the table's keys -- initialised after it -- the lanes' verdicts
    static_assert(2 * kCap >= (kWave - 1) * 8 * R && kSlots >= kWave, "the list's storage must hold a strip's pair positions, the keys' one word per lane");
    const int wave = __builtin_amdgcn_readfirstlane(threadIdx.x / kWave); // (uniform: the wave's LDS addresses stay in scalar registers)
    // this view's vertex and corner tables, V x 3 floats and F x 3 ids (V, F < 2^32 / 12 on this path, checked by the launcher)
    const uint32_t v_bytes = static_cast<uint32_t>(pairs.V) * 12u, vi_bytes = static_cast<uint32_t>(pairs.F) * 12u;
    flags = needed_pair_flags<float, R, kClassifyRounds>(
        flags, lane, strip_x0, y0, idx_rsrc, plane_bytes, buffer_rsrc(pairs.v_pix + int64_t(n) * pairs.V * 3, v_bytes), v_bytes,
        buffer_rsrc(pairs.vi + int64_t(n) * pairs.vi_sN, vi_bytes), vi_bytes, W, reinterpret_cast<uint32_t*>(s_list[wave]), reinterpret_cast<uint32_t*>(t_keys[wave]));
    if (__ballot(flags != 0) == 0) return; // (wave-uniform) seams only: the host has cleared grad_v_pix, nothing to add
  }
  // pixel 3 of a lane pairs with the NEXT lane's first pixel, so that lane loads for it
  uint32_t h3 = 0;
#pragma unroll
  for (int r = 0; r < R; ++r) h3 |= flags & (8u << (4 * r));
  const int left_h3 = __shfl_up(static_cast<int>(h3), 1);
  const bool load_any = flags != 0 || (lane > 0 && left_h3 != 0);

  float ax[R][4], ay[R][4];
#pragma unroll
  for (int r = 0; r < R; ++r)
#pragma unroll
    for (int j = 0; j < 4; ++j) ax[r][j] = ay[r][j] = 0.f;

  // a lane that loads nothing takes the offset beyond the plane for every row
  uint32_t ch_off[R + 1];
#pragma unroll
  for (int r = 0; r <= R; ++r) ch_off[r] = load_any ? row_off[r] : plane_bytes;
  for (int c = 0; c < C; ++c) {
    const float* ip = img_n + int64_t(c) * HW;
    const float* gp = go_n + int64_t(c) * HW;
    Row<float> ri[R + 1], rg[R + 1];
    // The 2 (R + 1) row loads of a channel in ONE round trip, the `next` shuffles after them.  Each load stays inside
    // plane c of this view's img / grad_output: the descriptors cover exactly its H W elements (c < C), and an element
    // beyond the end of its row reads 0 through the select below -- as does, by the range check, everything of a row
    // below the image, of a lane off the canvas and of a lane that needs nothing.
    const BufferRsrc i_rsrc = buffer_rsrc(ip, plane_bytes), g_rsrc = buffer_rsrc(gp, plane_bytes);
#pragma unroll
    for (int r = 0; r <= R; ++r) {
      const auto qi = __builtin_amdgcn_raw_buffer_load_b128(i_rsrc, ch_off[r], 0, 0);
      const auto qg = __builtin_amdgcn_raw_buffer_load_b128(g_rsrc, ch_off[r], 0, 0);
#pragma unroll
      for (int j = 0; j < 4; ++j) ri[r].v[j] = as_float(qi[j]), rg[r].v[j] = as_float(qg[j]);
    }
#pragma unroll
    for (int r = 0; r <= R; ++r) {
#pragma unroll
      for (int j = 1; j < 4; ++j) { // (element 0 lies in its row wherever the lane is on the canvas)
        ri[r].v[j] = x + j < W ? ri[r].v[j] : 0.f;
        rg[r].v[j] = x + j < W ? rg[r].v[j] : 0.f;
      }
    }
#pragma unroll
    for (int r = 0; r < R; ++r) { // lane 63's is never used: it is the halo lane; nor is row R's
      ri[r].next = __shfl_down(ri[r].v[0], 1);
      rg[r].next = __shfl_down(rg[r].v[0], 1);
    }
    add_pair_products<float, R>(ri, rg, ax, ay);
  }

  // ---- the pair phase of edge_scatter_pairs_kernel on this wave's own pairs; every lane stays to the end (ballots, DPP scans)
  const int wave = __builtin_amdgcn_readfirstlane(threadIdx.x / kWave); // (uniform: the wave's LDS addresses stay in scalar registers)
  const PairView<float> view{index_img + int64_t(n) * HW, pairs.v_pix + int64_t(n) * pairs.V * 3, pairs.vi + int64_t(n) * pairs.vi_sN,
                             pairs.bary_img + int64_t(n) * 3 * HW, pairs.grad_v_pix + int64_t(n) * pairs.V * 3, HW, W, pairs.M,
                             t_keys[wave], t_vals[wave]};

  table_init<kSlots>(t_keys[wave]);
  for (int i = lane; i < kSlots * 4; i += kWave) t_vals[wave][i] = 0;

  const unsigned long long lt = (1ull << lane) - 1ull;
  int grand = 0;
#pragma unroll
  for (int g = 0; g < 2 * R; ++g) {
    int t;
    prefix4(__popc((flags >> (4 * g)) & 15u), lt, t);
    grand += t;
  }
  if (grand <= kCap) { // (wave-uniform)
    // list layout: [horizontal pairs, row-major][vertical pairs, row-major]; the terms leave their registers here
    int n_h = 0, n_all = 0;
#pragma unroll
    for (int axis = 0; axis < 2; ++axis) {
#pragma unroll
      for (int r = 0; r < R; ++r) {
        append_flagged((flags >> (4 * R * axis + 4 * r)) & 15u, lt, n_all, s_list[wave], [&](int j) {
          return make_uint2((r << 8) | (lane * 4 + j), __builtin_bit_cast(uint32_t, axis == 0 ? ax[r][j] : ay[r][j]));
        });
      }
      if (axis == 0) n_h = n_all;
    }
    wave_lds_sync();

    // one pair per lane; a chunk of 64 lanes never mixes the two axes
    for (int axis = 0; axis < 2; ++axis) {
      const int l_begin = axis == 0 ? 0 : n_h, l_end = axis == 0 ? n_h : n_all;
      for (int t0 = l_begin; t0 < l_end; t0 += kWave) {
        const int t = t0 + lane;
        const bool act = t < l_end;
        int px = 0, y = 0;
        float term = 0.f;
        if (act) {
          const uint2 entry = s_list[wave][t];
          y = y0 + static_cast<int>(entry.x >> 8);
          px = strip_x0 + static_cast<int>(entry.x & 255u);
          term = __builtin_bit_cast(float, entry.y);
        }
        scatter_pair_axis<float>(axis, act, px, y, term, view);
      }
    }
  } else {
    // More than kCap of the strip's at most 63 x 4 x R x 2 pairs are needed: compaction has little to gain, so each lane
    // keeps its own pairs -- for each of its 4 R pixels and each axis one round in which every lane with that flag set
    // takes its pair (at least half of the lanes on average).  Any density; the list's storage holds the terms
    // meanwhile, all of them (dense: entry k of lane l at [k][l]), so that they do not occupy registers in the rounds.
    static_assert(2 * kCap >= kWave * 8 * R, "the list's storage must hold a strip's terms");
    uint32_t* s_terms = reinterpret_cast<uint32_t*>(s_list[wave]);
#pragma unroll
    for (int q = 0; q < 4 * R; ++q) {
      s_terms[q * kWave + lane] = __builtin_bit_cast(uint32_t, ax[q / 4][q % 4]);
      s_terms[(4 * R + q) * kWave + lane] = __builtin_bit_cast(uint32_t, ay[q / 4][q % 4]);
    }
    wave_lds_sync(); // (also: the table is initialised)
    for (int axis = 0; axis < 2; ++axis) {
#pragma unroll 1
      for (int k = 0; k < 4 * R; ++k) {
        const bool act = (flags >> (4 * R * axis + k)) & 1u;
        if (__ballot(act) == 0) continue;
        const float term = __builtin_bit_cast(float, s_terms[(4 * R * axis + k) * kWave + lane]);
        scatter_pair_axis<float>(axis, act, x + (k & 3), y0 + (k >> 2), term, view);
      }
    }
  }
  wave_lds_sync();
  table_flush<float, TableAcc, kSlots>(t_keys[wave], t_vals[wave], 4, 3, view.grad_n, 3, 0);
}

// SCATTER picks the body.  The clear runs in front of either: the accumulator of the pass that follows the dense body
// (grad_v_pix of the two-kernel fused route) is cleared here, spread over the whole grid -- one launch less per backward
// pass, which is what a small scene's step is made of.  The one-pass launch passes no zero_out, gdx or gdy (its
// accumulator must be clear BEFORE any of its workgroups runs); the dense launches pass no `pairs`.
template <typename T, int R, int WAVES, bool SCATTER = false>
__global__ __launch_bounds__(WAVES * kWave, SCATTER ? kOnepassWaves : 1) void edge_dots_kernel(
    const T* __restrict__ img, const T* __restrict__ grad_output, const int32_t* __restrict__ index_img, int C,
    int H, int W, int strips_x, T* __restrict__ gdx, T* __restrict__ gdy, int strip, T* __restrict__ zero_out,
    int64_t zero_count, PairArgs<T> pairs) {
  if (zero_out) {
    const int64_t step = int64_t(gridDim.x) * gridDim.y * blockDim.x;
    for (int64_t i = (int64_t(blockIdx.y) * gridDim.x + blockIdx.x) * blockDim.x + threadIdx.x; i < zero_count; i += step) zero_out[i] = T(0);
  }
  if constexpr (SCATTER) {
    static_assert(sizeof(T) == 4, "the one-pass body works on four-pixel lanes of float");
    edge_dots_onepass<R, WAVES>(img, grad_output, index_img, C, H, W, strips_x, strip, pairs);
  } else {
    edge_dots_dense<T, R, WAVES>(img, grad_output, index_img, C, H, W, strips_x, gdx, gdy, strip);
  }
}

// ---------------------------------------------------------------------------------------------
// Hook route, second kernel: the gather
// ---------------------------------------------------------------------------------------------
// Output of one pixel that takes part in at least one pair with differing indices ("edge pixel").
// ic/ir/id/il/iu: indices of the pixel and its right/down/left/up neighbours, already forced equal
// to ic where the pair is outside the reference's stencil domain.
template <typename T>
__device__ __forceinline__ void edge_pixel(
    const T* __restrict__ v_n, const int32_t* __restrict__ vi_n, const T* __restrict__ gdx_n,
    const T* __restrict__ gdy_n, int64_t pix, int x, int y, int W, int32_t ic, int32_t ir, int32_t id,
    int32_t il, int32_t iu, T M, T& ox, T& oy, T& oz, int32_t* centre_vids = nullptr) {
  T cx = T(0), cy = T(0), cz = T(0); // own centre contributions (gc)
  T rx = T(0), rz = T(0);            // as right pixel of the left neighbour's stencil (gr)
  T dy = T(0), dz = T(0);            // as down pixel of the upper neighbour's stencil (gd)
  TriInfo<T> tc;
  load_tri<T>(v_n, vi_n, ic, tc);
  if (centre_vids) {
    centre_vids[0] = tc.i0, centre_vids[1] = tc.i1, centre_vids[2] = tc.i2;
  }
  T gA, zA, gB, zB;
  if (ic != ir) {
    TriInfo<T> tn;
    load_tri<T>(v_n, vi_n, ir, tn);
    eval_pair<T, 0>(v_n, tc, tn, ic, ir, x, y, gdx_n[pix], M, gA, zA, gB, zB);
    cx += gA;
    cz += zA;
  }
  if (ic != id) {
    TriInfo<T> tn;
    load_tri<T>(v_n, vi_n, id, tn);
    eval_pair<T, 1>(v_n, tc, tn, ic, id, x, y, gdy_n[pix], M, gA, zA, gB, zB);
    cy += gA;
    cz += zA;
  }
  if (il != ic) {
    TriInfo<T> tn;
    load_tri<T>(v_n, vi_n, il, tn);
    eval_pair<T, 0>(v_n, tn, tc, il, ic, x - 1, y, gdx_n[pix - 1], M, gA, zA, gB, zB);
    rx += gB;
    rz += zB;
  }
  if (iu != ic) {
    TriInfo<T> tn;
    load_tri<T>(v_n, vi_n, iu, tn);
    eval_pair<T, 1>(v_n, tn, tc, iu, ic, x, y - 1, gdy_n[pix - W], M, gA, zA, gB, zB);
    dy += gB;
    dz += zB;
  }
  // edge_grad_kernel.cu:427-445 negates and accumulates; order = the single-threaded reference
  // order (upper neighbour's stencil, left neighbour's stencil, own stencil).
  ox = (T(0) + (-rx)) + (-cx);
  oy = (T(0) + (-dy)) + (-cy);
  oz = ((T(0) + (-dz)) + (-rz)) + (-cz);
}

// Generic fallback (any W): one pixel per lane.
template <typename T>
__global__ __launch_bounds__(kBlock) void edge_gather_kernel(
    const T* __restrict__ v_pix, const int32_t* __restrict__ vi,
    const int32_t* __restrict__ index_img, const T* __restrict__ gdx, const T* __restrict__ gdy,
    int64_t V, int64_t vi_sN, int H, int W, T M, T* __restrict__ out) {
  const int64_t HW = int64_t(H) * W;
  const int n = blockIdx.y;
  const int64_t pix = int64_t(blockIdx.x) * kBlock + threadIdx.x;
  if (pix >= HW) return;
  const int y = static_cast<int>(pix / W);
  const int x = static_cast<int>(pix - int64_t(y) * W);
  const int32_t* idx_n = index_img + int64_t(n) * HW;

  // stencil domain of the reference: centres with x < W-1 && y < H-1 (edge_grad_kernel.cu:270)
  const bool own = (x < W - 1) && (y < H - 1);
  const bool left = (x >= 1) && (y < H - 1); // pair (x-1,y)-(x,y), centre (x-1,y)
  const bool up = (y >= 1) && (x < W - 1);   // pair (x,y-1)-(x,y), centre (x,y-1)
  const int32_t ic = idx_n[pix];
  const int32_t ir = own ? idx_n[pix + 1] : ic;
  const int32_t id = own ? idx_n[pix + W] : ic;
  const int32_t il = left ? idx_n[pix - 1] : ic;
  const int32_t iu = up ? idx_n[pix - W] : ic;
  T ox = T(0), oy = T(0), oz = T(0);
  if (ic != ir || ic != id || ic != il || ic != iu) {
    edge_pixel<T>(
        v_pix + int64_t(n) * V * 3, vi + int64_t(n) * vi_sN, gdx + int64_t(n) * HW, gdy + int64_t(n) * HW, pix,
        x, y, W, ic, ir, id, il, iu, M, ox, oy, oz);
  }
  T* o = out + int64_t(n) * 3 * HW + pix;
  o[0] = ox;
  o[HW] = oy;
  o[2 * HW] = oz;
}

// W % 4 == 0: a wave owns 256 consecutive pixels (4 per lane, 16-byte index loads and output
// stores).  Only ~1 pixel in 5 is an edge pixel, scattered, so running the heavy classification
// per lane-pixel would execute it for every wave at ~20 % lane utilisation; instead the edge
// pixels of the 256 are COMPACTED (ballot + popcount ranks -> LDS list) and classified 64 at a
// time at near-full utilisation; results go through an LDS tile and leave as dense float4 stores.
template <typename T>
__global__ __launch_bounds__(kBlock) void edge_gather4_kernel(
    const T* __restrict__ v_pix, const int32_t* __restrict__ vi,
    const int32_t* __restrict__ index_img, const T* __restrict__ gdx, const T* __restrict__ gdy,
    int64_t V, int64_t vi_sN, int H, int W, T M, T* __restrict__ out, int strip) {
  using V4 = typename Vec4<T>::type;
  constexpr int kWaves = kBlock / kWave;
  constexpr int kPix = kWave * 4;
  __shared__ __attribute__((aligned(16))) T s_out[kWaves][3][kPix];
  __shared__ uint16_t s_list[kWaves][kPix];
  __shared__ int32_t s_nb[kWaves][4][kPix]; // right/down/left/up neighbour index per pixel

  const int64_t HW = int64_t(H) * W;
  const int n = blockIdx.y;
  const int wave = threadIdx.x / kWave, lane = threadIdx.x & (kWave - 1);
  const int64_t wave_pix0 = (int64_t(tile_index(strip)) * kWaves + wave) * kPix;
  if (wave_pix0 >= HW) return;
  const int64_t pix0 = wave_pix0 + lane * 4;
  const bool in_range = pix0 < HW;
  const int32_t* idx_n = index_img + int64_t(n) * HW;
  const int y = in_range ? static_cast<int>(pix0 / W) : 0;
  const int x0 = in_range ? static_cast<int>(pix0 - int64_t(y) * W) : 0;

  int32_t c[4] = {-1, -1, -1, -1}, u[4], d[4];
  if (in_range) {
    const int4 q = *reinterpret_cast<const int4*>(idx_n + pix0);
    c[0] = q.x, c[1] = q.y, c[2] = q.z, c[3] = q.w;
  }
#pragma unroll
  for (int j = 0; j < 4; ++j) u[j] = d[j] = c[j];
  if (in_range && y >= 1) {
    const int4 q = *reinterpret_cast<const int4*>(idx_n + pix0 - W);
    u[0] = q.x, u[1] = q.y, u[2] = q.z, u[3] = q.w;
  }
  if (in_range && y < H - 1) {
    const int4 q = *reinterpret_cast<const int4*>(idx_n + pix0 + W);
    d[0] = q.x, d[1] = q.y, d[2] = q.z, d[3] = q.w;
  }
  // horizontal neighbours across lanes: previous lane's last / next lane's first pixel
  int32_t lprev = __shfl_up(c[3], 1), rnext = __shfl_down(c[0], 1);
  if (in_range && lane == 0 && x0 >= 1) lprev = idx_n[pix0 - 1];
  if (in_range && lane == kWave - 1 && x0 + 4 < W) rnext = idx_n[pix0 + 4];

  bool e[4];
  int32_t nr[4], nd[4], nl[4], nu[4];
#pragma unroll
  for (int j = 0; j < 4; ++j) {
    const int x = x0 + j;
    // stencil domain of the reference: centres with x < W-1 && y < H-1 (edge_grad_kernel.cu:270)
    const bool own = in_range && (x < W - 1) && (y < H - 1);
    const bool left = in_range && (x >= 1) && (y < H - 1);
    const bool up = in_range && (y >= 1) && (x < W - 1);
    nr[j] = own ? (j < 3 ? c[(j + 1) & 3] : rnext) : c[j];
    nd[j] = own ? d[j] : c[j];
    nl[j] = left ? (j > 0 ? c[(j + 3) & 3] : lprev) : c[j];
    nu[j] = up ? u[j] : c[j];
    e[j] = c[j] != nr[j] || c[j] != nd[j] || c[j] != nl[j] || c[j] != nu[j];
  }

  // zero the output tile, publish neighbour indices, compact the edge pixels
  const V4 zero4 = V4{T(0), T(0), T(0), T(0)};
#pragma unroll
  for (int k = 0; k < 3; ++k) *reinterpret_cast<V4*>(&s_out[wave][k][lane * 4]) = zero4;
  *reinterpret_cast<int4*>(&s_nb[wave][0][lane * 4]) = make_int4(nr[0], nr[1], nr[2], nr[3]);
  *reinterpret_cast<int4*>(&s_nb[wave][1][lane * 4]) = make_int4(nd[0], nd[1], nd[2], nd[3]);
  *reinterpret_cast<int4*>(&s_nb[wave][2][lane * 4]) = make_int4(nl[0], nl[1], nl[2], nl[3]);
  *reinterpret_cast<int4*>(&s_nb[wave][3][lane * 4]) = make_int4(nu[0], nu[1], nu[2], nu[3]);
  const unsigned long long lt = (1ull << lane) - 1ull;
  int total = 0;
#pragma unroll
  for (int j = 0; j < 4; ++j) {
    const unsigned long long m = __ballot(e[j]);
    if (e[j]) s_list[wave][total + __popcll(m & lt)] = static_cast<uint16_t>(lane * 4 + j);
    total += __popcll(m);
  }
  wave_lds_sync();

  const T* v_n = v_pix + int64_t(n) * V * 3;
  const int32_t* vi_n = vi + int64_t(n) * vi_sN;
  const T* gdx_n = gdx + int64_t(n) * HW;
  const T* gdy_n = gdy + int64_t(n) * HW;
  for (int t0 = 0; t0 < total; t0 += kWave) {
    const int t = t0 + lane;
    if (t < total) {
      const int local = s_list[wave][t];
      const int64_t pix = wave_pix0 + local;
      const int py = static_cast<int>(pix / W);
      const int px = static_cast<int>(pix - int64_t(py) * W);
      const int32_t ic = idx_n[pix];
      T ox, oy, oz;
      edge_pixel<T>(
          v_n, vi_n, gdx_n, gdy_n, pix, px, py, W, ic, s_nb[wave][0][local], s_nb[wave][1][local],
          s_nb[wave][2][local], s_nb[wave][3][local], M, ox, oy, oz);
      s_out[wave][0][local] = ox;
      s_out[wave][1][local] = oy;
      s_out[wave][2][local] = oz;
    }
  }
  wave_lds_sync();
  if (in_range) {
    T* o = out + int64_t(n) * 3 * HW + pix0;
#pragma unroll
    for (int k = 0; k < 3; ++k) *reinterpret_cast<V4*>(o + int64_t(k) * HW) = *reinterpret_cast<const V4*>(&s_out[wave][k][lane * 4]);
  }
}

// ---------------------------------------------------------------------------------------------
// Fused route, second kernel of the two: the scatter of pairs
// ---------------------------------------------------------------------------------------------
// Image rows per wave of edge_scatter_pairs_kernel (its tile: 256 x kPairRows pixels): 2 against 4, 1 and 8 rows and
// against narrower tiles, profiles/NOTES.md 3.5 (B') and R11, "pair tile".
constexpr int kPairRows = 2;

// Instead of materialising grad_v_pix_img [N,3,H,W] (80 % exact zeros) for a separate C=3 interpolate backward to
// scatter, the contributions are multiplied by the pixel's barycentrics and scattered to the triangle's
// vertices right away (edge_grad_estimator.py:168-176 + interpolate_kernel.cu:271-279 fused).
// A per-pixel formulation (as in edge_gather4_kernel, which must own its output pixel) evaluates every
// differing pixel pair twice -- once from each end -- inside four divergent branches; that arithmetic was
// 60 % of such a kernel, which is instruction-issue bound.
// Here the unit of work is the PAIR: a wave compacts the horizontal pairs (x,y)-(x+1,y) and the vertical
// pairs (x,y)-(x,y+1) of its 256 x kPairRows tile whose indices differ (same stencil domain, edge_grad_kernel.cu:270),
// one pair per lane, evaluates it ONCE with the axis as a compile-time constant, and scatters both ends'
// contributions (pixel A: -gA on the axis, -zA on z; pixel B: -gB, -zB; each times its own pixel's
// barycentrics) through the run reduction of segscatter.hpp with six corner slots (A0..A2, B0..B2) and
// two components each.
// Any width, any element-aligned pointers: the index rows are the only wide global access of this kernel (Quad, above),
// everything else is per pair.
// The kernel is bound by the dependent loads of each 64-pair round (list -> index -> corners -> vertices) at six waves
// per SIMD, and its waves' work varies with the number of pairs in their tile: more, shorter waves keep more rounds in
// flight and even out the tail.  It serves double and the float calls below a megapixel; the others scatter inside
// edge_dots_kernel.
template <typename T>
__global__ __launch_bounds__(kBlock, sizeof(T) == 4 ? 4 : 2) void edge_scatter_pairs_kernel(
    const T* __restrict__ v_pix, const int32_t* __restrict__ vi, const int32_t* __restrict__ index_img,
    const T* __restrict__ bary_img, const T* __restrict__ gdx, const T* __restrict__ gdy, int64_t V, int64_t vi_sN,
    int H, int W, int strips_x, T M, T* __restrict__ grad_v_pix, int strip) {
  constexpr int kWaves = kBlock / kWave;
  constexpr int kRows = kPairRows;
  constexpr int kCap = kWave * 4 * 2 * 2; // pairs of two rows, both axes: the most one list build can hold
  __shared__ uint16_t s_list[kWaves][kCap];
  constexpr int kSlots = kEdgeSlots;
  __shared__ int32_t t_keys[kWaves][kSlots];
  __shared__ TableAcc t_vals[kWaves][kSlots * 4];

  const int64_t HW = int64_t(H) * W;
  const int n = blockIdx.y;
  const int wave = threadIdx.x / kWave, lane = threadIdx.x & (kWave - 1);
  const int wg = tile_index(strip) * kWaves + wave;
  const int ry = wg / strips_x, sx = wg - ry * strips_x;
  const int y_base = ry * kRows;
  if (y_base >= H) return;
  const int x0 = (sx * kWave + lane) * 4;
  const bool in_x = x0 < W;
  const int32_t* idx_n = index_img + int64_t(n) * HW;
  const T* v_n = v_pix + int64_t(n) * V * 3;
  const int32_t* vi_n = vi + int64_t(n) * vi_sN;
  const T* gdx_n = gdx + int64_t(n) * HW;
  const T* gdy_n = gdy + int64_t(n) * HW;
  const T* bary_n = bary_img + int64_t(n) * 3 * HW;
  T* grad_n = grad_v_pix + int64_t(n) * V * 3;

  table_init<kSlots>(t_keys[wave]);
  for (int i = lane; i < kSlots * 4; i += kWave) t_vals[wave][i] = 0;

  // index rows y_base .. y_base+kRows of this lane's 4 pixels, one batch
  int32_t row[kRows + 1][4];
#pragma unroll
  for (int r = 0; r <= kRows; ++r) {
    const int y = y_base + r;
    if (in_x && y < H) {
      const int32_t* rp = idx_n + int64_t(y) * W + x0;
      if (x0 + 4 <= W) {
        const Quad<int32_t> q = *reinterpret_cast<const Quad<int32_t>*>(rp);
        row[r][0] = q.x, row[r][1] = q.y, row[r][2] = q.z, row[r][3] = q.w;
      } else { // the end of a row whose width is not a multiple of four
#pragma unroll
        for (int j = 0; j < 4; ++j) row[r][j] = x0 + j < W ? rp[j] : -1;
      }
    } else {
#pragma unroll
      for (int j = 0; j < 4; ++j) row[r][j] = -1;
    }
  }
  // pair flags of the lane's pixels: bit j of hf[r] / vf[r] = horizontal / vertical pair starting at pixel j of row r
  uint32_t hf[kRows], vf[kRows];
#pragma unroll
  for (int r = 0; r < kRows; ++r) {
    const int y = y_base + r;
    int32_t rnext = __shfl_down(row[r][0], 1);
    if (in_x && y < H && lane == kWave - 1 && x0 + 4 < W) rnext = idx_n[int64_t(y) * W + x0 + 4];
    hf[r] = vf[r] = 0;
#pragma unroll
    for (int j = 0; j < 4; ++j) {
      const bool own = in_x && (x0 + j < W - 1) && (y < H - 1); // stencil domain of the reference
      const int32_t nr = j < 3 ? row[r][(j + 1) & 3] : rnext;
      if (own && row[r][j] != nr) hf[r] |= 1u << j;
      if (own && row[r][j] != row[r + 1][j]) vf[r] |= 1u << j;
    }
  }
  const unsigned long long lt = (1ull << lane) - 1ull;

  // rows are processed in groups whose pair lists fit the LDS list: all rows normally, two and two
  // when the tile is so dense that they would not
  int grand = 0;
#pragma unroll
  for (int r = 0; r < kRows; ++r) {
    int t;
    prefix4(__popc(hf[r]), lt, t);
    grand += t;
    prefix4(__popc(vf[r]), lt, t);
    grand += t;
  }
  const int rows_per_group = grand <= kCap ? kRows : (kRows < 2 ? kRows : 2);
  for (int r0 = 0; r0 < kRows; r0 += rows_per_group) {
    // list layout: [horizontal pairs of the group, row-major][vertical pairs, row-major].  (The build and the rounds
    // below are those of edge_dots_onepass, written out here: through append_flagged / scatter_pair_axis this kernel's
    // machine code changes -- profiles/NOTES.md R11.)
    int n_h = 0, n_all = 0;
    wave_lds_sync(); // the previous group's list and staging are no longer read
#pragma unroll
    for (int axis = 0; axis < 2; ++axis) {
#pragma unroll
      for (int r = 0; r < kRows; ++r) {
        if (r < r0 || r >= r0 + rows_per_group) continue;
        const uint32_t f = axis == 0 ? hf[r] : vf[r];
        int t;
        int pos = n_all + prefix4(__popc(f), lt, t);
        n_all += t;
#pragma unroll
        for (int j = 0; j < 4; ++j) {
          if (f & (1u << j)) s_list[wave][pos++] = static_cast<uint16_t>((r << 8) | (lane * 4 + j));
        }
      }
      if (axis == 0) n_h = n_all;
    }
    wave_lds_sync();

    // one pair per lane; a chunk of 64 lanes never mixes the two axes
    for (int axis = 0; axis < 2; ++axis) {
      const int l_begin = axis == 0 ? 0 : n_h, l_end = axis == 0 ? n_h : n_all;
      for (int t0 = l_begin; t0 < l_end; t0 += kWave) {
        const int t = t0 + lane;
        const bool act = t < l_end;
        int px = 0, y = 0;
        T term = T(0);
        if (act) {
          const int entry = s_list[wave][t];
          y = y_base + (entry >> 8);
          px = sx * (kWave * 4) + (entry & 255);
          term = (axis == 0 ? gdx_n : gdy_n)[int64_t(y) * W + px];
        }
        if (axis == 0) {
          scatter_pair_round<T, 0, kSlots>(act, px, y, term, idx_n, v_n, vi_n, bary_n, HW, W, M, t_keys[wave], t_vals[wave], grad_n);
        } else {
          scatter_pair_round<T, 1, kSlots>(act, px, y, term, idx_n, v_n, vi_n, bary_n, HW, W, M, t_keys[wave], t_vals[wave], grad_n);
        }
      }
    }
  }
  wave_lds_sync();
  table_flush<T, TableAcc, kSlots>(t_keys[wave], t_vals[wave], 4, 3, grad_n, 3, 0);
}

// ---------------------------------------------------------------------------------------------
// Launchers
// ---------------------------------------------------------------------------------------------
inline bool aligned_to(const void* p, size_t a) {
  return reinterpret_cast<uintptr_t>(p) % a == 0;
}

// the grid of every launch of edge_dots_kernel: strips of 63 lanes (lane 63 = halo) x bands of one workgroup's rows
struct DotsGrid {
  int strips_x;
  dim3 grid;
  int strip; // xcd_strip: workgroups of 16 image rows stay on one XCD
};
inline DotsGrid edge_dots_grid(int64_t N, int64_t H, int64_t W) {
  const int strips_x = static_cast<int>(ceil_div(W, (kWave - 1) * 4));
  const int bands_y = static_cast<int>(ceil_div(H, kStripRows * kDotsWaves));
  return {strips_x, dim3(static_cast<unsigned>(int64_t(strips_x) * bands_y), static_cast<unsigned>(N)),
          xcd_strip(int64_t(strips_x) * (16 / (kStripRows * kDotsWaves)))};
}

// The dense body: any width and any element-aligned placement (Quad).  zero_out: see edge_dots_kernel.
template <typename T>
int launch_edge_dots(const T* img, const T* grad_output, const int32_t* index_img, int64_t N, int64_t C, int64_t H, int64_t W, T* gdx, T* gdy, hipStream_t stream, T* zero_out, int64_t zero_count) {
  const DotsGrid g = edge_dots_grid(N, H, W);
  DRTK_LAUNCH((edge_dots_kernel<T, kStripRows, kDotsWaves>), g.grid, dim3(kDotsWaves * kWave), 0, stream, img, grad_output, index_img, (int)C, (int)H, (int)W, g.strips_x, gdx, gdy, g.strip, zero_out, zero_count, PairArgs<T>{});
  DRTK_RETURN_IF_LAUNCH_FAILED();
  return DRTK_OK;
}

// The one-pass body; pairs.grad_v_pix is clear already.
inline int launch_edge_onepass(const float* img, const float* grad_output, const int32_t* index_img, int64_t N, int64_t C, int64_t H, int64_t W, const PairArgs<float>& pairs, hipStream_t stream) {
  const DotsGrid g = edge_dots_grid(N, H, W);
  DRTK_LAUNCH((edge_dots_kernel<float, kStripRows, kDotsWaves, true>), g.grid, dim3(kDotsWaves * kWave), 0, stream, img, grad_output, index_img, (int)C, (int)H, (int)W, g.strips_x, static_cast<float*>(nullptr), static_cast<float*>(nullptr), g.strip, static_cast<float*>(nullptr), int64_t(0), pairs);
  DRTK_RETURN_IF_LAUNCH_FAILED();
  return DRTK_OK;
}

// Hook route: dots + gather.
template <typename T>
int edge_grad_backward_impl(
    const T* v_pix, const T* img, const int32_t* index_img, const int32_t* vi, const T* grad_output,
    int64_t N, int64_t V, int64_t C, int64_t vi_sN, int64_t H, int64_t W, double max_dp_dr, T* out,
    void* workspace, hipStream_t stream) {
  const int64_t HW = H * W;
  if (N * HW == 0) return DRTK_OK;
  T* gdx = static_cast<T*>(workspace);
  T* gdy = gdx + N * HW;
  const int st = launch_edge_dots<T>(img, grad_output, index_img, N, C, H, W, gdx, gdy, stream, static_cast<T*>(nullptr), 0);
  if (st != DRTK_OK) return st;
  // the dots take any placement; this only picks the gather's kernel
  const bool vec = (W % 4 == 0) && aligned_to(img, 4 * sizeof(T)) && aligned_to(grad_output, 4 * sizeof(T)) &&
      aligned_to(workspace, 4 * sizeof(T)) && aligned_to(index_img, 16) && aligned_to(out, 4 * sizeof(T));
  if (vec) {
    const dim3 gridB(static_cast<unsigned>(ceil_div(HW, kBlock * 4)), static_cast<unsigned>(N));
    DRTK_LAUNCH((edge_gather4_kernel<T>), gridB, dim3(kBlock), 0, stream, v_pix, vi, index_img, gdx, gdy, V, vi_sN, (int)H, (int)W, static_cast<T>(max_dp_dr), out, xcd_strip(ceil_div(16 * W, kBlock * 4)));
  } else {
    const dim3 gridB(static_cast<unsigned>(ceil_div(HW, kBlock)), static_cast<unsigned>(N));
    DRTK_LAUNCH((edge_gather_kernel<T>), gridB, dim3(kBlock), 0, stream, v_pix, vi, index_img, gdx, gdy, V, vi_sN, (int)H, (int)W, static_cast<T>(max_dp_dr), out);
  }
  DRTK_RETURN_IF_LAUNCH_FAILED();
  return DRTK_OK;
}

// Float calls of the fused route with at least this many pixels (all views) take the one pass.  No shape class measured
// slower in one pass (profiles/NOTES.md R7.1 "Dispatch", R8.1; profiles/r07/edge_onepass_ab.txt, profiles/r08/edge_prune_ab.txt),
// so the rule is not about speed: below a megapixel a call is two launches either way, and the suite's timing contracts
// (tests/test_gpu_parity.py, tests/test_gpu_bench_contract.py) name BOTH kernels on small float scenes.
constexpr int64_t kOnepassMinPixels = int64_t(1) << 20;
// DRTK_AMD_EDGE_ONEPASS in the environment overrides the size rule -- 1: every float call, 0: none -- so that the one-pass
// body is tested on strips of a few rows (tests/test_gpu_edge_onepass.py) and both routes can be timed from one library.
inline bool edge_onepass_wanted(int64_t pixels) {
  const char* e = std::getenv("DRTK_AMD_EDGE_ONEPASS"); // read per call: a test switches it inside one process
  if (e && e[0] && !e[1] && (e[0] == '0' || e[0] == '1')) return e[0] == '1';
  return pixels >= kOnepassMinPixels;
}

// Fused route: one pass, or dots + scatter_pairs.
template <typename T>
int edge_grad_backward_fused_impl(
    const T* v_pix, const T* img, const int32_t* index_img, const int32_t* vi, const T* bary_img,
    const T* grad_output, int64_t N, int64_t V, int64_t C, int64_t F, int64_t vi_sN, int64_t H, int64_t W,
    double max_dp_dr, T* grad_v_pix, void* workspace, hipStream_t stream) {
  const int64_t HW = H * W;
  if (N * HW == 0) { // (otherwise grad_v_pix is cleared inside the first kernel)
    if (N * V > 0 && fill_bytes_async(grad_v_pix, 0, sizeof(T) * N * V * 3, stream) != DRTK_OK) return DRTK_ERR_LAUNCH;
    return DRTK_OK;
  }
  if constexpr (std::is_same<T, float>::value) {
    // (the one-pass body addresses a view's planes and tables with 32-bit byte offsets; a view beyond that -- a gigapixel,
    // 357 M vertices or triangles -- takes the two kernels, which address with pointers)
    const bool addressable = HW <= (int64_t(1) << 30) - 8 && V < (int64_t(1) << 32) / 12 && F < (int64_t(1) << 32) / 12;
    if (edge_onepass_wanted(N * HW) && addressable) {
      // The workspace is not touched.  grad_v_pix is cleared by a launch of its own: spread over the grid of the
      // scattering kernel the fill would race other workgroups' atomics.
      if (N * V > 0 && fill_bytes_async(grad_v_pix, 0, sizeof(T) * N * V * 3, stream) != DRTK_OK) return DRTK_ERR_LAUNCH;
      return launch_edge_onepass(img, grad_output, index_img, N, C, H, W, PairArgs<T>{v_pix, vi, bary_img, grad_v_pix, V, vi_sN, F, static_cast<T>(max_dp_dr)}, stream);
    }
  }
  // Two kernels for every shape and every element-aligned placement of the tensors (two planes of workspace): both
  // fetch four adjacent pixels per access with the alignment of the element and handle the end of a row whose width is
  // not a multiple of four lane by lane.
  T* gdx = static_cast<T*>(workspace);
  T* gdy = gdx + N * HW;
  const int st = launch_edge_dots<T>(img, grad_output, index_img, N, C, H, W, gdx, gdy, stream, grad_v_pix, N * V * 3);
  if (st != DRTK_OK) return st;
  const int strips_x = static_cast<int>(ceil_div(W, kWave * 4));
  const int64_t waves = int64_t(strips_x) * ceil_div(H, kPairRows);
  const dim3 grid(static_cast<unsigned>(ceil_div(waves, kBlock / kWave)), static_cast<unsigned>(N));
  const int strip = xcd_strip(ceil_div(int64_t(strips_x) * (16 / kPairRows), kBlock / kWave));
  DRTK_LAUNCH((edge_scatter_pairs_kernel<T>), grid, dim3(kBlock), 0, stream, v_pix, vi, index_img, bary_img, gdx, gdy, V, vi_sN, (int)H, (int)W, strips_x, static_cast<T>(max_dp_dr), grad_v_pix, strip);
  DRTK_RETURN_IF_LAUNCH_FAILED();
  return DRTK_OK;
}

// ---------------------------------------------------------------------------------------------
// What the C entry points share
// ---------------------------------------------------------------------------------------------
// the two planes of pair terms (gdx, gdy); never an empty allocation
int edge_workspace_bytes(drtk_dtype_t dtype, int64_t N, int64_t H, int64_t W, size_t* bytes) {
  if (!bytes || N < 0 || H < 0 || W < 0 || !valid_dtype(dtype)) return DRTK_ERR_INVALID_ARGUMENT;
  const size_t b = size_t(2) * N * H * W * dtype_size(dtype);
  *bytes = b > 0 ? b : 16;
  return DRTK_OK;
}

// The argument check of both entry points, DRTK_OK to go on.  Sizes and dtype first, then the workspace's alignment,
// then the pointers, each under the size condition that makes it required, the workspace's size last.  The entries
// differ in their own tensors: the fused route reads bary_img and writes `out` per vertex (required as soon as there
// is a vertex, pixels or not: it is cleared), the hook route has no bary_img and writes `out` per pixel.
int check_edge_args(
    bool fused, drtk_dtype_t dtype, const void* v_pix, const void* img, const int32_t* index_img, const int32_t* vi,
    const void* bary_img, const void* grad_output, int64_t N, int64_t V, int64_t C, int64_t F, int64_t vi_sN, int64_t H,
    int64_t W, const void* out, const void* workspace, size_t workspace_bytes) {
  if (bad_image(N, H, W) || V < 0 || C < 0 || F < 0 || bad_view_stride(vi_sN, F * 3) || !valid_dtype(dtype)) return DRTK_ERR_INVALID_ARGUMENT;
  if (!aligned_to(workspace, 16)) return DRTK_ERR_INVALID_ARGUMENT; // include/drtk_amd.h, alignment
  size_t need = 0;
  if (edge_workspace_bytes(dtype, N, H, W, &need) != DRTK_OK) return DRTK_ERR_INVALID_ARGUMENT;
  if (fused && N * V > 0 && !out) return DRTK_ERR_INVALID_ARGUMENT;
  if (N * H * W > 0) {
    if (!index_img || !(fused ? bary_img : out) || !workspace) return DRTK_ERR_INVALID_ARGUMENT;
    if ((N * V > 0 && !v_pix) || (F > 0 && !vi)) return DRTK_ERR_INVALID_ARGUMENT;
    if (C > 0 && (!img || !grad_output)) return DRTK_ERR_INVALID_ARGUMENT;
    if (workspace_bytes < need) return DRTK_ERR_WORKSPACE_TOO_SMALL;
  }
  return DRTK_OK;
}

} // namespace
} // namespace drtk_amd

using namespace drtk_amd;

extern "C" int drtk_amd_edge_grad_backward_workspace_bytes(
    drtk_dtype_t dtype, int64_t N, int64_t H, int64_t W, size_t* bytes) {
  return edge_workspace_bytes(dtype, N, H, W, bytes);
}

extern "C" int drtk_amd_edge_grad_backward_fused_workspace_bytes(
    drtk_dtype_t dtype, int64_t N, int64_t H, int64_t W, size_t* bytes) {
  return edge_workspace_bytes(dtype, N, H, W, bytes);
}

extern "C" int drtk_amd_edge_grad_backward(
    drtk_dtype_t dtype, const void* v_pix, const void* img, const int32_t* index_img,
    const int32_t* vi, const void* grad_output, int64_t N, int64_t V, int64_t C, int64_t F,
    int64_t vi_sN, int64_t H, int64_t W, double max_dp_dr, void* grad_v_pix_img, void* workspace,
    size_t workspace_bytes, drtk_stream_t stream) {
  const int ok = check_edge_args(false, dtype, v_pix, img, index_img, vi, nullptr, grad_output, N, V, C, F, vi_sN, H, W, grad_v_pix_img, workspace, workspace_bytes);
  if (ok != DRTK_OK) return ok;
  const size_t es = dtype_size(dtype);
  if (N > kMaxViewsPerLaunch) return for_view_slices(N, [&](int64_t n0, int64_t n) { // (every slice reuses the front of the workspace: stream order)
    return drtk_amd_edge_grad_backward(
        dtype, advance(v_pix, n0 * V * 3, es), advance(img, n0 * C * H * W, es), advance_typed(index_img, n0 * H * W),
        advance_typed(vi, n0 * vi_sN), advance(grad_output, n0 * C * H * W, es), n, V, C, F, vi_sN, H, W, max_dp_dr,
        advance(grad_v_pix_img, n0 * 3 * H * W, es), workspace, workspace_bytes, stream);
  });
  return dispatch_dtype(dtype, [&](auto tag) {
    using T = decltype(tag);
    return edge_grad_backward_impl<T>(
        static_cast<const T*>(v_pix), static_cast<const T*>(img), index_img, vi, static_cast<const T*>(grad_output), N, V, C, vi_sN, H, W,
        max_dp_dr, static_cast<T*>(grad_v_pix_img), workspace, static_cast<hipStream_t>(stream));
  });
}

extern "C" int drtk_amd_edge_grad_backward_fused(
    drtk_dtype_t dtype, const void* v_pix, const void* img, const int32_t* index_img,
    const int32_t* vi, const void* bary_img, const void* grad_output, int64_t N, int64_t V, int64_t C,
    int64_t F, int64_t vi_sN, int64_t H, int64_t W, double max_dp_dr, void* grad_v_pix,
    void* workspace, size_t workspace_bytes, drtk_stream_t stream) {
  const int ok = check_edge_args(true, dtype, v_pix, img, index_img, vi, bary_img, grad_output, N, V, C, F, vi_sN, H, W, grad_v_pix, workspace, workspace_bytes);
  if (ok != DRTK_OK) return ok;
  const size_t es = dtype_size(dtype);
  if (N > kMaxViewsPerLaunch) return for_view_slices(N, [&](int64_t n0, int64_t n) {
    return drtk_amd_edge_grad_backward_fused(
        dtype, advance(v_pix, n0 * V * 3, es), advance(img, n0 * C * H * W, es), advance_typed(index_img, n0 * H * W),
        advance_typed(vi, n0 * vi_sN), advance(bary_img, n0 * 3 * H * W, es), advance(grad_output, n0 * C * H * W, es), n, V, C, F,
        vi_sN, H, W, max_dp_dr, advance(grad_v_pix, n0 * V * 3, es), workspace, workspace_bytes, stream);
  });
  return dispatch_dtype(dtype, [&](auto tag) {
    using T = decltype(tag);
    return edge_grad_backward_fused_impl<T>(
        static_cast<const T*>(v_pix), static_cast<const T*>(img), index_img, vi, static_cast<const T*>(bary_img),
        static_cast<const T*>(grad_output), N, V, C, F, vi_sN, H, W, max_dp_dr, static_cast<T*>(grad_v_pix), workspace,
        static_cast<hipStream_t>(stream));
  });
}
