// drtk_amd_ext mesh-geometry operators -- drtk/utils/geometry.py of the reference (face_info, vert_normals,
// face_attribute_to_vert, face_dpdt, vert_binormals) over drtk_amd_geometry_* (csrc/geometry.hip): a face pass and a
// vertex pass that sums through the vertex incidence, each way, without float atomics.
// Also this package's mesh regulariser on the same passes: cotangent_weights and mesh_laplacian.
#include "topology_cache.hpp"

#include <algorithm>

namespace {
using namespace drtk_amd_torch;

constexpr int64_t kChunk = DRTK_GEOMETRY_CHUNK;

// ---------------------------------------------------------------------------------------------
// Vertex incidence: the chunked CSR (topology_cache.hpp) over rows b*V + vertex of the keys b*V + vi[b,f,k], entries
// f*3+k ascending within a row, only the rows longer than DRTK_GEOMETRY_CHUNK cut into chunks.  An index outside [0, V)
// would make the kernels read out of bounds.
// ---------------------------------------------------------------------------------------------
struct Incidence {
  Tensor vi32; // int32 [B,F,3] contiguous
  Tensor entries; // int32 [3*B*F]
  ChunkedCsr csr; // rows B*V
  int64_t B = 1, F = 0, V = 0;
};

Incidence build_incidence(const Tensor& t, int64_t V, const char* op) {
  Incidence inc;
  inc.B = t.size(0), inc.F = t.size(1), inc.V = V;
  TORCH_CHECK(V >= 0 && V < (int64_t(1) << 31), op, "(): expected the vertex count to fit in int32");
  const int64_t R = inc.B * V, E = 3 * inc.B * inc.F;
  TORCH_CHECK(E < (int64_t(1) << 31) && R < (int64_t(1) << 31), op, "(): mesh too large for int32 incidence");
  const Tensor tl = t.detach().to(at::kLong).contiguous();
  inc.vi32 = t.detach().to(at::kInt).contiguous();
  const Tensor keys = (tl + (at::arange(inc.B, tl.options()) * V).view({inc.B, 1, 1})).reshape({-1});
  inc.csr = build_chunked_csr(keys, R, kChunk, /*chunk_every_row=*/false, tl);
  TORCH_CHECK(E == 0 || (inc.csr.lo >= 0 && inc.csr.hi < V), op, "(): vi contains a vertex index outside [0, ", V, ")");
  inc.entries = at::remainder(inc.csr.perm, std::max<int64_t>(3 * inc.F, 1)).to(at::kInt);
  inc.csr.perm.reset();
  return inc;
}

// Cached by the identity and version of the index tensor as incidence_of hands it over, and the vertex count.
PinnedLruCache<Incidence>& incidence_cache() {
  static PinnedLruCache<Incidence> c;
  return c;
}

// vi [F,3] / [B,F,3] (B = 1 or N; a stride-0 expand counts as 1) -> its incidence over V vertices
Incidence incidence_of(const Tensor& vi, int64_t N, int64_t V, const char* op) {
  TORCH_CHECK(vi.defined() && vi.layout() == at::kStrided, op, "(): expected vi to be a strided tensor");
  TORCH_CHECK(vi.scalar_type() == at::kInt || vi.scalar_type() == at::kLong, op,
              "(): expected vi to be int32 or int64, got ", vi.scalar_type());
  TORCH_CHECK((vi.dim() == 2 && vi.size(1) == 3) || (vi.dim() == 3 && vi.size(2) == 3), op,
              "(): expected vi of shape [F,3] or [B,F,3]");
  Tensor t = vi.dim() == 2 ? vi.unsqueeze(0) : vi;
  if (t.size(0) > 1 && t.stride(0) == 0) t = t.narrow(0, 0, 1);
  TORCH_CHECK(t.size(0) == 1 || t.size(0) == N, op, "(): expected the batch size of vi to be 1 or ", N, ", got ",
              t.size(0));
  CacheKey key;
  append_tensor_identity(key, t);
  key.push_back(V);
  return incidence_cache().get(key, t, [&] {
    check_not_capturing(t.device(), op, "vertex incidence of this index tensor", "vi");
    return build_incidence(t, V, op);
  });
}

// Incidence tensors travel through autograd contexts as saved data
void save_incidence(AutogradContext* ctx, const std::string& k, const Incidence& inc) {
  ctx->saved_data[k + "vi"] = inc.vi32;
  ctx->saved_data[k + "entries"] = inc.entries;
  ctx->saved_data[k + "sizes"] = std::vector<int64_t>{inc.B, inc.F, inc.V};
  inc.csr.save(ctx, k);
}
Incidence load_incidence(AutogradContext* ctx, const std::string& k) {
  Incidence inc;
  inc.vi32 = ctx->saved_data[k + "vi"].toTensor();
  inc.entries = ctx->saved_data[k + "entries"].toTensor();
  const auto s = ctx->saved_data[k + "sizes"].toIntVector();
  inc.B = s[0], inc.F = s[1], inc.V = s[2];
  inc.csr = ChunkedCsr::load(ctx, k);
  return inc;
}

int64_t vi_stride(const Incidence& inc) {
  return inc.B == 1 ? 0 : inc.F * 3;
}

Tensor prep_v(const Tensor& v, const char* op) {
  TORCH_CHECK(v.is_cuda(), op, "(): drtk_amd implements the MI355X (HIP) path only; got CPU tensors");
  TORCH_CHECK(v.dim() == 3 && v.size(2) == 3, op, "(): expected v of shape [N, V, 3]");
  dtype_of(v, op);
  return v.contiguous();
}
Tensor like_v(const Tensor& t, const Tensor& v, const char* op, const char* what) {
  TORCH_CHECK(t.device() == v.device(), op, "(): expected ", what, " on the device of v");
  return t.to(v.scalar_type()).contiguous();
}

// out [N,V,A] (+ sums [N,V,3]) = per-vertex sums of src rows: [N,F,A] (per_corner false) or [N,F,3,A]
Tensor vertex_gather(const Tensor& src, bool per_corner, int64_t A, const Incidence& inc, int64_t N, bool normalize,
                     Tensor* sums, const char* op) {
  const drtk_dtype_t dt = dtype_of(src, op);
  auto out = out_empty({N, inc.V, A}, src.options());
  Tensor s;
  if (sums) s = out_empty({N, inc.V, 3}, src.options());
  size_t bytes = 0;
  check_status(drtk_amd_geometry_vertex_gather_workspace_bytes(dt, N, inc.B, inc.csr.C, A, &bytes), op);
  Tensor ws = bytes ? alloc_workspace(bytes, src) : Tensor();
  const bool chunks = inc.csr.C > 0;
  check_status(
      drtk_amd_geometry_vertex_gather(
          dt, src.data_ptr(), inc.F * A * (per_corner ? 3 : 1), per_corner ? 1 : 0, A, inc.csr.crow.data_ptr<int32_t>(),
          inc.entries.data_ptr<int32_t>(), chunks ? inc.csr.chunk_ptr.data_ptr<int32_t>() : nullptr,
          chunks ? inc.csr.chunk_begin.data_ptr<int32_t>() : nullptr, chunks ? inc.csr.chunk_row.data_ptr<int32_t>() : nullptr,
          inc.csr.C, inc.B, N, inc.V, inc.F, normalize ? 1 : 0, out.data_ptr(), sums ? s.data_ptr() : nullptr,
          ws.defined() ? ws.data_ptr() : nullptr, bytes, current_stream(src)),
      op);
  if (sums) *sums = s;
  return out;
}

// grad [N,F,A] = sum over each face's corners of g [N,V,A] (through F.normalize's backward when sums is defined)
Tensor face_gather(const Tensor& g, const Tensor& sums, const Incidence& inc, int64_t N, int64_t A, const char* op) {
  auto out = out_empty({N, inc.F, A}, g.options());
  check_status(drtk_amd_geometry_face_gather(
                   dtype_of(g, op), g.data_ptr(), sums.defined() ? sums.data_ptr() : nullptr,
                   inc.vi32.data_ptr<int32_t>(), vi_stride(inc), N, inc.V, inc.F, A, out.data_ptr(), current_stream(g)),
               op);
  return out;
}

const void* ptr_or_null(const Tensor& t) {
  return t.defined() ? t.data_ptr() : nullptr;
}

// face pass forward; outputs that are not wanted are left undefined
struct FaceOut {
  Tensor normals, areas, edges, dpdt, dpdt_u, v012;
};
FaceOut face_forward(const Tensor& v, const Incidence& inc, const Tensor& vt, const Incidence* tinc, bool normals,
                     bool areas, bool edges, bool dpdt, bool dpdt_u, bool v012, const char* op) {
  const int64_t N = v.size(0), F = inc.F;
  const auto o = v.options();
  FaceOut r;
  if (normals) r.normals = out_empty({N, F, 3}, o);
  if (areas) r.areas = out_empty({N, F, 1}, o);
  if (edges) r.edges = out_empty({N, F, 3, 3}, o);
  if (dpdt) r.dpdt = out_empty({N, F, 2, 3}, o);
  if (dpdt_u) r.dpdt_u = out_empty({N, F, 3}, o);
  if (v012) r.v012 = out_empty({N, F, 3, 3}, o);
  check_status(
      drtk_amd_geometry_face_forward(
          dtype_of(v, op), v.data_ptr(), v.size(1) * 3, inc.vi32.data_ptr<int32_t>(), vi_stride(inc),
          tinc ? vt.data_ptr() : nullptr, tinc ? vt.size(1) * 2 : 0, tinc ? tinc->vi32.data_ptr<int32_t>() : nullptr,
          N, v.size(1), tinc ? tinc->V : 0, F, normals ? r.normals.data_ptr() : nullptr,
          areas ? r.areas.data_ptr() : nullptr, edges ? r.edges.data_ptr() : nullptr,
          dpdt ? r.dpdt.data_ptr() : nullptr, dpdt_u ? r.dpdt_u.data_ptr() : nullptr,
          v012 ? r.v012.data_ptr() : nullptr, current_stream(v)),
      op);
  return r;
}

// face pass backward -> grad_v [N,V,3] (and grad_vt [N,T,2] when tinc is given)
// (only the reductions that are wanted: need_v / need_vt)
std::pair<Tensor, Tensor> face_backward(const Tensor& v, const Incidence& inc, const Tensor& vt, const Incidence* tinc,
                                        const Tensor& g_vert, const Tensor& sums, const Tensor& g_normals,
                                        const Tensor& g_areas, const Tensor& g_edges, const Tensor& g_dpdt,
                                        const Tensor& g_v012, bool need_v, bool need_vt, const char* op) {
  const int64_t N = v.size(0), F = inc.F;
  auto pos = out_empty({N, F, 3, 3}, v.options());
  Tensor uv = tinc ? out_empty({N, F, 3, 2}, v.options()) : Tensor();
  check_status(
      drtk_amd_geometry_face_backward(
          dtype_of(v, op), v.data_ptr(), v.size(1) * 3, inc.vi32.data_ptr<int32_t>(), vi_stride(inc),
          tinc ? vt.data_ptr() : nullptr, tinc ? vt.size(1) * 2 : 0, tinc ? tinc->vi32.data_ptr<int32_t>() : nullptr,
          N, v.size(1), tinc ? tinc->V : 0, F, ptr_or_null(g_vert), ptr_or_null(sums), ptr_or_null(g_normals),
          ptr_or_null(g_areas), ptr_or_null(g_edges), ptr_or_null(g_dpdt), ptr_or_null(g_v012), pos.data_ptr(),
          tinc ? uv.data_ptr() : nullptr, current_stream(v)),
      op);
  Tensor gv = need_v ? vertex_gather(pos, true, 3, inc, N, false, nullptr, op) : Tensor();
  Tensor gvt = tinc && need_vt ? vertex_gather(uv, true, 2, *tinc, N, false, nullptr, op) : Tensor();
  return {gv, gvt};
}

// Which inputs want a gradient is decided on the inputs as the caller passed them: the tensors the forward saves are the
// contiguous copies the kernels read, and a copy made inside Function::forward (grad mode off) never requires grad --
// an expanded, sliced or permuted v would silently get none.
// (v: the differentiable input -- the attribute for face_attribute_to_vert and given fnorms)
void save_requires_grad(AutogradContext* ctx, const Tensor& v, const Tensor& vt) {
  ctx->saved_data["v_requires_grad"] = v.requires_grad();
  ctx->saved_data["vt_requires_grad"] = vt.defined() && vt.requires_grad();
}
bool wants(AutogradContext* ctx, const char* k) {
  return ctx->saved_data[k].toBool();
}

// The backward passes are kernels, not differentiable graphs: under create_graph=True their second-order terms would be
// silently zero, so that is an error.
void no_double_backward(const char* op) {
  TORCH_CHECK(!at::GradMode::is_enabled(), op,
              "(): double backward (create_graph=True) is not supported by drtk_amd's geometry kernels; the PyTorch "
              "formulation (CPU tensors) supports it");
}

Tensor grad_or_undef(const Tensor& g, const Tensor& v) {
  return g.defined() ? g.to(v.scalar_type()).contiguous() : Tensor();
}

// ---------------------------------------------------------------------------------------------
// face_info
// ---------------------------------------------------------------------------------------------
using Tensor3 = std::tuple<Tensor, Tensor, Tensor>;

Tensor3 face_info_hip(const Tensor& v_, const Tensor& vi, bool normals, bool areas, bool edges) {
  c10::hip::OptionalHIPGuardMasqueradingAsCUDA guard(v_.device());
  const Tensor v = prep_v(v_, "face_info");
  TORCH_CHECK(normals || areas || edges, "face_info(): nothing to compute");
  const Incidence inc = incidence_of(vi, v.size(0), v.size(1), "face_info");
  FaceOut r = face_forward(v, inc, Tensor(), nullptr, normals, areas, edges, false, false, false, "face_info");
  const auto empty = at::empty({0}, v.options());
  return {normals ? r.normals : empty, areas ? r.areas : empty, edges ? r.edges : empty};
}

class FaceInfoFunction : public torch::autograd::Function<FaceInfoFunction> {
 public:
  static tensor_list forward(AutogradContext* ctx, const Tensor& v_, const Tensor& vi, bool normals, bool areas,
                             bool edges) {
    c10::hip::OptionalHIPGuardMasqueradingAsCUDA guard(v_.device());
    ctx->set_materialize_grads(false);
    const Tensor v = prep_v(v_, "face_info");
    TORCH_CHECK(normals || areas || edges, "face_info(): nothing to compute");
    const Incidence inc = incidence_of(vi, v.size(0), v.size(1), "face_info");
    ctx->save_for_backward({v});
    save_requires_grad(ctx, v_, Tensor());
    save_incidence(ctx, "", inc);
    at::AutoDispatchBelowADInplaceOrView g;
    FaceOut r = face_forward(v, inc, Tensor(), nullptr, normals, areas, edges, false, false, false, "face_info");
    const auto empty = at::empty({0}, v.options());
    return {normals ? r.normals : empty, areas ? r.areas : empty, edges ? r.edges : empty};
  }
  static tensor_list backward(AutogradContext* ctx, tensor_list go) {
    const Tensor v = ctx->get_saved_variables()[0];
    const Tensor gn = go[0].defined() && go[0].numel() ? grad_or_undef(go[0], v) : Tensor();
    const Tensor ga = go[1].defined() && go[1].numel() ? grad_or_undef(go[1], v) : Tensor();
    const Tensor ge = go[2].defined() && go[2].numel() ? grad_or_undef(go[2], v) : Tensor();
    if (!(gn.defined() || ga.defined() || ge.defined()) || !wants(ctx, "v_requires_grad"))
      return {Tensor(), Tensor(), Tensor(), Tensor(), Tensor()};
    no_double_backward("face_info_backward");
    c10::hip::OptionalHIPGuardMasqueradingAsCUDA guard(v.device());
    const Incidence inc = load_incidence(ctx, "");
    auto gvs = face_backward(v, inc, Tensor(), nullptr, Tensor(), Tensor(), gn, ga, ge, Tensor(), Tensor(), true, false,
                             "face_info_backward");
    return {gvs.first, Tensor(), Tensor(), Tensor(), Tensor()};
  }
};
Tensor3 face_info_autograd(const Tensor& v, const Tensor& vi, bool normals, bool areas, bool edges) {
  auto r = FaceInfoFunction::apply(v, vi, normals, areas, edges);
  return {r[0], r[1], r[2]};
}

// ---------------------------------------------------------------------------------------------
// vert_normals (face normals from v, or given as fnorms) and face_attribute_to_vert
// ---------------------------------------------------------------------------------------------
Tensor vert_normals_hip(const Tensor& v_, const Tensor& vi, const c10::optional<Tensor>& fnorms) {
  c10::hip::OptionalHIPGuardMasqueradingAsCUDA guard(v_.device());
  const Tensor v = prep_v(v_, "vert_normals");
  const int64_t N = v.size(0);
  const Incidence inc = incidence_of(vi, N, v.size(1), "vert_normals");
  Tensor fn;
  if (fnorms.has_value() && fnorms->defined()) {
    fn = like_v(*fnorms, v, "vert_normals", "fnorms");
    TORCH_CHECK(fn.dim() == 3 && fn.size(0) == N && fn.size(1) == inc.F && fn.size(2) == 3,
                "vert_normals(): expected fnorms of shape [N, F, 3]");
  } else {
    fn = face_forward(v, inc, Tensor(), nullptr, true, false, false, false, false, false, "vert_normals").normals;
  }
  return vertex_gather(fn, false, 3, inc, N, true, nullptr, "vert_normals");
}

class VertNormalsFunction : public torch::autograd::Function<VertNormalsFunction> {
 public:
  static tensor_list forward(AutogradContext* ctx, const Tensor& v_, const Tensor& vi) {
    c10::hip::OptionalHIPGuardMasqueradingAsCUDA guard(v_.device());
    ctx->set_materialize_grads(false);
    const Tensor v = prep_v(v_, "vert_normals");
    const Incidence inc = incidence_of(vi, v.size(0), v.size(1), "vert_normals");
    at::AutoDispatchBelowADInplaceOrView g;
    const Tensor fn = face_forward(v, inc, Tensor(), nullptr, true, false, false, false, false, false, "vert_normals").normals;
    Tensor sums;
    Tensor out = vertex_gather(fn, false, 3, inc, v.size(0), true, &sums, "vert_normals");
    ctx->save_for_backward({v, sums});
    save_requires_grad(ctx, v_, Tensor());
    save_incidence(ctx, "", inc);
    return {out};
  }
  static tensor_list backward(AutogradContext* ctx, tensor_list go) {
    const auto saved = ctx->get_saved_variables();
    const Tensor& v = saved[0];
    if (!go[0].defined() || !wants(ctx, "v_requires_grad")) return {Tensor(), Tensor()};
    no_double_backward("vert_normals_backward");
    c10::hip::OptionalHIPGuardMasqueradingAsCUDA guard(v.device());
    const Incidence inc = load_incidence(ctx, "");
    auto gvs = face_backward(v, inc, Tensor(), nullptr, grad_or_undef(go[0], v), saved[1], Tensor(), Tensor(), Tensor(),
                             Tensor(), Tensor(), true, false, "vert_normals_backward");
    return {gvs.first, Tensor()};
  }
};

// vert_normals with given face normals, and face_attribute_to_vert: per-vertex sums of a per-face attribute, normalised
// or not; the gradient goes to the attribute only.
class FaceToVertFunction : public torch::autograd::Function<FaceToVertFunction> {
 public:
  static tensor_list forward(AutogradContext* ctx, const Tensor& attr_, const Tensor& v_, const Tensor& vi,
                             bool normalize) {
    const char* op = normalize ? "vert_normals" : "face_attribute_to_vert";
    c10::hip::OptionalHIPGuardMasqueradingAsCUDA guard(v_.device());
    ctx->set_materialize_grads(false);
    TORCH_CHECK(v_.is_cuda(), op, "(): drtk_amd implements the MI355X (HIP) path only; got CPU tensors");
    TORCH_CHECK(v_.dim() >= 2, op, "(): expected v of shape [N, V, *]");
    dtype_of(v_, op);
    const int64_t N = v_.size(0);
    const Incidence inc = incidence_of(vi, N, v_.size(1), op);
    const Tensor attr = like_v(attr_, v_, op, normalize ? "fnorms" : "attr");
    TORCH_CHECK(attr.dim() == 3 && attr.size(0) == N && attr.size(1) == inc.F && (!normalize || attr.size(2) == 3), op,
                "(): expected ", normalize ? "fnorms of shape [N, F, 3]" : "attr of shape [N, F, A]");
    TORCH_CHECK(attr.size(2) >= 1, op, "(): expected at least one attribute channel");
    at::AutoDispatchBelowADInplaceOrView g;
    Tensor sums;
    Tensor out = vertex_gather(attr, false, attr.size(2), inc, N, normalize, normalize ? &sums : nullptr, op);
    ctx->save_for_backward({sums});
    save_requires_grad(ctx, attr_, Tensor());
    save_incidence(ctx, "", inc);
    ctx->saved_data["A"] = attr.size(2);
    ctx->saved_data["attr_dtype"] = static_cast<int64_t>(attr_.scalar_type());
    return {out};
  }
  static tensor_list backward(AutogradContext* ctx, tensor_list go) {
    const auto saved = ctx->get_saved_variables();
    if (!go[0].defined() || !wants(ctx, "v_requires_grad")) return {Tensor(), Tensor(), Tensor(), Tensor()};
    no_double_backward("face_attribute_to_vert_backward");
    c10::hip::OptionalHIPGuardMasqueradingAsCUDA guard(go[0].device());
    const Incidence inc = load_incidence(ctx, "");
    const int64_t A = ctx->saved_data["A"].toInt();
    const Tensor g = go[0].contiguous(); // dtype of v, in which the forward ran
    Tensor ga = face_gather(g, saved[0], inc, g.size(0), A, "face_attribute_to_vert_backward");
    return {ga.to(static_cast<at::ScalarType>(ctx->saved_data["attr_dtype"].toInt())), Tensor(), Tensor(), Tensor()};
  }
};

Tensor vert_normals_autograd(const Tensor& v, const Tensor& vi, const c10::optional<Tensor>& fnorms) {
  if (fnorms.has_value() && fnorms->defined()) return FaceToVertFunction::apply(*fnorms, v, vi, true)[0];
  return VertNormalsFunction::apply(v, vi)[0];
}

Tensor face_attribute_to_vert_hip(const Tensor& v, const Tensor& vi, const Tensor& attr_) {
  c10::hip::OptionalHIPGuardMasqueradingAsCUDA guard(v.device());
  TORCH_CHECK(v.is_cuda(), "face_attribute_to_vert(): drtk_amd implements the MI355X (HIP) path only; got CPU tensors");
  TORCH_CHECK(v.dim() >= 2, "face_attribute_to_vert(): expected v of shape [N, V, *]");
  dtype_of(v, "face_attribute_to_vert");
  const int64_t N = v.size(0);
  const Incidence inc = incidence_of(vi, N, v.size(1), "face_attribute_to_vert");
  const Tensor attr = like_v(attr_, v, "face_attribute_to_vert", "attr");
  TORCH_CHECK(attr.dim() == 3 && attr.size(0) == N && attr.size(1) == inc.F && attr.size(2) >= 1,
              "face_attribute_to_vert(): expected attr of shape [N, F, A]");
  return vertex_gather(attr, false, attr.size(2), inc, N, false, nullptr, "face_attribute_to_vert");
}
Tensor face_attribute_to_vert_autograd(const Tensor& v, const Tensor& vi, const Tensor& attr) {
  return FaceToVertFunction::apply(attr, v, vi, false)[0];
}

// ---------------------------------------------------------------------------------------------
// face_dpdt and vert_binormals (vi, vti: [F,3])
// ---------------------------------------------------------------------------------------------
struct DpdtArgs {
  Tensor v, vt;
  Incidence inc, tinc;
};
DpdtArgs dpdt_prep(const Tensor& v_, const Tensor& vt_, const Tensor& vi, const Tensor& vti, const char* op) {
  DpdtArgs a;
  a.v = prep_v(v_, op);
  TORCH_CHECK(vt_.dim() == 3 && vt_.size(2) == 2, op, "(): expected vt of shape [N, T, 2]");
  TORCH_CHECK(vt_.size(0) == a.v.size(0), op, "(): expected vt to have the same batch size as v, got ", vt_.size(0),
              " and ", a.v.size(0));
  a.vt = like_v(vt_, a.v, op, "vt");
  TORCH_CHECK(vi.dim() == 2 && vti.dim() == 2, op, "(): expected vi and vti of shape [F, 3]");
  TORCH_CHECK(vi.size(0) == vti.size(0), op, "(): expected vi and vti to list the same faces");
  a.inc = incidence_of(vi, a.v.size(0), a.v.size(1), op);
  a.tinc = incidence_of(vti, a.v.size(0), a.vt.size(1), op);
  return a;
}

std::tuple<Tensor, Tensor> face_dpdt_hip(const Tensor& v, const Tensor& vt, const Tensor& vi, const Tensor& vti) {
  c10::hip::OptionalHIPGuardMasqueradingAsCUDA guard(v.device());
  const DpdtArgs a = dpdt_prep(v, vt, vi, vti, "face_dpdt");
  FaceOut r = face_forward(a.v, a.inc, a.vt, &a.tinc, false, false, false, true, false, true, "face_dpdt");
  return {r.dpdt, r.v012};
}

class FaceDpdtFunction : public torch::autograd::Function<FaceDpdtFunction> {
 public:
  static tensor_list forward(AutogradContext* ctx, const Tensor& v, const Tensor& vt, const Tensor& vi,
                             const Tensor& vti) {
    c10::hip::OptionalHIPGuardMasqueradingAsCUDA guard(v.device());
    ctx->set_materialize_grads(false);
    const DpdtArgs a = dpdt_prep(v, vt, vi, vti, "face_dpdt");
    ctx->save_for_backward({a.v, a.vt});
    save_requires_grad(ctx, v, vt);
    save_incidence(ctx, "p", a.inc);
    save_incidence(ctx, "t", a.tinc);
    at::AutoDispatchBelowADInplaceOrView g;
    FaceOut r = face_forward(a.v, a.inc, a.vt, &a.tinc, false, false, false, true, false, true, "face_dpdt");
    return {r.dpdt, r.v012};
  }
  static tensor_list backward(AutogradContext* ctx, tensor_list go) {
    const auto saved = ctx->get_saved_variables();
    const Tensor &v = saved[0], &vt = saved[1];
    const bool need_v = wants(ctx, "v_requires_grad"), need_vt = wants(ctx, "vt_requires_grad");
    if (!(go[0].defined() || go[1].defined()) || !(need_v || need_vt)) return {Tensor(), Tensor(), Tensor(), Tensor()};
    no_double_backward("face_dpdt_backward");
    c10::hip::OptionalHIPGuardMasqueradingAsCUDA guard(v.device());
    const Incidence inc = load_incidence(ctx, "p"), tinc = load_incidence(ctx, "t");
    auto g = face_backward(v, inc, vt, &tinc, Tensor(), Tensor(), Tensor(), Tensor(), Tensor(), grad_or_undef(go[0], v),
                           grad_or_undef(go[1], v), need_v, need_vt, "face_dpdt_backward");
    return {g.first, g.second, Tensor(), Tensor()};
  }
};
std::tuple<Tensor, Tensor> face_dpdt_autograd(const Tensor& v, const Tensor& vt, const Tensor& vi, const Tensor& vti) {
  auto r = FaceDpdtFunction::apply(v, vt, vi, vti);
  return {r[0], r[1]};
}

Tensor vert_binormals_hip(const Tensor& v, const Tensor& vt, const Tensor& vi, const Tensor& vti) {
  c10::hip::OptionalHIPGuardMasqueradingAsCUDA guard(v.device());
  const DpdtArgs a = dpdt_prep(v, vt, vi, vti, "vert_binormals");
  const Tensor u = face_forward(a.v, a.inc, a.vt, &a.tinc, false, false, false, false, true, false, "vert_binormals").dpdt_u;
  return vertex_gather(u, false, 3, a.inc, a.v.size(0), true, nullptr, "vert_binormals");
}

class VertBinormalsFunction : public torch::autograd::Function<VertBinormalsFunction> {
 public:
  static tensor_list forward(AutogradContext* ctx, const Tensor& v, const Tensor& vt, const Tensor& vi,
                             const Tensor& vti) {
    c10::hip::OptionalHIPGuardMasqueradingAsCUDA guard(v.device());
    ctx->set_materialize_grads(false);
    const DpdtArgs a = dpdt_prep(v, vt, vi, vti, "vert_binormals");
    at::AutoDispatchBelowADInplaceOrView g;
    const Tensor u =
        face_forward(a.v, a.inc, a.vt, &a.tinc, false, false, false, false, true, false, "vert_binormals").dpdt_u;
    Tensor sums;
    Tensor out = vertex_gather(u, false, 3, a.inc, a.v.size(0), true, &sums, "vert_binormals");
    ctx->save_for_backward({a.v, a.vt, sums});
    save_requires_grad(ctx, v, vt);
    save_incidence(ctx, "p", a.inc);
    save_incidence(ctx, "t", a.tinc);
    return {out};
  }
  static tensor_list backward(AutogradContext* ctx, tensor_list go) {
    const auto saved = ctx->get_saved_variables();
    const Tensor &v = saved[0], &vt = saved[1];
    const bool need_v = wants(ctx, "v_requires_grad"), need_vt = wants(ctx, "vt_requires_grad");
    if (!go[0].defined() || !(need_v || need_vt)) return {Tensor(), Tensor(), Tensor(), Tensor()};
    no_double_backward("vert_binormals_backward");
    c10::hip::OptionalHIPGuardMasqueradingAsCUDA guard(v.device());
    const Incidence inc = load_incidence(ctx, "p"), tinc = load_incidence(ctx, "t");
    auto g = face_backward(v, inc, vt, &tinc, grad_or_undef(go[0], v), saved[2], Tensor(), Tensor(), Tensor(), Tensor(),
                           Tensor(), need_v, need_vt, "vert_binormals_backward");
    return {g.first, g.second, Tensor(), Tensor()};
  }
};
Tensor vert_binormals_autograd(const Tensor& v, const Tensor& vt, const Tensor& vi, const Tensor& vti) {
  return VertBinormalsFunction::apply(v, vt, vi, vti)[0];
}

// ---------------------------------------------------------------------------------------------
// cotangent_weights and mesh_laplacian (the mesh regulariser; no counterpart in the reference's library)
// ---------------------------------------------------------------------------------------------
Tensor cot_weights_forward(const Tensor& v, const Incidence& inc) {
  const int64_t N = v.size(0);
  auto w = out_empty({N, inc.F, 3}, v.options());
  check_status(drtk_amd_geometry_cot_weights(dtype_of(v, "cotangent_weights"), v.data_ptr(), v.size(1) * 3,
                                             inc.vi32.data_ptr<int32_t>(), vi_stride(inc), N, v.size(1), inc.F,
                                             w.data_ptr(), current_stream(v)),
               "cotangent_weights");
  return w;
}

Tensor cotangent_weights_hip(const Tensor& v_, const Tensor& vi) {
  c10::hip::OptionalHIPGuardMasqueradingAsCUDA guard(v_.device());
  const Tensor v = prep_v(v_, "cotangent_weights");
  return cot_weights_forward(v, incidence_of(vi, v.size(0), v.size(1), "cotangent_weights"));
}

class CotangentWeightsFunction : public torch::autograd::Function<CotangentWeightsFunction> {
 public:
  static tensor_list forward(AutogradContext* ctx, const Tensor& v_, const Tensor& vi) {
    c10::hip::OptionalHIPGuardMasqueradingAsCUDA guard(v_.device());
    ctx->set_materialize_grads(false);
    const Tensor v = prep_v(v_, "cotangent_weights");
    const Incidence inc = incidence_of(vi, v.size(0), v.size(1), "cotangent_weights");
    ctx->save_for_backward({v});
    save_requires_grad(ctx, v_, Tensor());
    save_incidence(ctx, "", inc);
    at::AutoDispatchBelowADInplaceOrView g;
    return {cot_weights_forward(v, inc)};
  }
  static tensor_list backward(AutogradContext* ctx, tensor_list go) {
    const Tensor v = ctx->get_saved_variables()[0];
    if (!go[0].defined() || !wants(ctx, "v_requires_grad")) return {Tensor(), Tensor()};
    no_double_backward("cotangent_weights_backward");
    c10::hip::OptionalHIPGuardMasqueradingAsCUDA guard(v.device());
    const Incidence inc = load_incidence(ctx, "");
    const Tensor gw = grad_or_undef(go[0], v);
    const int64_t N = v.size(0);
    auto pos = out_empty({N, inc.F, 3, 3}, v.options());
    check_status(drtk_amd_geometry_cot_weights_backward(
                     dtype_of(v, "cotangent_weights_backward"), v.data_ptr(), v.size(1) * 3,
                     inc.vi32.data_ptr<int32_t>(), vi_stride(inc), N, v.size(1), inc.F, gw.data_ptr(), pos.data_ptr(),
                     current_stream(v)),
                 "cotangent_weights_backward");
    return {vertex_gather(pos, true, 3, inc, N, false, nullptr, "cotangent_weights_backward"), Tensor()};
  }
};
Tensor cotangent_weights_autograd(const Tensor& v, const Tensor& vi) {
  return CotangentWeightsFunction::apply(v, vi)[0];
}

// x [N,V,C] and the weights the kernels read: undefined (uniform), or [B,F,3] contiguous in x's dtype with B = 1 or N
// (a stride-0 expand counts as 1)
struct LaplacianArgs {
  Tensor x, w;
  Incidence inc;
};
LaplacianArgs laplacian_prep(const Tensor& x_, const Tensor& vi, const c10::optional<Tensor>& weights) {
  const char* op = "mesh_laplacian";
  LaplacianArgs a;
  TORCH_CHECK(x_.is_cuda(), op, "(): drtk_amd implements the MI355X (HIP) path only; got CPU tensors");
  TORCH_CHECK(x_.dim() == 3 && x_.size(2) >= 1, op, "(): expected x of shape [N, V, C] with C >= 1");
  dtype_of(x_, op);
  a.x = x_.contiguous();
  const int64_t N = a.x.size(0);
  a.inc = incidence_of(vi, N, a.x.size(1), op);
  if (weights.has_value() && weights->defined()) {
    Tensor w = weights->dim() == 2 ? weights->unsqueeze(0) : *weights;
    TORCH_CHECK(w.dim() == 3 && w.size(1) == a.inc.F && w.size(2) == 3 && (w.size(0) == 1 || w.size(0) == N), op,
                "(): expected weights of shape [F, 3], [1, F, 3] or [N, F, 3]");
    if (w.size(0) > 1 && w.stride(0) == 0) w = w.narrow(0, 0, 1);
    a.w = like_v(w, a.x, op, "weights");
  }
  return a;
}

Tensor laplacian_apply(const Tensor& x, const Tensor& w, const Incidence& inc, const char* op) {
  const drtk_dtype_t dt = dtype_of(x, op);
  const int64_t N = x.size(0), C = x.size(2);
  auto out = out_empty({N, inc.V, C}, x.options());
  size_t bytes = 0;
  check_status(drtk_amd_geometry_laplacian_workspace_bytes(dt, N, inc.B, inc.csr.C, C, &bytes), op);
  Tensor ws = bytes ? alloc_workspace(bytes, x) : Tensor();
  const bool chunks = inc.csr.C > 0;
  check_status(
      drtk_amd_geometry_laplacian(
          dt, x.data_ptr(), C, inc.vi32.data_ptr<int32_t>(), vi_stride(inc), ptr_or_null(w),
          w.defined() && w.size(0) > 1 ? inc.F * 3 : 0, inc.csr.crow.data_ptr<int32_t>(), inc.entries.data_ptr<int32_t>(),
          chunks ? inc.csr.chunk_ptr.data_ptr<int32_t>() : nullptr, chunks ? inc.csr.chunk_begin.data_ptr<int32_t>() : nullptr,
          chunks ? inc.csr.chunk_row.data_ptr<int32_t>() : nullptr, inc.csr.C, inc.B, N, inc.V, inc.F, out.data_ptr(),
          ws.defined() ? ws.data_ptr() : nullptr, bytes, current_stream(x)),
      op);
  return out;
}

Tensor mesh_laplacian_hip(const Tensor& x, const Tensor& vi, const c10::optional<Tensor>& weights) {
  c10::hip::OptionalHIPGuardMasqueradingAsCUDA guard(x.device());
  const LaplacianArgs a = laplacian_prep(x, vi, weights);
  return laplacian_apply(a.x, a.w, a.inc, "mesh_laplacian");
}

class MeshLaplacianFunction : public torch::autograd::Function<MeshLaplacianFunction> {
 public:
  static tensor_list forward(AutogradContext* ctx, const Tensor& x, const Tensor& vi,
                             const c10::optional<Tensor>& weights) {
    c10::hip::OptionalHIPGuardMasqueradingAsCUDA guard(x.device());
    ctx->set_materialize_grads(false);
    const LaplacianArgs a = laplacian_prep(x, vi, weights);
    const bool has_w = a.w.defined();
    const bool need_w = has_w && weights->requires_grad();
    ctx->save_for_backward({need_w ? a.x : Tensor(), a.w});
    ctx->saved_data["x_requires_grad"] = x.requires_grad();
    ctx->saved_data["w_requires_grad"] = need_w;
    if (has_w) {
      // the gradient takes the shape and dtype of the weights as they were passed (an expanded [N,F,3] gets per-view rows)
      ctx->saved_data["w_sizes"] = weights->sizes().vec();
      ctx->saved_data["w_dtype"] = static_cast<int64_t>(weights->scalar_type());
    }
    save_incidence(ctx, "", a.inc);
    at::AutoDispatchBelowADInplaceOrView g;
    return {laplacian_apply(a.x, a.w, a.inc, "mesh_laplacian")};
  }
  static tensor_list backward(AutogradContext* ctx, tensor_list go) {
    const bool need_x = ctx->saved_data["x_requires_grad"].toBool(), need_w = ctx->saved_data["w_requires_grad"].toBool();
    if (!go[0].defined() || !(need_x || need_w)) return {Tensor(), Tensor(), Tensor()};
    no_double_backward("mesh_laplacian_backward");
    c10::hip::OptionalHIPGuardMasqueradingAsCUDA guard(go[0].device());
    const auto saved = ctx->get_saved_variables();
    const Tensor &x = saved[0], &w = saved[1];
    const Incidence inc = load_incidence(ctx, "");
    const Tensor g = go[0].contiguous(); // dtype of x, in which the forward ran
    Tensor gx, gw;
    if (need_x) gx = laplacian_apply(g, w, inc, "mesh_laplacian_backward"); // the operator is symmetric
    if (need_w) {
      const auto sizes = ctx->saved_data["w_sizes"].toIntVector();
      const int64_t N = g.size(0), wB = sizes.size() == 3 ? sizes[0] : 1;
      gw = out_empty({wB, inc.F, 3}, g.options());
      check_status(drtk_amd_geometry_laplacian_grad_weights(
                       dtype_of(g, "mesh_laplacian_backward"), g.data_ptr(), x.data_ptr(), g.size(2),
                       inc.vi32.data_ptr<int32_t>(), vi_stride(inc), N, inc.V, inc.F, wB, gw.data_ptr(), current_stream(g)),
                   "mesh_laplacian_backward");
      gw = gw.view(sizes).to(static_cast<at::ScalarType>(ctx->saved_data["w_dtype"].toInt()));
    }
    return {gx, Tensor(), gw};
  }
};
Tensor mesh_laplacian_autograd(const Tensor& x, const Tensor& vi, const c10::optional<Tensor>& weights) {
  return MeshLaplacianFunction::apply(x, vi, weights)[0];
}

// ---------------------------------------------------------------------------------------------
// incidence and cache (extension)
// ---------------------------------------------------------------------------------------------
std::tuple<Tensor, Tensor> vertex_incidence(const Tensor& vi, int64_t num_vertices) {
  TORCH_CHECK(vi.dim() == 2 || vi.dim() == 3, "vertex_incidence(): expected vi of shape [F,3] or [B,F,3]");
  const Incidence inc = incidence_of(vi, vi.dim() == 3 ? vi.size(0) : 1, num_vertices, "vertex_incidence");
  return {inc.csr.crow, inc.entries};
}
std::vector<int64_t> geometry_cache_stats() {
  return incidence_cache().stats();
}
void geometry_cache_clear() {
  incidence_cache().clear();
}

Tensor3 face_info_cpu(const Tensor&, const Tensor&, bool, bool, bool) {
  no_cpu("face_info");
}
Tensor vert_normals_cpu(const Tensor&, const Tensor&, const c10::optional<Tensor>&) {
  no_cpu("vert_normals");
}
Tensor face_attribute_to_vert_cpu(const Tensor&, const Tensor&, const Tensor&) {
  no_cpu("face_attribute_to_vert");
}
std::tuple<Tensor, Tensor> face_dpdt_cpu(const Tensor&, const Tensor&, const Tensor&, const Tensor&) {
  no_cpu("face_dpdt");
}
Tensor vert_binormals_cpu(const Tensor&, const Tensor&, const Tensor&, const Tensor&) {
  no_cpu("vert_binormals");
}
Tensor cotangent_weights_cpu(const Tensor&, const Tensor&) {
  no_cpu("cotangent_weights");
}
Tensor mesh_laplacian_cpu(const Tensor&, const Tensor&, const c10::optional<Tensor>&) {
  no_cpu("mesh_laplacian");
}

} // namespace

TORCH_LIBRARY_FRAGMENT(drtk_amd_ext, m) {
  m.def("face_info(Tensor v, Tensor vi, bool normals, bool areas, bool edges) -> (Tensor, Tensor, Tensor)");
  m.def("vert_normals(Tensor v, Tensor vi, Tensor? fnorms=None) -> Tensor");
  m.def("face_attribute_to_vert(Tensor v, Tensor vi, Tensor attr) -> Tensor");
  m.def("face_dpdt(Tensor v, Tensor vt, Tensor vi, Tensor vti) -> (Tensor, Tensor)");
  m.def("vert_binormals(Tensor v, Tensor vt, Tensor vi, Tensor vti) -> Tensor");
  m.def("cotangent_weights(Tensor v, Tensor vi) -> Tensor");
  m.def("mesh_laplacian(Tensor x, Tensor vi, Tensor? weights=None) -> Tensor");
  m.def("vertex_incidence(Tensor vi, int num_vertices) -> (Tensor, Tensor)", &vertex_incidence);
  m.def("geometry_cache_stats() -> int[]", &geometry_cache_stats);
  m.def("geometry_cache_clear() -> ()", &geometry_cache_clear);
}
TORCH_LIBRARY_IMPL(drtk_amd_ext, Autograd, m) {
  m.impl("face_info", &face_info_autograd);
  m.impl("vert_normals", &vert_normals_autograd);
  m.impl("face_attribute_to_vert", &face_attribute_to_vert_autograd);
  m.impl("face_dpdt", &face_dpdt_autograd);
  m.impl("vert_binormals", &vert_binormals_autograd);
  m.impl("cotangent_weights", &cotangent_weights_autograd);
  m.impl("mesh_laplacian", &mesh_laplacian_autograd);
}
TORCH_LIBRARY_IMPL(drtk_amd_ext, CUDA, m) {
  m.impl("face_info", &face_info_hip);
  m.impl("vert_normals", &vert_normals_hip);
  m.impl("face_attribute_to_vert", &face_attribute_to_vert_hip);
  m.impl("face_dpdt", &face_dpdt_hip);
  m.impl("vert_binormals", &vert_binormals_hip);
  m.impl("cotangent_weights", &cotangent_weights_hip);
  m.impl("mesh_laplacian", &mesh_laplacian_hip);
}
TORCH_LIBRARY_IMPL(drtk_amd_ext, CPU, m) {
  m.impl("face_info", &face_info_cpu);
  m.impl("vert_normals", &vert_normals_cpu);
  m.impl("face_attribute_to_vert", &face_attribute_to_vert_cpu);
  m.impl("face_dpdt", &face_dpdt_cpu);
  m.impl("vert_binormals", &vert_binormals_cpu);
  m.impl("cotangent_weights", &cotangent_weights_cpu);
  m.impl("mesh_laplacian", &mesh_laplacian_cpu);
}
