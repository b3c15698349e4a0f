// drtk_amd_ext::skin -- linear blend skinning over drtk_amd_skin_* (csrc/skin.hip): the posed vertices and the gradients
// to the rest pose, the weights and the joint transforms, without float atomics.  The gradient to the transforms is a
// many-to-few reduction through the JOINT INCIDENCE of joint_idx (CSR over joints, every row chunked), built here with
// ATen where joint_idx lives and cached by the tensor's identity and the joint count (topology_cache.hpp).
#include "topology_cache.hpp"

namespace {
using namespace drtk_amd_torch;

constexpr int64_t kChunk = DRTK_SKIN_CHUNK;

// The chunked CSR over joints of the slots' joints, every row cut into chunks; an empty slot (-1) is keyed J, so it
// sorts behind every joint and belongs to no row.  Entries i*K+k ascending within a joint.  An index outside [-1, J) would
// make the kernels read out of bounds.
struct JointIncidence {
  Tensor idx32; // int32 [V,K] contiguous
  Tensor entries; // int32 [V*K] (the first crow[J] are entries; the rest are the empty slots)
  ChunkedCsr csr; // rows J; chunk_row is the joint of each chunk
  int64_t V = 0, K = 0, J = 0;
};

JointIncidence build_joint_incidence(const Tensor& t, int64_t J, const char* op) {
  JointIncidence inc;
  inc.V = t.size(0), inc.K = t.size(1), inc.J = J;
  const int64_t E = inc.V * inc.K;
  TORCH_CHECK(J >= 0 && J < (int64_t(1) << 27) && E < (int64_t(1) << 31), op, "(): mesh too large for int32 joint incidence");
  inc.idx32 = t.detach().to(at::kInt).contiguous();
  const Tensor tl = t.detach().to(at::kLong).contiguous().reshape({-1});
  inc.csr = build_chunked_csr(at::where(tl < 0, at::full_like(tl, J), tl), J, kChunk, /*chunk_every_row=*/true, tl);
  TORCH_CHECK(E == 0 || (inc.csr.lo >= -1 && inc.csr.hi < J), op, "(): joint_idx contains a joint index outside [-1, ", J, ")");
  inc.entries = inc.csr.perm.to(at::kInt);
  inc.csr.perm.reset();
  return inc;
}

PinnedLruCache<JointIncidence>& joint_incidence_cache() {
  static PinnedLruCache<JointIncidence> c;
  return c;
}

JointIncidence joint_incidence_of(const Tensor& idx, int64_t J, const char* op) {
  TORCH_CHECK(idx.defined() && idx.layout() == at::kStrided, op, "(): expected joint_idx to be a strided tensor");
  TORCH_CHECK(idx.scalar_type() == at::kInt || idx.scalar_type() == at::kLong, op,
              "(): expected joint_idx to be int32 or int64, got ", idx.scalar_type());
  TORCH_CHECK(idx.dim() == 2, op, "(): expected joint_idx of shape [V, K]");
  TORCH_CHECK(idx.size(1) >= 1 && idx.size(1) <= DRTK_SKIN_MAX_SLOTS, op, "(): expected 1 <= K <= ", DRTK_SKIN_MAX_SLOTS,
              " slots per vertex, got K = ", idx.size(1));
  CacheKey key;
  append_tensor_identity(key, idx);
  key.push_back(J);
  return joint_incidence_cache().get(key, idx, [&] {
    check_not_capturing(idx.device(), op, "joint incidence of this index tensor", "joint_idx");
    return build_joint_incidence(idx, J, op);
  });
}

// What the kernels read.  v: one row [V,3] (v_sN = 0) or N of them; transforms: read in place where rows 0..2 of a joint
// are 12 consecutive elements (a [..., :3, :] view of a 4x4 tensor is), copied otherwise.
struct SkinArgs {
  Tensor v, w, t;
  JointIncidence inc;
  int64_t N = 0, V = 0, J = 0, K = 0, v_sN = 0, t_sN = 0, t_sJ = 12;
};
SkinArgs skin_prep(const Tensor& v_, const Tensor& idx, const Tensor& w_, const Tensor& t_) {
  const char* op = "skin";
  SkinArgs a;
  TORCH_CHECK(v_.is_cuda(), op, "(): drtk_amd implements the MI355X (HIP) path only; got CPU tensors");
  dtype_of(v_, op);
  TORCH_CHECK((v_.dim() == 2 || v_.dim() == 3) && v_.size(-1) == 3, op, "(): expected v of shape [N, V, 3], [1, V, 3] or [V, 3]");
  TORCH_CHECK(t_.dim() == 4 && (t_.size(2) == 3 || t_.size(2) == 4) && t_.size(3) == 4, op,
              "(): expected transforms of shape [N, J, 3, 4] or [N, J, 4, 4]");
  TORCH_CHECK(t_.device() == v_.device() && w_.device() == v_.device() && idx.device() == v_.device(), op,
              "(): expected joint_idx, joint_weights and transforms on the device of v");
  TORCH_CHECK(t_.scalar_type() == v_.scalar_type() && w_.scalar_type() == v_.scalar_type(), op,
              "(): expected joint_weights and transforms to have the dtype of v, got ", w_.scalar_type(), " and ",
              t_.scalar_type(), " for ", v_.scalar_type());
  a.N = t_.size(0), a.J = t_.size(1);
  Tensor v = v_.dim() == 2 ? v_.unsqueeze(0) : v_;
  a.V = v.size(1);
  TORCH_CHECK(v.size(0) == 1 || v.size(0) == a.N, op, "(): expected the batch size of v to be 1 or ", a.N, ", got ", v.size(0));
  if (v.size(0) > 1 && v.stride(0) == 0) v = v.narrow(0, 0, 1); // a stride-0 expand is read as one row
  a.v = v.contiguous();
  a.v_sN = a.v.size(0) == 1 ? 0 : a.V * 3;
  a.inc = joint_incidence_of(idx, a.J, op);
  a.K = a.inc.K;
  TORCH_CHECK(a.inc.V == a.V, op, "(): expected joint_idx of shape [V, K] with V = ", a.V, ", got ", a.inc.V);
  TORCH_CHECK(w_.dim() == 2 && w_.size(0) == a.V && w_.size(1) == a.K, op, "(): expected joint_weights of the shape of joint_idx");
  a.w = w_.contiguous();
  const bool in_place = t_.stride(3) == 1 && t_.stride(2) == 4 && (a.J <= 1 || t_.stride(1) >= 12) &&
                        (a.N <= 1 || t_.stride(0) == 0 || t_.stride(0) >= (a.J - 1) * (a.J > 1 ? t_.stride(1) : 0) + 12);
  a.t = in_place ? t_ : t_.contiguous();
  a.t_sJ = a.J > 1 ? a.t.stride(1) : 12;
  a.t_sN = a.N > 1 ? a.t.stride(0) : 0;
  return a;
}

Tensor skin_apply(const SkinArgs& a) {
  auto out = out_empty({a.N, a.V, 3}, a.v.options());
  check_status(drtk_amd_skin_forward(dtype_of(a.v, "skin"), a.v.data_ptr(), a.v_sN, a.inc.idx32.data_ptr<int32_t>(),
                                     a.w.data_ptr(), a.t.data_ptr(), a.t_sN, a.t_sJ, a.N, a.V, a.J, a.K, out.data_ptr(),
                                     current_stream(a.v)),
               "skin");
  return out;
}

Tensor skin_hip(const Tensor& v, const Tensor& idx, const Tensor& w, const Tensor& t) {
  c10::hip::OptionalHIPGuardMasqueradingAsCUDA guard(v.device());
  return skin_apply(skin_prep(v, idx, w, t));
}

class SkinFunction : public torch::autograd::Function<SkinFunction> {
 public:
  static tensor_list forward(AutogradContext* ctx, const Tensor& v, const Tensor& idx, const Tensor& w, const Tensor& t) {
    c10::hip::OptionalHIPGuardMasqueradingAsCUDA guard(v.device());
    ctx->set_materialize_grads(false);
    const SkinArgs a = skin_prep(v, idx, w, t);
    ctx->save_for_backward({a.v, a.w, a.t});
    // decided on the inputs as passed: the copies the kernels read never require grad
    ctx->saved_data["need"] = std::vector<int64_t>{v.requires_grad(), w.requires_grad(), t.requires_grad()};
    ctx->saved_data["v_sizes"] = v.sizes().vec();
    ctx->saved_data["t_rows"] = t.size(2);
    ctx->saved_data["strides"] = std::vector<int64_t>{a.N, a.V, a.J, a.K, a.v_sN, a.t_sN, a.t_sJ};
    ctx->saved_data["idx"] = a.inc.idx32;
    ctx->saved_data["entries"] = a.inc.entries;
    a.inc.csr.save(ctx, "");
    at::AutoDispatchBelowADInplaceOrView g;
    return {skin_apply(a)};
  }
  static tensor_list backward(AutogradContext* ctx, tensor_list go) {
    const auto need = ctx->saved_data["need"].toIntVector();
    if (!go[0].defined() || !(need[0] || need[1] || need[2])) return {Tensor(), Tensor(), Tensor(), Tensor()};
    // the backward passes are kernels, not differentiable graphs: their second-order terms would be silently zero
    TORCH_CHECK(!at::GradMode::is_enabled(), "skin_backward(): double backward (create_graph=True) is not supported by "
                "drtk_amd's skinning kernels; the PyTorch formulation (CPU tensors) supports it");
    c10::hip::OptionalHIPGuardMasqueradingAsCUDA guard(go[0].device());
    const auto saved = ctx->get_saved_variables();
    const Tensor &v = saved[0], &w = saved[1], &t = saved[2];
    const auto s = ctx->saved_data["strides"].toIntVector();
    const int64_t N = s[0], V = s[1], J = s[2], K = s[3], v_sN = s[4], t_sN = s[5], t_sJ = s[6];
    const ChunkedCsr csr = ChunkedCsr::load(ctx, "");
    const Tensor g = go[0].contiguous(); // dtype of v, in which the forward ran
    const auto v_sizes = ctx->saved_data["v_sizes"].toIntVector();
    const int64_t gv_B = v_sizes.size() == 3 ? v_sizes[0] : 1;
    const int64_t rows = ctx->saved_data["t_rows"].toInt();
    Tensor gv, gw, gt, ws;
    if (need[0]) gv = out_empty({gv_B, V, 3}, g.options());
    if (need[1]) gw = out_empty({V, K}, g.options());
    size_t bytes = 0;
    const drtk_dtype_t dt = dtype_of(g, "skin_backward");
    if (need[2]) {
      gt = out_empty({N, J, rows, 4}, g.options());
      check_status(drtk_amd_skin_backward_workspace_bytes(dt, N, csr.C, &bytes), "skin_backward");
      if (bytes) ws = alloc_workspace(bytes, g);
    }
    auto iptr = [&](const char* k) { return ctx->saved_data[k].toTensor().data_ptr<int32_t>(); };
    check_status(
        drtk_amd_skin_backward(
            dt, g.data_ptr(), v.data_ptr(), v_sN, iptr("idx"), w.data_ptr(), t.data_ptr(), t_sN, t_sJ,
            csr.crow.data_ptr<int32_t>(), iptr("entries"), csr.chunk_ptr.data_ptr<int32_t>(),
            csr.chunk_begin.data_ptr<int32_t>(), csr.chunk_row.data_ptr<int32_t>(), csr.C, N, V, J, K, gv_B,
            gv.defined() ? gv.data_ptr() : nullptr, gw.defined() ? gw.data_ptr() : nullptr, rows,
            gt.defined() ? gt.data_ptr() : nullptr, ws.defined() ? ws.data_ptr() : nullptr, bytes, current_stream(g)),
        "skin_backward");
    if (gv.defined()) gv = gv.view(v_sizes);
    return {gv, Tensor(), gw, gt};
  }
};
Tensor skin_autograd(const Tensor& v, const Tensor& idx, const Tensor& w, const Tensor& t) {
  return SkinFunction::apply(v, idx, w, t)[0];
}
Tensor skin_cpu(const Tensor&, const Tensor&, const Tensor&, const Tensor&) {
  no_cpu("skin");
}

std::tuple<Tensor, Tensor> joint_incidence(const Tensor& idx, int64_t num_joints) {
  const JointIncidence inc = joint_incidence_of(idx, num_joints, "joint_incidence");
  return {inc.csr.crow, inc.entries};
}
std::vector<int64_t> skin_cache_stats() {
  return joint_incidence_cache().stats();
}
void skin_cache_clear() {
  joint_incidence_cache().clear();
}

} // namespace

TORCH_LIBRARY_FRAGMENT(drtk_amd_ext, m) {
  m.def("skin(Tensor v, Tensor joint_idx, Tensor joint_weights, Tensor transforms) -> Tensor");
  m.def("joint_incidence(Tensor joint_idx, int num_joints) -> (Tensor, Tensor)", &joint_incidence);
  m.def("skin_cache_stats() -> int[]", &skin_cache_stats);
  m.def("skin_cache_clear() -> ()", &skin_cache_clear);
}
TORCH_LIBRARY_IMPL(drtk_amd_ext, Autograd, m) {
  m.impl("skin", &skin_autograd);
}
TORCH_LIBRARY_IMPL(drtk_amd_ext, CUDA, m) {
  m.impl("skin", &skin_hip);
}
TORCH_LIBRARY_IMPL(drtk_amd_ext, CPU, m) {
  m.impl("skin", &skin_cpu);
}
