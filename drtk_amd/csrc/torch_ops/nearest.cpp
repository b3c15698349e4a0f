// drtk_amd_ext::nearest_points -- closest-point queries over drtk_amd_nearest_* (csrc/nearest.hip): the squared distance to,
// and the index of, the nearest target of every query point, and the gradients to both point sets without atomics.  The
// gradient to the targets is a many-to-few reduction through the STABLE sort of the indices, which change every step: the
// sort runs here on the device (at::sort, stable), only when that gradient is asked for, with no host read.
#include "common.hpp"

namespace {
using namespace drtk_amd_torch;

// What the kernels read of one point set: [B,count,3], B = 1 (shared by the views: a batch of 1, a 2-D tensor or a stride-0
// expand, read as one row) or N.  Read in place where a point is 3 consecutive elements and rows and views do not overlap
// (a [..., :3] slice of an [N,P,4] or [N,P,6] tensor, a slice of views); copied otherwise.
struct Points {
  Tensor t;
  int64_t B = 1, count = 0, sN = 0, sP = 3;
};
Points prep_points(const Tensor& x_, const char* name) {
  const char* op = "nearest_points";
  TORCH_CHECK(x_.defined() && x_.layout() == at::kStrided, op, "(): expected ", name, " to be a strided tensor");
  TORCH_CHECK((x_.dim() == 2 || x_.dim() == 3) && x_.size(-1) == 3, op, "(): expected ", name, " of shape [N, P, 3], [1, P, 3] or [P, 3]");
  Tensor x = x_.dim() == 2 ? x_.unsqueeze(0) : x_;
  if (x.size(0) > 1 && x.stride(0) == 0) x = x.narrow(0, 0, 1);
  Points a;
  a.B = x.size(0), a.count = x.size(1);
  const int64_t row = a.count > 1 ? x.stride(1) : 0;
  const bool in_place = x.stride(2) == 1 && (a.count <= 1 || row >= 3) && (a.B <= 1 || x.stride(0) >= (a.count - 1) * row + 3);
  a.t = in_place ? x : x.contiguous();
  a.sP = a.count > 1 ? a.t.stride(1) : 3;
  a.sN = a.B > 1 ? a.t.stride(0) : 0;
  return a;
}

struct NearestArgs {
  Points p, q;
  int64_t N = 0;
};
NearestArgs nearest_prep(const Tensor& p, const Tensor& q) {
  const char* op = "nearest_points";
  TORCH_CHECK(p.is_cuda(), op, "(): drtk_amd implements the MI355X (HIP) path only; got CPU tensors");
  dtype_of(p, op);
  TORCH_CHECK(q.device() == p.device(), op, "(): expected q on the device of p");
  TORCH_CHECK(q.scalar_type() == p.scalar_type(), op, "(): expected q to have the dtype of p, got ", q.scalar_type(), " for ",
              p.scalar_type());
  NearestArgs a;
  a.p = prep_points(p, "p");
  a.q = prep_points(q, "q");
  // the batch of the tensors as given (a stride-0 expand still says N)
  const int64_t pb = p.dim() == 3 ? p.size(0) : 1, qb = q.dim() == 3 ? q.size(0) : 1;
  a.N = pb == 1 ? qb : pb;
  TORCH_CHECK((pb == a.N || pb == 1) && (qb == a.N || qb == 1), op, "(): expected the batch sizes of p and q to be equal or 1, got ", pb,
              " and ", qb);
  TORCH_CHECK(a.p.count < (int64_t(1) << 31) - DRTK_NEAREST_QUERIES && a.q.count < (int64_t(1) << 31) - DRTK_NEAREST_QUERIES, op,
              "(): too many points for 32-bit indices");
  return a;
}

// -> (dist2 [N,P], idx int32 [N,P])
std::pair<Tensor, Tensor> nearest_apply(const NearestArgs& a) {
  const Tensor& p = a.p.t;
  const int64_t N = a.N, P = a.p.count, M = a.q.count;
  Tensor dist2 = out_empty({N, P}, p.options());
  Tensor idx = out_empty({N, P}, p.options().dtype(at::kInt));
  const drtk_dtype_t dt = dtype_of(p, "nearest_points");
  size_t bytes = 0;
  check_status(drtk_amd_nearest_forward_workspace_bytes(dt, N, P, M, &bytes), "nearest_points");
  Tensor ws;
  if (bytes) ws = alloc_workspace(bytes, p);
  check_status(drtk_amd_nearest_forward(dt, p.data_ptr(), a.p.sN, a.p.sP, a.q.t.data_ptr(), a.q.sN, a.q.sP, N, P, M,
                                        dist2.data_ptr(), idx.data_ptr<int32_t>(), ws.defined() ? ws.data_ptr() : nullptr, bytes,
                                        current_stream(p)),
               "nearest_points");
  return {dist2, idx};
}

std::tuple<Tensor, Tensor> nearest_hip(const Tensor& p, const Tensor& q) {
  c10::hip::OptionalHIPGuardMasqueradingAsCUDA guard(p.device());
  auto r = nearest_apply(nearest_prep(p, q));
  return {r.first, r.second.to(at::kLong)};
}

class NearestFunction : public torch::autograd::Function<NearestFunction> {
 public:
  static tensor_list forward(AutogradContext* ctx, const Tensor& p, const Tensor& q) {
    c10::hip::OptionalHIPGuardMasqueradingAsCUDA guard(p.device());
    ctx->set_materialize_grads(false);
    const NearestArgs a = nearest_prep(p, q);
    at::AutoDispatchBelowADInplaceOrView g;
    auto r = nearest_apply(a);
    ctx->save_for_backward({a.p.t, a.q.t});
    ctx->saved_data["idx"] = r.second;
    ctx->saved_data["need"] = std::vector<int64_t>{p.requires_grad(), q.requires_grad()};
    ctx->saved_data["p_sizes"] = p.sizes().vec();
    ctx->saved_data["q_sizes"] = q.sizes().vec();
    ctx->saved_data["dims"] = std::vector<int64_t>{a.N, a.p.count, a.q.count, a.p.sN, a.p.sP, a.q.sN, a.q.sP};
    Tensor idx64 = r.second.to(at::kLong);
    ctx->mark_non_differentiable({idx64});
    return {r.first, idx64};
  }
  static tensor_list backward(AutogradContext* ctx, tensor_list go) {
    const auto need = ctx->saved_data["need"].toIntVector();
    if (!go[0].defined() || !(need[0] || need[1])) return {Tensor(), Tensor()};
    // the backward passes are kernels, not differentiable graphs: their second-order terms would be silently zero
    TORCH_CHECK(!at::GradMode::is_enabled(), "nearest_points_backward(): double backward (create_graph=True) is not supported by "
                "drtk_amd's closest-point kernels; the PyTorch formulation (CPU tensors) supports it");
    c10::hip::OptionalHIPGuardMasqueradingAsCUDA guard(go[0].device());
    const auto saved = ctx->get_saved_variables();
    const Tensor &p = saved[0], &q = saved[1];
    const Tensor idx = ctx->saved_data["idx"].toTensor();
    const auto d = ctx->saved_data["dims"].toIntVector();
    const int64_t N = d[0], P = d[1], M = d[2];
    const auto p_sizes = ctx->saved_data["p_sizes"].toIntVector();
    const auto q_sizes = ctx->saved_data["q_sizes"].toIntVector();
    const int64_t gp_B = p_sizes.size() == 3 ? p_sizes[0] : 1, gq_B = q_sizes.size() == 3 ? q_sizes[0] : 1;
    const Tensor g = go[0].contiguous(); // dtype of p, in which the forward ran
    const drtk_dtype_t dt = dtype_of(g, "nearest_points_backward");
    Tensor gp, gq, order, ws;
    size_t bytes = 0;
    if (need[0]) gp = out_empty({gp_B, P, 3}, g.options());
    if (need[1]) {
      gq = out_empty({gq_B, M, 3}, g.options());
      // per view the stable ascending sort of the indices: equal targets keep ascending i, the -1 rows come first
      order = std::get<1>(at::sort(idx, /*stable=*/true, /*dim=*/1, /*descending=*/false)).to(at::kInt);
      check_status(drtk_amd_nearest_backward_workspace_bytes(dt, N, P, M, 1, &bytes), "nearest_points_backward");
      if (bytes) ws = alloc_workspace(bytes, g);
    }
    // (an empty gradient has no storage to hand over, and nothing to compute)
    const bool work = (gp.defined() && gp.numel() > 0) || (gq.defined() && gq.numel() > 0);
    if (work) {
      check_status(drtk_amd_nearest_backward(dt, g.data_ptr(), p.data_ptr(), d[3], d[4], q.data_ptr(), d[5], d[6],
                                             idx.data_ptr<int32_t>(), order.defined() ? order.data_ptr<int32_t>() : nullptr, N, P,
                                             M, gp_B, gp.defined() ? gp.data_ptr() : nullptr, gq_B,
                                             gq.defined() ? gq.data_ptr() : nullptr, ws.defined() ? ws.data_ptr() : nullptr,
                                             bytes, current_stream(g)),
                   "nearest_points_backward");
    }
    if (gp.defined()) gp = gp.view(p_sizes);
    if (gq.defined()) gq = gq.view(q_sizes);
    return {gp, gq};
  }
};
std::tuple<Tensor, Tensor> nearest_autograd(const Tensor& p, const Tensor& q) {
  auto r = NearestFunction::apply(p, q);
  return {r[0], r[1]};
}
std::tuple<Tensor, Tensor> nearest_cpu(const Tensor&, const Tensor&) {
  no_cpu("nearest_points");
}

} // namespace

TORCH_LIBRARY_FRAGMENT(drtk_amd_ext, m) {
  m.def("nearest_points(Tensor p, Tensor q) -> (Tensor, Tensor)");
}
TORCH_LIBRARY_IMPL(drtk_amd_ext, Autograd, m) {
  m.impl("nearest_points", &nearest_autograd);
}
TORCH_LIBRARY_IMPL(drtk_amd_ext, CUDA, m) {
  m.impl("nearest_points", &nearest_hip);
}
TORCH_LIBRARY_IMPL(drtk_amd_ext, CPU, m) {
  m.impl("nearest_points", &nearest_cpu);
}
