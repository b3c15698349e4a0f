// drtk_amd_ext::forward_kinematics -- pose to skinning transforms over drtk_amd_kinematics_* (csrc/kinematics.hip): the
// matrices `skin` reads and the posed joints, and the gradients to the rotations, the rest joints and the root
// translation, one launch each way.  The SCHEDULE of the parent list (joints by level, children in CSR form) is built on
// the host with one read of `parents` and cached (topology_cache.hpp): a tensor by its identity, a Python sequence by its
// contents, either with the device the schedule lives on.
#include "topology_cache.hpp"

#include <algorithm>
#include <array>

namespace {
using namespace drtk_amd_torch;

struct Schedule {
  Tensor pack; // int32 on the device: parents [J] | order [J] | level_start [D+1] | child_crow [J+1] | child_entries [J-roots]
  int64_t J = 0, D = 0, roots = 0;
  const int32_t* ptr(int64_t off) const { return pack.data_ptr<int32_t>() + off; }
  const int32_t* parents() const { return ptr(0); }
  const int32_t* order() const { return ptr(J); }
  const int32_t* level_start() const { return ptr(2 * J); }
  const int32_t* child_crow() const { return ptr(2 * J + D + 1); }
  const int32_t* child_entries() const { return ptr(3 * J + D + 2); }
};

Schedule build_schedule(const std::vector<int64_t>& p, const at::Device& device, const char* op) {
  Schedule s;
  const int64_t J = static_cast<int64_t>(p.size());
  s.J = J;
  std::vector<int32_t> depth(J, 0);
  for (int64_t j = 0; j < J; ++j) {
    TORCH_CHECK_VALUE(p[j] == -1 || (p[j] >= 0 && p[j] < j), op, "(): expected parents[j] == -1 (a root) or 0 <= parents[j] < j, got parents[",
                      j, "] = ", p[j]);
    depth[j] = p[j] < 0 ? 0 : depth[p[j]] + 1;
    s.D = std::max<int64_t>(s.D, depth[j] + 1);
    s.roots += p[j] < 0;
  }
  std::vector<int32_t> h(static_cast<size_t>(4 * J + s.D + 2 - s.roots), 0);
  int32_t* parents = h.data();
  int32_t* order = parents + J;
  int32_t* level_start = order + J;
  int32_t* child_crow = level_start + s.D + 1;
  int32_t* child_entries = child_crow + J + 1;
  for (int64_t j = 0; j < J; ++j) {
    parents[j] = static_cast<int32_t>(p[j]);
    ++level_start[depth[j] + 1];
    if (p[j] >= 0) ++child_crow[p[j] + 1];
  }
  for (int64_t l = 0; l < s.D; ++l) level_start[l + 1] += level_start[l];
  for (int64_t j = 0; j < J; ++j) child_crow[j + 1] += child_crow[j];
  std::vector<int32_t> lfill(level_start, level_start + s.D + 1), cfill(child_crow, child_crow + J + 1);
  for (int64_t j = 0; j < J; ++j) { // ascending j: a level's joints and a joint's children come out ascending
    order[lfill[depth[j]]++] = static_cast<int32_t>(j);
    if (p[j] >= 0) child_entries[cfill[p[j]]++] = static_cast<int32_t>(j);
  }
  s.pack = at::tensor(h, at::TensorOptions().dtype(at::kInt)).to(device);
  return s;
}

PinnedLruCache<Schedule>& schedule_cache() {
  static PinnedLruCache<Schedule> c;
  return c;
}

// key: [0, ...identity of the tensor...] or [1, ...contents of the sequence...], then the device the schedule lives on
Schedule schedule_of(const std::optional<Tensor>& pt, at::IntArrayRef pl, const at::Device& device, const char* op) {
  CacheKey key;
  if (pt.has_value()) {
    const Tensor& t = *pt;
    TORCH_CHECK_VALUE(t.layout() == at::kStrided && t.dim() == 1, op, "(): expected parents of shape [J]");
    TORCH_CHECK_TYPE(t.scalar_type() == at::kInt || t.scalar_type() == at::kLong, op,
                     "(): expected parents to be int32 or int64, got ", t.scalar_type());
    key.push_back(0);
    append_tensor_identity(key, t);
  } else {
    key.reserve(pl.size() + 3);
    key.push_back(1);
    key.insert(key.end(), pl.begin(), pl.end());
  }
  key.push_back(static_cast<int64_t>(device.type()));
  key.push_back(static_cast<int64_t>(device.index()));
  return schedule_cache().get(key, pt.has_value() ? *pt : Tensor(), [&] {
    check_not_capturing(device, op, "kinematic schedule of this parent list", "parents");
    std::vector<int64_t> p;
    if (pt.has_value()) {
      const Tensor host = pt->detach().to(at::kCPU, at::kLong).contiguous(); // the one host read
      p.assign(host.data_ptr<int64_t>(), host.data_ptr<int64_t>() + host.numel());
    } else {
      p.assign(pl.begin(), pl.end());
    }
    return build_schedule(p, device, op);
  });
}

// What the kernels read.  The rotations in place through their strides; the joints as one row [J,3] (c_sN = 0) or N.
struct FkArgs {
  Tensor rot, joints, tr;
  Schedule sched;
  int64_t N = 0, J = 0, c_sN = 0, joints_B = 1;
  int mat = 0;
  std::array<int64_t, 4> rs{{0, 0, 0, 0}};
};
FkArgs fk_prep(const Tensor& rot, const Tensor& joints_, const std::optional<Tensor>& pt, at::IntArrayRef pl,
               const std::optional<Tensor>& tr) {
  const char* op = "forward_kinematics";
  FkArgs a;
  TORCH_CHECK(rot.is_cuda(), op, "(): drtk_amd implements the MI355X (HIP) path only; got CPU tensors");
  dtype_of(rot, op);
  TORCH_CHECK((rot.dim() == 3 && rot.size(2) == 3) || (rot.dim() == 4 && rot.size(2) == 3 && rot.size(3) == 3), op,
              "(): expected rotations of shape [N, J, 3] or [N, J, 3, 3]");
  a.N = rot.size(0), a.J = rot.size(1), a.mat = rot.dim() == 4;
  TORCH_CHECK(a.J <= DRTK_FK_MAX_JOINTS, op, "(): expected at most ", DRTK_FK_MAX_JOINTS, " joints on the kernel route, got ", a.J);
  TORCH_CHECK((joints_.dim() == 2 || joints_.dim() == 3) && joints_.size(-1) == 3 && joints_.size(-2) == a.J &&
                  (joints_.dim() == 2 || joints_.size(0) == 1 || joints_.size(0) == a.N),
              op, "(): expected joints of shape [J, 3], [1, J, 3] or [N, J, 3] with J = ", a.J);
  TORCH_CHECK(joints_.device() == rot.device() && joints_.scalar_type() == rot.scalar_type(), op,
              "(): expected joints on the device and in the dtype of rotations");
  a.rot = rot;
  for (int d = 0; d < rot.dim(); ++d) a.rs[d] = rot.stride(d);
  Tensor c = joints_.dim() == 2 ? joints_.unsqueeze(0) : joints_;
  a.joints_B = c.size(0);
  if (c.size(0) > 1 && c.stride(0) == 0) c = c.narrow(0, 0, 1); // a stride-0 expand is read as one row
  a.joints = c.contiguous();
  a.c_sN = a.joints.size(0) == 1 ? 0 : a.J * 3;
  if (tr.has_value()) {
    TORCH_CHECK(tr->dim() == 2 && tr->size(0) == a.N && tr->size(1) == 3, op, "(): expected translation of shape [N, 3]");
    TORCH_CHECK(tr->device() == rot.device() && tr->scalar_type() == rot.scalar_type(), op,
                "(): expected translation on the device and in the dtype of rotations");
    a.tr = tr->contiguous();
  }
  a.sched = schedule_of(pt, pl, rot.device(), op);
  TORCH_CHECK_VALUE(a.sched.J == a.J, op, "(): expected parents of length J = ", a.J, ", got ", a.sched.J);
  return a;
}

std::tuple<Tensor, Tensor> fk_apply(const FkArgs& a) {
  auto transforms = out_empty({a.N, a.J, 3, 4}, a.rot.options());
  auto posed = out_empty({a.N, a.J, 3}, a.rot.options());
  check_status(drtk_amd_kinematics_forward(dtype_of(a.rot, "forward_kinematics"), a.rot.data_ptr(), a.mat, a.rs.data(),
                                           a.joints.data_ptr(), a.c_sN, a.tr.defined() ? a.tr.data_ptr() : nullptr,
                                           a.sched.parents(), a.sched.order(), a.sched.level_start(), a.sched.D, a.N, a.J,
                                           transforms.data_ptr(), posed.data_ptr(), current_stream(a.rot)),
               "forward_kinematics");
  return {transforms, posed};
}

std::tuple<Tensor, Tensor> fk_hip(const Tensor& rot, const Tensor& joints, const std::optional<Tensor>& pt,
                                  at::IntArrayRef pl, const std::optional<Tensor>& tr) {
  c10::hip::OptionalHIPGuardMasqueradingAsCUDA guard(rot.device());
  return fk_apply(fk_prep(rot, joints, pt, pl, tr));
}

class FkFunction : public torch::autograd::Function<FkFunction> {
 public:
  static tensor_list forward(AutogradContext* ctx, const Tensor& rot, const Tensor& joints, const std::optional<Tensor>& pt,
                             std::vector<int64_t> pl, const std::optional<Tensor>& tr) {
    c10::hip::OptionalHIPGuardMasqueradingAsCUDA guard(rot.device());
    ctx->set_materialize_grads(false);
    const FkArgs a = fk_prep(rot, joints, pt, pl, tr);
    ctx->save_for_backward({a.rot, a.joints, a.tr.defined() ? a.tr : Tensor()});
    // decided on the inputs as passed: the copies the kernels read never require grad
    ctx->saved_data["need"] = std::vector<int64_t>{rot.requires_grad(), joints.requires_grad(), tr.has_value() && tr->requires_grad()};
    ctx->saved_data["joint_sizes"] = joints.sizes().vec();
    ctx->saved_data["dims"] = std::vector<int64_t>{a.N, a.J, a.c_sN, a.mat, a.sched.D, a.sched.roots, a.joints_B, a.rs[0], a.rs[1], a.rs[2], a.rs[3]};
    ctx->saved_data["schedule"] = a.sched.pack;
    at::AutoDispatchBelowADInplaceOrView g;
    const auto out = fk_apply(a);
    return {std::get<0>(out), std::get<1>(out)};
  }
  static tensor_list backward(AutogradContext* ctx, tensor_list go) {
    const auto need = ctx->saved_data["need"].toIntVector();
    if ((!go[0].defined() && !go[1].defined()) || !(need[0] || need[1] || need[2]))
      return {Tensor(), Tensor(), Tensor(), Tensor(), Tensor()};
    // the backward pass is a kernel, not a differentiable graph: its second-order terms would be silently zero
    TORCH_CHECK(!at::GradMode::is_enabled(), "forward_kinematics_backward(): double backward (create_graph=True) is not "
                "supported by drtk_amd's kinematics kernels; the PyTorch formulation (CPU tensors) supports it");
    const auto saved = ctx->get_saved_variables();
    const Tensor &rot = saved[0], &joints = saved[1], &tr = saved[2];
    c10::hip::OptionalHIPGuardMasqueradingAsCUDA guard(rot.device());
    const auto d = ctx->saved_data["dims"].toIntVector();
    const int64_t N = d[0], J = d[1], c_sN = d[2], mat = d[3], D = d[4], roots = d[5], joints_B = d[6];
    const int64_t rs[4] = {d[7], d[8], d[9], d[10]};
    Schedule sched;
    sched.pack = ctx->saved_data["schedule"].toTensor();
    sched.J = J, sched.D = D, sched.roots = roots;
    Tensor gA, gP; // in the dtype of the rotations, in which the forward ran; an absent one is zero and is not allocated
    if (go[0].defined()) gA = go[0].contiguous();
    if (go[1].defined()) gP = go[1].contiguous();
    const auto opts = rot.options();
    Tensor gr, gc, gt, ws;
    if (need[0]) gr = mat ? out_empty({N, J, 3, 3}, opts) : out_empty({N, J, 3}, opts);
    // a per-view or an expanded rest pose: one row per view (autograd adds an expand's rows); one row: the rows added here
    const int64_t gc_B = joints_B == 1 ? 1 : N;
    if (need[1]) gc = out_empty({gc_B, J, 3}, opts);
    if (need[2]) gt = out_empty({N, 3}, opts);
    size_t bytes = 0;
    const drtk_dtype_t dt = dtype_of(rot, "forward_kinematics_backward");
    check_status(drtk_amd_kinematics_backward_workspace_bytes(dt, N, J, need[1] ? gc_B : 0, &bytes), "forward_kinematics_backward");
    if (bytes) ws = alloc_workspace(bytes, rot);
    check_status(drtk_amd_kinematics_backward(
                     dt, gA.defined() ? gA.data_ptr() : nullptr, gP.defined() ? gP.data_ptr() : nullptr, rot.data_ptr(),
                     static_cast<int>(mat), rs, joints.data_ptr(), c_sN, tr.defined() ? tr.data_ptr() : nullptr, sched.parents(),
                     sched.order(), sched.level_start(), D, sched.child_crow(), sched.child_entries(), N, J,
                     gr.defined() ? gr.data_ptr() : nullptr, gc_B, gc.defined() ? gc.data_ptr() : nullptr,
                     gt.defined() ? gt.data_ptr() : nullptr, ws.defined() ? ws.data_ptr() : nullptr, bytes, current_stream(rot)),
                 "forward_kinematics_backward");
    if (gc.defined()) gc = gc.view(ctx->saved_data["joint_sizes"].toIntVector());
    return {gr, gc, Tensor(), Tensor(), gt};
  }
};
std::tuple<Tensor, Tensor> fk_autograd(const Tensor& rot, const Tensor& joints, const std::optional<Tensor>& pt,
                                       at::IntArrayRef pl, const std::optional<Tensor>& tr) {
  const auto out = FkFunction::apply(rot, joints, pt, pl.vec(), tr);
  return {out[0], out[1]};
}
std::tuple<Tensor, Tensor> fk_cpu(const Tensor&, const Tensor&, const std::optional<Tensor>&, at::IntArrayRef,
                                  const std::optional<Tensor>&) {
  no_cpu("forward_kinematics");
}

// (order [J], level_start [D+1], child_crow [J+1], child_entries) of the cached schedule, on the HIP device `device_index`
std::tuple<Tensor, Tensor, Tensor, Tensor> kinematic_schedule(const std::optional<Tensor>& pt, at::IntArrayRef pl, int64_t device_index) {
  const at::Device device(at::kCUDA, static_cast<c10::DeviceIndex>(device_index));
  c10::hip::OptionalHIPGuardMasqueradingAsCUDA guard(device);
  const Schedule s = schedule_of(pt, pl, device, "kinematic_schedule");
  const int64_t J = s.J, D = s.D;
  return {s.pack.narrow(0, J, J), s.pack.narrow(0, 2 * J, D + 1), s.pack.narrow(0, 2 * J + D + 1, J + 1),
          s.pack.narrow(0, 3 * J + D + 2, J - s.roots)};
}
std::vector<int64_t> kinematics_cache_stats() {
  return schedule_cache().stats();
}
void kinematics_cache_clear() {
  schedule_cache().clear();
}

} // namespace

TORCH_LIBRARY_FRAGMENT(drtk_amd_ext, m) {
  m.def("forward_kinematics(Tensor rotations, Tensor joints, Tensor? parents, int[] parents_list, Tensor? translation) -> (Tensor, Tensor)");
  m.def("kinematic_schedule(Tensor? parents, int[] parents_list, int device_index) -> (Tensor, Tensor, Tensor, Tensor)", &kinematic_schedule);
  m.def("kinematics_cache_stats() -> int[]", &kinematics_cache_stats);
  m.def("kinematics_cache_clear() -> ()", &kinematics_cache_clear);
}
TORCH_LIBRARY_IMPL(drtk_amd_ext, Autograd, m) {
  m.impl("forward_kinematics", &fk_autograd);
}
TORCH_LIBRARY_IMPL(drtk_amd_ext, CUDA, m) {
  m.impl("forward_kinematics", &fk_hip);
}
TORCH_LIBRARY_IMPL(drtk_amd_ext, CPU, m) {
  m.impl("forward_kinematics", &fk_cpu);
}
