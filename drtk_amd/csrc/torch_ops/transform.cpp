// drtk_amd_ext::transform_pinhole -- the pinhole case of drtk/transform.py + drtk/utils/projection.py in one kernel each
// way, over drtk_amd_transform_pinhole[_backward]; drtk_amd_ext::transform_distort -- the same with its distortion camera
// models, over drtk_amd_transform_distort[_backward].
#include "common.hpp"

namespace {
using namespace drtk_amd_torch;

// ---------------------------------------------------------------------------------------------
// transform_pinhole -- drtk_amd extension backing the pinhole fast path of drtk_amd.transform
// (reference: pure PyTorch, drtk/transform.py:13-119).  Differentiable with respect to v only.
// ---------------------------------------------------------------------------------------------
struct TransformArgs {
  Tensor v, campos, camrot, focal, princpt;
  int64_t N, V, v_sN;
};
TransformArgs transform_prep(
    const Tensor& v, const Tensor& campos, const Tensor& camrot, const Tensor& focal, const Tensor& princpt) {
  TORCH_CHECK(v.is_cuda(), "transform(): drtk_amd implements the MI355X (HIP) path only; got CPU tensors");
  TORCH_CHECK(v.dim() == 3 && v.size(2) == 3, "transform(): expected v of shape [N, V, 3] or [1, V, 3]");
  const int64_t N = campos.size(0);
  TORCH_CHECK(campos.dim() == 2 && campos.size(1) == 3, "transform(): expected campos of shape [N, 3]");
  TORCH_CHECK(camrot.dim() == 3 && camrot.size(0) == N && camrot.size(1) == 3 && camrot.size(2) == 3,
              "transform(): expected camrot of shape [N, 3, 3]");
  TORCH_CHECK(focal.dim() == 3 && focal.size(0) == N && focal.size(1) == 2 && focal.size(2) == 2,
              "transform(): expected focal of shape [N, 2, 2]");
  TORCH_CHECK(princpt.dim() == 2 && princpt.size(0) == N && princpt.size(1) == 2,
              "transform(): expected princpt of shape [N, 2]");
  TORCH_CHECK(v.size(0) == N || v.size(0) == 1, "transform(): batch size of v must be 1 or match the cameras");
  TransformArgs a;
  const auto dt = v.scalar_type();
  a.v = v.contiguous();
  a.campos = campos.to(dt).contiguous();
  a.camrot = camrot.to(dt).contiguous();
  a.focal = focal.to(dt).contiguous();
  a.princpt = princpt.to(dt).contiguous();
  a.N = N;
  a.V = v.size(1);
  a.v_sN = (v.size(0) == 1 && N != 1) ? 0 : v.size(1) * 3;
  return a;
}

Tensor transform_pinhole_hip(
    const Tensor& v, const Tensor& campos, const Tensor& camrot, const Tensor& focal, const Tensor& princpt) {
  const drtk_dtype_t dt = dtype_of(v, "transform");
  c10::hip::OptionalHIPGuardMasqueradingAsCUDA guard(v.device());
  const TransformArgs a = transform_prep(v, campos, camrot, focal, princpt);
  auto v_pix = out_empty({a.N, a.V, 3}, v.options());
  check_status(
      drtk_amd_transform_pinhole(
          dt, a.v.data_ptr(), a.v_sN, a.campos.data_ptr(), a.camrot.data_ptr(), a.focal.data_ptr(),
          a.princpt.data_ptr(), a.N, a.V, v_pix.data_ptr(), nullptr, current_stream(v)),
      "transform");
  return v_pix;
}

Tensor transform_pinhole_backward_hip(
    const Tensor& v, const Tensor& campos, const Tensor& camrot, const Tensor& focal, const Tensor& princpt,
    const Tensor& grad_v_pix) {
  const drtk_dtype_t dt = dtype_of(v, "transform_backward");
  c10::hip::OptionalHIPGuardMasqueradingAsCUDA guard(v.device());
  const TransformArgs a = transform_prep(v, campos, camrot, focal, princpt);
  const auto g = grad_v_pix.to(v.scalar_type()).contiguous();
  auto grad_v = at::empty_like(a.v); // [1,V,3] (summed over views) or [N,V,3]
  check_status(
      drtk_amd_transform_pinhole_backward(
          dt, a.v.data_ptr(), a.v_sN, a.campos.data_ptr(), a.camrot.data_ptr(), a.focal.data_ptr(),
          a.princpt.data_ptr(), g.data_ptr(), a.N, a.V, grad_v.data_ptr(), current_stream(v)),
      "transform_backward");
  return grad_v;
}

Tensor transform_pinhole_cpu(const Tensor&, const Tensor&, const Tensor&, const Tensor&, const Tensor&) {
  no_cpu("transform");
}

Tensor transform_pinhole_op(
    const Tensor& v, const Tensor& campos, const Tensor& camrot, const Tensor& focal, const Tensor& princpt) {
  static auto op = c10::Dispatcher::singleton()
                       .findSchemaOrThrow("drtk_amd_ext::transform_pinhole", "")
                       .typed<decltype(transform_pinhole_op)>();
  return op.call(v, campos, camrot, focal, princpt);
}

class TransformPinholeFunction : public torch::autograd::Function<TransformPinholeFunction> {
 public:
  static tensor_list forward(
      AutogradContext* ctx, const Tensor& v, const Tensor& campos, const Tensor& camrot, const Tensor& focal,
      const Tensor& princpt) {
    ctx->set_materialize_grads(false);
    ctx->save_for_backward({v, campos, camrot, focal, princpt});
    at::AutoDispatchBelowADInplaceOrView g;
    return {transform_pinhole_op(v, campos, camrot, focal, princpt)};
  }
  static tensor_list backward(AutogradContext* ctx, tensor_list grad_outputs) {
    const auto saved = ctx->get_saved_variables();
    if (!saved[0].requires_grad() || !grad_outputs[0].defined()) return {Tensor(), Tensor(), Tensor(), Tensor(), Tensor()};
    auto gv = transform_pinhole_backward_hip(saved[0], saved[1], saved[2], saved[3], saved[4], grad_outputs[0]);
    return {gv, Tensor(), Tensor(), Tensor(), Tensor()};
  }
};

Tensor transform_pinhole_autograd(
    const Tensor& v, const Tensor& campos, const Tensor& camrot, const Tensor& focal, const Tensor& princpt) {
  return TransformPinholeFunction::apply(v, campos, camrot, focal, princpt)[0];
}

// ---------------------------------------------------------------------------------------------
// transform_distort -- the distortion camera models (radial-tangential, fisheye, fisheye62 + lookup table) of
// drtk/utils/projection.py:56-310,618-644 over drtk_amd_transform_distort[_backward].  Returns (v_pix, v_cam);
// v_cam is an empty tensor unless need_v_cam.  Differentiable with respect to v only, through both outputs.
// ---------------------------------------------------------------------------------------------
using OptTensor = std::optional<Tensor>;

struct DistortArgs {
  TransformArgs t;
  Tensor coeff, fov, modes, lut, spacing;
  const int32_t* modes_ptr = nullptr;
  const void* lut_ptr = nullptr;
  const void* spacing_ptr = nullptr;
  int64_t Hl = 0, Wl = 0;
  int ncoef = 0;
};
DistortArgs distort_prep(
    const Tensor& v, const Tensor& campos, const Tensor& camrot, const Tensor& focal, const Tensor& princpt,
    int64_t mode_all, const OptTensor& mode_per_view, const Tensor& coeff, const Tensor& fov, const OptTensor& lut,
    const OptTensor& lut_spacing) {
  DistortArgs a;
  a.t = transform_prep(v, campos, camrot, focal, princpt);
  const int64_t N = a.t.N;
  const auto dt = v.scalar_type();
  TORCH_CHECK(mode_all >= 0 && mode_all <= 3, "transform(): distortion mode id must be 0 (pinhole), 1 (radial-tangential), 2 (fisheye) or 3 (fisheye62)");
  TORCH_CHECK(coeff.dim() == 2 && coeff.size(0) == N && (coeff.size(1) == 4 || coeff.size(1) == 5 || coeff.size(1) == 8),
              "transform(): expected distortion_coeff of shape [N, 4], [N, 5] or [N, 8]");
  TORCH_CHECK(fov.numel() == N, "transform(): expected fov with one value per camera");
  a.ncoef = static_cast<int>(coeff.size(1));
  a.coeff = coeff.to(dt).contiguous();
  a.fov = fov.to(dt).reshape({N}).contiguous();
  if (mode_per_view.has_value() && mode_per_view->defined()) {
    TORCH_CHECK(mode_per_view->scalar_type() == at::kInt && mode_per_view->dim() == 1 && mode_per_view->size(0) == N &&
                    mode_per_view->device() == v.device(),
                "transform(): expected the per-view modes as an int32 tensor of shape [N] on the device of v");
    a.modes = mode_per_view->contiguous();
    a.modes_ptr = a.modes.data_ptr<int32_t>();
  }
  if (lut.has_value() && lut->defined()) {
    TORCH_CHECK(lut_spacing.has_value() && lut_spacing->defined(), "lookup table spacing must be provided along with vector field");
    TORCH_CHECK(lut->dim() == 4 && lut->size(0) == N && lut->size(1) == 2 && lut->size(2) >= 1 && lut->size(3) >= 1,
                "transform(): expected lut_vector_field of shape [N, 2, H_lut, W_lut]");
    TORCH_CHECK(lut_spacing->dim() == 2 && lut_spacing->size(0) == N && lut_spacing->size(1) == 2,
                "transform(): expected lut_spacing of shape [N, 2]");
    a.lut = lut->to(dt).contiguous();
    a.spacing = lut_spacing->to(dt).contiguous();
    a.lut_ptr = a.lut.data_ptr();
    a.spacing_ptr = a.spacing.data_ptr();
    a.Hl = lut->size(2), a.Wl = lut->size(3);
  }
  for (const Tensor* t : {&a.t.campos, &a.t.camrot, &a.t.focal, &a.t.princpt, &a.coeff, &a.fov})
    TORCH_CHECK(t->device() == v.device(), "transform(): all tensors must be on the device of v");
  return a;
}

std::tuple<Tensor, Tensor> transform_distort_hip(
    const Tensor& v, const Tensor& campos, const Tensor& camrot, const Tensor& focal, const Tensor& princpt,
    int64_t mode_all, const OptTensor& mode_per_view, const Tensor& coeff, const Tensor& fov, bool cull_outside_fov,
    const OptTensor& lut, const OptTensor& lut_spacing, bool need_v_cam) {
  const drtk_dtype_t dt = dtype_of(v, "transform");
  c10::hip::OptionalHIPGuardMasqueradingAsCUDA guard(v.device());
  const DistortArgs a = distort_prep(v, campos, camrot, focal, princpt, mode_all, mode_per_view, coeff, fov, lut, lut_spacing);
  auto v_pix = out_empty({a.t.N, a.t.V, 3}, v.options());
  auto v_cam = need_v_cam ? out_empty({a.t.N, a.t.V, 3}, v.options()) : at::empty({0}, v.options());
  check_status(
      drtk_amd_transform_distort(
          dt, a.t.v.data_ptr(), a.t.v_sN, a.t.campos.data_ptr(), a.t.camrot.data_ptr(), a.t.focal.data_ptr(),
          a.t.princpt.data_ptr(), static_cast<int>(mode_all), a.modes_ptr, a.coeff.data_ptr(), a.ncoef, a.fov.data_ptr(),
          cull_outside_fov ? 1 : 0, a.lut_ptr, a.spacing_ptr, a.Hl, a.Wl, a.t.N, a.t.V, v_pix.data_ptr(),
          need_v_cam ? v_cam.data_ptr() : nullptr, current_stream(v)),
      "transform");
  return {v_pix, v_cam};
}

Tensor transform_distort_backward_hip(
    const Tensor& v, const Tensor& campos, const Tensor& camrot, const Tensor& focal, const Tensor& princpt,
    int64_t mode_all, const OptTensor& mode_per_view, const Tensor& coeff, const Tensor& fov, bool cull_outside_fov,
    const OptTensor& lut, const OptTensor& lut_spacing, const Tensor& grad_v_pix, const Tensor& grad_v_cam) {
  const drtk_dtype_t dt = dtype_of(v, "transform_backward");
  c10::hip::OptionalHIPGuardMasqueradingAsCUDA guard(v.device());
  const DistortArgs a = distort_prep(v, campos, camrot, focal, princpt, mode_all, mode_per_view, coeff, fov, lut, lut_spacing);
  Tensor gp, gc;
  if (grad_v_pix.defined()) {
    TORCH_CHECK(grad_v_pix.numel() == a.t.N * a.t.V * 3, "transform_backward(): grad_v_pix must be [N, V, 3]");
    gp = grad_v_pix.to(v.scalar_type()).contiguous();
  }
  if (grad_v_cam.defined()) {
    TORCH_CHECK(grad_v_cam.numel() == a.t.N * a.t.V * 3, "transform_backward(): grad_v_cam must be [N, V, 3]");
    gc = grad_v_cam.to(v.scalar_type()).contiguous();
  }
  auto grad_v = at::empty_like(a.t.v); // [1,V,3] (summed over views) or [N,V,3]
  check_status(
      drtk_amd_transform_distort_backward(
          dt, a.t.v.data_ptr(), a.t.v_sN, a.t.campos.data_ptr(), a.t.camrot.data_ptr(), a.t.focal.data_ptr(),
          a.t.princpt.data_ptr(), static_cast<int>(mode_all), a.modes_ptr, a.coeff.data_ptr(), a.ncoef, a.fov.data_ptr(),
          cull_outside_fov ? 1 : 0, a.lut_ptr, a.spacing_ptr, a.Hl, a.Wl, gp.defined() ? gp.data_ptr() : nullptr,
          gc.defined() ? gc.data_ptr() : nullptr, a.t.N, a.t.V, grad_v.data_ptr(), current_stream(v)),
      "transform_backward");
  return grad_v;
}

std::tuple<Tensor, Tensor> transform_distort_cpu(
    const Tensor&, const Tensor&, const Tensor&, const Tensor&, const Tensor&, int64_t, const OptTensor&, const Tensor&,
    const Tensor&, bool, const OptTensor&, const OptTensor&, bool) {
  no_cpu("transform");
}

std::tuple<Tensor, Tensor> transform_distort_op(
    const Tensor& v, const Tensor& campos, const Tensor& camrot, const Tensor& focal, const Tensor& princpt,
    int64_t mode_all, const OptTensor& mode_per_view, const Tensor& coeff, const Tensor& fov, bool cull_outside_fov,
    const OptTensor& lut, const OptTensor& lut_spacing, bool need_v_cam) {
  static auto op = c10::Dispatcher::singleton()
                       .findSchemaOrThrow("drtk_amd_ext::transform_distort", "")
                       .typed<decltype(transform_distort_op)>();
  return op.call(v, campos, camrot, focal, princpt, mode_all, mode_per_view, coeff, fov, cull_outside_fov, lut, lut_spacing, need_v_cam);
}

class TransformDistortFunction : public torch::autograd::Function<TransformDistortFunction> {
 public:
  static tensor_list forward(
      AutogradContext* ctx, const Tensor& v, const Tensor& campos, const Tensor& camrot, const Tensor& focal,
      const Tensor& princpt, int64_t mode_all, const OptTensor& mode_per_view, const Tensor& coeff, const Tensor& fov,
      bool cull_outside_fov, const OptTensor& lut, const OptTensor& lut_spacing, bool need_v_cam) {
    ctx->set_materialize_grads(false);
    ctx->save_for_backward({v, campos, camrot, focal, princpt, coeff, fov, mode_per_view.value_or(Tensor()),
                            lut.value_or(Tensor()), lut_spacing.value_or(Tensor())});
    ctx->saved_data["mode_all"] = mode_all;
    ctx->saved_data["cull"] = cull_outside_fov;
    at::AutoDispatchBelowADInplaceOrView g;
    auto out = transform_distort_op(v, campos, camrot, focal, princpt, mode_all, mode_per_view, coeff, fov, cull_outside_fov,
                                    lut, lut_spacing, need_v_cam);
    if (!need_v_cam) ctx->mark_non_differentiable({std::get<1>(out)});
    return {std::get<0>(out), std::get<1>(out)};
  }
  static tensor_list backward(AutogradContext* ctx, tensor_list grad_outputs) {
    const auto s = ctx->get_saved_variables();
    tensor_list none(13);
    const bool any = grad_outputs[0].defined() || (grad_outputs[1].defined() && grad_outputs[1].numel() > 0);
    if (!s[0].requires_grad() || !any) return none;
    auto opt = [](const Tensor& t) { return t.defined() ? OptTensor(t) : OptTensor(); };
    none[0] = transform_distort_backward_hip(
        s[0], s[1], s[2], s[3], s[4], ctx->saved_data["mode_all"].toInt(), opt(s[7]), s[5], s[6],
        ctx->saved_data["cull"].toBool(), opt(s[8]), opt(s[9]), grad_outputs[0],
        grad_outputs[1].defined() && grad_outputs[1].numel() > 0 ? grad_outputs[1] : Tensor());
    return none;
  }
};

std::tuple<Tensor, Tensor> transform_distort_autograd(
    const Tensor& v, const Tensor& campos, const Tensor& camrot, const Tensor& focal, const Tensor& princpt,
    int64_t mode_all, const OptTensor& mode_per_view, const Tensor& coeff, const Tensor& fov, bool cull_outside_fov,
    const OptTensor& lut, const OptTensor& lut_spacing, bool need_v_cam) {
  auto out = TransformDistortFunction::apply(v, campos, camrot, focal, princpt, mode_all, mode_per_view, coeff, fov,
                                             cull_outside_fov, lut, lut_spacing, need_v_cam);
  return {out[0], out[1]};
}

} // namespace

TORCH_LIBRARY_FRAGMENT(drtk_amd_ext, m) {
  m.def("transform_pinhole(Tensor v, Tensor campos, Tensor camrot, Tensor focal, Tensor princpt) -> Tensor");
  m.def(
      "transform_distort(Tensor v, Tensor campos, Tensor camrot, Tensor focal, Tensor princpt, int mode_all, "
      "Tensor? mode_per_view, Tensor coeff, Tensor fov, bool cull_outside_fov, Tensor? lut, Tensor? lut_spacing, "
      "bool need_v_cam) -> (Tensor, Tensor)");
}
TORCH_LIBRARY_IMPL(drtk_amd_ext, Autograd, m) {
  m.impl("transform_pinhole", &transform_pinhole_autograd);
  m.impl("transform_distort", &transform_distort_autograd);
}
TORCH_LIBRARY_IMPL(drtk_amd_ext, CUDA, m) {
  m.impl("transform_pinhole", &transform_pinhole_hip);
  m.impl("transform_distort", &transform_distort_hip);
}
TORCH_LIBRARY_IMPL(drtk_amd_ext, CPU, m) {
  m.impl("transform_pinhole", &transform_pinhole_cpu);
  m.impl("transform_distort", &transform_distort_cpu);
}
