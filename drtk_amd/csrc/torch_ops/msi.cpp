// msi_ext::msi -- src/msi/msi_module.cpp:23-177 and the host side of src/msi/msi_kernel.cu:411-628.
#include "common.hpp"

namespace {
using namespace drtk_amd_torch;

// the reference's checks (msi_kernel.cu:419-519)
void msi_check(
    const Tensor& ray_o, const Tensor& ray_d, const Tensor& texture, int64_t sub_step_count, double min_inv_r,
    double max_inv_r, double stop_thresh) {
  TORCH_CHECK(sub_step_count > 0, "msi(): expected step_size > 0, but got ", sub_step_count);
  TORCH_CHECK(stop_thresh > 0 && stop_thresh < 1, "msi(): expected 0 < stop_thresh < 1, but got ", stop_thresh);
  TORCH_CHECK(
      min_inv_r > max_inv_r, "msi(): expected min_inv_r to be greater than max_inv_r, but got min_inv_r:", min_inv_r,
      " and max_inv_r: ", max_inv_r);
  TORCH_CHECK(ray_o.defined() && ray_d.defined() && texture.defined(), "msi(): expected all inputs not be undefined");
  TORCH_CHECK(
      ray_o.device() == ray_d.device() && ray_o.device() == texture.device(),
      "msi(): expected all inputs to be on same device, but input ray_o is ", ray_o.device(), ", ray_d is ", ray_d.device(),
      ", texture is ", texture.device());
  const auto tex_dtype = texture.scalar_type();
  TORCH_CHECK(
      tex_dtype == at::kDouble || tex_dtype == at::kFloat || tex_dtype == at::kHalf,
      "msi(): expected texture to be of type Double, Float or Half, but got type ", tex_dtype);
  TORCH_CHECK(
      ray_o.scalar_type() == at::kFloat && ray_d.scalar_type() == at::kFloat,
      "msi(): expected ray_o and ray_d to be of type Float, but input ray_o is  ", ray_o.scalar_type(), " and ray_d is ",
      ray_d.scalar_type());
  TORCH_CHECK(
      ray_o.layout() == at::kStrided && ray_d.layout() == at::kStrided && texture.layout() == at::kStrided,
      "msi(): expected all inputs to have torch.strided layout");
  TORCH_CHECK(
      ray_o.dim() == 2 && ray_d.dim() == 2 && texture.dim() == 4,
      "msi(): expected ray_o and ray_d to have 2 dimensions, and texture to have 4 dimension, but got ray_o with size ",
      ray_o.sizes(), ", ray_d with size ", ray_d.sizes(), ", texture with size ", texture.sizes());
  TORCH_CHECK(
      ray_o.size(1) == 3 && ray_d.size(1) == 3 && texture.size(1) == 4,
      "msi(): expected ray_o, ray_d to have size 3 along the dimension 1,  and texture to have size 4 along the dimension 1, "
      "but got ray_o with size ",
      ray_o.sizes(), ", ray_d with size ", ray_d.sizes(), ", texture with size ", texture.sizes());
  TORCH_CHECK(
      ray_o.size(0) == ray_d.size(0),
      "msi(): expected ray_o, ray_d to have the same size along the dimension 0, but got ray_o with size ", ray_o.sizes(),
      ", ray_d with size ", ray_d.sizes());
}

Tensor msi_hip(
    const Tensor& ray_o, const Tensor& ray_d, const Tensor& texture, int64_t sub_step_count, double min_inv_r,
    double max_inv_r, double stop_thresh) {
  msi_check(ray_o, ray_d, texture, sub_step_count, min_inv_r, max_inv_r, stop_thresh);
  // float and double kernels only: half precision arrives through autocast, which casts it to float (as the reference's
  // DISPATCH_FLOAT, kernel_utils.h:35-57, has no half branch either)
  const drtk_dtype_t dt = dtype_of(texture, "msi_forward_kernel");
  c10::hip::OptionalHIPGuardMasqueradingAsCUDA guard(texture.device());
  const int64_t N = ray_o.size(0);
  TORCH_CHECK(N == 0 || texture.numel() > 0, "msi(): expected a non-empty texture, but got texture with size ", texture.sizes());
  const auto o_c = ray_o.contiguous(), d_c = ray_d.contiguous(), tex_c = texture.contiguous();
  auto out = out_empty({N, 4}, texture.options());
  check_status(
      drtk_amd_msi_forward(
          dt, o_c.data_ptr<float>(), d_c.data_ptr<float>(), tex_c.data_ptr(), N, texture.size(0), texture.size(2), texture.size(3),
          static_cast<int>(sub_step_count), min_inv_r, max_inv_r, stop_thresh, out.data_ptr(), current_stream(texture)),
      "msi");
  return out;
}

Tensor msi_backward_hip(
    const Tensor& rgba_img, const Tensor& rgba_img_grad, const Tensor& ray_o, const Tensor& ray_d, const Tensor& texture,
    int64_t sub_step_count, double min_inv_r, double max_inv_r, double stop_thresh) {
  const drtk_dtype_t dt = dtype_of(texture, "msi_backward_kernel");
  c10::hip::OptionalHIPGuardMasqueradingAsCUDA guard(texture.device());
  const auto o_c = ray_o.contiguous(), d_c = ray_d.contiguous(), tex_c = texture.contiguous();
  const auto out_c = rgba_img.contiguous(), go_c = rgba_img_grad.to(texture.scalar_type()).contiguous();
  auto grad_texture = out_empty(texture.sizes(), texture.options()); // zero-filled by the call
  check_status(
      drtk_amd_msi_backward(
          dt, go_c.data_ptr(), out_c.data_ptr(), o_c.data_ptr<float>(), d_c.data_ptr<float>(), tex_c.data_ptr(), ray_o.size(0),
          texture.size(0), texture.size(2), texture.size(3), static_cast<int>(sub_step_count), min_inv_r, max_inv_r, stop_thresh,
          grad_texture.data_ptr(), current_stream(texture)),
      "msi_backward");
  return grad_texture;
}

// arguments are judged first, so a bad call reads the same with and without a device
Tensor msi_cpu(
    const Tensor& ray_o, const Tensor& ray_d, const Tensor& texture, int64_t sub_step_count, double min_inv_r,
    double max_inv_r, double stop_thresh) {
  msi_check(ray_o, ray_d, texture, sub_step_count, min_inv_r, max_inv_r, stop_thresh);
  no_cpu("msi");
}

Tensor msi_op(
    const Tensor& ray_o, const Tensor& ray_d, const Tensor& texture, int64_t sub_step_count, double min_inv_r,
    double max_inv_r, double stop_thresh) {
  static auto op = c10::Dispatcher::singleton().findSchemaOrThrow("msi_ext::msi", "").typed<decltype(msi_op)>();
  return op.call(ray_o, ray_d, texture, sub_step_count, min_inv_r, max_inv_r, stop_thresh);
}

class MSIFunction : public torch::autograd::Function<MSIFunction> {
 public:
  static tensor_list forward(
      AutogradContext* ctx, const Tensor& ray_o, const Tensor& ray_d, const Tensor& texture, int64_t sub_step_count,
      double min_inv_r, double max_inv_r, double stop_thresh) {
    ctx->set_materialize_grads(false);
    ctx->saved_data["data"] = std::make_tuple(texture.requires_grad(), sub_step_count, min_inv_r, max_inv_r, stop_thresh);
    Tensor rgba_img;
    {
      at::AutoDispatchBelowADInplaceOrView g;
      rgba_img = msi_op(ray_o, ray_d, texture, sub_step_count, min_inv_r, max_inv_r, stop_thresh);
    }
    ctx->save_for_backward({ray_o, ray_d, texture, rgba_img});
    return {rgba_img};
  }
  static tensor_list backward(AutogradContext* ctx, tensor_list grad_outputs) {
    bool requires_grad;
    int64_t sub_step_count;
    double min_inv_r, max_inv_r, stop_thresh;
    std::tie(requires_grad, sub_step_count, min_inv_r, max_inv_r, stop_thresh) =
        ctx->saved_data["data"].to<std::tuple<bool, int64_t, double, double, double>>();
    tensor_list grads(7); // the rays get no gradient; the other arguments are not tensors
    if (!requires_grad || !grad_outputs[0].defined()) return grads;
    const auto saved = ctx->get_saved_variables();
    grads[2] = msi_backward_hip(
        saved[3], grad_outputs[0], saved[0], saved[1], saved[2], sub_step_count, min_inv_r, max_inv_r, stop_thresh);
    return grads;
  }
};

Tensor msi_autograd(
    const Tensor& ray_o, const Tensor& ray_d, const Tensor& texture, int64_t sub_step_count, double min_inv_r,
    double max_inv_r, double stop_thresh) {
  return MSIFunction::apply(ray_o, ray_d, texture, sub_step_count, min_inv_r, max_inv_r, stop_thresh)[0];
}

Tensor msi_autocast(
    const Tensor& ray_o, const Tensor& ray_d, const Tensor& texture, int64_t sub_step_count, double min_inv_r,
    double max_inv_r, double stop_thresh) {
  c10::impl::ExcludeDispatchKeyGuard no_autocast(c10::DispatchKey::Autocast);
  return msi_op(
      at::autocast::cached_cast(at::kFloat, ray_o), at::autocast::cached_cast(at::kFloat, ray_d),
      at::autocast::cached_cast(at::kFloat, texture), sub_step_count, min_inv_r, max_inv_r, stop_thresh);
}

} // namespace

// schema: verbatim from the reference
TORCH_LIBRARY(msi_ext, m) {
  m.def(
      "msi(Tensor ray_o, Tensor ray_d, Tensor texture, int sub_step_count, float min_inv_r, float max_inv_r, float stop_thresh) -> Tensor");
}
TORCH_LIBRARY_IMPL(msi_ext, Autograd, m) {
  m.impl("msi", &msi_autograd);
}
TORCH_LIBRARY_IMPL(msi_ext, Autocast, m) {
  m.impl("msi", msi_autocast);
}
TORCH_LIBRARY_IMPL(msi_ext, CUDA, m) {
  m.impl("msi", &msi_hip);
}
TORCH_LIBRARY_IMPL(msi_ext, CPU, m) { // the reference registers no CPU kernel either
  m.impl("msi", &msi_cpu);
}
