// drtk_amd_ext::mipmap_pyramid -- the mip chain of one texture, over drtk_amd_mipmap_pyramid / drtk_amd_mipmap_pyramid_backward
// (include/drtk_amd.h).  No reference counterpart.  Host-only C++; the CPU key raises.
#include "common.hpp"

namespace {
using namespace drtk_amd_torch;

constexpr int64_t kMaxLevels = 11; // what mipmap_grid_sampler_2d takes

int64_t max_levels(int64_t H, int64_t W) {
  int64_t m = std::min(H, W), levels = 0;
  while (m >= 1 && levels < kMaxLevels) m >>= 1, ++levels;
  return levels;
}

void pyramid_check(const Tensor& input, int64_t levels) {
  TORCH_CHECK(input.defined(), "mipmap_pyramid(): expected input to be defined");
  TORCH_CHECK(
      input.is_floating_point(), "mipmap_pyramid(): expected input to have floating point type, but input has ", input.dtype());
  TORCH_CHECK(input.layout() == at::kStrided, "mipmap_pyramid(): expected input to have torch.strided layout");
  TORCH_CHECK(
      input.dim() == 4, "mipmap_pyramid(): expected input.ndim == 4 ([N, C, H, W]), but got input with sizes ", input.sizes());
  dtype_of(input, "mipmap_pyramid"); // float32 and float64 only, like the sampler
  const int64_t C = input.size(1), H = input.size(2), W = input.size(3);
  TORCH_CHECK(
      H > 0 && W > 0, "mipmap_pyramid(): expected input to have non-empty spatial dimensions, but input has sizes ", input.sizes());
  TORCH_CHECK(C >= 1, "mipmap_pyramid(): expected at least one channel, but got input with sizes ", input.sizes());
  TORCH_CHECK(H * W < (int64_t(1) << 31), "mipmap_pyramid(): expected H * W to be less than 2147483648, but got H: ", H, ", W: ", W);
  const int64_t most = max_levels(H, W);
  TORCH_CHECK_VALUE(
      levels >= 1 && levels <= most, "mipmap_pyramid(): levels must be in [1, ", most, "] for a ", H, " x ", W,
      " texture (halving until the smaller side is 1, at most ", kMaxLevels, " levels), but got ", levels);
}

// the last two dimensions form a contiguous H x W plane (planes of at most one element always do)
bool planes_contiguous(const Tensor& t) {
  const int64_t H = t.size(2), W = t.size(3);
  return (W <= 1 || t.stride(3) == 1) && (H <= 1 || t.stride(2) == W);
}

// Level 0 is `input` itself; levels 1 and up are views into ONE allocation, back to back at multiples of 16 bytes -- the layout
// of the sampler's gradient pyramid (mipmap.cpp).
std::vector<Tensor> mipmap_pyramid_hip(const Tensor& input, int64_t levels) {
  pyramid_check(input, levels);
  TORCH_CHECK(input.is_cuda(), "mipmap_pyramid(): expected input to be on a cuda device");
  std::vector<Tensor> out = {input};
  if (levels == 1) return out;
  const drtk_dtype_t dt = dtype_of(input, "mipmap_pyramid");
  c10::hip::OptionalHIPGuardMasqueradingAsCUDA guard(input.device());
  const Tensor in = planes_contiguous(input) && input.stride(0) >= 0 && input.stride(1) >= 0 ? input : input.contiguous();
  const int64_t N = in.size(0), C = in.size(1), H = in.size(2), W = in.size(3);
  const int64_t per16 = 16 / static_cast<int64_t>(in.element_size());
  std::vector<int64_t> offs(levels, 0), sn(levels, 0);
  int64_t total = 0;
  for (int64_t l = 1; l < levels; ++l) {
    offs[l] = total;
    sn[l] = C * (H >> l) * (W >> l);
    total += (N * sn[l] + per16 - 1) / per16 * per16;
  }
  const Tensor flat = out_empty({total}, input.options());
  std::vector<void*> ptrs(levels, nullptr);
  for (int64_t l = 1; l < levels; ++l) {
    out.push_back(flat.narrow(0, offs[l], N * sn[l]).view({N, C, H >> l, W >> l}));
    ptrs[l] = out.back().data_ptr();
  }
  check_status(
      drtk_amd_mipmap_pyramid(
          dt, in.data_ptr(), in.stride(0), in.stride(1), N, C, H, W, static_cast<int>(levels), ptrs.data(), sn.data(),
          current_stream(input)),
      "mipmap_pyramid");
  return out;
}

std::vector<Tensor> mipmap_pyramid_cpu(const Tensor& input, int64_t levels) {
  pyramid_check(input, levels); // a bad call reads the same with and without a device
  no_cpu("mipmap_pyramid");
}

std::vector<Tensor> mipmap_pyramid_op(const Tensor& input, int64_t levels) {
  static auto op =
      c10::Dispatcher::singleton().findSchemaOrThrow("drtk_amd_ext::mipmap_pyramid", "").typed<decltype(mipmap_pyramid_op)>();
  return op.call(input, levels);
}

// grad_input [N,C,H,W] from the gradients of the levels; an undefined one is absent
Tensor mipmap_pyramid_backward_hip(const tensor_list& grads, const std::vector<int64_t>& sizes, const at::TensorOptions& options) {
  const int64_t N = sizes[0], C = sizes[1], H = sizes[2], W = sizes[3];
  const int levels = static_cast<int>(grads.size());
  const auto type = c10::typeMetaToScalarType(options.dtype());
  const drtk_dtype_t dt = type == at::kFloat ? DRTK_F32 : DRTK_F64;
  c10::hip::OptionalHIPGuardMasqueradingAsCUDA guard(options.device());
  std::vector<Tensor> holders(levels);
  std::vector<const void*> ptrs(levels, nullptr);
  std::vector<int64_t> sn(levels, 0);
  for (int l = 0; l < levels; ++l) {
    if (!grads[l].defined()) continue;
    TORCH_CHECK(
        grads[l].sizes() == at::IntArrayRef({N, C, H >> l, W >> l}), "mipmap_pyramid(): the gradient of level ", l, " has sizes ",
        grads[l].sizes());
    holders[l] = grads[l].to(type).contiguous();
    ptrs[l] = holders[l].data_ptr();
    sn[l] = C * (H >> l) * (W >> l);
  }
  Tensor grad_input = out_empty({N, C, H, W}, options);
  check_status(
      drtk_amd_mipmap_pyramid_backward(
          dt, ptrs.data(), sn.data(), N, C, H, W, levels, grad_input.data_ptr(),
          static_cast<drtk_stream_t>(c10::hip::getCurrentHIPStream(options.device().index()).stream())),
      "mipmap_pyramid_backward");
  return grad_input;
}

// The node returns `levels` tensors of which element 0 is the input itself: autograd hands an unmodified input back as an alias
// whose gradient arrives here, so g_0 is folded in by the same launch as every other level.  Nothing is saved but sizes.
class MipmapPyramidFunction : public torch::autograd::Function<MipmapPyramidFunction> {
 public:
  static tensor_list forward(AutogradContext* ctx, const Tensor& input, int64_t levels) {
    ctx->set_materialize_grads(false);
    ctx->saved_data["sizes"] = input.sizes().vec();
    ctx->saved_data["dtype"] = static_cast<int64_t>(input.scalar_type());
    ctx->saved_data["device"] = input.device();
    std::vector<Tensor> out;
    {
      at::AutoDispatchBelowADInplaceOrView g;
      out = mipmap_pyramid_op(input, levels);
    }
    out[0] = input;
    return out;
  }
  static tensor_list backward(AutogradContext* ctx, tensor_list grad_outputs) {
    tensor_list grads(2); // levels gets none
    bool any = false;
    for (const Tensor& g : grad_outputs) any = any || g.defined();
    if (!any) return grads;
    // the backward is a kernel, not a graph of differentiable operations: with create_graph=True its result would pass for a constant
    TORCH_CHECK(
        !at::GradMode::is_enabled(),
        "mipmap_pyramid(): double backward (create_graph=True) is not supported by drtk_amd's mipmap_pyramid kernels");
    const auto options = at::TensorOptions()
                             .dtype(static_cast<at::ScalarType>(ctx->saved_data["dtype"].toInt()))
                             .device(ctx->saved_data["device"].toDevice());
    grads[0] = mipmap_pyramid_backward_hip(grad_outputs, ctx->saved_data["sizes"].toIntVector(), options);
    return grads;
  }
};

std::vector<Tensor> mipmap_pyramid_autograd(const Tensor& input, int64_t levels) {
  pyramid_check(input, levels);
  if (levels == 1) { // [input]: nothing to differentiate (the CPU key still raises)
    at::AutoDispatchBelowADInplaceOrView g;
    return mipmap_pyramid_op(input, levels);
  }
  return MipmapPyramidFunction::apply(input, levels);
}

std::vector<Tensor> mipmap_pyramid_autocast(const Tensor& input, int64_t levels) {
  c10::impl::ExcludeDispatchKeyGuard no_autocast(c10::DispatchKey::Autocast);
  return mipmap_pyramid_op(at::autocast::cached_cast(at::kFloat, input), levels);
}

} // namespace

TORCH_LIBRARY_FRAGMENT(drtk_amd_ext, m) {
  m.def("mipmap_pyramid(Tensor input, int levels) -> Tensor[]");
}
TORCH_LIBRARY_IMPL(drtk_amd_ext, Autograd, m) {
  m.impl("mipmap_pyramid", &mipmap_pyramid_autograd);
}
TORCH_LIBRARY_IMPL(drtk_amd_ext, Autocast, m) {
  m.impl("mipmap_pyramid", mipmap_pyramid_autocast);
}
TORCH_LIBRARY_IMPL(drtk_amd_ext, CUDA, m) {
  m.impl("mipmap_pyramid", &mipmap_pyramid_hip);
}
TORCH_LIBRARY_IMPL(drtk_amd_ext, CPU, m) {
  m.impl("mipmap_pyramid", &mipmap_pyramid_cpu);
}
